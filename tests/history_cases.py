"""Helpers of tests/test_gpu_nonfinite_history.py: contexts that have seen nothing, the two non-vacuity conditions, the comparison that
names the first differing row, and the VAE-family / cache-logits entry points through the C ABI on a context of the caller's choice
(the façade routes them to one context per device, which other tests of the session have used).

A case is three steps (`run_case`): the clean call on a context that has run nothing else; on a second fresh context the poison
calls - every floating-point data operand NaN or +Inf, at least as large as the clean call in every dimension that sizes a workspace -
and then the clean call again.  Both results must be finite and bit-equal in every returned tensor.  Asserted in every case: each
poison call's own outputs are non-finite in every row, and hg_workspace_bytes is the same before and after the clean call on the
poisoned context (growth would mean ensure() zero-filled a buffer and the clean call ran on zeros, not on the poison)."""
import ctypes as C

import numpy as np
import torch

from hoigen_amd import _lib, synth, vae

POISONS = {"nan": float("nan"), "inf": float("inf")}
RANGE_REPORT = "left the fp16 range inside a tower"


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- contexts ---------------------------------------------------------------------------------------------------------------------------
def workspace_bytes(handle) -> int:
    n = C.c_uint64()
    assert _lib.lib().hg_workspace_bytes(handle, C.byref(n)) == 0
    return int(n.value)


def fresh_context(*modules):
    """Close the native context of façade modules (those that share one included): the next call creates a new one - hg_create, the
    recorded options, the weights - that has run nothing.  The torch parameters stay where they are."""
    for m in modules:
        m._ctx.close()
        for name in ("_loaded_sig", "_adapter_sig", "_text_sig", "_sig"):
            if hasattr(m, name):
                setattr(m, name, None)


def ok(handle, rc, what):
    assert rc == 0, (what, rc, _lib.lib().hg_last_error(handle))


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------
def flat(out):
    """every tensor of a result (a tensor, or nested tuples / lists / dicts of them), in a fixed order"""
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flat(o)]
    assert out is None, type(out)
    return []


def rows_of(t):
    t = t if t.dim() else t.reshape(1)
    return t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(-1, 1)


def first_difference(a, b):
    """where two results part: the tensor, its first differing row (rows = everything but the last dimension) and how many rows differ"""
    for i, (x, y) in enumerate(zip(flat(a), flat(b))):
        if x.shape != y.shape:
            return f"tensor {i}: shapes {tuple(x.shape)} and {tuple(y.shape)}"
        bad = (rows_of(x) != rows_of(y)).any(dim=-1).nonzero()      # (NaN != NaN: a non-finite row counts as differing)
        if bad.numel():
            r = int(bad[0])
            return f"tensor {i} of shape {tuple(x.shape)}: row {r} of {rows_of(x).shape[0]} ({bad.numel()} rows differ, the last one {int(bad[-1])})"
    return "no row"


def all_finite(out):
    return all(bool(torch.isfinite(t).all()) for t in flat(out) if t.is_floating_point())


def every_row_non_finite(out):
    """no row of any floating-point tensor of `out` is wholly finite"""
    return all(not bool(torch.isfinite(rows_of(t)).all(dim=-1).any()) for t in flat(out) if t.is_floating_point())


def same_bits(a, b):
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(fa, fb))


# ---- one case ---------------------------------------------------------------------------------------------------------------------------
REFERENCES = {}      # key -> the clean call's result on a context that has run nothing else (shared by the NaN and the Inf form: read-only)


def run_case(key, what, fresh, clean, poisons, handle, warm=None, report=False):
    """fresh(): a context that has run nothing; clean() -> result; poisons: calls that return what must be non-finite in every row;
    handle() -> the native handle of the context in use; warm (cross-entry cases): a call made on the second context BEFORE the poison
    - the clean call itself, on finite data - so that the buffers the poisoning entry point does not own have their size already;
    report: the poison may raise the towers' sticky range report (Inf only: NaN compares false), which the next call delivers - it
    is consumed before the clean call and the case says whether it came."""
    if key not in REFERENCES:
        fresh()
        ref = clean()
        assert all_finite(ref), f"{what}: the reference is not finite"
        REFERENCES[key] = ref
    ref = REFERENCES[key]
    fresh()
    if warm is not None:
        assert same_bits(warm(), ref), f"{what}: the same call on a second fresh context differs first at {first_difference(warm(), ref)}"
    for i, p in enumerate(poisons):
        out = p()
        torch.cuda.synchronize()
        assert every_row_non_finite(out), f"{what}: poison call {i} left a finite row: the case would pass vacuously"
    before = workspace_bytes(handle())
    reported = False
    try:
        got = clean()
    except RuntimeError as e:
        if not report or RANGE_REPORT not in str(e):
            raise
        reported = True
        assert workspace_bytes(handle()) == before
        got = clean()
    torch.cuda.synchronize()
    after = workspace_bytes(handle())
    if report:
        print(f"\nNONFINITE_HISTORY {what}: range report {'delivered and consumed' if reported else 'not raised'}")
    assert after == before, f"{what}: the workspace grew during the clean call ({before} -> {after} bytes): it ran on fresh zeros, not on the poison"
    assert all_finite(got), f"{what}: the clean call after the poison is not finite, first at {first_difference(got, ref)}"
    assert same_bits(got, ref), f"{what}: the clean call depends on the poisoned history, first at {first_difference(got, ref)}"
    return reported


# ---- VAE family and cache logits through the C ABI --------------------------------------------------------------------------------------
DIM = 512
_held = {}


def _modules():
    """the seeded Encoder / Generator / mlp_net as parameter holders on the device (never called: their forward goes to the shared context)"""
    if not _held:
        E, G, M = vae.Encoder(), vae.Generator(), vae.mlp_net(DIM, DIM, DIM)
        E.load_state_dict(synth.to_torch(synth.encoder_state_dict(2)))
        G.load_state_dict(synth.to_torch(synth.generator_state_dict(3)))
        M.load_state_dict(synth.to_torch(synth.mlp_net_state_dict(4)))
        g = torch.Generator().manual_seed(8)
        S, NC = 200, 24
        w = torch.randn(S, DIM, generator=g)
        lab = (torch.rand(S, NC, generator=g) < 0.2).float()
        _held.update(E=E.to(dev()), G=G.to(dev()), M=M.to(dev()), cache=[t.to(dev()).contiguous() for t in
                     (w / w.norm(dim=1, keepdim=True), -torch.ones(S), lab, lab.sum(0).clamp_min(1.0))], NC=NC)
    return _held


def load_family(h, vae_fused=None):
    """VAE (slot 0), mlp_net (slot 0) and a labelled cache model (slot 0) into the context h"""
    m, lib = _modules(), _lib.lib()
    if vae_fused is not None:
        ok(h, lib.hg_set_option(h, b"vae_fused", int(vae_fused)), "vae_fused")
    w = _lib.hg_vae_weights()
    m["E"]._weights(w)
    m["G"]._weights(w)
    ok(h, lib.hg_load_vae(h, 0, C.byref(w)), "hg_load_vae")
    t, M = _lib.tensor, m["M"]
    mw = _lib.hg_mlp_weights(DIM, DIM, DIM, t(M.net[0].weight), t(M.net[0].bias), t(M.net[2].weight), t(M.net[2].bias), t(M.net[4].weight),
                             t(M.net[4].bias))
    ok(h, lib.hg_load_mlp(h, 0, C.byref(mw)), "hg_load_mlp")
    cw = _lib.hg_cache_weights()
    cw.weight, cw.bias, cw.labels, cw.sample_lens = (t(x) for x in m["cache"])
    cw.S, cw.K, cw.C, cw.post_div = m["cache"][0].shape[0], DIM, m["NC"], 1.0
    ok(h, lib.hg_load_cache(h, 0, C.byref(cw)), "hg_load_cache")


def family_call(h, entry, x, eps=None, keep=None):
    """one call of `entry` ("vae", "generator", "mlp_net", "cache") on x [R, 512] (vae: and eps) -> tuple of outputs (keep: of these only)"""
    if keep is not None:
        outs = family_call(h, entry, x, eps)
        return tuple(outs[i] for i in keep)
    lib, R = _lib.lib(), x.shape[0]
    x = x.contiguous()
    if entry == "vae":
        eps = eps.contiguous()
        outs = tuple(torch.empty_like(x) for _ in range(4))      # mean, log_var, z, bias
        ok(h, lib.hg_vae_forward(h, 0, x.data_ptr(), eps.data_ptr(), R, *(o.data_ptr() for o in outs), stream()), "hg_vae_forward")
        return outs
    if entry == "generator":
        out = torch.empty_like(x)
        ok(h, lib.hg_generator(h, 0, x.data_ptr(), R, out.data_ptr(), stream()), "hg_generator")
    elif entry == "mlp_net":
        out = torch.empty_like(x)
        ok(h, lib.hg_mlp_net(h, 0, x.data_ptr(), R, out.data_ptr(), stream()), "hg_mlp_net")
    else:
        assert entry == "cache", entry
        out = torch.empty(R, _modules()["NC"], device=x.device)
        ok(h, lib.hg_cache_logits(h, 0, x.data_ptr(), R, out.data_ptr(), stream()), "hg_cache_logits")
    return (out,)


def family_rows(n, seed):
    """x (L2-normalised rows, what the VAE is fed) and eps [n, 512] on the device"""
    x = torch.from_numpy(synth.hg_normal((n, DIM), seed))
    return (x / x.norm(dim=1, keepdim=True)).to(dev()), torch.from_numpy(synth.hg_normal((n, DIM), seed + 1)).to(dev())


def to_dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())
