"""Every row of the residual stream of both towers, block by block, against fp64 (hg_test_image_stream / hg_test_text_stream).

The parity tests compare the rows that reach an output: the class row of every crop, the EOT row of every prompt.  The other rows - 196
of every 197-token crop, every text row after EOT (the mask is causal: they reach nothing), every row of a last block run on all rows -
meet the reference only through later attention, or not at all.  Here the hooks copy EVERY row of the stream into a trace after ln_pre /
the embedding and after every block, and each block is checked on its own:

(a) one-block step: ref = oracle resblock(trace[i]) in fp64 (oracle/clip_oracle.py, run on the device: torch's fp64 GEMMs are not the
    kernels under test), err = ||trace[i+1] - ref|| / ||ref - mean(ref)|| per row.  The step isolates the block, so the bound can follow
    each block's own error level: the separate-LayerNorm path (ln_fuse = 0, every row of the last block) is the BASELINE - kernels pinned
    by test_gpu_gemm.py / test_gpu_attention.py, none of the folded, hi / lo, pair or fused machinery - and for every path and block
      every row        err <= 2 x max over rows of the baseline's err      (a defect confined to some rows)
      median of rows   err <= 2 x median of the baseline's err             (a defect spread over every row, e.g. a lost lo half)
      baseline         err <= 1e-3 on every row                            (a gross ceiling)
    With option last_block_row0 = 1 the last entry holds the n selected rows (class / EOT rows) densely; medians are then taken over the
    baseline's same rows.
(b) bit for bit, every entry and every row: mlp_pair 1 against 0 with (mlp_pair_chunk, mlp_pair_fc_slots) in {(32, 32), (8, 30), (3, 24)},
    qkv_attn 2 / 1 / 0, text_ln_fold = 0 against ln_fuse = 0, and the hook's output against the entry point's.  A path that must equal
    another inherits its (a) numbers; if it does not, its own errors are computed and reported as well.
(c) drift: the last entry of every path against the oracle's whole tower in fp64 from the same input, median over rows <= 2 x the
    baseline's median on the same rows.

A failure names the block, the row as (sequence, token), its 256-row panel, the panel's XCD (panel mod 8) and its 128-row half.  Every
case, path and block prints the median and the worst row next to the baseline's (`-s`).
"""
import json
import os

import numpy as np
import pytest
import torch

from hoigen_amd import _lib, clip, synth
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 2.0
CEIL = 1e-3
HG_PROF_MLP_PAIR = 103
OPTS = ("last_block_row0", "ln_fuse", "stream_hilo", "mlp_pair", "mlp_pair_chunk", "mlp_pair_fc_slots", "qkv_attn", "text_ln_fold")
BASELINE = {"ln_fuse": 0, "last_block_row0": 0}
PAIR_SETTINGS = ((32, 32), (8, 30), (3, 24))

# (name, options, name of the path whose trace it must equal bit for bit - or None: checked against the oracle)
VISION_PATHS = [
    ("default", {"mlp_pair_chunk": 32, "mlp_pair_fc_slots": 32}, None),
    ("last_block_row0=0", {"last_block_row0": 0}, None),
    ("ln_fuse=0", {"ln_fuse": 0}, None),
    ("stream_hilo=0", {"stream_hilo": 0}, None),
    ("mlp_pair=0", {"mlp_pair": 0}, "default"),
    ("mlp_pair=0 last_block_row0=0", {"mlp_pair": 0, "last_block_row0": 0}, "last_block_row0=0"),
    ("mlp_pair=0 stream_hilo=0", {"mlp_pair": 0, "stream_hilo": 0}, "stream_hilo=0"),
] + [(f"mlp_pair chunk {c} fc_slots {s}", {"mlp_pair_chunk": c, "mlp_pair_fc_slots": s}, "default") for c, s in PAIR_SETTINGS[1:]] + [
    (f"qkv_attn={q}", {"qkv_attn": q}, "default") for q in (2, 1, 0)] + [
    ("qkv_attn=2 last_block_row0=0", {"qkv_attn": 2, "last_block_row0": 0}, "last_block_row0=0")]
TEXT_PATHS = [
    ("default", {"mlp_pair_chunk": 32, "mlp_pair_fc_slots": 32}, None),
    ("last_block_row0=0", {"last_block_row0": 0}, None),
    ("text_ln_fold=2", {"text_ln_fold": 2}, None),
    ("text_ln_fold=0", {"text_ln_fold": 0}, None),
    ("text_ln_fold=0 last_block_row0=0", {"text_ln_fold": 0, "last_block_row0": 0}, "baseline"),
    ("mlp_pair=0", {"mlp_pair": 0}, "default"),
    ("mlp_pair=0 last_block_row0=0", {"mlp_pair": 0, "last_block_row0": 0}, "last_block_row0=0"),
    ("mlp_pair=0 text_ln_fold=2", {"mlp_pair": 0, "text_ln_fold": 2}, "text_ln_fold=2"),
] + [(f"mlp_pair chunk {c} fc_slots {s}", {"mlp_pair_chunk": c, "mlp_pair_fc_slots": s}, "default") for c, s in PAIR_SETTINGS[1:]] + [
    (f"mlp_pair chunk {c} fc_slots {s} text_ln_fold=2", {"mlp_pair_chunk": c, "mlp_pair_fc_slots": s, "text_ln_fold": 2}, "text_ln_fold=2")
    for c, s in PAIR_SETTINGS[1:]]
DEFAULT_ONLY = [("default", {}, None)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


class Tower:
    """A ViT-B/16 CLIP on the device (fp32 module: the entry points return fp32) and its weights as the oracle sees them, in fp64 on
    the device (co.reference_weight_rounding: the fp16 roundings the HIP path holds)."""

    def __init__(self, raw):
        from oracle import clip_oracle as co
        d = dev()
        self.m = build_model(synth.to_torch(raw)).float().to(d)
        self.sd = {k: v.to(d, torch.float64) for k, v in co.reference_weight_rounding(raw).items()}
        self.defaults = {k: self.m.get_option(k) for k in OPTS}

    def options(self, opts):
        for k, v in {**self.defaults, **opts}.items():
            self.m.set_option(k, v)


_towers = {}


def tower(weights):
    if weights not in _towers:
        raw = synth.clip_state_dict(synth.VIT_B16, 0)
        if weights == "offset":      # as test_vitb16_offset_residual_stream_vs_oracle: |mean| >> spread
            raw["visual.ln_pre.bias"] = (raw["visual.ln_pre.bias"] + 6.0).astype(np.float32)
        elif weights == "small":     # as test_small_scale_residual_stream_vs_oracle: rows spread by ~0.02
            for k in ("visual.ln_pre.weight", "visual.ln_pre.bias"):
                raw[k] = (raw[k] * 0.02).astype(np.float32)
            for i in range(12):
                for k in ("attn.out_proj", "mlp.c_proj"):
                    for s in ("weight", "bias"):
                        key = f"visual.transformer.resblocks.{i}.{k}.{s}"
                        raw[key] = (raw[key] * 0.02).astype(np.float32)
        elif weights == "stress":
            raw = synth.stress_clip_state_dict(synth.VIT_B16, 0)
        _towers[weights] = Tower(raw)
    return _towers[weights]


@pytest.fixture(scope="module", autouse=True)
def _release_towers():
    yield
    for t in _towers.values():
        t.options({})
    _towers.clear()


def rel_rows(got, ref):
    """Per-row error relative to the row's centred norm (fp64, on the device -> CPU)."""
    ref = ref.double()
    num = (got.double() - ref).norm(dim=-1)
    den = (ref - ref.mean(dim=-1, keepdim=True)).norm(dim=-1).clamp_min(1e-300)
    return (num / den).cpu()


class Input:
    """One call: crops (vision) or token ids (text), its sequence length L and the stream row of each sequence's selected token."""

    def __init__(self, vision, x, truncate=False):
        self.vision, self.x, self.truncate = vision, x, truncate
        d = dev()
        if vision:
            self.n, self.L = x.shape[0], 197
            self.sel = torch.arange(self.n, device=d) * self.L
        else:
            eot = x.argmax(dim=-1)
            self.n = x.shape[0]
            self.L = int(eot.max()) + 1 if truncate else x.shape[1]
            self.sel = torch.arange(self.n, device=d) * self.L + eot.clamp(max=self.L - 1)

    def where(self, r, dense):
        row = int(self.sel[r]) if dense else int(r)
        return (f"sequence {row // self.L}, token {row % self.L}, 256-row panel {row // 256} (mod 8: {row // 256 % 8}), "
                f"128-row half {row // 128}")


def run(t, inp, opts):
    """The hook under `opts`; its output must equal the entry point's bit for bit.  -> (trace, last entry dense)."""
    t.options(opts)
    if inp.vision:
        out, tr = t.m.visual.forward_stream_trace(inp.x)
        want = t.m.visual(inp.x)
    else:
        out, tr = t.m.encode_text_stream_trace(inp.x, inp.truncate)
        t.m.truncate_text = inp.truncate
        want = t.m.encode_text(inp.x)
        t.m.truncate_text = True
    assert want.dtype == torch.float32 and torch.equal(out, want), f"{opts}: the hook's output differs from the entry point's"
    assert tr.shape[:2] == (13, inp.n * inp.L)
    dense = {**t.defaults, **opts}["last_block_row0"] != 0
    if dense:
        tr[-1][inp.n:] = 0      # (rows the hook leaves unwritten: compared bit for bit between paths)
    return tr, dense


def step_errors(t, inp, tr, dense):
    """(a): per block, the rows of trace[i+1] against the oracle's block on trace[i] in fp64."""
    from oracle import clip_oracle as co
    pre = "visual.transformer.resblocks." if inp.vision else "transformer.resblocks."
    n, L, D = inp.n, inp.L, tr.shape[-1]
    errs = []
    for i in range(tr.shape[0] - 1):
        ref = co.resblock(tr[i].double().view(n, L, D), t.sd, f"{pre}{i}.", D // 64, not inp.vision).reshape(n * L, D)
        if dense and i == tr.shape[0] - 2:
            errs.append(rel_rows(tr[i + 1][:n], ref[inp.sel]))
        else:
            errs.append(rel_rows(tr[i + 1], ref))
        del ref
    return errs


def tower_fp64(t, inp):
    """The oracle's whole tower in fp64 from the same input: the stream after the last block, every row."""
    from oracle import clip_oracle as co
    col = []
    if inp.vision:
        co.vision_tokens(t.sd, inp.x.double(), torch.float64, collect=col)
    else:
        ids = inp.x[:, :inp.L].long()
        co.text_transformer(t.sd, t.sd["token_embedding.weight"][ids], collect=col)
    return col[-1].reshape(inp.n * inp.L, -1)


def pair_launches(t, inp, opts):
    t.options(opts)
    if inp.vision:
        _, recs = _lib.profile(t.m.visual._ctx.handle, HG_PROF_MLP_PAIR, 64, lambda: t.m.visual(inp.x))
    else:
        t.m.truncate_text = inp.truncate
        _, recs = _lib.profile(t.m._ctx.handle, HG_PROF_MLP_PAIR, 64, lambda: t.m.encode_text(inp.x))
        t.m.truncate_text = True
    return len(recs)


def first_difference(a, b):
    for e in range(a.shape[0]):
        rows = (a[e] != b[e]).any(dim=-1).nonzero()
        if rows.numel():
            return e, int(rows[0])
    return None


def check_case(name, t, inp, paths, pair_expected=False):
    fails = []
    base_tr, _ = run(t, inp, BASELINE)
    base = step_errors(t, inp, base_tr, False)
    final = tower_fp64(t, inp)
    base_drift = rel_rows(base_tr[-1], final)
    sel = inp.sel.cpu()
    print(f"\n== {name}: {inp.n} sequences x {inp.L} tokens = {inp.n * inp.L} rows")
    for i, e in enumerate(base):
        print(f"   {name} | baseline | block {i:2d} | median {float(e.median()):.2e} max {float(e.max()):.2e}")
        if float(e.max()) > CEIL:
            r = int(e.argmax())
            fails.append(f"{name} baseline block {i}: {float(e.max()):.3e} > {CEIL} at {inp.where(r, False)}")
    print(f"   {name} | baseline | drift    | median {float(base_drift.median()):.2e} max {float(base_drift.max()):.2e}")
    traces = {"baseline": (base_tr, False)}
    errors = {}
    for pname, opts, same_as in paths:
        tr, dense = run(t, inp, opts)
        if same_as is not None:
            want, _ = traces[same_as]
            if torch.equal(tr, want):
                print(f"   {name} | {pname} | == {same_as} bit for bit (every entry, every row)")
                continue
            e, r = first_difference(tr, want)
            fails.append(f"{name} {pname}: not bit-identical to {same_as}: first at entry {e}, {inp.where(r, dense and e == 12)}")
        traces[pname] = (tr, dense)
        errs = step_errors(t, inp, tr, dense)
        errors[pname] = errs
        for i, e in enumerate(errs):
            rows = sel if (dense and i == len(errs) - 1) else slice(None)
            bmax, bmed = float(base[i].max()), float(base[i][rows].median())
            emax, emed = float(e.max()), float(e.median())
            print(f"   {name} | {pname} | block {i:2d} | median {emed:.2e} max {emax:.2e} | baseline median {bmed:.2e} max {bmax:.2e}")
            if emax > FACTOR * bmax:
                r = int(e.argmax())
                fails.append(f"{name} {pname} block {i}: worst row {emax:.3e} > {FACTOR} x baseline max {bmax:.3e} at "
                             f"{inp.where(r, dense and i == len(errs) - 1)}")
            if emed > FACTOR * bmed:
                fails.append(f"{name} {pname} block {i}: median {emed:.3e} > {FACTOR} x baseline median {bmed:.3e}")
        got = tr[-1][:inp.n] if dense else tr[-1]
        drift = rel_rows(got, final[inp.sel] if dense else final)
        bd = float(base_drift[sel].median()) if dense else float(base_drift.median())
        print(f"   {name} | {pname} | drift    | median {float(drift.median()):.2e} max {float(drift.max()):.2e} | baseline median {bd:.2e}")
        if float(drift.median()) > FACTOR * bd:
            fails.append(f"{name} {pname} drift: median {float(drift.median()):.3e} > {FACTOR} x baseline median {bd:.3e}")
        del got
    if pair_expected:
        n = pair_launches(t, inp, {})
        if n != 11:
            fails.append(f"{name}: {n} MLP pair launches in the default path, expected 11 (one per block but the last)")
    t.options({})
    del traces
    torch.cuda.empty_cache()
    assert not fails, "\n".join(fails)


def hoi600(n=None):
    g0 = json.load(open(f"{G}/g0_tokens.json"))
    return clip.tokenize(g0["hoi600"]["text"][:n])


def crops(n, seed):
    return torch.from_numpy(synth.crops(n, 224, seed=seed)).to(dev())


@pytest.mark.parametrize("B,paths,pair", [
    (2, DEFAULT_ONLY, False),       # 394 rows: the separate-LayerNorm path
    (3, DEFAULT_ONLY, False),       # 591 rows: LayerNorm folded, hi / lo stream, no pair launch
    (11, VISION_PATHS, True),       # 2 167 rows: 9 panels (XCD 0 has two), the last one a single 128-row half
    (41, VISION_PATHS, True),       # 8 077 rows: 32 panels, a ragged second half
], ids=["B2", "B3", "B11", "B41"])
def test_vision_stream_every_row_every_block(B, paths, pair):
    check_case(f"vision B={B}", tower("default"), Input(True, crops(B, 300 + B)), paths, pair)


@pytest.mark.parametrize("weights", ["offset", "small", "stress"])
def test_vision_stream_other_weights(weights):
    """An offset stream (ln_pre.bias + 6), a stream whose rows spread by ~0.02 (the lo half below e5m2's normal range unless scaled) and
    the outlier weights of synth.stress_clip_state_dict: 11 crops, the pair launch and the hi / lo stream on."""
    check_case(f"vision B=11 {weights}", tower(weights), Input(True, crops(11, 78)), DEFAULT_ONLY, True)


@pytest.mark.parametrize("T,truncate,paths,pair", [
    (5, False, DEFAULT_ONLY, False),      # 385 rows: the separate path
    (27, False, TEXT_PATHS, True),        # 2 079 rows: the smallest with the pair launch on; an odd number of 128-row halves
    (64, False, TEXT_PATHS, True),        # 4 928 rows: an odd number of halves
    (600, True, TEXT_PATHS, True),        # 600 HICO prompts truncated to max(EOT) + 1 = 13 tokens: the generation pipeline's shape
], ids=["5x77", "27x77", "64x77", "600xLeff"])
def test_text_stream_every_row_every_block(T, truncate, paths, pair):
    ids = hoi600(T).to(dev())
    inp = Input(False, ids, truncate)
    if truncate:
        assert inp.L == 13, inp.L
    check_case(f"text {T}x{inp.L}", tower("default"), inp, paths, pair)


def test_stream_hooks_refuse_what_they_cannot_trace():
    """HG_ERR_INVALID (RuntimeError here) for more than one chunk of crops / one text pass and for a vision tower with adapters."""
    t = tower("default")
    with pytest.raises(RuntimeError, match="hg_test_image_stream"):
        t.m.visual.forward_stream_trace(torch.zeros(257, 3, 224, 224, device=dev()))
    with pytest.raises(RuntimeError, match="one pass"):
        t.m.encode_text_stream_trace(hoi600(900 - 600).repeat(3, 1).to(dev()), truncate=False)
    torch.cuda.empty_cache()
    sd = synth.to_torch(synth.clip_state_dict(synth.TINY, 10))
    sd.update(synth.to_torch(synth.adapter_state_dict(synth.TINY, 11)))
    mc = build_model(sd, use_adapter=True, adapter_pos="all").float().to(dev())
    with pytest.raises(RuntimeError, match="adapters"):
        mc.visual.forward_stream_trace(torch.from_numpy(synth.crops(2, synth.TINY["image_resolution"], seed=5)).to(dev()))
