"""The text tower's fused in_proj + causal attention kernel (hoigen_amd/csrc/hg_qkv_attn_text.hip, option qkv_attn_text) against the two
kernels it replaces - the LayerNorm-folded in_proj GEMM and the causal attention launch - bit for bit: at the kernel (hg_test_qkv_attn,
fused bit 2 = the causal mask), through encode_text / encode_text_embeds / every entry of the stream trace of the ViT-B text tower in
both folded text_ln_fold forms, and through the width-768 text tower of ViT-L/14@336 (the 3 m K-tile schedule).  A work item of the
kernel is a PACK of floor(160 / L) whole sequences: a sequence must not see its pack neighbours, non-finite ones included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hoigen_amd import _lib, clip, synth
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(REPO, "tests", "golden")
TOL = 1e-3                       # the parity tolerance of tests/test_gpu_parity.py and of g12_vitl14_336_text.npz's own contract
HG_PROF_QKV_ATTN = _lib.HG_PROF_QKV_ATTN
CASES = [(600, 77, 8), (601, 77, 8), (37, 77, 8), (64, 16, 8), (50, 13, 8), (9, 1, 8), (33, 80, 8), (198, 77, 12), (40, 11, 12)]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def operands(n_seq, L, heads, seed):
    """As tests/test_gpu_attention.py: the centred fp16 copy, the in_proj weight, bias', column sums, (mean - centre, rstd)."""
    D = heads * 64
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(n_seq * L, D, device="cuda", generator=g)
    w = torch.randn(3 * D, D, device="cuda", generator=g) * D ** -0.5
    bias = torch.randn(3 * D, device="cuda", generator=g) * 0.3
    cs = w.half().float().sum(1)
    mr = torch.stack([torch.randn(n_seq * L, device="cuda", generator=g) * 0.05,
                      torch.rand(n_seq * L, device="cuda", generator=g) + 0.5], 1).contiguous()
    return a, w, bias, cs, mr


def call(ctx, ops, n_seq, L, heads, fused):
    a, w, bias, cs, mr = ops
    out = torch.empty(n_seq * L, heads * 64, device="cuda")
    rc = _lib.lib().hg_test_qkv_attn(ctx, a.data_ptr(), w.data_ptr(), bias.data_ptr(), cs.data_ptr(), mr.data_ptr(), n_seq, L,
                                     heads, int(fused), out.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, out


def run(ctx, ops, n_seq, L, heads, fused):
    rc, out = call(ctx, ops, n_seq, L, heads, fused)
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    return out


def sdpa_fp64(ops, n_seq, L, heads):
    """fp64 causal SDPA of the fp16-rounded q, k, v the folded in_proj defines."""
    a, w, bias, cs, mr = (t.double() for t in (ops[0].half(), ops[1].half(), ops[2], ops[3], ops[4]))
    qkv = ((a @ w.t() - mr[:, :1] * cs[None]) * mr[:, 1:] + bias[None]).half().double()
    q, k, v = (qkv.view(n_seq, L, 3, heads, 64)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)
    return o.permute(0, 2, 1, 3).reshape(n_seq * L, heads * 64)


# ---- 1. kernel level ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seq,L,heads", CASES)
def test_fused_causal_kernel_equals_gemm_then_causal_attention(ctx, n_seq, L, heads):
    """fused = 5 (the one kernel) against fused = 4 (folded GEMM, then the causal attention launch of that L) with torch.equal: full
    and short last packs, 2 / 10 / 12 / 160 / 14 sequences per pack, the longest sequence, both K-tile schedules (8 heads: 3 m + 2,
    12 heads: 3 m); repeated launches agree; and against fp64 SDPA at test_gpu_attention.py's tolerance for the fused pair.
    (Without the kernel the fused = 5 call is HG_ERR_INVALID: no L <= 80 is eligible for the vision kernel.)"""
    ops = operands(n_seq, L, heads, 3000 * L + 10 * n_seq + heads)
    got = run(ctx, ops, n_seq, L, heads, 5)
    want = run(ctx, ops, n_seq, L, heads, 4)
    diff = (got - want).abs().max().item()
    print(f"\n({n_seq}, {L}, {heads}): fused vs separate max abs diff {diff:.3e}")
    assert torch.equal(got, want), f"max abs diff {diff:.3e}, first row {int((got != want).any(1).nonzero()[0])}"
    for _ in range(3):
        assert torch.equal(got, run(ctx, ops, n_seq, L, heads, 5))
    ref = sdpa_fp64(ops, n_seq, L, heads)
    err = (got.double() - ref).abs().max().item()
    print(f"({n_seq}, {L}, {heads}): vs fp64 SDPA max abs err {err:.3e} of {ref.abs().max().item():.3e}")
    assert err <= 3e-3 * ref.abs().max().item()


def test_hook_rejects_what_the_causal_kernel_cannot_run(ctx):
    for n_seq, L, heads, fused in ((4, 81, 8, 5), (4, 77, 4, 5), (4, 77, 10, 5), (4, 77, 8, 7), (4, 77, 8, 8)):
        rc, _ = call(ctx, operands(n_seq, L, heads, 1), n_seq, L, heads, fused)
        assert rc != 0, (n_seq, L, heads, fused)


# ---- 2. pack isolation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seq,L,heads", [(37, 77, 8), (600, 77, 8), (64, 16, 8), (41, 77, 12)])
@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_non_finite_sequence_does_not_reach_its_pack_neighbours(ctx, n_seq, L, heads, poison):
    """Every odd sequence non-finite (two sequences per pack at L = 77: every pack holds one): every even sequence comes out finite
    and with the bits of the all-finite run - its masked keys' K rows and the V rows behind its last row are a neighbour's."""
    D = heads * 64
    ops = operands(n_seq, L, heads, 11 * L + n_seq)
    clean = run(ctx, ops, n_seq, L, heads, 5).view(n_seq, L, D)
    a = ops[0].clone().view(n_seq, L, D)
    a[1::2] = poison
    if poison != poison:
        a[1::2, :, ::2] = float("inf")      # (both kinds in one row)
    out = run(ctx, (a.view(n_seq * L, D),) + ops[1:], n_seq, L, heads, 5).view(n_seq, L, D)
    assert not torch.isfinite(out[1::2]).all(dim=(1, 2)).any(), "a poisoned sequence came out finite"
    assert torch.isfinite(out[0::2]).all(), f"sequences {(~torch.isfinite(out[0::2]).all(dim=(1, 2))).nonzero().flatten().tolist()} (x 2) poisoned"
    assert torch.equal(out[0::2], clean[0::2])


# ---- 3. tower level ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g0():
    return json.load(open(f"{G}/g0_tokens.json"))


@pytest.fixture(scope="module")
def fullA():
    m = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).to(dev())
    yield m
    del m
    torch.cuda.empty_cache()


class options:
    def __init__(self, m, **kw):
        self.m, self.kw = m, kw

    def __enter__(self):
        self.prev = {k: self.m.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            self.m.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.m.set_option(k, v)


def rel_l2(a, b):
    a = a.detach().float().cpu().numpy().astype(np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape and np.isfinite(a).all()
    rows = np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)
    return np.linalg.norm(a - b) / np.linalg.norm(b), rows.max()


@pytest.mark.parametrize("fold", [1, 2])
def test_encode_text_is_bit_identical_with_the_option_on(fullA, g0, fold):
    """The 600 + 81 + 117 prompts, 77 tokens and truncated, qkv_attn_text 1 and 2 against 0, encode_text and encode_text_embeds; and
    once against the reference's outputs (g3) with the option on, at test_gpu_parity.py's tolerance."""
    g3 = dict(np.load(f"{G}/g3_vitb16_text.npz"))
    try:
        for name in ("hoi600", "obj81", "verb117"):
            ids = clip.tokenize(g0[name]["text"]).to(dev())
            emb = fullA.token_embedding(ids).float()
            for trunc in (True, False):
                fullA.truncate_text = trunc
                outs = {}
                for mode in (0, 1, 2):
                    with options(fullA, text_ln_fold=fold, qkv_attn_text=mode):
                        outs[mode] = (fullA.encode_text(ids).float(), fullA.encode_text_embeds(emb, ids))
                for mode in (1, 2):
                    assert torch.equal(outs[mode][0], outs[0][0]), f"encode_text {name} trunc={trunc} fold={fold} qkv_attn_text={mode}"
                    assert torch.equal(outs[mode][1], outs[0][1]), f"encode_text_embeds {name} trunc={trunc} fold={fold} qkv_attn_text={mode}"
                whole, worst = rel_l2(outs[2][0], g3[name])
                print(f"\nencode_text {name} trunc={trunc} text_ln_fold={fold} qkv_attn_text=2 vs reference: {whole:.3e}, worst row {worst:.3e}")
                assert whole <= TOL and worst <= TOL
    finally:
        fullA.truncate_text = True


@pytest.mark.parametrize("fold", [1, 2])
@pytest.mark.parametrize("row0", [0, 1])
def test_every_entry_of_the_stream_trace_is_bit_identical(fullA, g0, fold, row0):
    """Every row of the residual stream after every block (600 prompts x 77 tokens and truncated to 13), options 1 and 2 against 0."""
    ids = clip.tokenize(g0["hoi600"]["text"]).to(dev())
    for trunc in (False, True):
        want = None
        for mode in (0, 2, 1):
            with options(fullA, text_ln_fold=fold, last_block_row0=row0, qkv_attn_text=mode):
                out, tr = fullA.encode_text_stream_trace(ids, trunc)
            if row0:
                tr[-1][ids.shape[0]:] = 0      # (rows the hook leaves unwritten)
            if want is None:
                want = (out, tr)
                continue
            assert torch.equal(out, want[0]), (trunc, mode)
            for e in range(tr.shape[0]):
                assert torch.equal(tr[e], want[1][e]), f"trunc={trunc} qkv_attn_text={mode}: entry {e} differs"
            del tr
        del want
        torch.cuda.empty_cache()


def test_width_768_text_tower_is_bit_identical_and_meets_its_reference(g0):
    """ViT-L/14@336: text width 768, 12 heads = 12 K-tiles (the 3 m schedule), 198 prompts; the fixture's own 1e-3 contract."""
    want = np.load(f"{G}/g12_vitl14_336_text.npz")["verb117_obj81"]
    m = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_L14_336, 0))).to(dev())
    ids = clip.tokenize(g0["verb117"]["text"] + g0["obj81"]["text"]).to(dev())
    try:
        for fold in (1, 2):
            for trunc in (True, False):
                m.truncate_text = trunc
                outs = {}
                for mode in (0, 1, 2):
                    with options(m, text_ln_fold=fold, qkv_attn_text=mode):
                        outs[mode] = m.encode_text(ids).float()
                assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0]), (fold, trunc)
                whole, worst = rel_l2(outs[2], want)
                print(f"\nViT-L/14 text tower fold={fold} trunc={trunc} qkv_attn_text=2 vs reference: {whole:.3e}, worst row {worst:.3e}")
                assert whole <= TOL and worst <= TOL
        m.truncate_text = False
        with options(m, qkv_attn_text=2):
            _, recs = _lib.profile(m._ctx.handle, HG_PROF_QKV_ATTN, 64, lambda: m.encode_text(ids))
        assert len(recs) == m.transformer.layers - 1 and all(r[1:4] == (198, 77, 12) for r in recs), recs
    finally:
        del m
        torch.cuda.empty_cache()


# ---- 4. it really ran --------------------------------------------------------------------------------------------------------
def test_launch_counts_under_the_profiler(fullA, g0):
    ids = clip.tokenize(g0["hoi600"]["text"]).to(dev())
    layers = fullA.transformer.layers
    fullA.encode_text(ids)
    try:
        for trunc, L in ((False, 77), (True, int(ids.argmax(-1).max()) + 1)):
            fullA.truncate_text = trunc
            for mode, row0, n in ((2, 1, layers - 1), (2, 0, layers), (0, 1, 0), (0, 0, 0)):
                with options(fullA, qkv_attn_text=mode, last_block_row0=row0):
                    _, recs = _lib.profile(fullA._ctx.handle, HG_PROF_QKV_ATTN, 64, lambda: fullA.encode_text(ids))
                assert len(recs) == n, (trunc, mode, row0, recs)
                assert all(r[1:4] == (600, L, 8) for r in recs), recs
    finally:
        fullA.truncate_text = True


# ---- 5. options --------------------------------------------------------------------------------------------------------------
def test_option_round_trip_range_and_environment(fullA, g0):
    fullA.encode_text(clip.tokenize(g0["obj81"]["text"][:4]).to(dev()))      # (creates the native context)
    assert fullA.get_option("qkv_attn_text") == 0, "the default stays 0"
    for v in (1, 2, 0):
        fullA.set_option("qkv_attn_text", v)
        assert fullA.get_option("qkv_attn_text") == v and fullA.visual.get_option("qkv_attn_text") == v
    for bad in (3, -1):
        with pytest.raises(RuntimeError, match="qkv_attn_text"):
            fullA._ctx.set_option("qkv_attn_text", bad)
        assert fullA.get_option("qkv_attn_text") == 0
    code = ("import ctypes\nfrom hoigen_amd import _lib\nL = _lib.lib()\nh = L.hg_create(0)\nv = ctypes.c_int32(-9)\n"
            "assert L.hg_get_option(h, b'qkv_attn_text', ctypes.byref(v)) == 0\nprint('value', v.value)\nL.hg_destroy(h)\n")
    for env, want in (("2", 2), ("1", 1), (None, 0), ("7", 0)):
        e = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
        e.pop("HG_QKV_ATTN_TEXT", None)
        if env is not None:
            e["HG_QKV_ATTN_TEXT"] = env
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert f"value {want}" in r.stdout, (env, r.stdout)


def test_vision_kernel_is_unharmed_by_the_text_kernel_on_the_same_context():
    """Both kernels raise their own dynamic-LDS attribute and share the context's workspace: vision, text, vision on ONE context give the
    vision bits of a fresh context - at the kernels (hg_test_qkv_attn) and through a model whose two towers alternate."""
    L_ = _lib.lib()
    vis = operands(40, 197, 12, 21)
    txt = operands(198, 77, 12, 22)
    txt8 = operands(64, 77, 8, 23)
    fresh = L_.hg_create(0)
    want = run(fresh, vis, 40, 197, 12, 1)
    L_.hg_destroy(fresh)
    h = L_.hg_create(0)
    try:
        first = run(h, vis, 40, 197, 12, 1)
        t1 = run(h, txt, 198, 77, 12, 5)
        t2 = run(h, txt8, 64, 77, 8, 5)
        again = run(h, vis, 40, 197, 12, 1)
        assert torch.equal(first, want) and torch.equal(again, want)
        assert torch.equal(t1, run(h, txt, 198, 77, 12, 4)) and torch.equal(t2, run(h, txt8, 64, 77, 8, 4))
    finally:
        L_.hg_destroy(h)
    m = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).to(dev())
    img = torch.from_numpy(synth.crops(40, 224, seed=7)).to(dev())
    ids = clip.tokenize(json.load(open(f"{G}/g0_tokens.json"))["hoi600"]["text"]).to(dev())
    base = m.encode_image(img)
    m.set_option("qkv_attn_text", 2)
    a = m.encode_image(img)
    m.encode_text(ids)
    b = m.encode_image(img)
    assert torch.equal(a, base) and torch.equal(b, base)
