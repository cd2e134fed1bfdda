"""Every kernel of hoigen_amd/csrc/hg_elem.hip on its own, through hg_test_elem (one launcher per call, the caller's device buffers in the
kernels' own types): the arithmetic kernels against the float64 reference and the per-element bound of tests/elem_bound.py, data movement
and conversions bit for bit against a numpy / torch indexing expression, and the refusals of the launchers (nothing written).  Prints
one line per kernel and family: ELEM_RATIO <kernel> <family> <worst |err| / B>."""
import ctypes as C

import numpy as np
import pytest
import torch

import elem_bound as eb
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = -1
(LN16, LN32, LNRS, RSC, FIN, FOLD, CROWS, HILO, CCOLS, IM2COL, EMBED, ADDPOS, GATHER, ARGMAX, CLAMP, POISON, TO16, TO32, REM, TRANS, L2, PROMPTS,
 LOSS, SPLIT) = range(24)
S16 = 203.25      # the fp16 number of the byte pattern 0x5A5A: sentinel of the fp16 buffers
S32 = 777.0


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # (a copy: the cached cases are read-only)


def host(t):
    return t.cpu().numpy()


def call(ctx, op, p=(), i=(), n=0):
    a = _lib.hg_test_elem_args()
    for k, t in enumerate(p):
        a.p[k] = None if t is None else (t if isinstance(t, int) else t.data_ptr())
    for k, v in enumerate(i):
        a.i[k] = int(v)
    a.n = int(n)
    rc = _lib.lib().hg_test_elem(ctx, op, C.byref(a), None)
    torch.cuda.synchronize()
    return rc


def ok(ctx, *a, **k):
    rc = call(ctx, *a, **k)
    assert rc == 0, _lib.lib().hg_last_error(ctx)


def refused(ctx, *a, **k):
    assert call(ctx, *a, **k) == INVALID
    assert b"invalid" in _lib.lib().hg_last_error(ctx).lower()


class Ratios:
    def __init__(self):
        self.w = {}

    def note(self, kernel, family, r):
        self.w[(kernel, family)] = max(self.w.get((kernel, family), 0.0), r)

    def check(self):
        for (kernel, family), r in sorted(self.w.items()):
            print(f"ELEM_RATIO {kernel} {family} {r:.3f}")
        bad = {k: v for k, v in self.w.items() if not v <= 1.0}
        assert not bad, bad


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = {2: np.uint16, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(u), b.view(u))


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------
def ln16(ctx, x, w, b, M, D, gather=None, rows_per_seq=0, in_row_mul=1):
    out = torch.full((M, D), S16, dtype=torch.float16, device="cuda")
    ok(ctx, LN16, (x, w, b, out, gather), (M, D, rows_per_seq, in_row_mul))
    return host(out)


def ln32(ctx, x, w, b, M, D, pos=None, cls=None, L=1):
    out = torch.full((M, D), S32, device="cuda")
    ok(ctx, LN32, (x, w, b, out, pos, cls), (M, D, L))
    return host(out)


def rowstats(ctx, x, M, D, gamma=None, with_muc=True):
    x16 = torch.full((M, D), S16, dtype=torch.float16, device="cuda")
    mr = torch.full((M, 2), S32, device="cuda")
    mu = torch.full((M,), S32, device="cuda")
    muc = torch.full((M,), S32, device="cuda")
    ok(ctx, RSC, (x, x16, mr, mu, muc if with_muc else None, gamma), (M, D))
    return {"x16": host(x16), "mr": host(mr), "mu": host(mu), "muc": host(muc)}


def ln_rowstats(ctx, x, w, b, M, D, ld16=0, pos=None, cls=None, L=1, with_muc=True):
    xio = x.clone()
    x16 = torch.full((M, ld16 or D), S16, dtype=torch.float16, device="cuda")
    mr = torch.full((M, 2), S32, device="cuda")
    mu = torch.full((M,), S32, device="cuda")
    muc = torch.full((M,), S32, device="cuda")
    ok(ctx, LNRS, (xio, w, b, x16, mr, mu, muc if with_muc else None, pos, cls), (M, D, L, ld16))
    return {"x": host(xio), "x16": host(x16), "mr": host(mr), "mu": host(mu), "muc": host(muc)}


@pytest.mark.parametrize("D", eb.DS)
def test_layernorm_within_the_bound(ctx, D):
    w, b = eb.make_affine(D)
    wd, bd = dev(w), dev(b)
    R = Ratios()
    for M in eb.MS:
        clean = None
        for family in eb.ROW_FAMILIES:
            x = eb.make_rows(family, M, D)
            xd = dev(x)
            y16, y32 = ln16(ctx, xd, wd, bd, M, D).astype(f32), ln32(ctx, xd, wd, bd, M, D)
            if family == "randn":
                clean = (y16, y32)
            if family == "nonfinite":
                bad = eb.nonfinite_rows(M)
                good = [r for r in range(M) if r not in bad]
                for y, y0 in zip((y16, y32), clean):
                    assert not np.isfinite(y[bad]).any() and same_bits(y[good], y0[good])
                continue
            for name, y, f16 in (("layernorm_f16", y16, True), ("layernorm_f32", y32, False)):
                want, B = eb.layernorm_reference(x, w, b, f16)
                if family == "constant":      # zero-variance rows: beta bit for bit, not a bound
                    eb.check_constant_layernorm(family, x, y, b.astype(np.float16).astype(f32) if f16 else b)
                    keep = np.arange(M) % 3 != 0
                    y, want, B = y[keep], want[keep], B[keep]
                R.note(name, family, eb.worst(y, want, B))
    R.check()


def test_layernorm_launchers_refuse_what_the_kernels_cannot_do(ctx):
    M = 3
    x = torch.randn(M, 1028, device="cuda")
    w, b = torch.ones(1028, device="cuda"), torch.zeros(1028, device="cuda")
    o16 = torch.full((M, 1100), S16, dtype=torch.float16, device="cuda")
    o32 = torch.full((M, 1100), S32, device="cuda")
    mr, mu = torch.full((M, 2), S32, device="cuda"), torch.full((M,), S32, device="cuda")
    x0 = x.clone()
    for D in (1028, 770):
        refused(ctx, LN16, (x, w, b, o16, None), (M, D, 0, 1))
        refused(ctx, LN32, (x, w, b, o32, None, None), (M, D, 1))
        refused(ctx, LNRS, (x, w, b, o16, mr, mu, None, None, None), (M, D, 1, 0))
        refused(ctx, RSC, (x, o16, mr, mu, None, None), (M, D))
    D = 256
    refused(ctx, LN32, (x, w, b, o32, w, None), (M, D, 1))                               # pos without cls
    refused(ctx, LNRS, (x, w, b, o16, mr, mu, None, w, None), (M, D, 1, 0))
    refused(ctx, LNRS, (x, w, b, o16, mr, mu, None, None, None), (M, D, 1, 252))         # ld16 < D
    refused(ctx, LNRS, (x, w, b, o16, mr, mu, None, None, None), (M, D, 1, 258))         # ld16 % 4
    assert bool((o16 == S16).all()) and bool((o32 == S32).all()) and bool((mr == S32).all()) and bool((mu == S32).all())
    assert torch.equal(x, x0)


def test_layernorm_f16_addressing(ctx):
    D = 260
    w, b = (dev(t) for t in eb.make_affine(D))
    # every L-th row
    M, L = 7, 5
    x = eb.make_rows("wide", M * L, D)
    dense = ln16(ctx, dev(x[::L]), w, b, M, D)
    assert same_bits(ln16(ctx, dev(x), w, b, M, D, in_row_mul=L), dense)
    # gather: row r of the output reads row r * rows_per_seq + clamp(gather[r])
    rps = 6
    idx = np.array([0, rps - 1, -3, rps + 2, 2], np.int32)
    M = len(idx)
    x = eb.make_rows("offset", M * rps, D)
    rows = np.arange(M) * rps + np.clip(idx, 0, rps - 1)
    assert same_bits(ln16(ctx, dev(x), w, b, M, D, gather=dev(idx), rows_per_seq=rps), ln16(ctx, dev(x[rows]), w, b, M, D))


@pytest.mark.parametrize("D", [260, 1024])
def test_pos_cls_rows(ctx, D):
    """ln_pre's addressing: row r is (r % L == 0 ? cls : x[r]) + pos[r % L] first - whatever x holds in the class rows"""
    L, M = 5, 15
    w, b = (dev(t) for t in eb.make_affine(D))
    x = eb.make_rows("randn", M, D).copy()
    pos, cls = eb.make_rows("small", L, D), eb.make_rows("wide", 1, D)[0]
    eff = x + pos[np.arange(M) % L]
    eff[::L] = cls[None] + pos[0][None]
    x[::L] = np.nan
    xd, pd, cd, ed = dev(x), dev(pos), dev(cls), dev(eff)
    want, B = eb.layernorm_reference(eff, *eb.make_affine(D), False)
    y = ln32(ctx, xd, w, b, M, D, pd, cd, L)
    assert same_bits(y, ln32(ctx, ed, w, b, M, D)) and eb.worst(y, want, B) <= 1.0
    a, e = ln_rowstats(ctx, xd, w, b, M, D, 0, pd, cd, L), ln_rowstats(ctx, ed, w, b, M, D)
    for k in a:
        assert same_bits(a[k], e[k]), k
    assert eb.worst(a["x"], want, B) <= 1.0


@pytest.mark.parametrize("D", eb.DS)
def test_layernorm_rowstats_is_layernorm_then_rowstats_cast(ctx, D):
    w, b = eb.make_affine(D)
    wd, bd = dev(w), dev(b)
    R = Ratios()
    for M in eb.MS:
        for family in ("randn", "offset", "constant"):
            x = eb.make_rows(family, M, D)
            xd = dev(x)
            y = ln32(ctx, xd, wd, bd, M, D)
            two = rowstats(ctx, dev(y), M, D)
            for ld16 in (0, D + 64):
                one = ln_rowstats(ctx, xd, wd, bd, M, D, ld16)
                assert same_bits(one["x"], y)
                assert same_bits(one["x16"][:, :D], two["x16"]) and bool((one["x16"][:, D:] == S16).all())
                for k in ("mr", "mu", "muc"):
                    assert same_bits(one[k], two[k]), k
            assert bool((ln_rowstats(ctx, xd, wd, bd, M, D, with_muc=False)["muc"] == S32).all())
            r = eb.family_stats_ratios("randn", y, one["mr"], one["mu"], one["x16"][:, :D].astype(f32))
            for k, v in r.items():
                R.note(f"layernorm_rowstats.{k}", family, v)
    R.check()


@pytest.mark.parametrize("D", eb.DS)
def test_rowstats_cast_within_the_bound(ctx, D):
    gamma = eb.make_affine(D)[0]
    gd = dev(gamma)
    R = Ratios()
    for M in eb.MS:
        clean = None
        for family in eb.ROW_FAMILIES:
            x = eb.make_rows(family, M, D)
            xd = dev(x)
            for g, gdev in ((None, None), (gamma, gd)):
                got = rowstats(ctx, xd, M, D, gdev)
                nomuc = rowstats(ctx, xd, M, D, gdev, with_muc=False)
                assert bool((nomuc["muc"] == S32).all()) and all(same_bits(nomuc[k], got[k]) for k in ("x16", "mr", "mu"))
                assert same_bits(got["muc"], got["mu"])
                if family == "randn" and g is None:
                    clean = got
                if family == "nonfinite":
                    if g is None:
                        bad = eb.nonfinite_rows(M)
                        good = [r for r in range(M) if r not in bad]
                        for k in ("x16", "mr", "mu"):
                            assert same_bits(got[k][good], clean[k][good]), k
                        assert not np.isfinite(got["mu"][bad]).any() and not np.isfinite(got["mr"][bad, 1]).any()
                        assert not np.isfinite(got["x16"][bad].astype(f32)).any()
                    continue
                assert not np.any(got["mr"][:, 0]), "mr[:, 0] == 0 exactly"
                r = eb.family_stats_ratios(family, x, got["mr"], got["mu"], got["x16"].astype(f32), g)
                for k, v in r.items():
                    R.note(f"rowstats_cast{'_gamma' if g is not None else ''}.{k}", family, v)
    R.check()


# ---- finalize_stats ------------------------------------------------------------------------------------------------------------------------
def finalize(ctx, stats, mu, M, nt, gw, centred, with_muc=True, flag=None):
    mr = torch.full((M, 2), S32, device="cuda")
    muio = dev(mu)
    muc = torch.full((M,), S32, device="cuda")
    ok(ctx, FIN, (dev(stats), mr, muio, muc if with_muc else None, flag), (M, nt, gw, int(centred)))
    return {"mr": host(mr), "mu": host(muio), "muc": host(muc)}


@pytest.mark.parametrize("nt,gw", [(2, 64), (4, 64), (8, 64), (12, 64), (16, 64), (12, 32)])
def test_finalize_stats_within_the_bound(ctx, nt, gw):
    R = Ratios()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for M in (1, 255, 256, 257):
        for centred in (False, True):
            clean = None
            for family in ("randn", "offset", "small", "wide", "nonfinite"):
                stats, mu = eb.make_stats(family, M, nt, gw, centred)
                got = finalize(ctx, stats, mu, M, nt, gw, centred, flag=flag)
                nomuc = finalize(ctx, stats, mu, M, nt, gw, centred, with_muc=False)
                assert bool((nomuc["muc"] == S32).all()) and same_bits(nomuc["mr"], got["mr"]) and same_bits(nomuc["mu"], got["mu"])
                assert same_bits(got["muc"], mu), "muc is the old mu"
                if centred:
                    assert same_bits(got["mu"], mu), "mu stays when the statistics are those of centred values"
                if family == "randn":
                    clean = got
                if family == "nonfinite":
                    bad = eb.nonfinite_rows(M)
                    good = [r for r in range(M) if r not in bad]
                    assert same_bits(got["mr"][good], clean["mr"][good]) and same_bits(got["mu"][good], clean["mu"][good])
                    assert not np.isfinite(got["mr"][bad]).any()
                    continue
                r = eb.finalize_ratios(stats, mu, gw, centred, got["mr"], got["mu"])
                for k, v in r.items():
                    R.note(f"finalize_stats{'_nt12' if nt == 12 else ''}.{k}", family, v)
    assert int(flag) == 0, "no row of these families leaves fp16's range, and a non-finite row never raises the flag (NaN compares false)"
    R.check()


@pytest.mark.parametrize("nt", [12, 8])
def test_finalize_stats_range_flag(ctx, nt):
    """rows of zero M2 whose one group mean lies 65 000 / 66 000 from the centre: only the second leaves fp16's 65 504"""
    M, gw = 5, 64

    def stats_at(dist):
        st = np.zeros((M, nt, 2), f32)
        st[3, nt - 3, 0] = gw * dist
        return st

    mu = np.zeros(M, f32)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    finalize(ctx, stats_at(65000.0), mu, M, nt, gw, False, flag=flag)
    assert int(flag) == 0
    finalize(ctx, stats_at(66000.0), mu, M, nt, gw, True, flag=flag)
    assert int(flag) == 0, "never written when centred"
    finalize(ctx, stats_at(-66000.0), mu, M, nt, gw, False, flag=flag)
    assert int(flag) == 1
    finalize(ctx, stats_at(1.0), mu, M, nt, gw, False, flag=flag)
    assert int(flag) == 1, "sticky: a later clean call does not clear it"


# ---- fold_ln --------------------------------------------------------------------------------------------------------------------------------
def fold(ctx, w16, gamma, beta, bias, N, K, with_csg=True):
    wf = torch.full((N, K), S16, dtype=torch.float16, device="cuda")
    cs, bf, csg = (torch.full((N,), S32, device="cuda") for _ in range(3))
    ok(ctx, FOLD, (dev(w16), dev(gamma), dev(beta), None if bias is None else dev(bias), wf, cs, bf, csg if with_csg else None), (N, K))
    return {"wf16": host(wf), "cs": host(cs), "bf": host(bf), "csg": host(csg) if with_csg else None, "csg_buf": host(csg)}


@pytest.mark.parametrize("N,K", [(1, 64), (5, 64), (128, 768), (7, 1000)])
def test_fold_ln(ctx, N, K):
    R = Ratios()
    for family in eb.FOLD_FAMILIES:
        w16, gamma, beta, bias = eb.make_fold(family, N, K)
        for bs in (bias, None):
            for with_csg in (True, False):
                got = fold(ctx, w16, gamma, beta, bs, N, K, with_csg)
                assert same_bits(got["wf16"], eb.fold_wf16_expected(w16, gamma)), "wf16 = fp16(fl(w gamma))"
                if not with_csg:
                    assert bool((got["csg_buf"] == S32).all())
                for k, v in eb.fold_ratios(w16, gamma, beta, bs, got).items():
                    R.note(f"fold_ln.{k}", family, v)
    R.check()


def test_fold_ln_empty_and_refused(ctx):
    w16, gamma, beta, bias = eb.make_fold("randn", 5, 64)
    wf = torch.full((5, 64), S16, dtype=torch.float16, device="cuda")
    cs, bf = torch.full((5,), S32, device="cuda"), torch.full((5,), S32, device="cuda")
    p = (dev(w16), dev(gamma), dev(beta), dev(bias), wf, cs, bf, None)
    ok(ctx, FOLD, p, (0, 64))           # nothing to fold: success without a launch
    refused(ctx, FOLD, p, (5, 0))
    assert bool((wf == S16).all()) and bool((cs == S32).all()) and bool((bf == S32).all())


# ---- copies -----------------------------------------------------------------------------------------------------------------------------------
LO_VALUES = np.array([0, 0.5, -0.5, 1, -1, 1.5, -1.75, 2, 3, -3.5, 4, -6, 7], np.float16)      # e5m2 numbers: the top byte of the fp16 is all of it


@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("row_stride,B", [(1, 200), (197, 3)])
def test_copy_rows_hilo(ctx, D, row_stride, B):
    """the stream as centre + hi + lo / 1024 with lo in gemm_ring2's tile-fragment order (elem_bound.lo_fragment_order: a scatter written
    from the comments, not from the kernel's index expression); every sum is exact in fp32"""
    rows = (B - 1) * row_stride + 1
    Rp = (rows + 127) // 128 * 128
    g = np.random.default_rng(D + row_stride)
    hi = (g.integers(-128, 129, (Rp, D)) / 8.0).astype(np.float16)
    lo = LO_VALUES[g.integers(0, len(LO_VALUES), (Rp, D))]
    assert not np.any(lo.view(np.uint16) & 0xFF)
    muc = (g.integers(-256, 257, Rp) / 4.0).astype(f32)
    want64 = muc.astype(np.float64)[:, None] + hi.astype(np.float64) + lo.astype(np.float64) / 1024
    assert np.array_equal(want64.astype(f32).astype(np.float64), want64)
    lo_buf = eb.lo_fragment_order((lo.view(np.uint16) >> 8).astype(np.uint8))
    out = torch.full((B, D), S32, device="cuda")
    ok(ctx, HILO, (dev(hi), dev(lo_buf), dev(muc), out), (B, row_stride, D))
    assert same_bits(host(out), want64[::row_stride][:B].astype(f32))


def test_copy_rows_and_cols(ctx):
    D, rs = 12, 7
    idx = np.array([0, rs - 1, -3, rs + 2, 3], np.int32)
    B = len(idx)
    x = eb.make_rows("randn", B * rs, D)
    out = torch.full((B, D), S32, device="cuda")
    ok(ctx, CROWS, (dev(x), out, dev(idx)), (B, rs, D))
    assert same_bits(host(out), x[np.arange(B) * rs + np.clip(idx, 0, rs - 1)])
    ok(ctx, CROWS, (dev(x), out, None), (B, rs, D))
    assert same_bits(host(out), x[::rs])
    R_, N, ld = 37, 9, 12
    x = eb.make_rows("wide", R_, ld)
    out = torch.full((R_, N), S32, device="cuda")
    ok(ctx, CCOLS, (dev(x), out), (ld, R_, N))
    assert same_bits(host(out), x[:, :N])


def test_copy_launchers_refuse(ctx):
    """D that is no multiple of the 256-column tile, and element counts past the kernels' int index (nothing is read or written)"""
    t = torch.full((64,), S32, device="cuda")
    h = torch.full((64,), S16, dtype=torch.float16, device="cuda")
    refused(ctx, HILO, (h, h, t, t), (1, 1, 320))
    refused(ctx, HILO, (h, h, t, t), (1 << 23, 1, 256))
    refused(ctx, CROWS, (t, t, None), (1 << 16, 1, 1 << 15))
    assert bool((t == S32).all())


@pytest.mark.parametrize("R_,p", [(32, 16), (64, 32), (28, 14), (21, 7)])
@pytest.mark.parametrize("B", [1, 3])
def test_im2col(ctx, R_, p, B):
    g = R_ // p
    K = 3 * p * p
    Kp = (K + 63) // 64 * 64
    img = torch.randn(B, 3, R_, R_, generator=torch.Generator().manual_seed(R_ + p + B))
    want = torch.nn.functional.unfold(img, kernel_size=p, stride=p).transpose(1, 2).reshape(B * g * g, K).half()
    ldo = K if p % 8 == 0 else Kp
    out = torch.full((B * g * g, ldo), float("nan"), dtype=torch.float16, device="cuda")
    ok(ctx, IM2COL, (img.cuda(), out), (B, R_, p))
    got = out.cpu()
    assert same_bits(got[:, :K].numpy(), want.numpy())
    assert bool((got[:, K:] == 0).all()), "pad columns 3 p^2 .. Kp - 1 are zeros"


def test_im2col_refuses_a_ragged_grid(ctx):
    out = torch.full((4, 768), S16, dtype=torch.float16, device="cuda")
    refused(ctx, IM2COL, (torch.zeros(1, 3, 30, 30, device="cuda"), out), (1, 30, 16))
    assert bool((out == S16).all())


# ---- text-side gathers ---------------------------------------------------------------------------------------------------------------------------
def test_embed_add_pos_gather_rows(ctx):
    T, L, ld, D, vocab = 3, 5, 7, 8, 11
    g = np.random.default_rng(3)
    table, pos = g.standard_normal((vocab, D)).astype(f32), g.standard_normal((L, D)).astype(f32)
    ids = g.integers(0, vocab, (T, ld)).astype(np.int32)
    ids[0, 1], ids[1, 4], ids[2, 0], ids[:, L:] = -1, vocab + 5, vocab - 1, 10 ** 6      # (the columns behind L are never read)
    x = torch.full((T * L, D), S32, device="cuda")
    ok(ctx, EMBED, (dev(ids), dev(table), dev(pos), x), (ld, T, L, D, vocab))
    want = table[np.clip(ids[:, :L], 0, vocab - 1)] + pos[None]
    assert same_bits(host(x), want.reshape(T * L, D))
    R_, Lfull = 3, 6
    prompts = g.standard_normal((R_ * Lfull, D)).astype(f32)
    x = torch.full((R_ * (L - 1), D), S32, device="cuda")
    ok(ctx, ADDPOS, (dev(prompts), dev(pos), x), (Lfull, R_, L - 1, D))
    assert same_bits(host(x), (prompts.reshape(R_, Lfull, D)[:, :L - 1] + pos[None, :L - 1]).reshape(-1, D))
    rid = np.array([3, -1, vocab + 5, 0, vocab - 1], np.int32)
    out = torch.full((len(rid), D), S32, device="cuda")
    ok(ctx, GATHER, (dev(rid), dev(table), out), (len(rid), D, vocab))
    assert same_bits(host(out), table[np.clip(rid, 0, vocab - 1)])
    # rows are moved in 16-byte chunks: a width that is no multiple of 4 is refused, not cut short
    x = torch.full((T * L, 6), S32, device="cuda")
    refused(ctx, EMBED, (dev(ids), dev(table), dev(pos), x), (ld, T, L, 6, vocab))
    refused(ctx, ADDPOS, (dev(prompts), dev(pos), x), (Lfull, R_, L - 1, 6))
    refused(ctx, GATHER, (dev(rid), dev(table), x), (len(rid), 6, vocab))
    assert bool((x == S32).all())


@pytest.mark.parametrize("n_ctx", [0, 5])
def test_assemble_prompts(ctx, n_ctx):
    R_, Cn, L, D = 3, 4, 6, 8
    ls = L - 1 - n_ctx
    g = np.random.default_rng(n_ctx)
    prefix, suffix = g.standard_normal((Cn, D)).astype(f32), g.standard_normal((Cn, max(ls, 1), D)).astype(f32)
    cx, bias = g.standard_normal((max(n_ctx, 1), D)).astype(f32), g.standard_normal((R_, D)).astype(f32)
    target = np.array([-1, Cn, 2], np.int32)
    t = np.clip(target, 0, Cn - 1)
    want = np.empty((R_, L, D), f32)
    want[:, 0] = prefix[t]
    want[:, 1:1 + n_ctx] = cx[None, :n_ctx] + bias[:, None]
    want[:, 1 + n_ctx:] = suffix[t][:, :ls]
    out = torch.full((R_ * L, D), S32, device="cuda")
    ok(ctx, PROMPTS, (dev(prefix), dev(suffix[:, :ls] if ls else suffix), dev(cx), dev(bias), dev(target), out), (R_, Cn, L, n_ctx, D))
    assert same_bits(host(out), want.reshape(R_ * L, D))
    refused(ctx, PROMPTS, (dev(prefix), dev(suffix), dev(cx), dev(bias), dev(target), out), (R_, Cn, L, L, D))


@pytest.mark.parametrize("L", [1, 63, 64, 65, 77, 130])
def test_eot_argmax(ctx, L):
    g = np.random.default_rng(L)
    ids = g.integers(0, 1000, (6, L)).astype(np.int32)
    ids[0, 0], ids[1, L - 1] = 5000, 5000                          # the maximum at either end
    ids[2, :] = 7                                                  # all equal: the first
    ids[3, L // 2], ids[3, L - 1] = 4000, 4000                     # a tie: the first occurrence
    ids[4, :] = -np.arange(L) - 5                                  # negative ids
    want = torch.from_numpy(ids.astype(np.int64)).argmax(1).numpy().astype(np.int32)
    assert want[2] == 0 and want[3] == L // 2
    eot = torch.full((6,), -7, dtype=torch.int32, device="cuda")
    mx = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok(ctx, ARGMAX, (dev(ids), eot, mx), (6, L))
    assert np.array_equal(host(eot), want) and int(mx) == int(want.max())
    eot.fill_(-7)
    ok(ctx, ARGMAX, (dev(ids), eot, None), (6, L))
    assert np.array_equal(host(eot), want)


@pytest.mark.parametrize("n", [1, 256, 257])
def test_clamp_eot(ctx, n):
    Leff = 10
    g = np.random.default_rng(n)
    over = g.integers(-3, 13, n).astype(np.int32)
    over[0] = Leff
    under = np.minimum(over, Leff - 1)
    under[-1] = Leff - 1
    for v, hit in ((over, 1), (under, 0)):
        for use in ((True, True), (True, False), (False, True), (False, False)):
            buf = dev(v)
            f1, f2 = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
            ok(ctx, CLAMP, (buf, buf, f1 if use[0] else None, f2 if use[1] else None), (n, Leff))      # in place
            assert np.array_equal(host(buf), np.clip(v, 0, Leff - 1))
            assert int(f1) == (hit if use[0] else 0) and int(f2) == (hit if use[1] else 0)


@pytest.mark.parametrize("n", [1, 255, 1024 * 256 + 77])
def test_poison_if_flag(ctx, n):
    for flag in (0, 1):
        out = torch.full((n + 3,), S32, device="cuda")
        ok(ctx, POISON, (out, torch.full((1,), flag, dtype=torch.int32, device="cuda")), n=n)
        assert bool(torch.isnan(out[:n]).all() if flag else (out[:n] == S32).all()) and bool((out[n:] == S32).all())


# ---- conversions ---------------------------------------------------------------------------------------------------------------------------------
SPECIAL = f32([0.0, -0.0, 1e-7, -3e-8, 6.1e-5, 65504.0, 65519.9, 65520.0, 1e5, -1e5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 1.5 * 2.0 ** -25])


def conv_input(n, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal(n) * 10.0 ** g.integers(-8, 5, n)).astype(f32)
    k = min(n, len(SPECIAL))
    x[:k] = SPECIAL[:k] if n >= len(SPECIAL) else SPECIAL[g.permutation(len(SPECIAL))[:k]]
    return x


@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055])
@pytest.mark.parametrize("offset", [0, 1])
def test_dtype_conversions(ctx, n, offset):
    """offset 1: the pointers are one element past a 16-byte boundary, so the scalar path runs; 0: the vector path and its scalar tail"""
    x = conv_input(n, n + offset)
    src = torch.zeros(n + 9, device="cuda")
    src[offset:offset + n] = dev(x)
    o16 = torch.full((n + 9,), S16, dtype=torch.float16, device="cuda")
    ok(ctx, TO16, (src[offset:], o16[offset:]), n=n)
    want16 = torch.from_numpy(x).half().numpy()
    got = host(o16)
    assert same_bits(got[offset:offset + n], want16) and bool((np.delete(got, np.s_[offset:offset + n]) == S16).all())
    o32 = torch.full((n + 9,), S32, device="cuda")
    ok(ctx, TO32, (o16[offset:], o32[offset:]), n=n)
    got = host(o32)
    assert same_bits(got[offset:offset + n], want16.astype(f32)) and bool((np.delete(got, np.s_[offset:offset + n]) == S32).all())
    ok(ctx, REM, (src[offset:], o16[offset:]), n=n)
    assert same_bits(host(o16)[offset:offset + n], eb.remainder_expected(x))


@pytest.mark.parametrize("rows,cols", [(1, 5), (64, 3), (513, 130)])
def test_transpose_to_f16(ctx, rows, cols):
    x = conv_input(rows * cols, rows).reshape(rows, cols)
    want = torch.from_numpy(x).half().numpy()
    for in_dtype, src in ((0, dev(x)), (1, dev(want))):
        out = torch.full((cols, rows), S16, dtype=torch.float16, device="cuda")
        ok(ctx, TRANS, (src, out), (in_dtype, rows, cols))
        assert same_bits(host(out), np.ascontiguousarray(want.T))


@pytest.mark.parametrize("L", [2, 33, 34, 50])
@pytest.mark.parametrize("E", [32, 96])
def test_split_global_local(ctx, L, E):
    B, G = 2, L - 1
    tok = eb.make_rows("randn", B * L, E)
    want = tok.reshape(B, L, E)
    for with_glob in (True, False):
        glob = torch.full((B, E), S32, device="cuda")
        local = torch.full((B, E, G), S32, device="cuda")
        ok(ctx, SPLIT, (dev(tok), glob if with_glob else None, local), (B, L, E))
        assert same_bits(host(local), np.ascontiguousarray(want[:, 1:].transpose(0, 2, 1)))
        assert same_bits(host(glob), want[:, 0]) if with_glob else bool((glob == S32).all())


def test_split_global_local_refuses(ctx):
    tok = torch.zeros(2 * 5, 48, device="cuda")
    out = torch.full((2, 48, 4), S32, device="cuda")
    refused(ctx, SPLIT, (tok, None, out), (2, 5, 48))
    refused(ctx, SPLIT, (tok, out, None), (2, 5, 32))
    assert bool((out == S32).all())


# ---- reductions ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 63, 64, 65, 512])
def test_l2_normalize(ctx, D):
    x = eb.make_rows("wide", 9, D).copy()
    x[1], x[2] = 1e-20, 1e18          # (512 x 1e36 overflows fp32: that row is expected as zeros, elem_bound.l2_reference)
    x[3, ::2] *= -1e-20
    x[6] = eb.make_rows("offset", 9, D)[6]
    want, B = eb.l2_reference(x)
    out = torch.full((9, D), S32, device="cuda")
    ok(ctx, L2, (dev(x), out), (9, D))
    R = Ratios()
    R.note("l2_normalize", "wide+1e-20+1e18", eb.worst(host(out), want, B))
    R.check()


@pytest.mark.parametrize("R_,D", [(1, 1), (5, 51), (70, 1000)])
def test_vae_loss(ctx, R_, D):
    g = np.random.default_rng(R_ * D)
    recon, x, mean, logvar = (g.standard_normal((R_, D)).astype(f32) for _ in range(4))
    want, B = eb.vae_loss_reference(recon, x, mean, logvar)
    loss = torch.full((1,), S32, device="cuda")
    ok(ctx, LOSS, (dev(recon), dev(x), dev(mean), dev(logvar), loss), (R_, D))
    R = Ratios()
    R.note("vae_loss", "randn", eb.worst(host(loss), want, B))
    R.check()
    loss.fill_(S32)
    ok(ctx, LOSS, (dev(recon), dev(x), dev(mean), dev(logvar), loss), (0, D))
    assert float(loss) == 0.0, "no rows: the loss is zeroed and nothing launched"
