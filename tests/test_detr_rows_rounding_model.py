"""The bound of tests/detr_rows_bound.py proved on the CPU: the restatement of the DETR row kernels stays inside it on every family and
width, the bound is finite everywhere (ln_bound's q < sigma / 2), the post-norm's loops and the tail's register pieces are the same
arithmetic, the bit-exact statements hold for the restatement itself, and each wrong kernel is outside the bound or off by bits in a
named family.  No GPU, no library."""
import numpy as np
import pytest

import detr_rows_bound as rb

MS = (1, 3, 4, 5, 33)
NORM_DS = (4, 128, 132, 256, 384, 512, 640)
TAIL_DS = (128, 256, 384, 512)
SEED = 5


@pytest.mark.parametrize("family", rb.NORM_FAMILIES)
@pytest.mark.parametrize("D", NORM_DS)
def test_the_postnorm_restatement_stays_inside_the_bound(family, D):
    worst = 0.0
    for M in MS:
        c = rb.make_postnorm(family, M, D, SEED)
        want, bound = rb.reference_postnorm(c), rb.bounds_postnorm(c)
        assert np.isfinite(bound).all(), "q < sigma / 2 must hold"
        res = rb.model_postnorm(c)
        fails, r = rb.judge_norm(res, M, want, bound, c["pos"])
        assert not fails, (M, fails)
        worst = max(worst, r)
        # the loops' trips and the register pieces accumulate in the same order
        assert rb.same_bits(rb.wave_ln_loops(c["x"], c["g"], c["b"]), rb._wave_ln(c["x"], c["g"], c["b"])), (M, "wave_ln_loops != _wave_ln")
        if family == "constant":
            assert rb.same_bits(res["x"][:M], np.broadcast_to(c["b"], (M, D)).copy()), "a constant row gives the norm's bias bit for bit"
        for kw in (dict(with_pos=False), dict(with_copy=False)):
            alt = rb.model_postnorm(c, **kw)
            assert rb.same_bits(alt["x"], res["x"]) and rb.same_bits(alt["x16"], res["x16"])
    print(f"postnorm {family} D {D}: worst |err| / bound {worst:.3f}")


@pytest.mark.parametrize("family", rb.NORM_FAMILIES)
@pytest.mark.parametrize("D", TAIL_DS)
def test_the_tail_restatement_stays_inside_the_bound(family, D):
    worst = [0.0, 0.0]
    for M in MS:
        for n_sl in (0, 1, 16):
            for with_b2 in (True, False):
                c = rb.make_tail(family, M, D, n_sl, SEED, with_b2)
                s, y, o = rb.reference_tail(c)
                Es, Ey, Eo = rb.bounds_tail(c)
                assert np.isfinite(Ey).all() and np.isfinite(Eo).all(), "q < sigma / 2 must hold"
                res = rb.model_tail(c)
                fails, r = rb.judge_norm({k: v for k, v in res.items() if k != "out"}, M, y, Ey, c["qpos"])
                assert not fails, (M, n_sl, with_b2, fails)
                ro = rb.worst_ratio(res["out"][:M], o, Eo)
                assert ro <= 1.0 and np.isnan(res["out"][M:]).all(), (M, n_sl, with_b2, ro)
                worst = [max(worst[0], r), max(worst[1], ro)]
                if family in rb.BITWISE_FAMILIES:      # the slice sum is exact: the restatement's pre-norm sum is the float64 one
                    v = c["x"].astype(np.float64) + (c["b2"] if with_b2 else 0.0) + c["part"].astype(np.float64).sum(0)
                    assert np.array_equal(v, s) and np.array_equal(v.astype(np.float32).astype(np.float64), v)
                    assert rb.same_bits(res["x"][:M], rb._wave_ln(v.astype(np.float32), c["g3"], c["be3"]))
                if family == "constant":
                    assert rb.same_bits(res["x"][:M], np.broadcast_to(c["be3"], (M, D)).copy())
                assert not rb.same_bits(res["x"][:M], res["out"][:M]), "the stream is not the final norm's output"
                assert rb.same_bits(rb.model_tail(c, with_out=False)["x"], res["x"])
    print(f"tail {family} D {D}: worst |err| / bound: stream {worst[0]:.3f}, out {worst[1]:.3f}")


def entry_layouts(B, T, D):
    """name -> (element strides (batch, token), flat size): sequence-first, batch-first, and rows 8 elements apart"""
    return {"seq_first": ((D, B * D), B * T * D), "batch_first": ((T * D, D), B * T * D), "gap": ((T * (D + 8), D + 8), B * T * (D + 8))}


def flat_of(logical, strides, size, fill=np.nan):
    B, T, D = logical.shape
    flat = np.full(size, fill, np.float32)
    b, t = np.divmod(np.arange(B * T), T)
    flat[(b * strides[0] + t * strides[1])[:, None] + np.arange(D)[None, :]] = logical.reshape(B * T, D)
    return flat


@pytest.mark.parametrize("family", ("randn", "f16edge"))
def test_the_bit_exact_statements_hold_for_the_entry_and_exit_restatements(family):
    for B, T, D in ((1, 1, 4), (3, 5, 260), (1, 33, 128), (3, 1, 516), (3, 33, 512)):
        src, pos = rb.make_entry(family, B, T, D, SEED)
        M = B * T
        for name, (st, size) in entry_layouts(B, T, D).items():
            res = rb.model_entry(flat_of(src, st, size), flat_of(pos, st, size), *st, *st, B, T, D)
            assert not rb.pads_intact(res, M, False)
            x, p = src.reshape(M, D), pos.reshape(M, D)
            with np.errstate(over="ignore", invalid="ignore"):
                want16, wantp16 = x.astype(np.float16).astype(np.float32), (x + p).astype(np.float16).astype(np.float32)
            assert rb.same_bits(res["x"][:M], x) and rb.same_bits(res["posb"][:M], p), name
            assert rb.same_bits(res["x16"][:M], want16) and rb.same_bits(res["xp16"][:M], wantp16), name
            # null pos / null tgt: +0 is read
            nop = rb.model_entry(flat_of(src, st, size), None, *st, 0, 0, B, T, D)
            assert rb.same_bits(nop["posb"][:M], np.zeros((M, D), np.float32)) and rb.same_bits(nop["xp16"][:M], rb._sum16(x, np.zeros_like(x), None))
            notgt = rb.model_entry(None, flat_of(pos, st, size), 0, 0, *st, B, T, D)
            assert rb.same_bits(notgt["x"][:M], np.zeros((M, D), np.float32)) and rb.same_bits(notgt["x16"][:M], np.zeros((M, D), np.float32))
            assert rb.same_bits(notgt["xp16"][:M], rb._sum16(np.zeros_like(p), p, None))      # (+0 + -0 is +0: not fp16(p))
            # exit: out = x at the caller's strides, the gaps untouched
            out = rb.model_exit(x, *st, B, T, D, size)
            assert rb.same_bits(out, flat_of(src, st, size))
    if family == "f16edge":      # the family does what its name says
        x, p = rb.make_f16edge(len(rb.F16_EDGE_PAIRS), 4)
        one = rb._sum16(x, p, None)
        assert (rb.bits(one) != rb.bits(rb._sum16(x, p, "xp16_two_roundings"))).any()
        assert (rb.bits(rb._cvt(x, None)) != rb.bits(rb._cvt(x, "truncate_f16"))).any()
        h = rb._cvt(x, None)
        assert np.isinf(h).any() and (np.signbit(h) & (h == 0)).any() and ((np.abs(h) < 2.0 ** -14) & (h != 0)).any()
        assert (np.signbit(x) & (x == 0) & ~np.signbit(rb._sum16(x, np.zeros_like(x), None))).any(), "-0 + (+0) is +0"


def _norm_verdict(kind, c, mutant, **kw):
    """does the judge see the mutant?  -> list of failures"""
    M = c["M"]
    if kind == "postnorm":
        want, bound = rb.reference_postnorm(c), rb.bounds_postnorm(c)
        exact = rb.model_postnorm(c)["x"] if c["family"] in rb.BITWISE_FAMILIES else None
        return rb.judge_norm(rb.model_postnorm(c, mutant), M, want, bound, c["pos"], exact)[0]
    _, y, o = rb.reference_tail(c)
    _, Ey, Eo = rb.bounds_tail(c)
    good = rb.model_tail(c)
    exact = good["x"] if c["family"] in rb.BITWISE_FAMILIES else None
    res = rb.model_tail(c, mutant)
    fails = rb.judge_norm({k: v for k, v in res.items() if k != "out"}, M, y, Ey, c["qpos"], exact)[0]
    if not rb.worst_ratio(res["out"][:M], o, Eo) <= 1.0:
        fails.append("out: outside the bound")
    if rb.same_bits(res["x"][:M], res["out"][:M]):
        fails.append("the stream is the final norm's output")
    return fails


# mutant -> (kernel, family, shape) in which it is shown to be caught; the shapes are among those the GPU test runs
CATCHES = {
    "one_pass_variance": ("postnorm", "offset", dict(M=5, D=256)),
    "eps_missing": ("postnorm", "tiny", dict(M=5, D=256)),
    "eps_1e-6": ("postnorm", "tiny", dict(M=5, D=256)),
    "variance_over_d_minus_1": ("postnorm", "randn", dict(M=5, D=640)),
    "gain_bias_swapped": ("postnorm", "randn", dict(M=5, D=128)),
    "xp16_two_roundings": ("postnorm", "randn", dict(M=33, D=256)),
    "truncate_f16": ("postnorm", "randn", dict(M=5, D=128)),
    "columns_from_256_unwritten": ("postnorm", "randn", dict(M=5, D=384)),
    "rows_beyond_m_written": ("postnorm", "randn", dict(M=5, D=128)),
    "b2_per_slice": ("tail", "randn", dict(M=5, D=256, n_sl=16)),
    "final_norm_written_back": ("tail", "randn", dict(M=5, D=256, n_sl=1)),
}


@pytest.mark.parametrize("mutant", sorted(CATCHES))
def test_a_wrong_norm_kernel_is_caught(mutant):
    kind, family, shape = CATCHES[mutant]
    c = rb.make_postnorm(family, seed=SEED, **shape) if kind == "postnorm" else rb.make_tail(family, seed=SEED, **shape)
    assert not _norm_verdict(kind, c, None), "the right kernel passes"
    fails = _norm_verdict(kind, c, mutant)
    print(f"{mutant}: caught by {kind} `{family}` {shape}: {fails[0] if fails else 'NOT CAUGHT'}")
    assert fails
    if mutant in rb.NORM_MUTANTS and kind == "postnorm" and shape["D"] <= 512:      # the tail shares the arithmetic: it is caught there too
        t = rb.make_tail(family, shape["M"], shape["D"], 1, SEED)
        assert _norm_verdict("tail", t, mutant), "the tail's judge misses it"


def test_a_constant_row_without_eps_is_nan():
    c = rb.make_postnorm("constant", 5, 128, SEED)
    assert np.isnan(rb.model_postnorm(c, "eps_missing")["x"][:5]).all()
    assert _norm_verdict("postnorm", c, "eps_missing")


ENTRY_CATCHES = {
    "xp16_two_roundings": ("f16edge", (1, 5, 128), "seq_first"),
    "truncate_f16": ("f16edge", (1, 5, 128), "seq_first"),
    "pos_strides_swapped": ("randn", (3, 5, 128), "seq_first"),
    "columns_from_256_unwritten": ("randn", (3, 5, 260), "gap"),
}


@pytest.mark.parametrize("mutant", sorted(ENTRY_CATCHES))
def test_a_wrong_entry_kernel_is_off_by_bits(mutant):
    family, (B, T, D), layout = ENTRY_CATCHES[mutant]
    src, pos = rb.make_entry(family, B, T, D, SEED)
    st, size = entry_layouts(B, T, D)[layout]
    args = (flat_of(src, st, size), flat_of(pos, st, size), *st, *st, B, T, D)
    good, bad = rb.model_entry(*args), rb.model_entry(*args, mutant=mutant)
    off = [k for k in good if not rb.same_bits(good[k], bad[k])]
    print(f"{mutant}: caught by entry `{family}` B {B} S {T} D {D} {layout}: bits of {off} differ")
    assert off
    if mutant == "pos_strides_swapped":      # one token of one image cannot see it: the GPU test runs B = 3 with S = 5 and 33 as well
        one = rb.make_entry(family, 1, 1, D, SEED)
        a1 = (one[0].ravel(), one[1].ravel(), D, D, D, D, 1, 1, D)
        assert all(rb.same_bits(rb.model_entry(*a1)[k], rb.model_entry(*a1, mutant=mutant)[k]) for k in good)


def test_every_mutant_has_a_named_catch():
    assert set(rb.MUTANTS) == set(CATCHES) | set(ENTRY_CATCHES)
