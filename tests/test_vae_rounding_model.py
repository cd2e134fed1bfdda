"""The stage-wise per-element bound of tests/vae_bound.py and its two exact families, tested on the CPU: no GPU, no library.

`vae_bound.model` restates the arithmetic of hg_vae_fused.hip in its own order.  Three statements are proved here, at the hidden widths
(128, 128), (128, 384) - a one-block-pair stream that wraps inside the ring, eh != gh - and (2048, 4096):

* the correct restatement stays within the bound E on every input family: mean, log_var and bias at most 0.25 E (the bound sums the
  hidden layer's fp16 roundings in the worst case), z at most E (u |want| IS half an ulp just above a power of two, and the restatement's
  exp is correctly rounded; a kernel has the 1 ulp of expf left);
* `rounded` and `tiny` come out bit for bit as the float64 result with the hidden layer rounded once;
* every wrong kernel below is rejected - by the bound, or by a bit of an exact family - and the families named beside it reject it at
  every width (CATCHERS, BIT_CATCHERS), so that a family cannot lose its purpose unnoticed.

    #   mutant (vae_bound.MUTANTS)                                        rejected by
    1   f16_truncate     truncating fp16 conversion of h / g              rounded, bit for bit (the bound passes it: 0.98 E at most)
    2   f16_flush        flushed fp16 subnormals                          tiny, bit for bit and 2.2 - 9.8 E
    3   drop_block_*     last hidden block dropped from the mean,         randn, unit, outlier: 4.4 - 550 E; rounded by a bit where
                         log_var, bias (Encoder + Generator), bias        the sum is one of the exact ones
                         (Generator alone) sum
    4   drop_x_kstep     one 16-column k-step of x dropped                outlier 110 - 570 E, randn, unit 8.5 - 59 E, rounded, tiny
    5   bias_shift4      first-layer bias table shifted by four units     randn, unit, dead 59 - 1250 E, rounded
    6   no_kidx_perm     layer-2 weights without the vf_kidx permutation  randn, unit 63 - 800 E, rounded, tiny
    7   swap_mean_logvar mean and log_var output blocks swapped           randn, logvar 110 - 3200 E, rounded
    8   swap_z_halves    z column halves swapped as generator operand     randn, logvar 52 - 800 E
    9   exp_full_lv,     exp(lv) for exp(0.5 lv), exp2 for exp            randn, logvar > 1e6 E
        exp2
    10  no_relu          relu missing                                     dead 1470 - 6800 E, randn, rounded
    11  eps_neighbour    eps taken from the neighbouring row              randn, unit > 1e9 E
    12  block_twice      block nb - 1 accumulated twice                   randn, unit 10 - 550 E, rounded
    13  lv_bias_at_mean  log_var bias read at the mean bias's offset      randn, logvar 84 - 180 000 E, rounded

The comparison this replaces (relative L2 <= 1e-3 per row) passes 1, 2 and, on inputs without outlier columns, 4.
"""
import functools

import pytest
import torch

import vae_bound as vb

R = 40
WIDTHS = [(128, 128), (128, 384), (2048, 4096)]
# the families that must push a mutant beyond 2 E at every width
CATCHERS = {"f16_truncate": (), "f16_flush": ("tiny",),
            "drop_block_mean": ("randn", "unit", "outlier"), "drop_block_logvar": ("randn", "unit", "outlier"),
            "drop_block_bias": ("randn", "unit", "outlier"), "drop_block_gen": ("randn", "unit", "outlier"),
            "drop_x_kstep": ("outlier", "randn", "unit"), "bias_shift4": ("randn", "unit", "dead"), "no_kidx_perm": ("randn", "unit"),
            "swap_mean_logvar": ("randn", "logvar"), "swap_z_halves": ("randn", "logvar"), "exp_full_lv": ("randn", "logvar"),
            "exp2": ("randn", "logvar"), "no_relu": ("dead", "randn"), "eps_neighbour": ("randn", "unit"),
            "block_twice": ("randn", "unit"), "lv_bias_at_mean": ("randn", "logvar")}
# the exact families that must lose a bit of mean, log_var or the Generator-alone bias at every width
BIT_CATCHERS = {"f16_truncate": ("rounded", "tiny"), "f16_flush": ("tiny",), "drop_block_mean": ("rounded",),
                "drop_block_logvar": ("rounded",), "drop_block_gen": ("rounded",), "drop_x_kstep": ("rounded", "tiny"),
                "bias_shift4": ("rounded",), "no_kidx_perm": ("rounded", "tiny"), "swap_mean_logvar": ("rounded",),
                "no_relu": ("rounded",), "block_twice": ("rounded",), "lv_bias_at_mean": ("rounded",)}


@functools.lru_cache(maxsize=None)
def case(family, eh, gh):
    c = vb.make_case(family, eh, gh, R)
    return c, vb.enc_reference(c), (vb.exact_expected(c) if family in vb.EXACT_FAMILIES else None)


def judge(family, eh, gh, mutant=None):
    """(worst |err| / E over every tensor, bits differ from the exact expectation)"""
    c, enc, exact = case(family, eh, gh)
    out = vb.model(c, mutant)
    r = vb.ratios(c, out, enc_ref=enc)
    bits = exact is not None and any(not torch.equal(out[k], exact[k]) for k in exact)
    return r, bits


@pytest.mark.parametrize("eh,gh", WIDTHS)
def test_the_correct_restatement_stays_within_the_bound(eh, gh):
    for family in vb.FAMILIES:
        r, bits = judge(family, eh, gh)
        print(f"widths {eh} {gh} {family:8s} model " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
        assert not bits, f"{family}: the restatement is not the float64 result bit for bit"
        assert max(r[k] for k in ("mean", "log_var", "bias", "gen")) <= 0.25 and r["z"] <= 1.0, (family, r)


@pytest.mark.parametrize("eh,gh", WIDTHS)
@pytest.mark.parametrize("mutant", vb.MUTANTS)
def test_every_mutant_is_rejected(mutant, eh, gh):
    got = {family: judge(family, eh, gh, mutant) for family in vb.FAMILIES}
    print(f"{mutant} widths {eh} {gh}: " + "  ".join(f"{f} {max(r.values()):.2f}{' bits' if b else ''}" for f, (r, b) in got.items()))
    assert any(max(r.values()) > 1.0 or b for r, b in got.values()), got
    for family in CATCHERS[mutant]:
        assert max(got[family][0].values()) > 2.0, (family, got[family])
    for family in BIT_CATCHERS.get(mutant, ()):
        assert got[family][1], f"{family} does not lose a bit to {mutant}"


def test_every_mutant_is_alive_somewhere():
    """every mutant has a family that must reject it, and changes the restatement's bits there"""
    eh, gh = WIDTHS[1]
    for mutant in vb.MUTANTS:
        fams = CATCHERS[mutant] + BIT_CATCHERS.get(mutant, ())
        assert fams, mutant
        c, _, _ = case(fams[0], eh, gh)
        base, out = vb.model(c), vb.model(c, mutant)
        assert any(not torch.equal(base[k], out[k]) for k in base), mutant


def test_the_bound_does_not_see_what_the_exact_families_carry():
    """a truncating conversion stays inside E on every family: only the bit-for-bit expectation rejects it"""
    for family in vb.FAMILIES:
        r, _ = judge(family, *WIDTHS[1], "f16_truncate")
        assert max(r.values()) <= 1.0, (family, r)


def test_reference_quantities():
    """want and E of one element against a loop written out, and the exact families' hidden layer"""
    eh, gh = 128, 384
    c, enc, _ = case("randn", eh, gh)
    r, n = 7, 300
    x16 = c["x"][r].half().double()
    pre = [float((x16 * c["e_w0"][j].double()).sum() + c["e_b0"][j].double()) for j in range(eh)]
    S = [float((x16.abs() * c["e_w0"][j].double().abs()).sum() + c["e_b0"][j].double().abs()) for j in range(eh)]
    want, E = float(c["e_bm"][n]), 0.0
    acc_abs = 0.0
    for j in range(eh):
        h = max(pre[j], 0.0)
        e_pre = 513 * 2.0 ** -23 * S[j]
        t = h + e_pre
        e_h = e_pre + (2.0 ** -25 if t < 2.0 ** -14 else 2.0 ** -11 * t)
        w = float(c["e_wm"][n, j])
        want += h * w
        E += abs(w) * e_h
        acc_abs += (h + e_h) * abs(w)
    E += eh * 2.0 ** -23 * acc_abs + vb.U * abs(want)
    assert abs(float(enc["mean"][0][r, n]) - want) <= 1e-12 * abs(want)
    assert abs(float(enc["mean"][1][r, n]) - E) <= 1e-12 * E
    zw, zE = vb.z_reference(torch.tensor([[0.25]]), torch.tensor([[2.0]]), torch.tensor([[-3.0]]))
    e1 = 2.718281828459045
    assert abs(float(zw) - (0.25 - 3.0 * e1)) < 1e-14 and abs(float(zE) - (3.0 * e1 * 2.0 ** -23 + vb.U * abs(0.25 - 3.0 * e1))) < 1e-20
    for family in vb.EXACT_FAMILIES:
        c, _, _ = case(family, eh, gh)
        _, h, _, _ = vb.hidden(c["x"].double(), c["e_w0"].double(), c["e_b0"].double())
        h16 = vb.f16(h)
        if family == "rounded":
            assert float(((h16 != h) & (h > 0)).double().sum() / (h > 0).double().sum()) >= 0.1 and float(h.max()) < 65504
        else:
            assert float(((h16 > 0) & (h16 < 2.0 ** -14)).double().mean()) >= 0.25
