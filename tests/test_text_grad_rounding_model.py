"""The bounds and the gate of tests/text_grad_bound.py bite, shown without a GPU: the CPU restatements of the three backward kernels of
the text tower stay inside their per-element bounds on every input family, and a wrong kernel leaves them -

    no causal mask in the backward            attention bound (dQ, dK, dV)
    delta dropped from dS = P (dP - delta)    attention bound
    scale applied to dQ but not to dK         attention bound
    qgelu' without its second term            QuickGELU bound
    LayerNorm backward without mean(dyg xhat) LayerNorm bound
    an unscaled backward at |grad_out| ~ 1e-6 the tower gate (twice the scaled restatement's error against float64 autograd)

The whole-backward restatement rounds to fp16 at exactly these sites and nowhere else (tests/text_grad_bound.py, 2.): fp16(s grad_out);
per block the recomputed fp16(ln_1(x_in)), fp16(qkv), fp16(P) and fp16(att) of the forward attention, fp16(ln_2(x_mid)), fp16(u); then
fp16(g), df = fp16(. W_proj), du = fp16(df qgelu'(u)); fp16(g), da = fp16(. W_out), fp16(P) and fp16(dS) inside the attention backward,
fp16(dq | dk | dv).  The residual gradient, x_mid, both LayerNorm backwards, dh2, dh1 and the saved stream are fp32."""
import pytest
import torch

import text_grad_bound as tg
from hoigen_amd import synth

LENGTHS = (1, 2, 15, 16, 17, 33, 77, 80)


@pytest.mark.parametrize("family", tg.ATTN_FAMILIES)
def test_attention_backward_model_within_bound(family):
    top = 0.0
    for L in LENGTHS:
        qkv, dout = tg.make_attn(family, 2, L, 2, 1000 + L)
        ref = tg.attn_reference(qkv, dout, 2, L, 2)
        w = tg.worst(tg.attn_model(qkv, dout, 2, L, 2), ref)
        top = max(top, w)
        assert w <= 1.0, f"{family} L {L}: worst |err| / B {w:.3f}"
    print(f"TEXT_GRAD_RATIO attn model {family}: worst |err| / B {top:.3f}")


@pytest.mark.parametrize("mutant", tg.ATTN_MUTANTS)
def test_attention_backward_bound_rejects(mutant):
    for family in tg.ATTN_FAMILIES:
        for L in (16, 33, 77):
            qkv, dout = tg.make_attn(family, 1, L, 2, 2000 + L)
            ref = tg.attn_reference(qkv, dout, 1, L, 2)
            w = tg.worst(tg.attn_model(qkv, dout, 1, L, 2, mutant), ref)
            assert w > 1.0, f"{mutant} passes the bound on {family}, L {L}: {w:.3f}"


def test_attention_backward_single_token_is_exact():
    qkv, dout = tg.make_attn("randn", 3, 1, 2, 5)
    got = tg.attn_model(qkv, dout, 3, 1, 2)
    D = 128
    assert torch.equal(got[:, 2 * D:], dout.double()) and not got[:, :2 * D].any()


@pytest.mark.parametrize("D", (128, 512, 768))
@pytest.mark.parametrize("family", ("randn", "offset", "constant"))
def test_layernorm_backward_model_and_mutant(family, D):
    x, gamma, dy, g = tg.make_ln(family, 7, D, D + 3)
    ref = tg.ln_reference(x, gamma, dy, g)
    w = tg.worst(tg.ln_model(x, gamma, dy, g), ref)
    assert w <= 1.0, f"{family} D {D}: worst |err| / B {w:.3f}"
    assert torch.isfinite(ref["want"]).all()
    if family != "constant":      # (xhat = 0 on a constant row: the term the mutant drops is zero there)
        wm = tg.worst(tg.ln_model(x, gamma, dy, g, "no_xhat_term"), ref)
        assert wm > 1.0, f"no_xhat_term passes the bound on {family}, D {D}: {wm:.3f}"


def test_qgelu_backward_model_and_mutant():
    df, u = tg.make_qgelu(1 << 14, 9)
    ref = tg.qgelu_reference(df, u)
    assert tg.worst(tg.qgelu_model(df, u), ref) <= 1.0
    assert tg.worst(tg.qgelu_model(df, u, "first_term_only"), ref) > 1.0


def test_prompts_backward_model_is_the_plain_sum():
    g = torch.randn(130, 9, 8, generator=torch.Generator().manual_seed(3))
    gc, gb = tg.prompts_bwd_model(g, 4)
    assert torch.allclose(gc, g[:, 1:5].sum(0), atol=1e-4) and torch.allclose(gb, g[:, 1:5].sum(1), atol=1e-5)


@pytest.fixture(scope="module")
def tiny_case():
    return tg.tower_case(synth.TINY, 10, 5, 16, (5, 15, 9, 0, 12), 1.0)


def test_tower_restatement_close_to_float64_and_zero_beyond_eot(tiny_case):
    cfg, _, sd, prompts, tokenized, eot, go = tiny_case
    heads = cfg["transformer_heads"]
    ref = tg.tower_reference(sd, prompts, tokenized, go)
    got = tg.tower_backward_model(sd, prompts, eot, go, heads)
    errs = tg.rel_l2_per_prompt(got, ref, eot)
    print("TEXT_GRAD_TOWER tiny restatement rel L2 per prompt:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 5e-3      # (five fp16 roundings a block at 2^-11 each, two blocks: a few 1e-3 at the most)
    for r in range(5):
        assert not got[r, int(eot[r]) + 1:].any() and not ref[r, int(eot[r]) + 1:].any()


def test_tower_gate_rejects_unscaled_backward_at_1e_minus_6(tiny_case):
    cfg, _, sd, prompts, tokenized, eot, go = tiny_case
    heads = cfg["transformer_heads"]
    go6 = go * 1e-6
    ref = tg.tower_reference(sd, prompts, tokenized, go6)
    scaled = tg.rel_l2_per_prompt(tg.tower_backward_model(sd, prompts, eot, go6, heads), ref, eot)
    unscaled = tg.rel_l2_per_prompt(tg.tower_backward_model(sd, prompts, eot, go6, heads, "unscaled"), ref, eot)
    at1 = tg.rel_l2_per_prompt(tg.tower_backward_model(sd, prompts, eot, go, heads), tg.tower_reference(sd, prompts, tokenized, go), eot)
    print("TEXT_GRAD_TOWER tiny 1e-6 scaled", " ".join(f"{e:.2e}" for e in scaled), "| unscaled", " ".join(f"{e:.2e}" for e in unscaled))
    assert max(unscaled) > 2 * max(scaled), "the gate lets an unscaled backward through"
    assert max(scaled) <= 1.5 * max(at1) + 1e-6, "the power-of-two scale does not make the error independent of the magnitude"


def test_pow2_scale():
    go = torch.tensor([[0.0, 0.0], [3.0, -5.0], [1e-6, 2e-7], [1.0, 0.5], [float("inf"), 1.0]])
    s = tg.pow2_scale(go)
    assert s[:, 0].tolist()[:4] == [1.0, 0.25, 2.0 ** 20, 1.0]
    assert s[4, 0] == 2.0 ** -126
