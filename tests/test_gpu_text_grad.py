"""The input gradient of the frozen text tower on the HIP path (vae.TextEncoder(differentiable=True) -> hg_encode_text_embeds_save /
hg_text_backward_embeds) against the float64 autograd gradient of oracle.clip_oracle.text_encoder_embeds on the same fp16-rounded weights.

Metric: relative L2 per prompt over the positions <= EOT.  Gate: at most twice the error of the CPU restatement
(tests/text_grad_bound.py: tower_backward_model, which rounds where the kernels round) against the same float64 gradient on the same
inputs - never the code under test.  Factor two because MFMA accumulation order and the softmax sums' order move individual roundings
against torch's, not their number.  Then what must hold bit for bit: zeros behind EOT and behind the executed length, the forward's
bits, repeated calls, a prompt alone and inside a batch, a NaN neighbour.  Last, one training step of main_coop_vae.py:442-471 end to end.
Each test prints the measured figures (lines starting TEXT_GRAD_TOWER) before it asserts."""
import ctypes as C

import pytest
import torch
from torch import nn

import text_grad_bound as tg
from hoigen_amd import _lib, synth, vae
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(sd_np):
    m = build_model(synth.to_torch(sd_np)).float().to(DEV)
    m.requires_grad_(False)          # CLIP is frozen in the training loop (main_coop_vae.py:316-318)
    return m


def hip_grad(m, prompts, tokenized, grad_out, truncate=True):
    """-> (text features, grad_prompts) on the CPU through the differentiable facade"""
    m.truncate_text = truncate
    te = vae.TextEncoder(m, differentiable=True)
    p = prompts.to(DEV).requires_grad_()
    with torch.enable_grad():
        out = te(p, tokenized.to(DEV))
        out.backward(grad_out.to(DEV))
    torch.cuda.synchronize()
    return out.detach().cpu(), p.grad.cpu()


CASES = {      # name: (config, R, L, EOT positions)
    "tiny_r1": (synth.TINY, 1, 16, (9,)),
    "tiny_r5": (synth.TINY, 5, 16, (5, 15, 9, 0, 12)),
    "w512x2_l77": (tg.small_config(512, 2), 3, 77, (0, 40, 76)),
    "w512x12_l16": (tg.small_config(512, 12), 6, 16, (5, 15, 9, 12, 7, 15)),
    "w768x2_l16": (tg.small_config(768, 2), 3, 16, (4, 15, 9)),
}
_models = {}


def case(name, magnitude):
    cfg, R, L, eot = CASES[name]
    c = tg.tower_case(cfg, 10, R, L, eot, magnitude)
    if name not in _models:
        _models.clear()          # one model on the device at a time
        _models[name] = build(c[1])
    return c, _models[name]


@pytest.mark.parametrize("magnitude", (1.0, 1e-6))
@pytest.mark.parametrize("name", list(CASES))
def test_tower_gradient_within_twice_the_restatement(name, magnitude):
    (cfg, _, sd, prompts, tokenized, eot, go), m = case(name, magnitude)
    ref = tg.tower_reference(sd, prompts, tokenized, go)
    model = tg.rel_l2_per_prompt(tg.tower_backward_model(sd, prompts, eot, go, cfg["transformer_heads"]), ref, eot)
    _, got = hip_grad(m, prompts, tokenized, go)
    hip = tg.rel_l2_per_prompt(got, ref, eot)
    msg = (f"TEXT_GRAD_TOWER {name} |grad_out| {magnitude:g}: HIP " + " ".join(f"{e:.2e}" for e in hip) + " | restatement " +
           " ".join(f"{e:.2e}" for e in model))
    print(msg)
    assert all(h <= 2.0 * r for h, r in zip(hip, model)), msg
    for r in range(len(eot)):      # zeros by construction: the causal mask lets nothing reach a row behind EOT
        assert not got[r, int(eot[r]) + 1:].view(torch.int32).any(), f"{name}: prompt {r} has a gradient behind its EOT"


def test_one_block_backward_through_the_hook():
    (cfg, _, sd, prompts, _, _, _), m = case("tiny_r5", 1.0)
    heads = cfg["transformer_heads"]
    gen = torch.Generator().manual_seed(5)
    x_in = (prompts + 0.3 * torch.randn(prompts.shape, generator=gen)).contiguous()
    g = torch.randn(prompts.shape, generator=gen)
    p = "transformer.resblocks.1."
    ref = tg.block_reference(sd, p, x_in, g, heads)
    sd32 = {k: v.float() for k, v in sd.items()}
    e_model = float((tg.block_backward_model(sd32, p, x_in, g, heads).double() - ref).norm() / ref.norm())
    h = m._sync_text(torch.device(DEV))
    a = _lib.hg_test_elem_args()
    xd, gd = x_in.to(DEV), g.to(DEV)
    a.p[0], a.p[1] = xd.data_ptr(), gd.data_ptr()
    a.i[0], a.i[1], a.i[2] = 1, prompts.shape[0], prompts.shape[1]
    rc = _lib.lib().hg_test_text_grad(h, 6, C.byref(a), None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().hg_last_error(h)
    e_hip = float((gd.cpu().double() - ref).norm() / ref.norm())
    print(f"TEXT_GRAD_TOWER one block (tiny, block 1): HIP {e_hip:.2e} | restatement {e_model:.2e}")
    assert e_hip <= 2.0 * e_model


def test_exactness():
    (cfg, _, sd, prompts, tokenized, eot, go), m = case("tiny_r5", 1.0)
    out, got = hip_grad(m, prompts, tokenized, go, truncate=False)
    # the differentiable forward is the inference forward, bit for bit
    with torch.no_grad():
        plain = vae.TextEncoder(m)(prompts.to(DEV), tokenized.to(DEV)).cpu()
    assert torch.equal(out, plain)
    # two backward calls agree; a prompt's gradient is the same alone and inside the batch of five
    out2, got2 = hip_grad(m, prompts, tokenized, go, truncate=False)
    assert torch.equal(out, out2) and torch.equal(got, got2)
    for r in (1, 3):
        _, alone = hip_grad(m, prompts[r:r + 1], tokenized[r:r + 1], go[r:r + 1], truncate=False)
        assert torch.equal(alone[0], got[r]), f"prompt {r} alone differs from prompt {r} in the batch"
    # a NaN row in grad_out: that prompt's gradient is non-finite, the others do not move, and the next call is clean
    bad = go.clone()
    bad[2, 7] = float("nan")
    _, gnan = hip_grad(m, prompts, tokenized, bad, truncate=False)
    assert not torch.isfinite(gnan[2, : int(eot[2]) + 1]).all()
    keep = [0, 1, 3, 4]
    assert torch.equal(gnan[keep], got[keep])
    assert torch.equal(hip_grad(m, prompts, tokenized, go, truncate=False)[1], got)


def test_truncated_call():
    """EOT positions 3, 9 and 6 of 16: the truncated call executes 10 tokens.  It is held to the same gate, positions >= 10 are zeros
    bit for bit, and the test records whether it equals the full-length call bit for bit (nothing promises that: the GEMMs see
    another row count and the attention another length)."""
    cfg, _, sd, prompts, tokenized, eot, go = tg.tower_case(synth.TINY, 10, 3, 16, (3, 9, 6), 1.0)
    _, m = case("tiny_r5", 1.0)
    ref = tg.tower_reference(sd, prompts, tokenized, go)
    model = tg.rel_l2_per_prompt(tg.tower_backward_model(sd, prompts, eot, go, cfg["transformer_heads"]), ref, eot)
    of, full = hip_grad(m, prompts, tokenized, go, truncate=False)
    ot, trunc = hip_grad(m, prompts, tokenized, go, truncate=True)
    hip = tg.rel_l2_per_prompt(trunc, ref, eot)
    print(f"TEXT_GRAD_TOWER truncated 10 of 16: HIP " + " ".join(f"{e:.2e}" for e in hip) + " | restatement " +
          " ".join(f"{e:.2e}" for e in model) + f" | bit-identical to the full-length call: gradient {torch.equal(full, trunc)}, "
          f"features {torch.equal(of, ot)}")
    assert all(h <= 2.0 * r for h, r in zip(hip, model))
    assert not trunc[:, 10:].view(torch.int32).any()


def test_refusals():
    (cfg, _, sd, prompts, tokenized, eot, go), m = case("tiny_r5", 1.0)
    te = vae.TextEncoder(m, differentiable=True)
    p = prompts.to(DEV).requires_grad_()
    with torch.enable_grad():
        out = te(p, tokenized.to(DEV))
        (g,) = torch.autograd.grad(out.pow(2).sum(), p, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):      # double backward is refused, not silently zero
            g.sum().backward()
    # more than one pass of the text tower is refused with the row budget in the message
    h = m._sync_text(torch.device(DEV))
    R, L, D = 4097, 16, cfg["transformer_width"]
    big = torch.zeros(R, L, D, device=DEV)
    eo = torch.zeros(R, dtype=torch.int32, device=DEV)
    o = torch.empty(R, cfg["embed_dim"], device=DEV)
    saved = torch.empty(8, device=DEV)
    rc = _lib.lib().hg_encode_text_embeds_save(h, big.data_ptr(), eo.data_ptr(), R, L, o.data_ptr(), 0, saved.data_ptr(), None)
    assert rc != 0 and b"row budget" in _lib.lib().hg_last_error(h)


def test_training_step_end_to_end():
    """main_coop_vae.py:442-471 at small widths: torch netE / netG, PromptLearner_hoi and TextEncoder on the HIP path (both
    differentiable), vae_loss in torch.  ctx.grad and netG's first-layer weight.grad against the same step through the oracle in
    float64; gate: twice the error of the same step with the CPU restatement in the text tower's place."""
    (cfg, _, sd, _, _, _, _), m = case("tiny_r5", 1.0)
    D, E, heads, R, C_, L, n_ctx = cfg["transformer_width"], cfg["embed_dim"], cfg["transformer_heads"], 6, 3, 16, 5
    gen = torch.Generator().manual_seed(21)
    ids = torch.randint(1, cfg["vocab_size"] - 2, (C_, L), generator=gen)
    eot_c = torch.tensor([9, 12, 15])
    ids[torch.arange(C_), eot_c] = cfg["vocab_size"] - 1
    emb = sd["token_embedding.weight"][ids].float()
    target = torch.tensor([0, 2, 1, 1, 0, 2])
    feats = torch.randn(R, E, generator=gen)
    feats = feats / feats.norm(dim=-1, keepdim=True)
    eps = torch.randn(R, D, generator=gen)
    ctx0 = 0.02 * torch.randn(n_ctx, D, generator=gen)
    lin = {k: 0.05 * torch.randn(*s, generator=gen) for k, s in (("e0", (256, E)), ("em", (D, 256)), ("el", (D, 256)), ("g0", (256, D)),
                                                                 ("g2", (D, 256)))}

    def step(dtype, dev, text_fn, ctx=None):
        w = {k: v.to(device=dev, dtype=dtype).requires_grad_() for k, v in lin.items()}
        ctx = ctx0.to(device=dev, dtype=dtype).requires_grad_() if ctx is None else ctx
        f, e = feats.to(device=dev, dtype=dtype), eps.to(device=dev, dtype=dtype)
        with torch.enable_grad():
            hid = torch.relu(f @ w["e0"].T)
            mean, log_var = hid @ w["em"].T, hid @ w["el"].T
            z = torch.exp(0.5 * log_var) * e + mean
            bias = torch.relu(z @ w["g0"].T) @ w["g2"].T
            tf = text_fn(bias, ctx)
            tf = tf / tf.norm(dim=-1, keepdim=True)
            rec = (tf - f).pow(2).sum(1).mean()
            kld = -0.5 * (1 + log_var - mean.pow(2) - log_var.exp()).sum(dim=1).mean()
            (rec + kld).backward()
        return ctx.grad.detach().cpu().double(), w["g0"].grad.detach().cpu().double()

    def assemble(bias, ctx):
        e = emb.to(device=bias.device, dtype=bias.dtype)[target]
        return torch.cat([e[:, :1], ctx[None] + bias[:, None], e[:, 1 + n_ctx:]], 1)

    from oracle import clip_oracle as co
    ref = step(torch.float64, "cpu", lambda bias, ctx: co.text_encoder_embeds(sd, assemble(bias, ctx), ids[target], dtype=torch.float64))

    class Restated(torch.autograd.Function):
        @staticmethod
        def forward(c, prompts):
            c.save_for_backward(prompts)
            return tg.tower_forward_model(sd, prompts, eot_c[target], heads)[0]

        @staticmethod
        def backward(c, go):
            return tg.tower_backward_model(sd, c.saved_tensors[0], eot_c[target], go, heads)

    model = step(torch.float32, "cpu", lambda bias, ctx: Restated.apply(assemble(bias, ctx)))

    pl = vae.PromptLearner_hoi(["ride horse", "hold cup", "feed cat"], m, differentiable=True).float().to(DEV)
    pl.register_buffer("token_prefix", emb[:, :1].contiguous().to(DEV))
    pl.register_buffer("token_suffix", emb[:, 1 + n_ctx:].contiguous().to(DEV))
    pl.tokenized_prompts, pl._f32_key = ids.to(DEV), None
    te = vae.TextEncoder(m, differentiable=True)

    pl.ctx = nn.Parameter(ctx0.to(DEV))
    got = step(torch.float32, DEV, lambda bias, ctx: te(pl(bias, target.to(DEV)), pl.tokenized_prompts[target.to(DEV)]), pl.ctx)
    for what, a, b, r in (("ctx.grad", got[0], model[0], ref[0]), ("netG.net.0.weight.grad", got[1], model[1], ref[1])):
        e_hip, e_model = float((a - r).norm() / r.norm()), float((b - r).norm() / r.norm())
        print(f"TEXT_GRAD_TOWER training step {what}: HIP {e_hip:.2e} | restatement {e_model:.2e}")
        assert e_hip <= 2.0 * e_model, what
