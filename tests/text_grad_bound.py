"""What the backward of the frozen text tower (hoigen_amd/csrc/hg_text_grad.hip, hg_text_bwd.hip) is held to.  A plain module beside the
tests (tests/test_text_grad_rounding_model.py, tests/test_gpu_text_grad_kernels.py, tests/test_gpu_text_grad.py import it): no fixtures,
no GPU, no library.

1. The three new kernels, each against a float64 reference of the same fp16 / fp32 inputs and a bound PER OUTPUT ELEMENT that is the sum of
   the kernel's own roundings.  Rule: every element has |got - want| <= B.  u = 2^-24.

   text_attn_bwd_kernel (q, k, v, dO fp16; causal; scale 1/8).  In float64: s = q k^T / 8, P = softmax(s), dP = dO v^T,
   delta_i = sum_j P_ij dP_ij, dS = P (dP - delta), dV = P^T dO, dK = dS^T q / 8, dQ = dS k / 8.  The fp16 roundings are P and dS as MFMA
   operands and the three outputs (relative 2^-11, and half a subnormal step, 2^-25, where the value is below 2^-14); everything else is fp32
   and carried by explicit terms, because dS = P (dP - delta) cancels (a V with a common offset makes dP and delta large and equal):
       rp_i   = 2^-20 (1 + max_j sum_d |q_id k_jd| / 8)                  relative error of a probability of row i (scores and exp2 in fp32)
       a_ij   = 2^-21 sum_d |dO_id v_jd|                                 error of dP_ij (64 products accumulated in fp32)
       ed_i   = sum_j P_ij (rp_i |dP_ij| + a_ij) + 2^-22 sum_j P_ij |dP_ij|       error of delta_i
       eS_ij  = P_ij (a_ij + ed_i) + (rp_i + 2^-23) |dS_ij| + 2^-11 |dS_ij| + 2^-25   error of the fp16 operand dS_ij
       eP_ij  = (2^-11 + rp_i) P_ij + 2^-25                              error of the fp16 operand P_ij
       B(dV_jd) = 2^-11 |want| + 2^-25 + sum_i eP_ij |dO_id| + 2^-22 sum_i P_ij |dO_id|
       B(dK_jd) = 2^-11 |want| + 2^-25 + (sum_i eS_ij |q_id| + 2^-22 sum_i |dS_ij q_id|) / 8
       B(dQ_id) = 2^-11 |want| + 2^-25 + (sum_j eS_ij |k_jd| + 2^-22 sum_j |dS_ij k_jd|) / 8

   layernorm_bwd_kernel (all fp32): g += rstd (dyg - m1 - xhat m2), dyg = dy gamma, m1 = mean(dyg), m2 = mean(dyg xhat).  With
   c = log2(D) + 8 roundings for a wave-tree sum of D terms and its division:
       d = c u mean|x|                                                  error of the mean; the fp32 variance is the mean of (x - mean32)^2
       e_r = rstd^2 d^2 / 2 + c u                                       = var + d^2: relative error of rstd (d rstd / d var = -rstd^3 / 2; it
                                                                        shows where the variance is small against eps: constant rows)
       e_xh_j = rstd (d + 2 u |x_j|) + (c u + e_r) |xhat_j|             (x - mean cancels where the row has a common offset)
       e_m1 = c u mean|dyg|,   e_m2 = c u mean|dyg xhat| + mean(|dyg| e_xh)
       B_j = rstd (2 u |dyg_j| + e_m1 + |xhat_j| e_m2 + |m2| e_xh_j + 3 u (|dyg_j| + |m1| + |xhat_j m2|)) + (c u + e_r) |upd_j|
             + 2 u (|g_j| + |upd_j|)

   qgelu_bwd_kernel (df, u fp16 -> du fp16): du = df (sig + 1.702 u sig (1 - sig)), sig = sigmoid(1.702 u):
       B = 2^-11 |want| + 2^-25 + 2^-20 (1 + 1.702 |u|) |df| (sig + 1.702 |u| sig (1 - sig))

2. `tower_backward_model`: the whole backward restated in torch, fp32 where the kernels hold fp32, rounded to fp16 at exactly these sites and
   nowhere else (per block, blocks last to first; the tail first):
       tail      fp16(s_r grad_out)                                       the operand of the text_projection GEMM (its output is fp32)
       recompute fp16(ln_1(x_in)), fp16(qkv), the attention output fp16(att) (probabilities fp16 as MFMA operands), fp16(ln_2(x_mid)),
                 fp16(u) - the block again from its saved fp32 input, as the forward's plain launch sequence rounds it
       MLP       fp16(g) -> df = fp16(fp16(g) W_proj) -> du = fp16(df qgelu'(u)) -> dh2 fp32
       attention fp16(g) -> da = fp16(fp16(g) W_out) -> inside the kernel fp16(P), fp16(dS) -> fp16(dq | dk | dv) -> dh1 fp32
   The residual gradient g, both LayerNorm backwards, x_mid and the saved stream are fp32.  s_r = 2^-floor(log2 max_e |grad_out[r, e]|).
   The gate of the tower tests is this restatement's own error against the float64 autograd gradient, on the same inputs, times two:
   MFMA accumulation order and the softmax sums' order move individual roundings against torch's, not their number.
"""
import math

import numpy as np
import torch

import attention_bound as ab

HD = 64
U = 2.0 ** -24
ATTN_FAMILIES = ("randn", "sink", "ramp", "voffset")
ATTN_MUTANTS = ("no_causal", "no_delta", "scale_dq_only")
# the other restatements take one mutant each: ln_model "no_xhat_term", qgelu_model "first_term_only", tower_backward_model "unscaled"


def f16(t):
    return t.half().float()


def sub16(want):
    """2^-11 |want| + half a subnormal step: the rounding of an fp16 result"""
    return 2.0 ** -11 * want.abs() + 2.0 ** -25


# ---- attention backward -------------------------------------------------------------------------------------------------------------
def make_attn(family, n_seq, L, heads, seed):
    """qkv [n_seq * L, 3 * heads * 64] of tests/attention_bound.py's family and dout [n_seq * L, heads * 64], float32 holding fp16 values"""
    qkv = ab.make_qkv(family, n_seq, L, heads, seed)
    g = torch.Generator().manual_seed(int(seed) + 77)
    dout = torch.randn(n_seq * L, heads * HD, generator=g, dtype=torch.float64).half().float()
    return qkv, dout


def _heads(t, n_seq, L, heads):
    return t.view(n_seq, L, heads, HD).permute(0, 2, 1, 3).contiguous()


def _pack(dq, dk, dv, n_seq, L, heads):
    """three [n_seq, heads, L, 64] -> [n_seq * L, 3 * heads * 64], the kernel's dq | dk | dv layout"""
    return torch.cat([ab.rows(t, n_seq, L, heads) for t in (dq, dk, dv)], 1)


def attn_reference(qkv, dout, n_seq, L, heads):
    """float64: dict of want and B, each [n_seq * L, 3 * heads * 64]"""
    q, k, v = ab.split(qkv, n_seq, L, heads)
    do = _heads(dout.detach().cpu().half().double(), n_seq, L, heads)
    vis = torch.ones(L, L, dtype=torch.bool).tril()
    s = (q @ k.transpose(-1, -2) * 0.125).masked_fill(~vis, float("-inf"))
    P = torch.softmax(s, -1)
    dP = (do @ v.transpose(-1, -2)).masked_fill(~vis, 0.0)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dV, dK, dQ = P.transpose(-1, -2) @ do, dS.transpose(-1, -2) @ q * 0.125, dS @ k * 0.125
    sabs = (q.abs() @ k.abs().transpose(-1, -2) * 0.125).masked_fill(~vis, 0.0)
    rp = 2.0 ** -20 * (1.0 + sabs.max(-1, keepdim=True).values)
    a = 2.0 ** -21 * (do.abs() @ v.abs().transpose(-1, -2)).masked_fill(~vis, 0.0)
    ed = (P * (rp * dP.abs() + a)).sum(-1, keepdim=True) + 2.0 ** -22 * (P * dP.abs()).sum(-1, keepdim=True)
    eS = (P * (a + ed) + (rp + 2.0 ** -23 + 2.0 ** -11) * dS.abs() + 2.0 ** -25).masked_fill(~vis, 0.0)
    eP = ((2.0 ** -11 + rp) * P + 2.0 ** -25).masked_fill(~vis, 0.0)
    BV = sub16(dV) + eP.transpose(-1, -2) @ do.abs() + 2.0 ** -22 * (P.transpose(-1, -2) @ do.abs())
    BK = sub16(dK) + (eS.transpose(-1, -2) @ q.abs() + 2.0 ** -22 * (dS.abs().transpose(-1, -2) @ q.abs())) * 0.125
    BQ = sub16(dQ) + (eS @ k.abs() + 2.0 ** -22 * (dS.abs() @ k.abs())) * 0.125
    return {"want": _pack(dQ, dK, dV, n_seq, L, heads), "B": _pack(BQ, BK, BV, n_seq, L, heads)}


def _attn_bwd32(q, k, v, do, mutant=None):
    """the kernel's arithmetic on [n, h, L, 64] float32 tensors holding fp16 values -> dq, dk, dv float32 holding fp16 values"""
    L = q.shape[-2]
    vis = torch.ones(L, L, dtype=torch.bool).tril()
    if mutant == "no_causal":
        vis = torch.ones(L, L, dtype=torch.bool)
    s = ((q @ k.transpose(-1, -2)) * np.float32(0.125)).masked_fill(~vis, float("-inf"))
    e = torch.exp2(((s - s.max(-1, keepdim=True).values) * np.float32(1.4426950408889634)).double()).float()
    P = e * (1.0 / e.sum(-1, keepdim=True))
    dP = (do @ v.transpose(-1, -2)).masked_fill(~vis, 0.0)
    delta = (P * dP).sum(-1, keepdim=True)
    if mutant == "no_delta":
        delta = torch.zeros_like(delta)
    dS16, P16 = f16(P * (dP - delta)), f16(P)
    dv = P16.transpose(-1, -2) @ do
    dk = (dS16.transpose(-1, -2) @ q) * np.float32(1.0 if mutant == "scale_dq_only" else 0.125)
    dq = (dS16 @ k) * np.float32(0.125)
    return f16(dq), f16(dk), f16(dv)


def attn_model(qkv, dout, n_seq, L, heads, mutant=None):
    assert mutant is None or mutant in ATTN_MUTANTS, mutant
    q, k, v = (t.float() for t in ab.split(qkv, n_seq, L, heads))
    do = _heads(dout.detach().cpu().half().float(), n_seq, L, heads)
    return _pack(*_attn_bwd32(q, k, v, do, mutant), n_seq, L, heads).double()


def worst(got, ref):
    """largest |got - want| / B (0 / 0 counts as 0); inf where got is not finite"""
    got = got.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref["want"]).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / ref["B"])
    return float(r.max())


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------------
def make_ln(family, M, D, seed):
    """x, gamma, dy, g float32: randn rows, rows with a common offset of 30, constant rows (variance 0)"""
    gen = torch.Generator().manual_seed(int(seed))
    x = torch.randn(M, D, generator=gen)
    if family == "offset":
        x = 30.0 + 0.5 * x
    elif family == "constant":
        x = torch.full((M, D), 1.7) * (1.0 + torch.arange(M, dtype=torch.float32)[:, None])
    else:
        assert family == "randn", family
    gamma = 1.0 + 0.3 * torch.randn(D, generator=gen)
    return x.contiguous(), gamma, torch.randn(M, D, generator=gen), torch.randn(M, D, generator=gen)


def ln_bwd(x, gamma, dy, mutant=None):
    """the update rstd (dyg - mean(dyg) - xhat mean(dyg xhat)) in the dtype of x"""
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    xhat, dyg = xc * rstd, dy * gamma.to(x.dtype)
    m2 = (dyg * xhat).mean(-1, keepdim=True)
    if mutant == "no_xhat_term":
        m2 = torch.zeros_like(m2)
    return rstd * (dyg - dyg.mean(-1, keepdim=True) - xhat * m2)


def ln_reference(x, gamma, dy, g):
    x, gamma, dy, g = (t.detach().cpu().double() for t in (x, gamma, dy, g))
    D = x.shape[-1]
    c = math.log2(D) + 8
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)
    xhat, dyg = xc * rstd, dy * gamma
    m1, m2 = dyg.mean(-1, keepdim=True), (dyg * xhat).mean(-1, keepdim=True)
    upd = rstd * (dyg - m1 - xhat * m2)
    d = c * U * x.abs().mean(-1, keepdim=True)
    e_r = 0.5 * rstd * rstd * d * d + c * U
    e_xh = rstd * (d + 2 * U * x.abs()) + (c * U + e_r) * xhat.abs()
    e_m1 = c * U * dyg.abs().mean(-1, keepdim=True)
    e_m2 = c * U * (dyg * xhat).abs().mean(-1, keepdim=True) + (dyg.abs() * e_xh).mean(-1, keepdim=True)
    B = rstd * (2 * U * dyg.abs() + e_m1 + xhat.abs() * e_m2 + m2.abs() * e_xh + 3 * U * (dyg.abs() + m1.abs() + (xhat * m2).abs())) \
        + (c * U + e_r) * upd.abs() + 2 * U * (g.abs() + upd.abs())
    return {"want": g + upd, "B": B, "upd": upd}


def ln_model(x, gamma, dy, g, mutant=None):
    assert mutant in (None, "no_xhat_term"), mutant
    return (g.float() + ln_bwd(x.float(), gamma.float(), dy.float(), mutant)).double()


# ---- QuickGELU backward ---------------------------------------------------------------------------------------------------------------
def make_qgelu(n, seed):
    """df, u float32 holding fp16 values; u covers both tails (|u| up to about 12)"""
    gen = torch.Generator().manual_seed(int(seed))
    return f16(torch.randn(n, generator=gen)), f16(3.0 * torch.randn(n, generator=gen))


def qgelu_grad(u, mutant=None):
    sig = torch.sigmoid(1.702 * u)
    return sig if mutant == "first_term_only" else sig + 1.702 * u * sig * (1.0 - sig)


def qgelu_reference(df, u):
    df, u = df.detach().cpu().double(), u.detach().cpu().double()
    sig = torch.sigmoid(1.702 * u)
    want = df * qgelu_grad(u)
    B = sub16(want) + 2.0 ** -20 * (1.0 + 1.702 * u.abs()) * df.abs() * (sig + 1.702 * u.abs() * sig * (1.0 - sig))
    return {"want": want, "B": B}


def qgelu_model(df, u, mutant=None):
    assert mutant in (None, "first_term_only"), mutant
    return f16(df.float() * qgelu_grad(u.float(), mutant)).double()


# ---- the prompt learner's backward ----------------------------------------------------------------------------------------------------
def prompts_bwd_model(g, n_ctx, chunk=64):
    """float32 with the kernels' summation order: grad_bias[r] = ((g[r][1] + g[r][2]) + ...), grad_ctx[j] = chunks of `chunk` prompts in
    ascending order, then the chunks in ascending order; every partial sum starts from 0"""
    g = g.detach().cpu().float()
    R = g.shape[0]
    gb = torch.zeros(R, g.shape[2])
    for j in range(n_ctx):
        gb = gb + g[:, 1 + j]
    gc = torch.zeros(n_ctx, g.shape[2])
    for r0 in range(0, R, chunk):
        part = torch.zeros(n_ctx, g.shape[2])
        for r in range(r0, min(R, r0 + chunk)):
            part = part + g[r, 1:1 + n_ctx]
        gc = gc + part
    return gc, gb


# ---- the whole backward ---------------------------------------------------------------------------------------------------------------
def pow2_scale(grad_out):
    """s_r = 2^-floor(log2(max_e |grad_out[r, e]|)), 1 for an all-zero row; [R, 1] float32"""
    mx = grad_out.detach().abs().amax(-1, keepdim=True).double()
    ex = torch.where(mx > 0, torch.floor(torch.log2(torch.where(mx > 0, mx, torch.ones_like(mx)))), torch.zeros_like(mx))
    return torch.exp2(-ex.clamp(-126, 126)).float()


def _ln32(x, w, b):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    return xc * (1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-5)) * w + b


def _split_heads(t, heads):
    R, L, D = t.shape
    return t.view(R, L, heads, HD).permute(0, 2, 1, 3)


def _merge_heads(t):
    R, h, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(R, L, h * HD)


def _block_recompute(sd, p, x_in, heads):
    """the block from its fp32 input, rounded as the plain launch sequence rounds it -> qkv, x_mid, u (pre-activation), h2"""
    D = x_in.shape[-1]
    h1 = f16(_ln32(x_in, sd[p + "ln_1.weight"], sd[p + "ln_1.bias"]))
    qkv = f16(h1 @ sd[p + "attn.in_proj_weight"].T + sd[p + "attn.in_proj_bias"])
    q, k, v = (_split_heads(t, heads) for t in qkv.split(D, -1))
    L = x_in.shape[1]
    s = ((q @ k.transpose(-1, -2)) * np.float32(0.125)).masked_fill(~torch.ones(L, L, dtype=torch.bool).tril(), float("-inf"))
    att = f16(_merge_heads(f16(torch.softmax(s, -1)) @ v))
    x_mid = x_in + att @ sd[p + "attn.out_proj.weight"].T + sd[p + "attn.out_proj.bias"]
    h2 = f16(_ln32(x_mid, sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]))
    u32 = h2 @ sd[p + "mlp.c_fc.weight"].T + sd[p + "mlp.c_fc.bias"]
    return qkv, x_mid, f16(u32), u32


def tower_forward_model(sd, prompts, eot, heads):
    """fp32 stream with the forward's fp16 operands -> (text features [R, E], the stream entering every block, the last block's EOT rows)"""
    sd = {k: v.float() for k, v in sd.items() if not k.startswith("visual.")}
    x = prompts.detach().float() + sd["positional_embedding"][: prompts.shape[1]]
    saved = []
    n = len([k for k in sd if k.startswith("transformer.") and k.endswith(".attn.in_proj_weight")])
    for i in range(n):
        p = f"transformer.resblocks.{i}."
        saved.append(x)
        _, x_mid, _, u32 = _block_recompute(sd, p, x, heads)
        x = x_mid + f16(u32 * torch.sigmoid(1.702 * u32)) @ sd[p + "mlp.c_proj.weight"].T + sd[p + "mlp.c_proj.bias"]
    x_eot = x[torch.arange(x.shape[0]), eot]
    out = f16(_ln32(x_eot, sd["ln_final.weight"], sd["ln_final.bias"])) @ sd["text_projection"]
    return out, saved, x_eot


def block_backward_model(sd, p, x_in, g, heads):
    """one block: the gradient g [R, L, D] of its output -> of its input x_in, float32 (sd float32)"""
    D = x_in.shape[-1]
    qkv, x_mid, u, _ = _block_recompute(sd, p, x_in, heads)
    df = f16(f16(g) @ sd[p + "mlp.c_proj.weight"])
    du = f16(df * qgelu_grad(u))
    g = g + ln_bwd(x_mid, sd[p + "ln_2.weight"], du @ sd[p + "mlp.c_fc.weight"])
    da = f16(f16(g) @ sd[p + "attn.out_proj.weight"])
    q, k, v = (_split_heads(t, heads) for t in qkv.split(D, -1))
    dq, dk, dv = _attn_bwd32(q, k, v, _split_heads(da, heads))
    dqkv = torch.cat([_merge_heads(t) for t in (dq, dk, dv)], -1)
    return g + ln_bwd(x_in, sd[p + "ln_1.weight"], dqkv @ sd[p + "attn.in_proj_weight"])


def block_reference(sd, p, x_in, g, heads):
    """float64 autograd through oracle.clip_oracle.resblock"""
    from oracle import clip_oracle as co
    x = x_in.detach().double().requires_grad_()
    with torch.enable_grad():
        (co.resblock(x, sd, p, heads, True) * g.detach().double()).sum().backward()
    return x.grad


def tower_backward_model(sd, prompts, eot, grad_out, heads, mutant=None):
    """grad_prompts [R, L, D] float32: the HIP backward's arithmetic in torch (module docstring, 2.).  sd: float32 weights that are fp16
    numbers where the library holds fp16 (oracle.clip_oracle.reference_weight_rounding).  mutant "unscaled": s_r = 1"""
    assert mutant in (None, "unscaled"), mutant
    sd = {k: v.float() for k, v in sd.items() if not k.startswith("visual.")}
    _, saved, x_eot = tower_forward_model(sd, prompts, eot, heads)
    R, L, D = prompts.shape
    go = grad_out.detach().float()
    s = torch.ones(R, 1) if mutant == "unscaled" else pow2_scale(go)
    dhf = f16(go * s) @ sd["text_projection"].T
    g = torch.zeros(R, L, D)
    g[torch.arange(R), eot] = ln_bwd(x_eot, sd["ln_final.weight"], dhf)
    for i in reversed(range(len(saved))):
        g = block_backward_model(sd, f"transformer.resblocks.{i}.", saved[i], g, heads)
    return g * (1.0 / s)[:, :, None]


def tower_reference(sd, prompts, tokenized, grad_out):
    """float64 autograd through oracle.clip_oracle.text_encoder_embeds -> grad_prompts [R, L, D] float64"""
    from oracle import clip_oracle as co
    p = prompts.detach().double().requires_grad_()
    with torch.enable_grad():
        out = co.text_encoder_embeds(sd, p, tokenized, dtype=torch.float64)
        (out * grad_out.detach().double()).sum().backward()
    return p.grad


def rel_l2_per_prompt(got, ref, eot):
    """relative L2 of every prompt's gradient over the positions <= EOT; inf where got is not finite"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    out = []
    for r in range(ref.shape[0]):
        a, b = got[r, : int(eot[r]) + 1], ref[r, : int(eot[r]) + 1]
        out.append(float((a - b).norm() / b.norm()) if bool(torch.isfinite(a).all()) else float("inf"))
    return out


# the towers of the GPU tests beside synth.TINY: ViT-B/16's text tower (width 512) with two blocks or all twelve, and a width-768 one
# with two blocks; a small vocabulary and one vision block keep the seeded weights quick to make (the text path never reads the rest)
def small_config(width=512, layers=2):
    from hoigen_amd import synth
    return dict(synth.VIT_B16, vision_layers=1, vocab_size=1024, transformer_width=width, transformer_heads=width // 64,
                transformer_layers=layers)


def tower_case(cfg, seed, R, L, eot, magnitude):
    """seeded weights of a configuration (hoigen_amd.synth), prompts from its token embedding, grad_out ~ magnitude randn.
    -> (cfg, numpy state dict for build_model, float32 rounded weights for the references, prompts, tokenized, eot, grad_out)"""
    from hoigen_amd import synth
    from oracle import clip_oracle as co
    cfg = dict(cfg)
    sd_np = synth.clip_state_dict(cfg, seed)
    sd = {k: v for k, v in co.reference_weight_rounding(sd_np).items() if not k.startswith("visual.")}
    gen = torch.Generator().manual_seed(seed * 131 + R * 7 + L)
    ids = torch.randint(1, cfg["vocab_size"] - 2, (R, L), generator=gen)
    eot = torch.as_tensor(eot, dtype=torch.long)
    tokenized = ids.clone()
    tokenized[torch.arange(R), eot] = cfg["vocab_size"] - 1          # EOT = the largest id of the row
    prompts = sd["token_embedding.weight"][ids].float().contiguous()
    grad_out = (torch.randn(R, cfg["embed_dim"], generator=gen) * magnitude).float()
    return cfg, sd_np, sd, prompts, tokenized, eot, grad_out
