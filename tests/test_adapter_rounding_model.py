"""A rounding model of the instance adapter's fp16 design (hg_adapter.hip, run_adapter in hg_tower.hip), in plain torch on the CPU, and the
proof that the bound built on it bites.  No GPU, no library.

The model is the oracle's arithmetic (oracle.clip_oracle.adapter, float64) with ``.half()`` applied exactly where the kernels stage fp16:

* MFMA decoder (at most 32 prior tokens, or the sequence itself as memory): the stream copy, every weight matrix, the activation in front of
  every linear, q after scaling, K, V, the probabilities (their sum stays fp32), the attention output, and the decoder's output d (or e);
* fp32 one-lane-per-token kernels (more than 32 prior tokens): only the stream copy, the down_proj / up_proj weights and d;
* folded adapter (mode 2): e = [z_0 .. z_62, 1] in fp16 and Q = fp16 of the fp32 product built from the fp16 up_proj weight.

tests/test_gpu_adapter.py measures a kernel's error against the float64 oracle and allows it TWICE the model's worst-row error and 1.5 x its
median row on the same inputs (``rule``): room for fp32 accumulation order, __expf and the odd 1-ulp flip of an fp16 rounding, not for a
missing term.  The tests below put wrong kernels through the same rule - the model with one padded key unmasked, the mask shifted by
one key, the last token given its neighbour's result, z_63 left in e[63], the variance update without its cross term, with the
old[0] * sa part of that term dropped or flipped, the new mean without old[0] - and every one of them breaks it at every case tried.
The last three are dead while the fp16 copy is centred on the row's own mean (old[0] = 0, as in front of a tower's first block): they
run with the centre a preceding block leaves, away from the mean.
"""
import numpy as np
import pytest
import torch

from hoigen_amd import synth
from oracle import clip_oracle as co

PRE = "visual.transformer.resblocks.{}.adaptermlp."
MASKS = ("none", "suffix", "prefix", "third", "first", "last")
STREAMS = ("unit", "small", "outlier")
WORST, MEDIAN = 2.0, 1.5


def H(t):
    return t.float().half().double()


def ident(t):
    return t


def weights(cfg, seed, num_layers=1, block=0):
    """(float64 oracle state dict of one block's adapter, its key prefix)"""
    raw = synth.adapter_state_dict(cfg, seed, layers=[block], num_layers=num_layers)
    return {k: v.double() for k, v in co.as_tensors(raw).items()}, PRE.format(block)


def make_stream(kind, n_seq, L, D, seed):
    x = synth.hg_normal((n_seq, L, D), seed, 1.0)
    if kind == "small":        # rows of mean 30 and spread 0.02
        x = x * np.float32(0.02) + np.float32(30.0)
    elif kind == "outlier":    # a few channels 67 x the rest
        for ch in (5 % D, (D // 6 + 2) % D, (2 * D // 3 + 5) % D):
            x[..., ch] *= np.float32(67.0)
    else:
        assert kind == "unit"
    return torch.from_numpy(np.ascontiguousarray(x, np.float32))


def make_centre(x, seed, rel=0.05):
    """[n_seq, L] fp32: a centre of the fp16 copy away from the row's mean by about `rel` of the row's spread, either sign - where a
    preceding block's residual GEMM leaves it (the row's mean BEFORE that GEMM's update)"""
    off = torch.from_numpy(synth.hg_normal(tuple(x.shape[:2]), seed, 1.0))
    return (x.float().mean(-1) + np.float32(rel) * x.float().std(-1) * off).float()


def make_mask(kind, n_seq, N):
    """key_padding_mask [n_seq, N] (True = pad), different in every sequence where the kind allows it; never all keys of a sequence"""
    m = torch.zeros(n_seq, N, dtype=torch.bool)
    j = torch.arange(N)
    for i in range(n_seq):
        p = (1 + i) % N
        if kind == "suffix":
            m[i, N - p:] = p > 0
        elif kind == "prefix":
            m[i, :p] = True
        elif kind == "third":
            hit = (j + i) % 3 == 0
            m[i] = hit if i % 6 < 3 else ~hit
        elif kind == "first":
            m[i, 1:] = True
        elif kind == "last":
            m[i, :N - 1] = True
        else:
            assert kind == "none"
        if m[i].all():
            m[i, i % N] = False
    return m


def make_prior(n_seq, N, kind, seed):
    return torch.from_numpy(synth.hg_normal((n_seq, N, 64), seed, 1.0)), make_mask(kind, n_seq, N)


def n_chain(sd, pre):
    z = 0
    while pre + f"mhsa_layers.{z}.linear1.weight" in sd:
        z += 1
    return z


def last_layer(sd, pre, prior):
    return pre + (f"mhsa_layers.{n_chain(sd, pre) - 1}." if prior is not None else "mhsa.")


def oracle_parts(x, sd, pre, prior):
    """(z = the last decoder layer's norm3 without its affine part, a = the update) of co.adapter in float64"""
    x = x.double()
    down = torch.relu(co.linear(x, sd[pre + "down_proj.weight"], sd[pre + "down_proj.bias"]))
    if prior is not None:
        for z in range(n_chain(sd, pre)):
            down = co._decoder_layer_post(down, prior[0].double(), sd, pre + f"mhsa_layers.{z}.", prior[1])
    else:
        down = co._decoder_layer_post(down, down, sd, pre + "mhsa.", None)
    a = co.linear(down, sd[pre + "up_proj.weight"], sd[pre + "up_proj.bias"]) * sd[pre + "scale"]
    assert torch.equal(a, co.adapter(x, sd, pre, prior))
    lp = last_layer(sd, pre, prior)
    return (down - sd[lp + "norm3.bias"]) / sd[lp + "norm3.weight"], a


def q_matrix(sd, pre, prior, rnd=True, w_up16=False):
    """Q [D, 64] with a = Q e (hg_elem.hip adapter_q_kernel; tests/test_adapter_fold_math.py); rnd: as the device holds it (from the fp16
    up_proj weight, rounded to fp16); w_up16: only the first of the two"""
    lp = last_layer(sd, pre, prior)
    g3, b3 = sd[lp + "norm3.weight"], sd[lp + "norm3.bias"]
    scale, b_up = sd[pre + "scale"], sd[pre + "up_proj.bias"]
    w_up = H(sd[pre + "up_proj.weight"]) if rnd or w_up16 else sd[pre + "up_proj.weight"]
    p = scale[:, None] * w_up
    q = torch.empty_like(p)
    q[:, :63] = g3[None, :63] * p[:, :63] - g3[63] * p[:, 63:64]
    q[:, 63] = p @ b3 + scale * b_up
    return H(q) if rnd else q


def _norm(t):
    mu = t.mean(-1, keepdim=True)
    tc = t - mu
    return tc / torch.sqrt((tc * tc).mean(-1, keepdim=True) + 1e-5)


def _decoder(tgt, mem, sd, lp, mask, Hm):
    """one post-norm decoder layer up to (not including) norm3; tgt = the layer's fp32 residual, mem None = the sequence itself"""
    t16 = Hm(tgt)
    m16 = t16 if mem is None else Hm(mem)
    wi, bi = Hm(sd[lp + "multihead_attn.in_proj_weight"]), sd[lp + "multihead_attn.in_proj_bias"]
    q = Hm((t16 @ wi[:64].T + bi[:64]) * 32 ** -0.5)
    k = Hm(m16 @ wi[64:128].T + bi[64:128])
    v = Hm(m16 @ wi[128:].T + bi[128:])
    o = torch.empty_like(q)
    for h in range(2):
        sl = slice(32 * h, 32 * h + 32)
        s = q[..., sl] @ k[..., sl].transpose(1, 2)
        if mask is not None:
            s = s.masked_fill(mask[:, None, :], float("-inf"))
        p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        o[..., sl] = (Hm(p) @ v[..., sl]) / p.sum(dim=-1, keepdim=True)
    t2 = Hm(o) @ Hm(sd[lp + "multihead_attn.out_proj.weight"]).T + sd[lp + "multihead_attn.out_proj.bias"]
    tgt = co.layer_norm(tgt + t2, sd[lp + "norm2.weight"], sd[lp + "norm2.bias"])
    hid = torch.relu(Hm(tgt) @ Hm(sd[lp + "linear1.weight"]).T + sd[lp + "linear1.bias"])
    return tgt + Hm(hid) @ Hm(sd[lp + "linear2.weight"]).T + sd[lp + "linear2.bias"]


def model(x, sd, pre, prior, mode, lanes=False, rnd=True, mut=None, centre=None):
    """The design's arithmetic on x [n_seq, L, D] (fp32 values).  Returns {"a": update [n_seq, L, D]} and in mode 2 also "e" and "z".
    lanes: the fp32 one-lane-per-token decoder.  rnd = False: no rounding at all (then it is co.adapter).
    centre [n_seq, L] (modes 1 and 2): the centre of the fp16 copy, default the row's fp32 mean.
    mut: None | "unmask" | "shift" | "last_token" | "z63" - a wrong kernel (see the module docstring)."""
    x = x.double()
    Hs = H if rnd else ident
    Hm = H if rnd and not lanes else ident
    if prior is not None and mut in ("unmask", "shift"):
        pri, mask = prior
        mask = mask.clone()
        if mut == "shift":
            mask = torch.roll(mask, 1, dims=1)
        else:
            for i in range(mask.shape[0]):
                pad = mask[i].nonzero().flatten()
                if len(pad):
                    mask[i, pad[len(pad) // 2]] = False
        prior = (pri, mask)
    if mode == 0 or not rnd:
        xin = Hs(x)
    else:       # the centred copy: fp16(x - centre), the centre added back behind the product
        mu = (x.float().mean(-1) if centre is None else centre.float()).double()[..., None]
        xin = Hs(x - mu) + mu
    down = torch.relu(xin @ Hs(sd[pre + "down_proj.weight"]).T + sd[pre + "down_proj.bias"])
    layers = [pre + f"mhsa_layers.{z}." for z in range(n_chain(sd, pre))] if prior is not None else [pre + "mhsa."]
    for lp in layers:      # (between chained layers the activation stays fp32)
        t = _decoder(down, prior[0].double() if prior is not None else None, sd, lp, prior[1] if prior is not None else None, Hm)
        down = co.layer_norm(t, sd[lp + "norm3.weight"], sd[lp + "norm3.bias"])
    res = {}
    if mode == 2:
        z = _norm(t)
        e = z.clone()
        if mut != "z63":
            e[..., 63] = 1.0
        e = Hs(e)
        if mut == "last_token" and e.shape[1] > 1:
            e[:, -1] = e[:, -2]
        res["e"] = e
        res["z"] = torch.cat([e[..., :63], -e[..., :63].sum(-1, keepdim=True)], -1)
        res["a"] = e @ q_matrix(sd, pre, prior, rnd).T
        return res
    a = (Hs(down) @ Hs(sd[pre + "up_proj.weight"]).T + sd[pre + "up_proj.bias"]) * sd[pre + "scale"]
    if rnd:
        a = (x + a).float().double() - x      # the update as it is read back from the fp32 stream
    if mut == "last_token" and a.shape[1] > 1:
        a[:, -1] = a[:, -2]
    res["a"] = a
    return res


# ---- LayerNorm statistics: the kernels' own formulas in float32 numpy --------------------------------------------------------------
def rowstats_f32(x):
    """(mean, rstd) of the rows of x [M, D] in float32, in rowstats_cast_kernel's order of additions (hg_elem.hip): a lane holds the four
    columns 4 c .. 4 c + 3 of every 64th group c, adds (v0 + v1) + (v2 + v3) group after group, then the xor butterfly 32, 16 .. 1 over
    the wave's 64 lanes; the squared deviations the same way with fused multiply-adds.  D a multiple of 256."""
    f = np.float32
    x = np.asarray(x, f)
    M, D = x.shape
    v = x.reshape(M, D // 256, 64, 4)
    lanes = np.arange(64)

    def wave_sum(s):
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, 0]

    s = np.zeros((M, 64), f)
    for i in range(D // 256):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    mean = wave_sum(s) / f(D)
    q = np.zeros((M, 64), f)
    for i in range(D // 256):
        for k in range(4):
            d = (v[:, i, :, k] - mean[:, None]).astype(np.float64)
            q = (d * d + q.astype(np.float64)).astype(f)          # fmaf(d, d, q): the product is exact in float64
    return mean, f(1) / np.sqrt(wave_sum(q) / f(D) + f(1e-5))


def fold_stats_f32(x, e, q16, centre=None, cross=True, old_sign=1, mean_old=True):
    """hg_adapter.hip, folded epilogue: (mean, rstd) of x + Q e from those of x and three 64-wide products.  x [M, D] fp32, e [M, 64]
    (the kernel's fp16 output), q16 [D, 64] as the device holds it, centre [M] of the fp16 copy (default: the row's fp32 mean).
    Wrong kernels: cross = False drops the cross term of the variance update, old_sign = 0 / -1 drops / flips its old[0] * sa part,
    mean_old = False drops old[0] from the new mean."""
    f = np.float32
    x, e, q = np.asarray(x, f), np.asarray(e, f), np.asarray(q16, f)
    D = f(x.shape[1])
    mean_x, rstd_x = rowstats_f32(x)
    c = mean_x if centre is None else np.asarray(centre, f).reshape(-1)
    x16 = (x - c[:, None]).astype(np.float16).astype(f)
    g = (q.T @ q).astype(np.float16).astype(f)
    sa = e @ q.sum(0, dtype=f)
    cr = (e * (x16 @ q)).sum(1, dtype=f)
    qd = (e * (e @ g)).sum(1, dtype=f)
    old0 = mean_x - c                                       # mr[m][0] on entry: mean_x minus the centre of the copy
    var_x = f(1) / (rstd_x * rstd_x) - f(1e-5)
    dv = ((f(2) * (cr - f(old_sign) * old0 * sa) if cross else f(0)) + (qd - sa * sa / D)) / D
    var_y = np.maximum(var_x + dv, f(0))
    mr0 = (old0 if mean_old else f(0)) + sa / D
    return mr0.astype(np.float64) + c.astype(np.float64), (f(1) / np.sqrt(var_y + f(1e-5))).astype(np.float64)


def group_stats_f32(y):
    """the residual GEMM's epilogue + finalize_stats: per 64-column group (sum, sum of squared deviations from the group mean), combined"""
    f = np.float32
    y = np.asarray(y, f)
    M, D = y.shape
    g = y.reshape(M, D // 64, 64)
    s = g.sum(2, dtype=f)
    gm = s / f(64)
    m2 = ((g - gm[..., None]) ** 2).sum(2, dtype=f)
    mean = s.sum(1, dtype=f) / f(D)
    tot = (m2 + f(64) * (gm - mean[:, None]) ** 2).sum(1, dtype=f)
    return mean.astype(np.float64), (f(1) / np.sqrt(tot / f(D) + f(1e-5))).astype(np.float64)


def true_stats(y):
    y = np.asarray(y, np.float64)
    return y.mean(1), 1.0 / np.sqrt(y.var(1) + 1e-5)


def stat_errors(got, want):
    """the error of (mean, rstd) as it reaches a normalised value: |d mean| * rstd and |d rstd| / rstd, per row"""
    return np.abs(got[0] - want[0]) * want[1], np.abs(got[1] - want[1]) / want[1]


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def row_errors(a, ref):
    a, ref = a.double().reshape(-1, a.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    assert a.shape == ref.shape and torch.isfinite(a).all()
    return ((a - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).numpy()


def rule(kernel_rows, model_rows):
    """(ok, worst ratio, median ratio): the kernel's per-row errors against the model's on the same inputs"""
    kernel_rows, model_rows = np.asarray(kernel_rows, np.float64), np.asarray(model_rows, np.float64)
    rw = kernel_rows.max() / max(model_rows.max(), 1e-300)
    rm = np.median(kernel_rows) / max(np.median(model_rows), 1e-300)
    return bool(rw <= WORST and rm <= MEDIAN), float(rw), float(rm)


# ---- CPU tests -------------------------------------------------------------------------------------------------------------------------
CFG = dict(synth.TINY, vision_width=256)
SD1, P0 = weights(CFG, 13)
SD2, _ = weights(CFG, 13, num_layers=2)


def _case(L, N, kind, stream="unit", n_seq=3, seed=0):
    x = make_stream(stream, n_seq, L, 256, 900 + 7 * L + seed)
    prior = make_prior(n_seq, N, kind, 700 + N + seed) if N else None
    return x, prior


@pytest.mark.parametrize("sd", [SD1, SD2], ids=["one_layer", "two_layers"])
@pytest.mark.parametrize("L,N,kind", [(5, 0, "none"), (33, 6, "third"), (17, 40, "suffix")])
def test_model_without_roundings_is_the_oracle(sd, L, N, kind):
    x, prior = _case(L, N, kind)
    z, a = oracle_parts(x, sd, P0, prior)
    for mode in (0, 1, 2):
        got = model(x, sd, P0, prior, mode, lanes=N > 32, rnd=False)
        assert float((got["a"] - a).abs().max() / a.abs().max()) < 1e-12, mode
        if mode == 2:
            assert float((got["z"] - z).abs().max()) < 1e-11
            assert torch.equal(got["e"][..., 63], torch.ones_like(got["e"][..., 63]))


def _breaks(x, sd, prior, mode, lanes, mut):
    _, a = oracle_parts(x, sd, P0, prior)
    good = row_errors(model(x, sd, P0, prior, mode, lanes)["a"], a)
    bad = row_errors(model(x, sd, P0, prior, mode, lanes, mut=mut)["a"], a)
    assert rule(good, good)[0]                                   # the unmodified model passes, trivially
    assert good.max() < 1e-2, good.max()                         # ... and is itself at fp16 noise (outlier channels: 6e-3)
    ok, rw, rm = rule(bad, good)
    assert not ok, f"{mut}: worst-row ratio {rw:.2f}, median ratio {rm:.2f} stays inside the rule"
    return rw


@pytest.mark.parametrize("kind", ["suffix", "prefix", "third", "first", "last"])
@pytest.mark.parametrize("N", [6, 17, 32, 40])
@pytest.mark.parametrize("mut", ["unmask", "shift"])
def test_a_wrong_mask_breaks_the_rule(mut, N, kind):
    x, prior = _case(33, N, kind)
    mask = prior[1]
    assert not torch.equal(torch.roll(mask, 1, dims=1), mask) and mask.any()
    for mode in (0, 2) if N <= 32 else (0,):
        _breaks(x, SD1, prior, mode, N > 32, mut)


@pytest.mark.parametrize("L", [5, 17, 33, 64, 161, 224])
@pytest.mark.parametrize("N", [0, 17])
def test_the_last_token_given_its_neighbours_result_breaks_the_rule(L, N):
    x, prior = _case(L, N, "suffix")
    for mode in (0, 2):
        _breaks(x, SD1, prior, mode, False, "last_token")


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("N", [0, 17])
def test_z63_left_in_e_breaks_the_rule(stream, N):
    x, prior = _case(33, N, "third", stream)
    _breaks(x, SD1, prior, 2, False, "z63")


def _stat_case(stream, N, centred):
    x, prior = _case(65, N, "prefix", stream)
    centre = make_centre(x, 41) if centred else None
    e = model(x, SD1, P0, prior, 2, centre=centre)["e"].reshape(-1, 64)
    q16 = q_matrix(SD1, P0, prior)
    x2 = x.reshape(-1, 256)
    want = true_stats(x2.double().numpy() + (e @ q16.T).numpy())
    args = (x2.numpy(), e.numpy(), q16.numpy(), None if centre is None else centre.numpy())
    good = stat_errors(fold_stats_f32(*args), want)
    # (the formula itself stays below an fp16 ulp of a normalised value; 1.0e-4 in rstd on the small-spread stream, where Q^T Q's fp16
    # rounding is all of the variance)
    assert good[0].max() < 2.0 ** -11 and good[1].max() < 2.0 ** -11, (good[0].max(), good[1].max())
    return args, want, good


@pytest.mark.parametrize("centred", [False, True], ids=["mean", "centre"])
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("N", [0, 17])
def test_the_variance_update_without_its_cross_term_breaks_the_rule(stream, N, centred):
    args, want, good = _stat_case(stream, N, centred)
    bad = stat_errors(fold_stats_f32(*args, cross=False), want)
    assert np.array_equal(bad[0], good[0])                      # (the mean does not depend on it)
    ok, rw, rm = rule(bad[1], good[1])
    assert not ok, f"rstd without the cross term: worst-row ratio {rw:.2f}, median ratio {rm:.2f} stays inside the rule"


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("N", [0, 17])
@pytest.mark.parametrize("old_sign", [0, -1], ids=["dropped", "flipped"])
def test_the_old_mean_term_of_the_variance_update_breaks_the_rule(old_sign, stream, N):
    """2 (cr - old[0] sa): with the copy centred on the row's own mean old[0] is zero and the term is dead - every block of a tower but
    the first enters with the previous mean as the centre"""
    args, want, good = _stat_case(stream, N, True)
    bad = stat_errors(fold_stats_f32(*args, old_sign=old_sign), want)
    ok, rw, rm = rule(bad[1], good[1])
    assert not ok, f"old[0] * sa with sign {old_sign}: worst-row ratio {rw:.2f}, median ratio {rm:.2f} stays inside the rule"
    dead = stat_errors(fold_stats_f32(*args[:3], old_sign=old_sign), want)      # (centred on the mean the wrong kernel passes: the gap)
    assert np.array_equal(dead[1], stat_errors(fold_stats_f32(*args[:3]), want)[1])


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("N", [0, 17])
def test_the_new_mean_without_the_old_offset_breaks_the_rule(stream, N):
    args, want, good = _stat_case(stream, N, True)
    bad = stat_errors(fold_stats_f32(*args, mean_old=False), want)
    ok, rw, rm = rule(bad[0], good[0])
    assert not ok, f"mean without old[0]: worst-row ratio {rw:.2f}, median ratio {rm:.2f} stays inside the rule"
