"""What the fused in_proj + attention kernels (qkv_attn_kernel, qkv_attn_kernel_k1 in hg_qkv_attn.hip; qkv_attn_kernel_text,
qkv_attn_kernel_text_k2 in hg_qkv_attn_text.hip) are held to: the bounds of tests/gemm_bound.py (`gb`, epilogue 8) and
tests/attention_bound.py (`ab`), chained, PER OUTPUT ELEMENT.  A plain module beside the tests (tests/test_qkv_attn_rounding_model.py,
tests/test_gpu_qkv_attn_bound.py import it): no fixtures, no GPU, no library.  Neither bound is copied or loosened here.

A case is (a [M, K], w [3D, K], bias [3D], cs [3D], mr [M, 2]) with M = n_seq L, D = 64 heads, K = D or D + 64; a and w fp16 numbers,
cs the fp32 column sums of w, mr = (mean, rstd); and the mask: none (vision, 192 < L <= 208) or causal (text, L <= 80).

    stage P    qkv64 = rstd (a w^T - mean cs) + bias in float64, with gb's epilogue-8 bound B_P per element
    stage A    ab.reference(qkv16) = want and B_A per output element, qkv16 = the fp16 q | k | v the attention actually consumed

B_A is ab's bound with one term counted that ab leaves out: its first term, 2^-11 |want| for the fp16 rounding of the output, holds for
a normal fp16 result; below 2^-14 fp16 is subnormal with the absolute step 2^-24, so the rounding is worth up to 2^-25 whatever |want|
is (gb.f16_term counts the same for every fp16 GEMM output):

    B_A = ab's B - 2^-11 |want| + max(2^-11 |want|, 2^-25)

It was found by these tests, not fitted: `sel_sink`, causal, L = 59, heads 8, sequence 1, query 1, head 7, channel 56 has key 0 at
probability 1 - 3e-6 and v_0 = -7.8e-6 there; want = -7.769e-6, kernel and `model()` both return -7.808e-6, the nearest fp16
subnormal, 3.96e-8 off - 2.02 of ab's B (1.96e-8), 0.87 of B_A (4.56e-8).  ab's own families (1.5 randn or 7 + 0.05 randn in v) put no output
there often enough to have met it.

Rule: every output element has |got - want| <= B_A.  No global scale, no row norm, no element left out.  The fused kernels do not emit
qkv16, so it comes from one of two places, and never from the fused kernel:

    `select` families    it is known a priori, bit for bit (below): B_A alone judges the kernel - the only judge for heads = 6, where
                         3 D is no multiple of 256 and the two launches do not exist
    dense families       it is what the folded GEMM alone returned on the same operands (qkv_out of hg_test_qkv_attn_ex), itself held to
                         |qkv16 - qkv64| <= B_P in the same test; with torch.equal(fused, two launches) that closes the chain

Families (`make_case`; seeded, generated on the CPU):

    sel_*      every row of w has ONE non-zero, a signed power of two: q of head h selects the 64-column block h of a, k block
               (h + 1) % nb, v block (h + 2) % nb, nb = K / 64 - with K = D + 64 the extra block takes part in the rotation, so the last
               K-tile matters.  The signs are per (head, channel), the same for q and k (the scores do not see them), others for v.  rstd
               is 0.5, 1 or 2 per row, mean = 0, bias = 0 but for a constant 7 on the v columns of `uniform` / `voffset`.  Every fp32
               operation of the projection is then exact in any order (`select_is_exact` asserts it: fp32 in two K orders = float64,
               bit for bit) and qkv16 = fp16(qkv64), where the only rounding is that of 7 + small.  The rows of a are built in token
               space, a_i = fp16(x_i / rstd_i) with block b of x_i = noise randn + alpha_i u, one unit vector u of R^64 per sequence:
               the rotated blocks give ab's six attention patterns -
                 sel_randn     noise 1.5
                 sel_sink      alpha = 8, alpha_0 = 20, noise 0.5: key 0 stands 12 above the rest
                 sel_ramp      alpha linear from -60 to 60, noise 0.3, q rows of w 2^-3: the running maximum moves, scores reach +-56
                 sel_onehot    alpha = 16, alpha_{L // 2} = 40, noise 0.2: every other probability rounds to zero in fp16
                 sel_uniform   noise 1.5, q rows of w zero, v = 7 + 2^-5 x block (a on the grid 2^-9, so that 7 + small is exact in fp32)
                 sel_voffset   as sel_randn with that v
    randn, outlier, cancel, lnfold      gb's operands of those names at N = 3 D (gb.make_case; mean 0.02 randn in two thirds of the rows
               and 3 randn in the rest for lnfold).  Two changes: lnfold draws rstd log-uniform in [0.25, 4] (gb's 300 would push the
               scores to 1e5, where the fp32 rounding of a score dominates - a term B_A deliberately does not carry), and the q rows
               of w and of bias are scaled by a power of two so that the float64 reference's largest visible |score| is at most 64, the
               reach of ab's ramp (`score_cap` measures it).

`model(case, mutant)` is gb.model (epilogue 8) followed by ab.model's tile loop with the tile geometry of the fused kernels: keys
L .. 32 ceil(L / 32) - 1 of a sequence are the rows that follow it in its tile - a 208-row tile per sequence (vision) or the 160-row
pack of floor(160 / L) sequences (text) - that is a neighbour's rows, or the projection of a zero pad row behind the last sequence;
they are masked and their V rows read as zeros.  On finite data it equals ab.model of gb.model bit for bit.  Mutants, beside gb's
rstd_after_bias:

    neighbour_key       key L passes the mask (zero V row behind it): every query without the causal mask, query L - 1 with it
    neighbour_v         masked keys keep the neighbour's projected V row instead of zeros: dead on finite data (0 x v), a non-finite
                        neighbour poisons the sequence
    mr_by_tile_row      sequence g >= 1 of a pack takes (mean, rstd) from the rows shifted by one (text only: a vision tile holds one)
    bcs_heads_swapped   bias' and cs of head b of a pair are applied to head a
    k_wrong_head        k of head h + 1 is used for head h
    drop_e_columns      the K = D + 64 instance ignores its last K-tile
    mean_uncentred      the copy is taken as centred on the row mean: mr[:, 0] read as zero

Worst |err| / B_A over all elements: `model()` at the shapes of tests/test_qkv_attn_rounding_model.py (vision: L = 193, 197, 208,
heads 6 and 12, K = D and D + 64, 3 sequences; text: L = 1, 13, 33, 77, 80, heads 8 and 12, 2 floor(160 / L) + 1 sequences), and the
kernels as tests/test_gpu_qkv_attn_bound.py prints it (lines starting QKV_ATTN_RATIO) on an MI355X - sel_*: every L = 193 .. 208
(vision), every L = 1 .. 80 (text_k2, heads 8), twelve lengths (text, heads 12); dense: the lengths listed there.

                 model()                             kernels on an MI355X (heads)
    family       vision  vision_k1  text_k2  text    vision (6)  vision_k1 (6)  vision (12)  vision_k1 (12)  text_k2 (8)  text (12)
    sel_randn    0.625   0.659      0.846    0.796   0.705       0.702          0.801        0.810           0.904        0.827
    sel_sink     0.499   0.498      0.498    0.499   0.499       0.499          0.499        0.499           0.868        0.499
    sel_ramp     0.713   0.708      0.747    0.791   0.681       0.707          0.757        0.757           0.847        0.791
    sel_onehot   0       0          0.756    0.758   0           0              0            0               0.858        0.746
    sel_uniform  0.286   0.286      0.292    0.291   0.286       0.286          0.286        0.286           0.292        0.292
    sel_voffset  0.431   0.427      0.482    0.507   0.430       0.427          0.432        0.446           0.507        0.496
    randn        0.786   0.719      0.807    0.816   -           -              0.786        0.718           0.807        0.837
    outlier      0.729   0.735      0.790    0.834   -           -              0.798        0.735           0.776        0.834
    cancel       0.532   0.526      0.658    0.665   -           -              0.523        0.529           0.674        0.699
    lnfold       0.696   0.712      0.778    0.848   -           -              0.794        0.712           0.797        0.786

Stage P, worst |qkv16 - qkv64| / B_P: model() randn 0.757, outlier 0.873, cancel 0.315, lnfold 0.932; the folded GEMM on the device
(vision / vision_k1 / text_k2 / text operands) randn 0.549 / 0.559 / 0.678 / 0.555, outlier 0.760 / 0.740 / 0.842 / 0.755, cancel
0.145 / 0.128 / 0.236 / 0.137, lnfold 0.862 / 0.882 / 0.914 / 0.854.

No entry is above 1.  The kernels run more lengths than the model's columns, so their maxima are higher where the worst length is
not one of the model's (text_k2 `sel_randn`: 0.904; `sel_sink` 0.868 is the subnormal output of L = 59 above - every other length
of it stays at 0.499, the rounding of a single probability near 1); where the shapes coincide (`sel_uniform`, `sel_sink`, the dense
families at heads 12) kernel and model agree to two or three digits, as in tests/attention_bound.py.  On every sel_* case at heads 8 and
12 the folded GEMM returned the a-priori qkv16 bit for bit, and on every case with a two-launch counterpart the fused kernel equals it
bit for bit.  The dense rows at vision (12) and text_k2 (8) include the runs with 264 and 260 work items.
"""
import functools
import math

import torch

import attention_bound as ab
import gemm_bound as gb

SELECT = ("sel_randn", "sel_sink", "sel_ramp", "sel_onehot", "sel_uniform", "sel_voffset")
DENSE = ("randn", "outlier", "cancel", "lnfold")
FAMILIES = SELECT + DENSE
MUTANTS = ("neighbour_key", "neighbour_v", "mr_by_tile_row", "bcs_heads_swapped", "k_wrong_head", "drop_e_columns", "rstd_after_bias",
           "mean_uncentred")
HD = 64
VISION_TILE, TEXT_TILE = 208, 160
SCORE_CAP = 64.0


def tile_rows(causal):
    return TEXT_TILE if causal else VISION_TILE


def pack_size(L, causal):
    """sequences per work item"""
    return TEXT_TILE // L if causal else 1


def instance(heads, K, causal):
    """the kernel instance that runs this shape"""
    if causal:
        return "text" if (K // 64) % 3 == 0 else "text_k2"
    return "vision" if (K // 64) % 3 == 0 else "vision_k1"


def seed_of(family, n_seq, L, heads, extra, causal):
    return ((((FAMILIES.index(family) * 211 + L) * 1013 + n_seq) * 17 + heads) * 2 + int(bool(extra))) * 2 + int(bool(causal))


# ---- the `select` families ---------------------------------------------------------------------------------------------------------
def _select(family, n_seq, L, heads, extra, causal):
    D, K, M = heads * HD, heads * HD + extra, n_seq * L
    nb = K // HD
    g = torch.Generator().manual_seed(seed_of(family, n_seq, L, heads, extra, causal))

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    sub = family[4:]
    noise = {"randn": 1.5, "sink": 0.5, "ramp": 0.3, "onehot": 0.2, "uniform": 1.5, "voffset": 1.5}[sub]
    alpha = torch.zeros(L, dtype=torch.float64)
    if sub == "sink":
        alpha[:] = 8.0
        alpha[0] = 20.0
    elif sub == "ramp" and L > 1:
        alpha = torch.linspace(-60.0, 60.0, L, dtype=torch.float64)
    elif sub == "onehot":
        alpha[:] = 16.0
        alpha[ab.jstar(L)] = 40.0
    u = rn(n_seq, 1, 1, HD)
    u = u / u.norm(dim=-1, keepdim=True)
    x = noise * rn(n_seq, L, nb, HD) + alpha[None, :, None, None] * u
    rstd = 2.0 ** torch.randint(-1, 2, (M,), generator=g).double()
    a = (x.reshape(M, K) / rstd[:, None]).half().double()
    offset = sub in ("uniform", "voffset")
    if offset:
        a = (torch.round(a * 512.0) / 512.0).half().double()
    sign_qk = 2.0 * torch.randint(0, 2, (heads, HD), generator=g).double() - 1.0
    sign_v = 2.0 * torch.randint(0, 2, (heads, HD), generator=g).double() - 1.0
    mag = (0.0 if sub == "uniform" else 0.125 if sub == "ramp" else 1.0, 1.0, 2.0 ** -5 if offset else 1.0)
    val = torch.stack([mag[0] * sign_qk, mag[1] * sign_qk, mag[2] * sign_v], 0)                  # [3, heads, 64]
    col = ((torch.arange(heads)[None, :, None] + torch.arange(3)[:, None, None]) % nb) * HD + torch.arange(HD)[None, None, :]
    w = torch.zeros(3 * D, K, dtype=torch.float64)
    w[torch.arange(3 * D), col.reshape(-1)] = val.reshape(-1)
    bias = torch.zeros(3, heads, HD, dtype=torch.float64)
    if offset:
        bias[2] = 7.0
    bias = bias.reshape(-1)
    qkv64 = rstd[:, None] * (a[:, col.reshape(-1)] * val.reshape(-1)[None]) + bias[None]
    mr = torch.stack([torch.zeros(M, dtype=torch.float64), rstd], 1)
    return {"family": family, "a": a.float(), "w": w.float(), "bias": bias.float(), "cs": w.sum(1).float(), "mr": mr.float().contiguous(),
            "qkv64": qkv64, "qkv16": qkv64.half().float()}


def select_is_exact(c):
    """The a-priori qkv16 of a `select` case rests on this: the projection in fp32, K-tiles summed forwards and backwards, equals the
    float64 matmul bit for bit, and both equal the gathered qkv64 of the case."""
    a, w, K = c["a"], c["w"], c["K"]
    mean, rstd = c["mr"][:, :1], c["mr"][:, 1:]
    tiles = list(range(0, K, 64))
    got = []
    for order in (tiles, tiles[::-1]):
        acc = torch.zeros(c["M"], 3 * c["D"], dtype=torch.float32)
        for k0 in order:
            acc = acc + a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
        got.append((acc - c["cs"][None] * mean) * rstd + c["bias"][None])
    want = (a.double() @ w.double().t() - c["cs"].double()[None] * mean.double()) * rstd.double() + c["bias"].double()[None]
    return bool((got[0].double() == want).all() and (got[1].double() == want).all() and (want == c["qkv64"]).all())


# ---- the dense families --------------------------------------------------------------------------------------------------------------
def _visible(L, causal):
    vis = torch.ones(L, L, dtype=torch.bool)
    return vis.tril() if causal else vis


def score_cap(qkv, n_seq, L, heads, causal):
    """largest visible |q . k / 8| of a q | k | v matrix [M, 3D], float64"""
    x = qkv.detach().cpu().double().view(n_seq, L, 3, heads, HD)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)
    s = (q @ k.transpose(-1, -2) * 0.125).abs().masked_fill(~_visible(L, causal), 0.0)
    return float(s.max())


def _dense(family, n_seq, L, heads, extra, causal):
    D, K, M = heads * HD, heads * HD + extra, n_seq * L
    c0 = gb.make_case(family, M, 3 * D, K)
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c0.items()}
    if family == "lnfold":
        g = torch.Generator().manual_seed(seed_of(family, n_seq, L, heads, extra, causal))
        rstd = torch.exp(math.log(0.25) + (math.log(4.0) - math.log(0.25)) * torch.rand(M, generator=g, dtype=torch.float64))
        c["mr"][:, 1] = rstd.float()
    top = score_cap(gb.reference(c, 8)[0], n_seq, L, heads, causal)
    e = max(0, math.ceil(math.log2(top / SCORE_CAP))) if top > 0 else 0
    if e:
        c["w"][:D] = (c["w"][:D] * 2.0 ** -e).half().float()
        c["bias"][:D] *= 2.0 ** -e
        a64, w64 = c["a"].double(), c["w"][:D].double()
        c["acc"][:, :D], c["S"][:, :D], c["cs64"][:D] = a64 @ w64.t(), a64.abs() @ w64.abs().t(), w64.sum(1)
        c["cs"] = c["cs64"].float()
    c["qkv64"], c["B_P"] = gb.reference(c, 8)
    c["q_shift"] = e
    return c


@functools.lru_cache(maxsize=4)
def make_case(family, n_seq, L, heads, extra=0, causal=False):
    """One case, float32 on the CPU (a, w fp16 numbers): a [M, K], w [3D, K], bias, cs [3D], mr [M, 2]; qkv64 [M, 3D] float64; for the
    sel_* families qkv16 [M, 3D]; for the dense ones gb's acc, S, cs64 and B_P [M, 3D].  Cached and shared: leave it unchanged."""
    assert family in FAMILIES and extra in (0, 64), (family, extra)
    c = (_select if family in SELECT else _dense)(family, n_seq, L, heads, extra, causal)
    D = heads * HD
    c.update(family=family, n_seq=n_seq, L=L, heads=heads, D=D, K=D + extra, M=n_seq * L, N=3 * D, causal=bool(causal))
    return c


def poisoned(c, poison=float("nan")):
    """the case with every odd sequence non-finite (NaN: with Inf in every other column, both kinds in one row)"""
    a = c["a"].clone().view(c["n_seq"], c["L"], c["K"])
    a[1::2] = poison
    if poison != poison:
        a[1::2, :, ::2] = float("inf")
    return dict(c, a=a.view(c["M"], c["K"]))


def stage_p_ratio(qkv16, c):
    """worst |qkv16 - qkv64| / B_P of a dense case"""
    return gb._worst(qkv16, c["qkv64"], c["B_P"])


def reference(c, qkv16):
    """ab.reference of the q | k | v the attention consumed, under the case's mask; B with the subnormal-output term of the module
    docstring (ab's own bound stays in B_ab)"""
    ref = ab.reference(qkv16, c["n_seq"], c["L"], c["heads"], c["causal"])
    ref["B_ab"] = ref["B"]
    ref["B"] = ref["B"] + (2.0 ** -25 - 2.0 ** -11 * ref["want"].abs()).clamp_min(0.0)
    return ref


# ---- the CPU restatement ---------------------------------------------------------------------------------------------------------------
def project(c, mutant=None):
    """gb.model, epilogue 8, on the case -> qkv16 [M, 3D] float32 holding fp16 values"""
    n_seq, L, heads, D, K, M = c["n_seq"], c["L"], c["heads"], c["D"], c["K"], c["M"]
    p = dict(c)
    p.setdefault("x0", torch.zeros(1, 3 * D))
    if mutant == "drop_e_columns" and K > D:
        p["a"] = c["a"].clone()
        p["a"][:, D:] = 0.0
    if mutant == "mean_uncentred":
        p["mr"] = c["mr"].clone()
        p["mr"][:, 0] = 0.0
    if mutant == "mr_by_tile_row":
        G = pack_size(L, c["causal"])
        src = torch.arange(M)
        later = (src // L) % G >= 1
        src = torch.where(later, (src + 1).clamp_max(M - 1), src)
        p["mr"] = c["mr"][src].contiguous()
    if mutant == "bcs_heads_swapped":
        h = torch.arange(heads)
        h = torch.where(h % 2 == 0, h + 1, h)                                       # head a of a pair reads head b's
        src = (torch.arange(3)[:, None, None] * D + h[None, :, None] * HD + torch.arange(HD)[None, None, :]).reshape(-1)
        p["bias"], p["cs"] = c["bias"][src], c["cs"][src]
    return gb.model(p, 8, "rstd_after_bias" if mutant == "rstd_after_bias" else None)["out"]


def attend(qkv16, c, mutant=None):
    """ab.model's tile loop with the fused kernels' geometry: [M, D] float64 holding fp16 values"""
    n_seq, L, heads, D, M, causal = c["n_seq"], c["L"], c["heads"], c["D"], c["M"], c["causal"]
    q, k, v = (t.float() for t in ab.split(qkv16, n_seq, L, heads))
    if mutant == "k_wrong_head":
        k = torch.roll(k, -1, 1)
    nkt = (L + 31) // 32 + (1 if mutant == "neighbour_key" and L % 32 == 0 else 0)
    pad = nkt * 32 - L
    seq = torch.arange(n_seq)
    room = tile_rows(causal) - ((seq % pack_size(L, causal)) + 1) * L              # rows of the tile behind each sequence
    if pad:
        # the rows behind a sequence: the next sequences', then the projection of a zero pad row with mr = 0, which is bias'
        behind = torch.cat([qkv16.detach().cpu().float(), c["bias"].half().float()[None].expand(pad, -1)], 0)
        idx = ((seq + 1) * L)[:, None] + torch.arange(pad)[None, :]
        there = (torch.arange(pad)[None, :] < room[:, None])[:, None, :, None]      # beyond the tile: not the operands' rows at all
        nb = behind[idx.clamp_max(M + pad - 1)].view(n_seq, pad, 3, heads, HD).permute(2, 0, 3, 1, 4)
        kn = torch.where(there, nb[1], torch.zeros_like(nb[1]))
        if mutant == "k_wrong_head":
            kn = torch.roll(kn, -1, 1)
        vn = torch.where(there, nb[2], torch.zeros_like(nb[2])) if mutant == "neighbour_v" else torch.zeros_like(nb[2])
        k, v = torch.cat([k, kn], 2), torch.cat([v, vn], 2)
    cc = ab.C_LOG2E_8
    qi = torch.arange(L)[:, None]
    m = torch.full((n_seq, heads, L), -1.0e30, dtype=torch.float32)
    lsum = torch.zeros(n_seq, heads, L, dtype=torch.float32)
    o = torch.zeros(n_seq, heads, L, HD, dtype=torch.float32)
    for kt in range(nkt):
        key = torch.arange(kt * 32, kt * 32 + 32)[None, :]
        ok = (key < L).expand(L, 32)
        if causal:
            ok = ok & (key <= qi)
        ok = ok[None, None].expand(n_seq, 1, L, 32)
        if mutant == "neighbour_key":
            extra = (key == L) & ((qi == L - 1) if causal else (qi >= 0))
            ok = ok | (extra[None, None] & (room > 0)[:, None, None, None])
        s = q @ k[:, :, kt * 32:kt * 32 + 32].transpose(-1, -2)
        s = s.masked_fill(~ok, float("-inf"))
        mn = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp2(((m - mn) * cc).double()).float()
        m = mn
        mc = m * cc
        e = torch.exp2((s.double() * cc.double() - mc.double()[..., None]).float().double()).float()
        lsum = lsum * alpha + e.sum(-1)
        o = o * alpha[..., None] + e.half().float() @ v[:, :, kt * 32:kt * 32 + 32]
    inv = 1.0 / lsum
    return ab.rows((o * inv[..., None]).half().double(), n_seq, L, heads)


def model(c, mutant=None):
    """The fused kernels' arithmetic on the CPU: [M, D] float64 holding fp16 values.  mutant: one of MUTANTS (module docstring)."""
    assert mutant is None or mutant in MUTANTS, mutant
    return attend(project(c, mutant), c, mutant)


def alive(mutant, c, poison=False):
    """whether the mutant changes anything on this case (neighbour_v: on its poisoned form only)"""
    L, causal, n_seq = c["L"], c["causal"], c["n_seq"]
    if mutant == "neighbour_key":
        return L < tile_rows(causal)
    if mutant == "neighbour_v":
        # an even sequence with an odd one behind it inside its tile, and a key tile that reaches past L
        G = pack_size(L, causal)
        return poison and L % 32 != 0 and any(n + 1 < n_seq and (n % G + 1) * L < tile_rows(causal) for n in range(0, n_seq, 2))
    if mutant == "mr_by_tile_row":
        return pack_size(L, causal) >= 2 and n_seq >= 2
    if mutant == "drop_e_columns":
        return c["K"] > c["D"]
    if mutant in ("bcs_heads_swapped", "mean_uncentred"):
        return c["family"] in DENSE                       # sel_*: mean = 0 and the same bias' in every head
    if mutant == "rstd_after_bias":
        return c["family"] in DENSE + ("sel_uniform", "sel_voffset")      # the other sel_* have no bias
    if mutant == "k_wrong_head":
        return c["family"] != "sel_uniform" and L > 1     # q = 0, or one key: the probabilities do not see k
    return True
