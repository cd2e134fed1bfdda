"""What the DETR attention kernel (hoigen_amd/csrc/hg_detr_attn.hip: head dim 32, separate query and key lengths, a key padding mask)
is held to: tests/attention_bound.py restated.  An exact float64 softmax(q k^T / sqrt(32) + mask) v of the fp16-rounded inputs on the
CPU and a bound PER OUTPUT ELEMENT, the sum of the worst case of each fp16 rounding the kernel performs (they are tile_softmax_pv's).
A plain module beside the tests: no fixtures, no GPU, no library.

For the output element (query i, head, channel d), over the keys j that the mask leaves visible, with s_j = q_i . k_j / sqrt(32) and p
the normalised softmax:

    want = sum_j p_j v_jd          pav = sum_j p_j |v_jd|          Z = sum_j exp(s_j - max_j s)  (>= 1)          vsum = sum_j |v_jd|

    B = 2^-11 |want|          the output is rounded to fp16
      + 2^-11 pav             every probability is rounded to fp16; the row sum is fp32 of the UNROUNDED exponentials
      + 2^-25 vsum / Z        a probability below 2^-14 of the running maximum's is an fp16 subnormal: half of 2^-24 per key

Rule: every element of a sequence that has a visible key has |got - want| <= B; every element of a sequence WITHOUT a visible key is
NaN (what nn.MultiheadAttention gives: tests/test_detr_attn_rounding_model.py checks that on the CPU).  What the bound does not
carry is fp32 (scores over 32 exact products, v_exp_f32, the rescale, the P V accumulation over up to 1 792 keys, the division).

`model()` is the CPU restatement of the kernel's loop: 32-key tiles in order, a tile without a visible key skipped, masked keys at
-inf before the maximum, a running maximum that starts at -1e30 with rescale, P = fp16(exp2((s - m) c)), the row sum in fp32 from the
unrounded exponentials, O += P V in fp32 with the V rows behind Lk read as zeros, one fp16 rounding of the output - with the mutants
that tests/test_detr_attn_rounding_model.py proves the bound rejects.

Input families (`make_qkv`): those of tests/attention_bound.py with u a random unit vector of R^32 per (sequence, head).
Masks (`make_mask`; uint8 [n_seq, Lk], 1 = padded key):

    none       no mask
    rect       the keys are a flattened h x w grid, visible on the top-left vh x vw rectangle (right and bottom padding): periodic runs
    first / middle / last     one visible key
    head64     the first min(64, Lk - 1) keys masked: the first tiles met are fully masked while the running maximum is still -1e30
    midrun     a masked run in the middle that covers whole 32-key tiles where Lk allows
    perseq     sequence n takes kind n of (rect, head64, midrun, none, last, ...): different masks per sequence

Worst |err| / B per family over all masks as tests/test_gpu_detr_attention.py prints it (lines starting DETR_ATTN_RATIO) on an
MI355X (small: Lq = Lk in 1, 2, 31, 32, 33, 63, 64, 65, 97, 221, 3 sequences x 2 heads, every mask; large: 950, 1 280, 1 281, 1 444,
1 764, 1 792, 1 x 2, the rectangle and one more mask a length; cross: (Lq, Lk) = (1, 97), (33, 221), (100, 950), (100, 1 444)), beside
`model()` at the shapes of tests/test_detr_attn_rounding_model.py ((33, 33), (1, 97), (33, 221), (70, 130), every mask):

    family     model      kernel, small      kernel, large      kernel, cross
    randn      0.627      0.662              0.529              0.554
    sink       0.448      0.474              0.492              0.472
    ramp       0.818      0.871              0.590              0.810
    uniform    0.286      0.289              0.285              0.286
    voffset    0.441      0.463              0.403              0.405
    onehot     0.482      0.537              0.199              0.353

The kernel lands where the restatement lands (cross (33, 221) is the model's own shape: 0.554 and 0.810 to the digit).
"""
import numpy as np
import torch

FAMILIES = ("randn", "sink", "ramp", "uniform", "voffset", "onehot")
MASKS = ("none", "rect", "first", "middle", "last", "head64", "midrun", "perseq")
MUTANTS = ("scale", "mask_ignored", "mask_shift", "mask_neighbour", "masked_tile_nan", "drop_last", "flush", "pad_v_nan")
HD = 32
SCALE = 32.0 ** -0.5


def seed_of(family, Lq, Lk, mask="none", n_seq=0, heads=0):
    return (((FAMILIES.index(family) * 1009 + Lk) * 2003 + Lq) * 16 + MASKS.index(mask)) * 64 + n_seq * 8 + heads


def jstar(Lk):
    """the key the `onehot` family puts all the weight on"""
    return Lk // 2


def make_qkv(family, n_seq, Lq, Lk, heads, seed):
    """q [n_seq * Lq, heads * 32], k, v [n_seq * Lk, heads * 32] float32 on the CPU, every value an fp16 number"""
    g = torch.Generator().manual_seed(int(seed))

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    q, k, v = rn(n_seq, heads, Lq, HD), rn(n_seq, heads, Lk, HD), rn(n_seq, heads, Lk, HD)
    u = rn(n_seq, heads, 1, HD)
    u = u / u.norm(dim=-1, keepdim=True)
    if family in ("randn", "voffset"):
        q, k = 1.5 * q, 1.5 * k
        v = 1.5 * v if family == "randn" else 7.0 + 0.05 * v
    elif family == "sink":
        q, k = 0.5 * q + 8.0 * u, 0.5 * k
        k[:, :, 0] += 12.0 * u[:, :, 0]
        v = 1.5 * v
    elif family == "ramp":
        t = torch.linspace(-60.0, 60.0, Lk, dtype=torch.float64) if Lk > 1 else torch.zeros(1, dtype=torch.float64)
        q, k = 0.3 * q + 8.0 * u, 0.3 * k + t[None, None, :, None] * u
        v = 1.5 * v
    elif family == "uniform":
        q, k, v = 0.0 * q, 1.5 * k, 7.0 + 0.05 * v
    else:
        assert family == "onehot", family
        q, k = 0.2 * q + 16.0 * u, 0.2 * k
        k[:, :, jstar(Lk)] = 40.0 * u[:, :, 0]
        v = 1.5 * v

    def rows(t, L):
        return t.permute(0, 2, 1, 3).reshape(n_seq * L, heads * HD).half().float().contiguous()

    return rows(q, Lq), rows(k, Lk), rows(v, Lk)


def _one_mask(kind, Lk, n):
    """uint8 [Lk] of one sequence (n: its index, which varies the rectangle)"""
    m = np.zeros(Lk, np.uint8)
    if kind == "none":
        return m
    if kind == "rect":
        w = max(1, int(np.ceil(np.sqrt(Lk))))
        h = (Lk + w - 1) // w
        vw, vh = max(1, (w * (3 + n % 3)) // 6), max(1, (h * (5 - n % 2)) // 6)
        j = np.arange(Lk)
        m[(j % w >= vw) | (j // w >= vh)] = 1
        m[0] = 0
        return m
    if kind in ("first", "middle", "last"):
        m[:] = 1
        m[{"first": 0, "middle": Lk // 2, "last": Lk - 1}[kind]] = 0
        return m
    if kind == "head64":
        m[:min(64, Lk - 1)] = 1
        return m
    assert kind == "midrun", kind
    if Lk >= 160:
        a = (Lk // 3) // 32 * 32 - 5          # starts 5 keys before a tile, covers two whole tiles, ends 3 keys into the next
        m[a:a + 5 + 64 + 3] = 1
    else:
        m[Lk // 3:max(Lk // 3 + 1, 2 * Lk // 3)] = 1
        if m.all():
            m[0] = 0
    return m


PERSEQ = ("rect", "head64", "midrun", "none", "last", "first")


def make_mask(kind, n_seq, Lk):
    """uint8 [n_seq, Lk] torch tensor, or None for `none`; every sequence keeps a visible key"""
    if kind == "none":
        return None
    rowsm = [_one_mask(PERSEQ[n % len(PERSEQ)] if kind == "perseq" else kind, Lk, n) for n in range(n_seq)]
    return torch.from_numpy(np.stack(rowsm))


def split(t, n_seq, L, heads):
    """[n_seq * L, heads * 32] -> [n_seq, heads, L, 32] float64 of the fp16-rounded values"""
    return t.detach().cpu().half().double().view(n_seq, L, heads, HD).permute(0, 2, 1, 3).contiguous()


def rows(t, n_seq, L, heads):
    """[n_seq, heads, L, 32] -> [n_seq * L, heads * 32], the kernel's output layout"""
    return t.permute(0, 2, 1, 3).reshape(n_seq * L, heads * HD)


def reference(q, k, v, mask, n_seq, Lq, Lk, heads):
    """float64 on the CPU: dict of want, pav, Z, vsum, B - each [n_seq * Lq, heads * 32] - and `dead` [n_seq] bool: the sequences without
    a visible key (their rows of want are NaN)"""
    vis = torch.ones(n_seq, Lk, dtype=torch.bool) if mask is None else ~mask.bool().cpu()
    q64, k64, v64 = split(q, n_seq, Lq, heads), split(k, n_seq, Lk, heads), split(v, n_seq, Lk, heads)
    parts = {"want": [], "pav": [], "Z": [], "vsum": []}
    for n in range(n_seq):
        s = (q64[n] @ k64[n].transpose(-1, -2) * SCALE).masked_fill(~vis[n][None, None, :], float("-inf"))
        e = torch.exp(s - s.max(-1, keepdim=True).values)          # NaN throughout for a sequence without a visible key
        Z = e.sum(-1, keepdim=True)
        p = e / Z
        vsum = (vis[n].double()[None, :] @ v64[n].abs()).expand(-1, Lq, -1)
        for name, t in (("want", p @ v64[n]), ("pav", p @ v64[n].abs()), ("Z", Z.expand(-1, -1, HD)), ("vsum", vsum)):
            parts[name].append(rows(t[None], 1, Lq, heads))
    out = {name: torch.cat(ts, 0) for name, ts in parts.items()}
    out["B"] = bound(out)
    out["dead"] = ~vis.any(1)
    out["n_seq"], out["Lq"] = n_seq, Lq
    return out


def bound(ref):
    return 2.0 ** -11 * ref["want"].abs() + 2.0 ** -11 * ref["pav"] + 2.0 ** -25 * ref["vsum"] / ref["Z"]


def ratio(got, ref):
    """|got - want| / B per element of the sequences that have a visible key (0 / 0 counts as 0, x / 0 and a non-finite got as inf);
    the rows of the others are 0 where got is NaN and inf where it is not"""
    g = got.detach().cpu().double()
    err = (g - ref["want"]).abs()
    r = err / ref["B"]
    r = torch.where(err == 0, torch.zeros_like(r), r)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    dead = ref["dead"].repeat_interleave(ref["Lq"])[:, None].expand_as(r)
    return torch.where(dead, torch.where(torch.isnan(g), torch.zeros_like(r), torch.full_like(r, float("inf"))), r)


def worst(got, ref):
    return float(ratio(got, ref).max())


def onehot_exact_rows(got, v, mask, n_seq, Lq, Lk, heads):
    """`onehot` with key j* visible: every row must be fp16(v[j*]) bit for bit.  (mismatching elements, elements checked)"""
    j = jstar(Lk)
    v64 = split(v, n_seq, Lk, heads)
    want = rows(v64[:, :, j:j + 1].expand(-1, -1, Lq, -1), n_seq, Lq, heads).view(n_seq, Lq, -1)
    g = got.detach().cpu().double().view(n_seq, Lq, -1)
    seqs = [n for n in range(n_seq) if mask is None or not bool(mask[n, j])]
    return int(sum((g[n] != want[n]).sum() for n in seqs)), sum(g[n].numel() for n in seqs)


# ---- the CPU restatement of the kernel's loop -------------------------------------------------------------------------------------
C_LOG2E = torch.tensor(np.float32(0.17677669529663689) * np.float32(1.4426950408889634))          # the kernel's c, as fp32


def model(q, k, v, mask, n_seq, Lq, Lk, heads, mutant=None):
    """The kernel's arithmetic on the CPU, [n_seq * Lq, heads * 32] float64 holding fp16 values.  mutant: one of MUTANTS -
      scale            the softmax scale is 1 / 8 (head dim 64's)
      mask_ignored     no key is masked but those behind Lk
      mask_shift       key j takes the mask byte of key j + 1 (the last key its own)
      mask_neighbour   sequence n takes the mask row of sequence n + 1 (the last one the first's)
      masked_tile_nan  the running maximum starts at -inf and a tile without a visible key is not skipped: exp2(-inf - -inf)
      drop_last        the last tile is dropped when it is partial (Lk % 32 != 0)
      flush            probabilities below the smallest normal fp16 number become zero
      pad_v_nan        the V rows behind Lk hold NaN and are not read as zeros"""
    assert mutant is None or mutant in MUTANTS, mutant
    qf, kf, vf = (split(t, n_seq, L, heads).float() for t, L in ((q, Lq), (k, Lk), (v, Lk)))
    nkt = (Lk + 31) // 32
    pad = nkt * 32 - Lk
    msk = torch.zeros(n_seq, Lk, dtype=torch.bool) if mask is None or mutant == "mask_ignored" else mask.bool().cpu().clone()
    if mutant == "mask_shift":
        msk = torch.cat([msk[:, 1:], msk[:, -1:]], 1)
    if mutant == "mask_neighbour":
        msk = torch.roll(msk, -1, 0)
    msk = torch.cat([msk, torch.ones(n_seq, pad, dtype=torch.bool)], 1)
    if pad:
        kf = torch.cat([kf, kf[:, :, -1:].expand(-1, -1, pad, -1)], 2)
        vf = torch.cat([vf, torch.full_like(vf[:, :, :pad], float("nan") if mutant == "pad_v_nan" else 0.0)], 2)
    c = torch.tensor(np.float32(0.125) * np.float32(1.4426950408889634)) if mutant == "scale" else C_LOG2E
    nan_mut = mutant == "masked_tile_nan"
    m = torch.full((n_seq, heads, Lq), float("-inf") if nan_mut else -1.0e30, dtype=torch.float32)
    lsum = torch.zeros(n_seq, heads, Lq, dtype=torch.float32)
    o = torch.zeros(n_seq, heads, Lq, HD, dtype=torch.float32)
    for kt in range(nkt if not (mutant == "drop_last" and pad) else nkt - 1):
        tm = msk[:, kt * 32:kt * 32 + 32]                                          # [n_seq, 32]
        live = ~tm.all(1) if not nan_mut else torch.ones(n_seq, dtype=torch.bool)  # a tile without a visible key is skipped
        s = qf @ kf[:, :, kt * 32:kt * 32 + 32].transpose(-1, -2)                  # fp32 [n, h, Lq, 32]
        s = s.masked_fill(tm[:, None, None, :], float("-inf"))
        mn = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp2(((m - mn) * c).double()).float()
        mc = mn * c
        e = torch.exp2((s.double() * c.double() - mc.double()[..., None]).float().double()).float()      # v_exp_f32 of one fma
        p = e.half()
        if mutant == "flush":
            p = torch.where(p < 2.0 ** -14, torch.zeros_like(p), p)
        vt = vf[:, :, kt * 32:kt * 32 + 32]
        if mutant == "pad_v_nan" and pad and kt == nkt - 1:
            pv = (p.float()[..., None] * vt[:, :, None, :, :]).sum(-2)              # 0 * NaN stays NaN, as an MFMA has it
        else:
            pv = p.float() @ vt
        lv = live[:, None, None]
        m = torch.where(lv, mn, m)
        lsum = torch.where(lv, lsum * alpha + e.sum(-1), lsum)
        o = torch.where(lv[..., None], o * alpha[..., None] + pv, o)
    inv = 1.0 / lsum
    return rows((o * inv[..., None]).half().double(), n_seq, Lq, heads)


def alive(mutant, mask, n_seq, Lk):
    """whether the mutant changes anything for this mask and key length"""
    mk = torch.zeros(n_seq, Lk, dtype=torch.bool) if mask is None else mask.bool()
    if mutant == "scale":
        return int((~mk).sum(1).max()) >= 2
    if mutant == "mask_ignored":
        return bool(mk.any())
    if mutant == "mask_shift":
        return bool((mk[:, 1:] != mk[:, :-1]).any())
    if mutant == "mask_neighbour":
        return bool((torch.roll(mk, -1, 0) != mk).any())
    if mutant == "masked_tile_nan":      # a whole masked tile BEFORE the first visible key (behind one the maximum is finite already)
        pad = (-Lk) % 32
        t = torch.cat([mk, torch.ones(n_seq, pad, dtype=torch.bool)], 1).view(n_seq, -1, 32).all(2)
        return bool(t[:, 0].any())
    if mutant in ("drop_last", "pad_v_nan"):      # a partial last tile that is walked: it has a visible key
        return Lk % 32 != 0 and bool((~mk[:, Lk // 32 * 32:]).any())
    return True
