"""What the attention kernels (hg_attn.hip, hg_attn_long.hip; the attention half of hg_qkv_attn.hip and hg_qkv_attn_text.hip is held to
it on hard operands of its own, and one term more for subnormal outputs, by tests/qkv_attn_bound.py) are held to: an exact float64 softmax(q k^T / 8) v of the fp16-rounded inputs, computed on the CPU, and a bound PER
OUTPUT ELEMENT that is the sum of the worst case of each fp16 rounding tile_softmax_pv (hg_attn_dev.h) performs.  A plain module beside the
tests (tests/test_attention_rounding_model.py, tests/test_gpu_attention.py, tests/test_gpu_attention_long.py import it): no fixtures, no
GPU, no library.

For the output element (query i, head, channel d), over the keys j visible to i, with s_j = q_i . k_j / 8 and p the normalised softmax:

    want = sum_j p_j v_jd          pav = sum_j p_j |v_jd|          Z = sum_j exp(s_j - max_j s)  (>= 1)          vsum = sum_j |v_jd|

    B = 2^-11 |want|          the output is rounded to fp16
      + 2^-11 pav             every probability is rounded to fp16 (relative 2^-11); the row sum is fp32 of the UNROUNDED exponentials,
                              so the roundings do not cancel in the division
      + 2^-25 vsum / Z        a probability below 2^-14 of the running maximum's is an fp16 subnormal: absolute step 2^-24, half of it
                              per key, relative to a maximum that is at most the final one

Rule: every element has |got - want| <= B.  No global scale, no row norm, no element left out.  What the bound does not carry is fp32:
the score accumulation over 64 exact products, v_exp_f32, the rescale by exp2(m_old - m_new), the P V accumulation, the division - each
relative 2^-24 or so, three orders below 2^-11 at L <= 640.

`model()` is the CPU restatement of the kernels' tile loop (32-key tiles, running maximum with rescale, P = fp16(exp2((s - m) c)), row sum
in fp32 from the unrounded exponentials, O += P V in fp32, fp16 output), vectorised over queries, with the mutants that
tests/test_attention_rounding_model.py proves the bound catches.

Input families (`make_qkv`; seeded, rounded to fp16; u = a random unit vector of R^64 per (sequence, head)):

    randn     1.5 randn for q, k, v
    sink      q = 0.5 randn + 8 u, k = 0.5 randn, k[0] += 12 u: key 0 stands about 12 above the rest for every query
    ramp      q = 0.3 randn + 8 u, k = 0.3 randn + t_j u, t linear from -60 to 60 over the keys: the running maximum moves on every
              key tile, scores reach about +-60
    uniform   q = 0, v = 7 + 0.05 randn: the output is the mean of the visible V rows
    voffset   randn scores, v = 7 + 0.05 randn
    onehot    q = 0.2 randn + 16 u, k = 0.2 randn, k[j*] = 40 u for j* = L // 2: every other probability rounds to zero in fp16

Worst |err| / B over all elements, no mask / causal mask, as tests/test_gpu_attention.py and tests/test_gpu_attention_long.py print
it (lines starting ATTN_RATIO) on an MI355X, beside `model()` on the same inputs.  resident: every L = 1 .. 224, 3 sequences x 3 heads
(L <= 32 through the packed launch; the unpacked launch of L <= 32 measures the same to the digit where the worst L is <= 32).  long:
L = 225, 240, 241, 256, 257, 272, 273, 522, 543, 544, 577, 609, 639, 640, 2 sequences x 2 heads.

    family     model, L <= 224    resident kernel    model, L >= 225    long kernel
    randn      0.758 / 0.889      0.758 / 0.889      0.636 / 0.777      0.636 / 0.777
    sink       0.500 / 0.807      0.500 / 0.807      0.496 / 0.499      0.496 / 0.499
    ramp       0.874 / 0.941      0.883 / 0.941      0.704 / 0.754      0.748 / 0.754
    uniform    0.290 / 0.292      0.290 / 0.292      0.286 / 0.290      0.286 / 0.290
    voffset    0.461 / 0.528      0.461 / 0.528      0.433 / 0.453      0.433 / 0.453
    onehot     0     / 0.834      0     / 0.834      0     / 0.733      0     / 0.733

The kernels land where the restatement lands, to the digit in all but two entries: what separates them is the order of fp32 additions
and v_exp_f32.  At the
four lengths of tests/test_attention_rounding_model.py the model stays below 0.72; over every length it reaches 0.94 (`ramp`, causal,
L = 188, query 1: two visible keys of nearly equal weight, want = 0.5073 just above a power of two, where half an fp16 ulp IS 2^-11 |want|,
and both probability roundings fall the same way) - B is a worst case that inputs can approach, not a loose envelope.  On the 1.5 randn
inputs of the earlier tests (generated on the device, their shapes kept) the kernels reach 0.84 (resident), 0.81 (packed), 0.76 (long).
"""
import numpy as np
import torch

FAMILIES = ("randn", "sink", "ramp", "uniform", "voffset", "onehot")
MUTANTS = ("scale", "unmasked_key", "unmasked_key_zero_v", "flush", "diagonal", "drop_last")
HD = 64


def seed_of(family, L, causal, n_seq=0, heads=0):
    return ((FAMILIES.index(family) * 1009 + L) * 2 + int(bool(causal))) * 64 + n_seq * 8 + heads


def jstar(L):
    """the key the `onehot` family puts all the weight on"""
    return L // 2


def make_qkv(family, n_seq, L, heads, seed):
    """qkv [n_seq * L, 3 * heads * 64] float32 on the CPU, every value an fp16 number (the layout hg_test_attention takes)"""
    g = torch.Generator().manual_seed(int(seed))

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    q, k, v = rn(n_seq, heads, L, HD), rn(n_seq, heads, L, HD), rn(n_seq, heads, L, HD)
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
        t = torch.linspace(-60.0, 60.0, L, dtype=torch.float64) if L > 1 else torch.zeros(1, dtype=torch.float64)
        q, k = 0.3 * q + 8.0 * u, 0.3 * k + t[None, None, :, None] * u
        v = 1.5 * v
    elif family == "uniform":
        q, k, v = 0.0 * q, 1.5 * k, 7.0 + 0.05 * v
    else:
        assert family == "onehot", family
        q, k = 0.2 * q + 16.0 * u, 0.2 * k
        k[:, :, jstar(L)] = 40.0 * u[:, :, 0]
        v = 1.5 * v
    x = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4)          # [n_seq, L, 3, heads, 64]
    return x.reshape(n_seq * L, 3 * heads * HD).half().float().contiguous()


def split(qkv, n_seq, L, heads):
    """q, k, v [n_seq, heads, L, 64] float64 of the fp16-rounded qkv"""
    x = qkv.detach().cpu().half().double().view(n_seq, L, 3, heads, HD)
    return tuple(x[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))


def rows(t, n_seq, L, heads):
    """[n_seq, heads, L, 64] -> [n_seq * L, heads * 64], the kernels' output layout"""
    return t.permute(0, 2, 1, 3).reshape(n_seq * L, heads * HD)


def reference(qkv, n_seq, L, heads, causal):
    """float64 on the CPU: dict of want, pav, Z, vsum, B - each [n_seq * L, heads * 64] (Z repeated over a head's channels)"""
    vis = torch.ones(L, L, dtype=torch.bool)
    if causal:
        vis = vis.tril()
    step = max(1, (1 << 24) // (heads * L * L))          # sequences per pass: the [L, L] matrices of a pass stay within 128 MiB
    parts = {"want": [], "pav": [], "Z": [], "vsum": []}
    for n0 in range(0, n_seq, step):
        n = min(step, n_seq - n0)
        q, k, v = split(qkv.view(n_seq, L, -1)[n0:n0 + n], n, L, heads)
        s = (q @ k.transpose(-1, -2) * 0.125).masked_fill(~vis, float("-inf"))
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        Z = e.sum(-1, keepdim=True)
        p = e / Z
        for name, t in (("want", p @ v), ("pav", p @ v.abs()), ("Z", Z.expand(-1, -1, -1, HD)), ("vsum", vis.double() @ v.abs())):
            parts[name].append(rows(t, n, L, heads))
    out = {name: torch.cat(ts, 0) for name, ts in parts.items()}
    out["B"] = bound(out)
    return out


def bound(ref):
    return 2.0 ** -11 * ref["want"].abs() + 2.0 ** -11 * ref["pav"] + 2.0 ** -25 * ref["vsum"] / ref["Z"]


def ratio(got, ref):
    """|got - want| / B per element, float64 (B > 0 wherever a visible V value is not zero; 0 / 0 counts as 0, x / 0 as inf)"""
    err = (got.detach().cpu().double() - ref["want"]).abs()
    r = err / ref["B"]
    return torch.where(err == 0, torch.zeros_like(r), r)


def worst(got, ref):
    r = ratio(got, ref)
    return float(r.max()) if bool(torch.isfinite(got.detach().cpu()).all()) else float("inf")


def onehot_exact_rows(got, qkv, n_seq, L, heads, causal):
    """`onehot`: the rows that see key j* (all of them without the causal mask) must be fp16(v[j*]) bit for bit - every other
    probability is below exp(-70), zero in fp16, and the fp32 row sum is 1 to within 2^-12 (it is 1 exactly).  (mismatching elements,
    elements checked)"""
    v = split(qkv, n_seq, L, heads)[2]
    j = jstar(L)
    want = rows(v[:, :, j:j + 1].expand(-1, -1, L, -1), n_seq, L, heads).view(n_seq, L, -1)
    g = got.detach().cpu().double().view(n_seq, L, -1)
    i0 = j if causal else 0
    return int((g[:, i0:] != want[:, i0:]).sum()), g[:, i0:].numel()


def sweep(run, kernel, family, causal, lengths, n_seq, heads):
    """One family and mask over `lengths` through run(qkv, n_seq, L, heads, causal) -> [n_seq * L, heads * 64] (a kernel launch): every
    element within B, a second launch bit-identical, `onehot` rows exact.  Prints the worst |err| / B and where, then returns the list
    of failures (empty = pass) so that the caller asserts after every figure is out."""
    failures, top, top_L = [], 0.0, 0
    for L in lengths:
        qkv = make_qkv(family, n_seq, L, heads, seed_of(family, L, causal, n_seq, heads))
        ref = reference(qkv, n_seq, L, heads, causal)
        got = run(qkv, n_seq, L, heads, causal)
        w = worst(got, ref)
        if w > top:
            top, top_L = w, L
        if not w <= 1.0:
            r = ratio(got, ref)
            failures.append(f"L {L}: worst |err| / B {w:.3f}, {int((r > 1).sum())} of {r.numel()} elements above B")
        if not torch.equal(got, run(qkv, n_seq, L, heads, causal)):
            failures.append(f"L {L}: a second launch differs")
        if family == "onehot":
            bad, n = onehot_exact_rows(got, qkv, n_seq, L, heads, causal)
            if bad:
                failures.append(f"L {L}: {bad} of {n} elements are not fp16(v[j*])")
    print(f"ATTN_RATIO {kernel:9s} {family:8s} causal {int(bool(causal))} n_seq {n_seq} heads {heads} L {min(lengths)}..{max(lengths)}: "
          f"worst |err| / B {top:.3f} at L {top_L}")
    return failures


# ---- the CPU restatement of tile_softmax_pv and the loop around it -----------------------------------------------------------
C_LOG2E_8 = torch.tensor(1.4426950408889634, dtype=torch.float32) * 0.125          # the kernels' c = head_dim^-0.5 * log2(e), as fp32


def model(qkv, n_seq, L, heads, causal, mutant=None):
    """The kernels' arithmetic on the CPU, [n_seq * L, heads * 64] float64 holding fp16 values.  fp32 where the kernels hold fp32
    (torch's fp32 matmul for the two MFMA products: exact products, another order of the fp32 additions), fp16 where they round.
    Keys L .. 32 ceil(L / 32) - 1 are, as the kernels stage them, copies of row L - 1, and masked.  mutant: one of MUTANTS -
      scale                the softmax scale times 1.003
      unmasked_key         key L passes the mask (alive while L % 32 != 0 and the mask is not causal, where key <= query hides it)
      unmasked_key_zero_v  the same with a zero V row behind it, as the kernels that read V rows beyond L as zeros would have it
      flush                probabilities below the smallest normal fp16 number become zero
      diagonal             the last query of a 32-query tile does not see its own key (causal; alive from L = 32)
      drop_last            key L - 1 is masked"""
    assert mutant is None or mutant in MUTANTS, mutant
    q, k, v = (t.float() for t in split(qkv, n_seq, L, heads))
    nkt = (L + 31) // 32
    pad = nkt * 32 - L
    if pad:
        k = torch.cat([k, k[:, :, -1:].expand(-1, -1, pad, -1)], 2)
        vpad = v[:, :, -1:].expand(-1, -1, pad, -1)
        v = torch.cat([v, torch.zeros_like(vpad) if mutant == "unmasked_key_zero_v" else vpad], 2)
    c = C_LOG2E_8 * (np.float32(1.003) if mutant == "scale" else np.float32(1.0))
    qi = torch.arange(L)[:, None]
    m = torch.full((n_seq, heads, L), -1.0e30, dtype=torch.float32)
    lsum = torch.zeros(n_seq, heads, L, dtype=torch.float32)
    o = torch.zeros(n_seq, heads, L, HD, dtype=torch.float32)
    for kt in range(nkt):
        key = torch.arange(kt * 32, kt * 32 + 32)[None, :]
        ok = key < (L + 1 if mutant in ("unmasked_key", "unmasked_key_zero_v") else L)
        if mutant == "drop_last":
            ok = ok & (key != L - 1)
        if causal:
            ok = ok & (key <= qi)
            if mutant == "diagonal":
                ok = ok & ~((key == qi) & (qi % 32 == 31))
        ok = ok.expand(L, 32)
        s = q @ k[:, :, kt * 32:kt * 32 + 32].transpose(-1, -2)                   # fp32 [n, h, L, 32]
        s = s.masked_fill(~ok, float("-inf"))
        mn = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp2(((m - mn) * c).double()).float()
        m = mn
        mc = m * c
        e = torch.exp2((s.double() * c.double() - mc.double()[..., None]).float().double()).float()      # v_exp_f32 of one fma
        lsum = lsum * alpha + e.sum(-1)
        p = e.half()
        if mutant == "flush":
            p = torch.where(p < 2.0 ** -14, torch.zeros_like(p), p)
        o = o * alpha[..., None] + p.float() @ v[:, :, kt * 32:kt * 32 + 32]
    inv = 1.0 / lsum
    return rows((o * inv[..., None]).half().double(), n_seq, L, heads)


def alive(mutant, L, causal):
    """whether the mutant changes anything at this length and mask"""
    if mutant in ("unmasked_key", "unmasked_key_zero_v"):
        return L % 32 != 0 and not causal
    if mutant == "diagonal":
        return bool(causal) and L >= 32
    return True
