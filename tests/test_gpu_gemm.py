"""GEMM kernels (simple 128x128 and persistent ring) against a plain PyTorch fp32 matmul of the
fp16-rounded operands, every epilogue, ragged M, and ring == simple bit for bit (same k order).  Further down: every output element
against the float64 CPU reference and the per-element rounding bound of tests/gemm_bound.py, on exact, tiny, random and hard operands."""
import ctypes as C

import pytest
import torch

from hoigen_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def run(ctx, a, w, bias, epi, kernel, out0=None):
    M, K = a.shape
    N = w.shape[0]
    out = out0.clone() if out0 is not None else torch.empty(M, N, device="cuda")
    rc = _lib.lib().hg_test_gemm(ctx, a.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                 out.data_ptr(), M, N, K, epi, kernel, None)
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    torch.cuda.synchronize()
    return out


def ref(a, w, bias, epi, out0):
    y = a.half().float() @ w.half().float().t()
    if bias is not None:
        y = y + bias
    if epi == 1:
        y = y * torch.sigmoid(1.702 * y)
    if epi in (2, 6):
        y = torch.relu(y)
    if epi in (0, 1, 2):
        y = y.half().float()
    if epi == 3:
        y = out0 + y
    return y


SHAPES = [(1024, 256, 256), (2048, 768, 768), (197 * 16, 2304, 768), (197 * 12 + 5, 768, 3072), (513, 512, 1024),
          (4096, 3072, 768),
          # K-tile counts 5 and 6 (the K loop is instantiated per K-tile position: first / middle / last three), a
          # 256-row-tile case with a ragged last tile, and one with more than 256 tiles of 256x256
          (777, 512, 320), (2048, 768, 384), (256 * 33 + 100, 2048, 256),
          # exactly / almost one full round of 256x256 tiles -> the two-phase 256-row kernel, K-tile counts 4 and 5
          (8192, 2048, 256), (8192 - 60, 2048, 320)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4, 6])
def test_gemm_kernels(ctx, M, N, K, epi):
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K + epi)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    out0 = torch.randn(M, N, device="cuda", generator=g) if epi == 3 else None
    want = ref(a, w, bias, epi, out0)
    scale = want.abs().max().item()
    got1 = run(ctx, a, w, bias, epi, 1, out0)
    tol = (3e-3 if epi in (0, 1, 2) else 2e-5) * scale          # fp16 outputs: 1 ulp of fp16 at the top of the range
    assert (got1 - want).abs().max().item() <= tol, "simple kernel"
    got2 = run(ctx, a, w, bias, epi, 2, out0)
    assert (got2 - want).abs().max().item() <= tol, "ring kernel"
    assert torch.equal(got1, got2), "ring and simple kernels accumulate in the same order"
    if N % 256 == 0 and K >= 256 and M >= 512:      # two-workgroups-per-CU kernel (hg_gemm_duo.hip): same bits
        assert torch.equal(got1, run(ctx, a, w, bias, epi, 3, out0)), "duo and simple kernels accumulate in the same order"
        assert torch.equal(run(ctx, a, w, None, epi, 1, out0), run(ctx, a, w, None, epi, 3, out0)), "duo without bias"
    got_nb = run(ctx, a, w, None, epi, 2, out0)
    want_nb = ref(a, w, None, epi, out0)
    assert (got_nb - want_nb).abs().max().item() <= tol, "ring kernel without bias"


def test_ring_many_tiles_per_workgroup(ctx):
    """More tiles than CUs (persistent stream across tile boundaries, epilogue/vmcnt bookkeeping)."""
    M, N, K = 197 * 256, 768, 768
    g = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    bias = torch.randn(N, device="cuda", generator=g)
    for epi in (0, 3, 4):
        out0 = torch.randn(M, N, device="cuda", generator=g) if epi == 3 else None
        g1 = run(ctx, a, w, bias, epi, 1, out0)
        for _ in range(3):                      # repeated launches: races would show as flaky mismatches
            g2 = run(ctx, a, w, bias, epi, 2, out0)
            assert torch.equal(g1, g2)
            assert torch.equal(g1, run(ctx, a, w, bias, epi, 3, out0)), "duo kernel"
    want = ref(a, w, bias, 4, None)
    assert (g1 - want).abs().max().item() <= 2e-5 * want.abs().max().item()


# ---- the epilogues the vision tower actually runs: LayerNorm folded into the consumer GEMM (8, 9), residual update that
# ---- emits the centred fp16 copy and the row statistics (10), and the scaled variant behind the adapter (12)
def run_ln(ctx, a, w, bias, epi, kernel, *, cs=None, mr=None, mu=None, scale=None, x0=None):
    M, K = a.shape
    N = w.shape[0]
    p = lambda t: t.data_ptr() if t is not None else None
    if epi in (8, 9):
        out = torch.empty(M, N, device="cuda")
        rc = _lib.lib().hg_test_gemm_ln(ctx, p(a), p(w), p(bias), p(out), M, N, K, epi, kernel, p(cs), p(mr), None, None,
                                        None, None, None, None)
        assert rc == 0, _lib.lib().hg_last_error(ctx)
        torch.cuda.synchronize()
        return out
    out = x0.clone()
    out2 = torch.empty(M, N, device="cuda")
    mr_out = torch.empty(M, 2, device="cuda")
    mu_out = torch.empty(M, device="cuda")
    rc = _lib.lib().hg_test_gemm_ln(ctx, p(a), p(w), p(bias), p(out), M, N, K, epi, kernel, None, None, p(mu), p(scale),
                                    p(out2), p(mr_out), p(mu_out), None)
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    torch.cuda.synchronize()
    return out, out2, mr_out, mu_out


def _operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    return g, a, w, bias


# ragged M, K-tile counts 4 / 5 / 6 / 12 / 48; (8192, 2048, .) fills exactly one round of 256x256 tiles (two-phase loop),
# the others run the 128-row variants
LN_SHAPES = [(197 * 12 + 5, 768, 768), (256 * 33 + 100, 768, 256), (2048 + 37, 768, 320), (1024 + 3, 2304, 384),
             (4096 + 77, 768, 3072), (8192, 2048, 256), (8192 - 60, 2048, 768), (197 * 12 + 5, 2304, 832)]


@pytest.mark.parametrize("M,N,K", LN_SHAPES)
@pytest.mark.parametrize("epi", [8, 9])
def test_layernorm_folded_epilogues(ctx, M, N, K, epi):
    """rstd * (x16 W'^T - mean * cs) + b'  against the same expression in fp32 PyTorch."""
    g, a, w, bias = _operands(M, N, K, M + 3 * N + K + epi)
    mean = torch.randn(M, device="cuda", generator=g) * 0.3
    rstd = torch.rand(M, device="cuda", generator=g) * 1.5 + 0.5
    mr = torch.stack([mean, rstd], 1).contiguous()
    cs = w.half().float().sum(1)
    acc = a.half().float() @ w.half().float().t()
    want = rstd[:, None] * (acc - mean[:, None] * cs[None]) + bias
    if epi == 9:
        want = want * torch.sigmoid(1.702 * want)
    want = want.half().float()
    tol = 3e-3 * want.abs().max().item()
    first = None
    for it in range(3):                                        # repeated launches: a race shows as a flaky mismatch
        got = run_ln(ctx, a, w, bias, epi, 0, cs=cs, mr=mr)
        assert torch.isfinite(got).all()
        assert (got - want).abs().max().item() <= tol, f"launch {it}"
        first = got if first is None else first
        assert torch.equal(got, first), "same inputs, different bits"


# more residual shapes: K-tile counts 12, 13, 48 on full 128-row tiles; fewer tiles than CUs, several tiles per workgroup
RESID_SHAPES = LN_SHAPES[:5] + [(128 * 40, 768, 768), (128 * 37, 768, 832), (128 * 41, 768, 3072), (128 * 300, 768, 768),
                                (128 * 394, 768, 768), (128 * 24, 2304, 1024)]


@pytest.mark.parametrize("M,N,K", RESID_SHAPES)
def test_residual_epilogue_emits_copy_and_statistics(ctx, M, N, K):
    """EPI_RESID_LN_F32: x += acc + b; x16 = fp16(x - mu); (sum, M2) groups -> finalize_stats -> (mean - mu, rstd), mu = mean.
    ring2 (128x256, the product path) and the duo kernel must agree bit for bit on the stream and its copy."""
    g, a, w, bias = _operands(M, N, K, 5 * M + N + K)
    x0 = torch.randn(M, N, device="cuda", generator=g) * 2 + torch.randn(M, 1, device="cuda", generator=g)   # rows with offsets
    mu = x0.mean(1) + 0.05 * torch.randn(M, device="cuda", generator=g)      # "previous mean": close to, not equal to, the new one
    xr = x0 + a.half().float() @ w.half().float().t() + bias
    mean = xr.mean(1)
    rstd = 1.0 / torch.sqrt(xr.var(1, unbiased=False) + 1e-5)
    want16 = (xr - mu[:, None]).half().float()
    scale = xr.abs().max().item()
    ref_bits = None
    for kernel in (2, 3):
        for it in range(3):
            x, x16, mr_out, mu_out = run_ln(ctx, a, w, bias, 10, kernel, mu=mu, x0=x0)
            assert (x - xr).abs().max().item() <= 2e-5 * scale, (kernel, it)
            assert (x16 - want16).abs().max().item() <= 2e-3 * (xr - mu[:, None]).abs().max().item(), (kernel, it)
            assert (mu_out - mean).abs().max().item() <= 1e-5 * scale
            assert ((mr_out[:, 0] - (mean - mu)).abs().max().item()) <= 1e-5 * scale
            assert ((mr_out[:, 1] - rstd).abs() / rstd).max().item() <= 1e-4
            bits = (x, x16, mr_out, mu_out)
            if it == 0:
                first = bits
            for u, v in zip(bits, first):
                assert torch.equal(u, v), f"kernel {kernel} launch {it}: same inputs, different bits"
            if ref_bits is None:
                ref_bits = bits
            # the two kernels accumulate in the same order: stream and fp16 copy agree bit for bit (their row-statistics
            # reductions group the lanes differently: equal within the tolerances above only)
            assert torch.equal(x, ref_bits[0]) and torch.equal(x16, ref_bits[1]), f"kernel {kernel}: bits differ from ring2's"


@pytest.mark.parametrize("M,N,K", [(197 * 12 + 5, 768, 64), (256 * 33 + 100, 768, 64), (2048 + 37, 768, 128), (1024 + 3, 768, 192),
                                   (4096 + 77, 768, 256)])
def test_scaled_residual_epilogue_duo(ctx, M, N, K):
    """EPI_SCALE_RESID_LN_F32 (adapter up_proj, K = 64 in production: one K-tile per tile, the path that skips the
    vmcnt wait after a residual epilogue on every tile after the first)."""
    g, a, w, bias = _operands(M, N, K, 7 * M + N + K)
    x0 = torch.randn(M, N, device="cuda", generator=g)
    sc = torch.randn(N, device="cuda", generator=g) * 0.5
    mu = x0.mean(1)
    xr = x0 + (a.half().float() @ w.half().float().t() + bias) * sc
    mean = xr.mean(1)
    rstd = 1.0 / torch.sqrt(xr.var(1, unbiased=False) + 1e-5)
    scale = xr.abs().max().item()
    first = None
    for it in range(3):
        x, x16, mr_out, mu_out = run_ln(ctx, a, w, bias, 12, 0, mu=mu, scale=sc, x0=x0)
        assert (x - xr).abs().max().item() <= 2e-5 * scale
        assert (x16 - (xr - mu[:, None]).half().float()).abs().max().item() <= 2e-3 * (xr - mu[:, None]).abs().max().item()
        assert (mu_out - mean).abs().max().item() <= 1e-5 * scale
        assert ((mr_out[:, 1] - rstd).abs() / rstd).max().item() <= 1e-4
        first = (x, x16, mr_out) if first is None else first
        assert all(torch.equal(u, v) for u, v in zip((x, x16, mr_out), first))


@pytest.mark.parametrize("M,N,K", [(1024, 768, 64), (777, 512, 128), (2048 + 9, 256, 192)])
@pytest.mark.parametrize("epi", [0, 3, 4])
def test_duo_short_k(ctx, M, N, K, epi):
    """The duo kernel admits K >= 64: K-tile counts 1, 2, 3 against the simple kernel, bit for bit."""
    g, a, w, bias = _operands(M, N, K, M + N + K + epi)
    out0 = torch.randn(M, N, device="cuda", generator=g) if epi == 3 else None
    want = ref(a, w, bias, epi, out0)
    got1 = run(ctx, a, w, bias, epi, 1, out0)
    assert (got1 - want).abs().max().item() <= (3e-3 if epi == 0 else 2e-5) * want.abs().max().item()
    for _ in range(3):
        assert torch.equal(got1, run(ctx, a, w, bias, epi, 3, out0))


@pytest.mark.parametrize("M,N,K", [(197 * 12 + 5, 768, 768), (128 * 41, 768, 3072), (256 * 33 + 100, 768, 256), (128 * 394, 768, 768)])
def test_residual_stream_as_centre_hi_lo(ctx, M, N, K):
    """GemmArgs::hl: five residual updates in a row with the stream held as centre + hi + lo between them (the first
    reads fp32, the last writes fp32) against the same five updates on an fp32 stream: the final rows agree to what the halves
    carry (fp16 + fp16: 22 bits of x - centre; fp16 + bf8, the default build: 13-14 bits), the last copy and statistics agree,
    repeated runs are bit-identical; rows with a large common offset and 30x outlier columns included."""
    g, a, w, bias = _operands(M, N, K, 13 * M + N + K)
    x0 = torch.randn(M, N, device="cuda", generator=g) * 2 + 8 * torch.randn(M, 1, device="cuda", generator=g)
    x0[:, 5::97] *= 30.0
    mu0 = x0.mean(1) + 0.05 * torch.randn(M, device="cuda", generator=g)
    p = lambda t: t.data_ptr()

    def run(hilo):
        x, mu = x0.clone(), mu0.clone()
        out2, mr = torch.empty(M, N, device="cuda"), torch.empty(M, 2, device="cuda")
        rc = _lib.lib().hg_test_gemm_hilo(ctx, p(a), p(w), p(bias), p(x), M, N, K, 5, hilo, p(mu), p(out2), p(mr), None)
        assert rc == 0, _lib.lib().hg_last_error(ctx)
        torch.cuda.synchronize()
        return x, mu, out2, mr

    f32 = run(0)
    upd = a.half().float() @ w.half().float().t() + bias
    want = x0 + 5 * upd
    scale = want.abs().max().item()
    assert (f32[0] - want).abs().max().item() <= 1e-5 * scale
    hl = run(1)
    again = run(1)
    assert all(torch.equal(u, v) for u, v in zip(hl, again)), "same inputs, different bits"
    assert torch.isfinite(hl[0]).all()
    # against the fp32 stream: per element relative to the row's spread about its centre (what the halves are scaled to)
    spread = (want - want.mean(1, keepdim=True)).abs().amax(1, keepdim=True)
    err = ((hl[0] - f32[0]).abs() / spread).max().item()
    print(f"\\nhi/lo stream vs fp32 stream after 5 updates: max |diff| / row spread = {err:.2e}")
    bits = C.c_int32(0)
    assert _lib.lib().hg_get_option(ctx, b"stream_lo_bits", C.byref(bits)) == 0 and bits.value == 8
    # lo as bf8: the remainder (<= 2^-11 of the element) keeps two mantissa bits, <= 2^-14 of the element per update, and the
    # updates' errors add: 5 x 6.1e-5 of the row spread at most
    assert err <= 5 * 2.0 ** -14 * 1.02
    assert (hl[1] - f32[1]).abs().max().item() <= 1e-5 * scale                      # mean
    assert ((hl[3][:, 1] - f32[3][:, 1]).abs() / f32[3][:, 1]).max().item() <= 1e-4   # rstd
    assert (hl[2] - f32[2]).abs().max().item() <= 2e-3 * spread.max().item()          # last centred copy (fp16 grid)


# ---- per output element: the float64 CPU reference and the rounding bound of tests/gemm_bound.py (its docstring states the bound and the
# ---- input families), `exact` / `tiny` operands bit for bit, canary rows behind every buffer a kernel writes directly, the smallest shapes that
# ---- reach each code path.  Beside the checks above, never in place of them.
import gemm_bound as gb  # noqa: E402

CANARY_ROWS, CANARY = 256, 0x5A5A5A5A
KERNEL_NAMES = {0: "dispatch", 1: "simple", 2: "ring", 3: "duo"}


# eligibility as gemm_ring_ok / gemm_ring2_ok / gemm_ln_ok / gemm_duo_ok (hg_gemm_ring.hip, hg_gemm_ring2.hip, hg_gemm_duo.hip) have it
def ring_ok(M, N, K):
    return N % 256 == 0 and K % 64 == 0 and K >= 256 and M >= 512 and N <= 8192


def ring2_ok(M, N, K):
    return ring_ok(M, N, K) and N <= 3072


def ln_ok(M, N, K):
    return ring_ok(M, N, K) and N <= 3584


def duo_ok(M, N, K):
    return N % 256 == 0 and K % 64 == 0 and K >= 64 and M >= 512 and N <= 8192


def ring_big(M, N, resid=False):
    """whether launch_gemm_ring (hg_gemm_ring.hip) runs its own 256 x 256 tiles (hg_gemm_ring_body.h) - at least one full round of them -
    and does not hand the call to gemm_ring2's 128 x 256 tiles; epilogues 8 / 9 always run in the ring body, 10 follows other rules"""
    t256, t128 = -(-M // 256) * (N // 256), -(-M // 128) * (N // 256)
    rounds, rounds128 = -(-t256 // 256), -(-t128 // 256)
    big = t256 >= 256 and t256 / (rounds * 256.0) >= 0.9
    if not resid and not big and t256 >= 256 and rounds <= 0.8 * t128 / 256.0:
        big = True
    if resid and t256 >= 256 and rounds <= 0.8 * rounds128 + 1e-9:
        big = True
    return ring_ok(M, N, 256) and (big or not ring2_ok(M, N, 256))


def padded(rows, cols, init=None):
    """[rows + CANARY_ROWS, cols] float32 on the device: `init` (or zeros) in front, a fixed bit pattern behind"""
    buf = torch.full((rows + CANARY_ROWS, cols), CANARY, dtype=torch.int32, device="cuda").view(torch.float32)
    if init is not None:
        buf[:rows] = init
    return buf


def canary_intact(buf, rows):
    return bool((buf[rows:].view(torch.int32) == CANARY).all())


class Launcher:
    """One case's operands on the device, and its launches through the hooks: every output buffer carries CANARY_ROWS rows behind row M.
    The canary is a check of the KERNEL where the kernel writes the caller's buffer itself: `out` of epilogues 3, 4, 6 and the stream of
    10 / 12.  fp16 outputs (0, 1, 2, 8, 9), out2, mr_out and mu_out are written into the context's buffers and the hook copies M rows out:
    there the canary only checks the hook."""

    def __init__(self, ctx, c):
        self.ctx, self.c = ctx, c
        self.d = {k: c[k].cuda() for k in ("a", "w", "bias", "scale", "mu", "mr", "cs")}
        self.x0 = c["x0"][:c["M"]].cuda()

    def __call__(self, epi, kernel, bias=True):
        c, d, L = self.c, self.d, _lib.lib()
        M, N, K = c["M"], c["N"], c["K"]
        p = lambda t: t.data_ptr()
        b = p(d["bias"]) if bias else None
        out = padded(M, N, self.x0 if epi in (3, 10, 12) else None)
        bufs = [out]
        if epi in (0, 1, 2, 3, 4, 6):
            rc = L.hg_test_gemm(self.ctx, p(d["a"]), p(d["w"]), b, p(out), M, N, K, epi, kernel, None)
            res = {}
        elif epi in (8, 9):
            rc = L.hg_test_gemm_ln(self.ctx, p(d["a"]), p(d["w"]), b, p(out), M, N, K, epi, kernel, p(d["cs"]), p(d["mr"]), None, None,
                                   None, None, None, None)
            res = {}
        else:
            out2, mr_out, mu_out = padded(M, N), padded(M, 2), padded(M, 1)
            bufs += [out2, mr_out, mu_out]
            rc = L.hg_test_gemm_ln(self.ctx, p(d["a"]), p(d["w"]), b, p(out), M, N, K, epi, kernel, None, None, p(d["mu"]),
                                   p(d["scale"]) if epi == 12 else None, p(out2), p(mr_out), p(mu_out), None)
            res = {"out2": out2[:M], "mr_out": mr_out[:M], "mu_out": mu_out[:M, 0]}
        assert rc == 0, L.hg_last_error(self.ctx)
        torch.cuda.synchronize()
        for t in bufs:
            assert canary_intact(t, M), f"epilogue {epi} kernel {kernel}: rows >= M were written"
        res["out"] = out[:M]
        return res


def check_case(ctx, family, M, N, K, ratios_of_all_kernels=True):
    """Every epilogue the hooks reach, with and without bias, on every kernel that takes the shape: each element within B of the float64
    reference (the simple kernel, and ring / duo where there is no simple variant), `exact` / `tiny` bit for bit, the other kernels bit
    for bit equal to the simple one.  Prints the worst |err| / B per kernel and epilogue, then asserts."""
    c = gb.make_case(family, M, N, K)
    run_case = Launcher(ctx, c)
    failures, worst = [], {}

    def judge(kernel, epi, bias, got):
        r = gb.ratios(c, epi, {k: v.cpu() for k, v in got.items()}, bias=bias)
        for key, v in r.items():
            worst[(kernel, epi, key)] = max(worst.get((kernel, epi, key), 0.0), v)
            if not v <= 1.0:
                failures.append(f"{KERNEL_NAMES[kernel]} epilogue {epi} bias {int(bias)}: worst |err| / B of {key} {v:.3f}")

    plain = [] if family in gb.LN_FAMILIES + gb.RESID_FAMILIES else [0, 1, 2, 3, 4, 6]
    bitwise = {"exact": (0, 2, 3, 4, 6), "tiny": (0,)}.get(family, ())
    for epi in plain:
        for bias in (True, False):
            got1 = run_case(epi, 1, bias)
            judge(1, epi, bias, got1)
            if epi in bitwise and not torch.equal(got1["out"].cpu(), gb.exact_expected(c, epi, bias=bias)):
                failures.append(f"simple epilogue {epi} bias {int(bias)}: `{family}` operands, not the float64 result bit for bit")
            others = [0] + ([2] if ring_ok(M, N, K) else []) + ([3] if duo_ok(M, N, K) else [])
            for kernel in others:
                if not torch.equal(run_case(epi, kernel, bias)["out"], got1["out"]):
                    failures.append(f"{KERNEL_NAMES[kernel]} epilogue {epi} bias {int(bias)}: bits differ from the simple kernel's")
    if ln_ok(M, N, K) and family not in gb.RESID_FAMILIES:
        for epi in (8, 9):
            for bias in (True, False):
                got = run_case(epi, 2, bias)
                judge(2, epi, bias, got)
                if not torch.equal(run_case(epi, 0, bias)["out"], got["out"]):
                    failures.append(f"epilogue {epi} bias {int(bias)}: the dispatcher's launch differs from the ring kernel's")
    if duo_ok(M, N, K) and family not in gb.LN_FAMILIES:
        for bias in (True, False):
            ref_bits = None
            for kernel in ([2] if ring2_ok(M, N, K) else []) + [3]:
                got = run_case(10, kernel, bias)
                judge(kernel, 10, bias, got)
                if ref_bits is None:
                    ref_bits = got
                elif not (torch.equal(got["out"], ref_bits["out"]) and torch.equal(got["out2"], ref_bits["out2"])):
                    failures.append(f"epilogue 10 bias {int(bias)}: duo's stream or copy differs from ring2's")
            judge(3, 12, bias, run_case(12, 0, bias))
    for (kernel, epi, key), v in sorted(worst.items()):
        print(f"GEMM_RATIO {KERNEL_NAMES[kernel]} {epi} {family} {key} M {M} N {N} K {K}: worst |err| / B {v:.3f}")
    assert not failures, failures


# the simple kernel (N % 128, K % 64, any M): one row, a ragged single tile, two row tiles, the four-stage variant (grid <= CUs and
# >= 4 K-tiles: 130 x 384 x 256 and 257 x 128 x 3072), the two-stage variant on 288 tiles
SIMPLE_SHAPES = [(1, 128, 64), (127, 128, 64), (129, 256, 128), (130, 384, 256), (257, 128, 3072), (2179, 2048, 256)]
# ring / ring2 / duo (M >= 512, N % 256, K >= 256): ragged last tiles of the 128- and 256-row tiles on both sides of each boundary,
# K-tile counts 4, 5, 6, 7, 13 at M = 641, both N
RING_M = [512, 513, 639, 640, 641, 767, 769, 1025]
RING_SHAPES = [(M, 256, 256) for M in RING_M] + [(641, 256, K) for K in (320, 384, 448, 832)] + [(641, 768, 320)]
HARD_SHAPES = [(641, 256, 256), (641, 256, 832), (641, 768, 320), (2048, 768, 768)]


@pytest.mark.parametrize("M,N,K", SIMPLE_SHAPES + RING_SHAPES)
@pytest.mark.parametrize("family", ["exact", "tiny", "randn"])
def test_every_element_within_the_rounding_bound(ctx, family, M, N, K):
    check_case(ctx, family, M, N, K)


@pytest.mark.parametrize("M,N,K", HARD_SHAPES)
@pytest.mark.parametrize("family", ["outlier", "cancel"])
def test_hard_operands_within_the_rounding_bound(ctx, family, M, N, K):
    check_case(ctx, family, M, N, K)


@pytest.mark.parametrize("M,N,K", RING_SHAPES + [(2048, 768, 768)])
@pytest.mark.parametrize("family", list(gb.LN_FAMILIES + gb.RESID_FAMILIES))
def test_epilogue_specific_families_within_the_rounding_bound(ctx, family, M, N, K):
    """`lnfold` on the LayerNorm-folded epilogues 8 / 9; `offset`, `constant`, `wide` on the residual epilogues 10 / 12: stream, fp16 copy
    and row statistics"""
    check_case(ctx, family, M, N, K)


def test_constant_rows_have_zero_variance(ctx):
    """`constant`: x0 constant along every third row, a = 0, bias = 0: the update is zero, the returned row is x0, its mean exact and rstd
    1 / sqrt(1e-5)"""
    M, N, K = 641, 256, 256
    c = gb.make_case("constant", M, N, K)
    run_case = Launcher(ctx, c)
    for kernel in (2, 3):
        got = run_case(10, kernel)
        assert torch.equal(got["out"][::3].cpu(), c["x0"][:M:3])
        assert torch.equal(got["mu_out"][::3].cpu(), c["x0"][:M:3, 0]), "the mean of a constant row of few bits is exact"
        # (sum, M2) = (64 x, 0) exactly in every group: what is left is 1e-5 as fp32, one add, the square root and the reciprocal -
        # 8 ulp of fp32 covers them (half an ulp each for the IEEE operations, one each if sqrt and reciprocal are the approximate ones)
        rstd = got["mr_out"][::3, 1].cpu().double()
        assert ((rstd - 1e-5 ** -0.5).abs() <= 1e-5 ** -0.5 * 2.0 ** -21).all(), float((rstd - 1e-5 ** -0.5).abs().max())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact_operands_on_the_large_shapes(ctx, M, N, K):
    """The shapes of test_gemm_kernels (256 x 256 two-phase tiles, many tiles per workgroup) with `exact` operands: fp32 outputs and the
    fp16 outputs of epilogues 0 / 2 bit for bit the float64 result on every kernel; QuickGELU within B on the simple kernel and bit for
    bit across kernels"""
    c = gb.make_case("exact", M, N, K)
    run_case = Launcher(ctx, c)
    kernels = [1, 0] + ([2] if ring_ok(M, N, K) else []) + ([3] if duo_ok(M, N, K) else [])
    failures = []
    for epi in (0, 2, 3, 4, 6):
        want = gb.exact_expected(c, epi).cuda()
        for kernel in kernels:
            if not torch.equal(run_case(epi, kernel)["out"], want):
                failures.append(f"{KERNEL_NAMES[kernel]} epilogue {epi}: not the float64 result bit for bit")
    got1 = run_case(1, 1)
    w = gb.ratios(c, 1, {"out": got1["out"].cpu()})["out"]
    print(f"GEMM_RATIO simple 1 exact out M {M} N {N} K {K}: worst |err| / B {w:.3f}")
    assert w <= 1.0
    for kernel in kernels[1:]:
        if not torch.equal(run_case(1, kernel)["out"], got1["out"]):
            failures.append(f"{KERNEL_NAMES[kernel]} epilogue 1: bits differ from the simple kernel's")
    assert not failures, failures


# ---- the arguments hg_test_gemm / hg_test_gemm_ln cannot set, through hg_test_gemm_ex: lda > K, ldc > N, the patch embedding's row map
# ---- (5), the scaled residual (7), the centred-copy ReLU GEMM with its split (11), two destinations (out_hi)
KERNEL_NAMES[4] = "ring2"
JUNK = 1000.0          # behind column K of every row of a: a kernel that reads past K shows it


def run_ex(ctx, c, epi, kernel, *, bias=True, lda_pad=64, ldc_pad=8, G=0, L=0, pos=True, n_split=0, two_outputs=False, expect_rc=0):
    """One hg_test_gemm_ex launch of case c -> out [rows, N] float32 on the device (two_outputs: the halves side by side again).  a is
    passed with row stride K + lda_pad, the outputs with row stride (their width) + ldc_pad; asserts that the canary rows behind each
    output and its columns beyond the width are intact.  The kernel writes the caller's buffer itself for the fp32 epilogues (3, 4, 5, 6,
    7, 11): there the canaries check the kernel.  fp16 outputs (0, 1, 2) come back through the hook's own copy of M rows x N columns, so
    for them the canaries check the hook only; what checks the kernel's use of ldc there is the result itself."""
    M, N, K = c["M"], c["N"], c["K"]
    p = lambda t: t.data_ptr() if t is not None else None
    a = torch.full((M, K + lda_pad), JUNK, device="cuda")
    a[:, :K] = c["a"].cuda()
    rows = (M // G) * L if epi == 5 else M
    width = max(n_split, N - n_split) if two_outputs else N
    init = c["x0"][:rows].cuda() if epi in (3, 5, 7) else None
    outs = []
    for h in range(2 if two_outputs else 1):
        buf = padded(rows, width + ldc_pad)
        buf.view(torch.int32)[:rows] = CANARY
        if init is not None:
            buf[:rows, :N] = init
        outs.append(buf)
    w, b = c["w"].cuda(), c["bias"].cuda() if bias else None
    posd = c["pos"][:L].contiguous().cuda() if epi == 5 and pos else None
    sc, mu, cs = (c[k].cuda() for k in ("scale", "mu", "cs"))
    args = _lib.hg_test_gemm_ex_args(a=p(a), w=p(w), bias=p(b), out=p(outs[0]), out_hi=p(outs[1]) if two_outputs else None, pos=p(posd),
                                     scale=p(sc) if epi == 7 else None, mu=p(mu) if epi == 11 else None, cs=p(cs) if epi == 11 else None,
                                     M=M, N=N, K=K, lda=K + lda_pad, ldc=width + ldc_pad, epi=epi, kernel=kernel, G=G, L=L, n_split=n_split)
    rc = _lib.lib().hg_test_gemm_ex(ctx, C.byref(args), None)
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, _lib.lib().hg_last_error(ctx))
    if rc:
        return None
    widths = [n_split, N - n_split] if two_outputs else [N]
    for buf, wd in zip(outs, widths):
        assert canary_intact(buf, rows), f"epilogue {epi} kernel {kernel}: rows behind the output were written"
        assert bool((buf[:rows, wd:].view(torch.int32) == CANARY).all()), f"epilogue {epi} kernel {kernel}: columns beyond the output's width were written"
    return torch.cat([buf[:rows, :wd] for buf, wd in zip(outs, widths)], 1).contiguous()


def check_ex(ctx, c, epi, kernels, exact, **kw):
    """kernels[0] within B of the float64 reference (and bit for bit on `exact` operands), the others bit for bit equal to it"""
    ref_kw = {k: v for k, v in kw.items() if k in ("bias", "G", "L", "pos", "n_split") and not (k == "n_split" and epi != 11)}
    first = None
    for kernel in kernels:
        got = run_ex(ctx, c, epi, kernel, **kw)
        if first is None:
            first = got
            w = gb.ratios(c, epi, {"out": got.cpu()}, **ref_kw)["out"]
            print(f"GEMM_RATIO {KERNEL_NAMES[kernel]} {epi} {c['family']} out M {c['M']} N {c['N']} K {c['K']}: worst |err| / B {w:.3f}")
            assert w <= 1.0, (KERNEL_NAMES[kernel], epi, kw, w)
            if exact:
                assert torch.equal(got.cpu(), gb.exact_expected(c, epi, **ref_kw)), (KERNEL_NAMES[kernel], epi, kw)
        else:
            assert torch.equal(got, first), f"{KERNEL_NAMES[kernel]} epilogue {epi} {kw}: bits differ from {KERNEL_NAMES[kernels[0]]}'s"


@pytest.mark.parametrize("G,L,n_img", [(4, 5, 130), (196, 197, 3)])
@pytest.mark.parametrize("family", ["exact", "randn"])
def test_patch_embedding_epilogue(ctx, family, G, L, n_img):
    """Epilogue 5 on the simple, gemm_ring2 (128 x 256 tiles) and duo kernels: output row b L + 1 + t, with and without the positional
    rows; the class-token rows b L keep what they held (reference() expects them with B = 0).  At these sizes kernels 0, 2 and 4 are all
    gemm_ring2 (ring_big is false); the 256 x 256 ring kernel: test_ring_kernel_256_row_tiles_patch_embedding."""
    assert not ring_big(n_img * G, 256)
    M, N, K = n_img * G, 256, 256
    c = gb.make_case(family, M, N, K, n_img * L)
    for pos in (True, False):
        for bias in (True, False):
            check_ex(ctx, c, 5, [1, 0, 2, 3, 4], family == "exact", G=G, L=L, pos=pos, bias=bias)
    got = run_ex(ctx, c, 5, 1, G=G, L=L)
    assert torch.equal(got[::L].cpu(), c["x0"][:n_img * L:L]), "class-token rows"


@pytest.mark.parametrize("family,M,N,K,kernels", [(f, *shape) for f in ("exact", "randn") for shape in
                                                  [(129, 128, 64, [1, 0]), (641, 256, 256, [1, 0, 2, 4]), (641, 256, 832, [1, 0, 2, 4])]]
                         + [("exact", 8192, 2048, 256, [1, 2])])
def test_scaled_residual_epilogue(ctx, family, M, N, K, kernels):
    """Epilogue 7, out += (acc + bias) scale[n]: simple kernel at one K-tile, simple / ring2 at 4 and 13 K-tiles, and the 256 x 256 ring
    kernel (which only a full round of tiles reaches)"""
    assert ring_big(M, N, resid=True) == (M >= 8192)
    c = gb.make_case(family, M, N, K)
    for bias in (True, False) if M < 8192 else (True,):
        check_ex(ctx, c, 7, kernels, family == "exact", bias=bias)


@pytest.mark.parametrize("epi", [0, 1, 2, 3, 4, 6])
@pytest.mark.parametrize("family", ["exact", "randn"])
def test_leading_dimensions(ctx, family, epi):
    """lda = K + 64 (junk behind column K) and ldc = N + 8 on the simple, gemm_ring2 and duo kernels (kernels 0, 2 and 4 are all
    gemm_ring2 at this size; epilogue 3 through the dispatcher is duo), fp16 and fp32 outputs; the canary columns behind column N check
    the kernel for the fp32 outputs (3, 4, 6) only.  The 256 x 256 ring kernel: test_ring_kernel_256_row_tiles_leading_dimensions."""
    assert not ring_big(641, 256)
    c = gb.make_case(family, 641, 256, 320)
    check_ex(ctx, c, epi, [1, 0, 2, 3, 4], family == "exact" and epi != 1)


@pytest.mark.parametrize("K", [768, 832])
@pytest.mark.parametrize("family", ["exact", "randn"])
def test_centred_copy_relu_epilogue(ctx, family, K):
    """Epilogue 11 (simple kernel): relu(W (x16 + mu) + b) from the centred copy, lda = K + 64; n_split = 64: ReLU below the split, linear
    above it"""
    c = gb.make_case(family, 130, 128, K)
    for n_split in (0, 64):
        for bias in (True, False):
            check_ex(ctx, c, 11, [1, 0], family == "exact", n_split=n_split, bias=bias)
    want = gb.reference(c, 11, n_split=64)[0]
    assert bool((want[:, 64:] < 0).any()) and bool((want[:, :64] == 0).any()), "the case exercises both sides of the split"


@pytest.mark.parametrize("epi", [4, 6])
@pytest.mark.parametrize("family", ["exact", "randn"])
def test_two_destinations(ctx, family, epi):
    """out_hi / n_split (the VAE encoder's mean | log_var GEMM): N = 1024 split at 512 on the simple, gemm_ring2 and duo kernels (kernels
    0, 2 and 4 are all gemm_ring2 at this size), each half in a buffer of its own with canary rows behind it and canary columns beside
    it.  The 256 x 256 ring kernel: test_ring_kernel_256_row_tiles_two_destinations."""
    assert not ring_big(641, 1024)
    c = gb.make_case(family, 641, 1024, 256)
    for bias in (True, False):
        check_ex(ctx, c, epi, [1, 0, 2, 3, 4], family == "exact", n_split=512, two_outputs=True, bias=bias)


# The 256 x 256 tiles of hg_gemm_ring_body.h (the kernel the towers' large GEMMs run, the patch embedding at batch 256 among them) take a
# call only when it fills at least one round of them (ring_big): one full-round shape each for what the tests above reach on gemm_ring2
# only, `exact` operands - bit for bit the float64 result on the simple kernel, the ring kernel bit for bit equal to it.
def test_ring_kernel_256_row_tiles_patch_embedding(ctx):
    """Epilogue 5 on gemm_ring<4, two-phase>: 2048 images x 4 patches, N = 2048: 256 tiles of 256 x 256, ldc = N + 8; row map, class rows"""
    G, L, n_img, N, K = 4, 5, 2048, 2048, 256
    assert ring_big(n_img * G, N)
    c = gb.make_case("exact", n_img * G, N, K, n_img * L)
    for pos in (True, False):
        check_ex(ctx, c, 5, [1, 2], True, G=G, L=L, pos=pos)
    got = run_ex(ctx, c, 5, 2, G=G, L=L)
    assert torch.equal(got[::L].cpu(), c["x0"][:n_img * L:L]), "class-token rows"


@pytest.mark.parametrize("epi", [4, 6])
def test_ring_kernel_256_row_tiles_two_destinations(ctx, epi):
    """out_hi / n_split on gemm_ring<4, two-phase>: 16384 x 1024 split at 512, 256 tiles of 256 x 256, each half with row stride 520"""
    M, N, K = 16384, 1024, 256
    assert ring_big(M, N)
    check_ex(ctx, gb.make_case("exact", M, N, K), epi, [1, 2], True, n_split=512, two_outputs=True)


@pytest.mark.parametrize("epi", [0, 1, 4])
def test_ring_kernel_256_row_tiles_leading_dimensions(ctx, epi):
    """lda = K + 64 and ldc = N + 8 on gemm_ring<4, two-phase> with the non-residual epilogues, fp16 and fp32: 8192 x 2048 x 256"""
    M, N, K = 8192, 2048, 256
    assert ring_big(M, N)
    check_ex(ctx, gb.make_case("exact", M, N, K), epi, [1, 2], epi != 1)


def test_gemm_ex_refuses_what_the_kernel_does_not_take(ctx):
    """HG_ERR_INVALID (-1) and no launch: M < 512 on the ring kernels and duo, K < 256 on ring / ring2, N % 256 on them, epilogue 7 on
    duo, epilogue 11 anywhere but the simple kernel"""
    small = gb.make_case("randn", 129, 128, 64)
    for kernel in (2, 3, 4):
        run_ex(ctx, small, 4, kernel, expect_rc=-1)
    ok = gb.make_case("randn", 641, 256, 256)
    run_ex(ctx, ok, 7, 3, expect_rc=-1)
    run_ex(ctx, ok, 11, 2, expect_rc=-1)
    run_ex(ctx, ok, 4, 1, lda_pad=4, expect_rc=-1)
    run_ex(ctx, ok, 5, 1, G=4, L=4, expect_rc=-1)


def run_ex10(ctx, c, gamma=None, chain=0, stop=0, bias=True, pad=8):
    """Epilogue 10 on gemm_ring2 through hg_test_gemm_ex: lda = K + 64, ldc = ld2 = ld3 = N + pad -> x, out2, out3 [M, N], mr_out, mu_out;
    asserts the canary rows and columns of x and the 0x5A5A (203.25) columns behind N of the fp16 copies"""
    M, N, K = c["M"], c["N"], c["K"]
    p = lambda t: t.data_ptr() if t is not None else None
    a = torch.full((M, K + 64), JUNK, device="cuda")
    a[:, :K] = c["a"].cuda()
    x = padded(M, N + pad)
    x[:M, :N] = c["x0"][:M].cuda()
    out2, out3, mr_out, mu_out = padded(M, N + pad), padded(M, N + pad), padded(M, 2), padded(M, 1)
    w, b, mu = c["w"].cuda(), c["bias"].cuda() if bias else None, c["mu"].cuda()
    args = _lib.hg_test_gemm_ex_args(a=p(a), w=p(w), bias=p(b), out=p(x), mu=p(mu), gamma=p(gamma), out2=p(out2),
                                     out3=p(out3) if gamma is not None else None, mr_out=p(mr_out), mu_out=p(mu_out), M=M, N=N, K=K,
                                     lda=K + 64, ldc=N + pad, epi=10, kernel=4, chain=chain, stop=stop)
    rc = _lib.lib().hg_test_gemm_ex(ctx, C.byref(args), None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().hg_last_error(ctx)
    for buf in (x, out2, out3, mr_out, mu_out):
        assert canary_intact(buf, M)
    assert bool((x[:M, N:].view(torch.int32) == CANARY).all()), "columns behind N of the stream were written"
    for buf in (out2,) + ((out3,) if gamma is not None else ()):
        assert bool((buf[:M, N:] == 203.25).all()), "columns behind N of an fp16 copy were written"
    return {"out": x[:M, :N].contiguous(), "out2": out2[:M, :N].contiguous(), "out3": out3[:M, :N].contiguous(), "mr_out": mr_out[:M],
            "mu_out": mu_out[:M, 0]}


@pytest.mark.parametrize("M,N,K", [(641, 256, 256), (769, 768, 320)])
@pytest.mark.parametrize("family", ["exact", "randn"])
def test_residual_epilogue_own_strides_and_gamma_scaled_copy(ctx, family, M, N, K):
    """GemmArgs::ld2 / gamma / out3 / hl on gemm_ring2 (the text tower's text_ln_fold = 1 default writes its scaled copy this way).
    fp32 stream (hl 0): stream, statistics and copy within the bounds of tests/gemm_bound.py with ld2 != N, the stream bit for bit
    what hg_test_gemm_ln returns; with gamma the copy is fp16((x - mu) gamma) of the returned stream within one fp16 rounding and the
    two fp32 operations.  Stream as centre + hi + lo (hl 1, 2, 3): gamma changes neither the hi half in out2 nor the statistics nor the
    final stream, by a single bit; out3 is the scaled copy of the value out2 is the rounding of; after the last launch out2 is the
    scaled copy of the returned stream."""
    c = gb.make_case(family, M, N, K)
    gamma = (1.0 + c["scale"]).cuda()
    g64, mu64 = gamma.cpu().double(), c["mu"].double()
    plain = run_ex10(ctx, c)
    r = gb.ratios(c, 10, {k: v.cpu() for k, v in plain.items()})
    print(f"GEMM_RATIO ring2 10 {family} ld2 M {M} N {N} K {K}: " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r
    assert torch.equal(plain["out"], Launcher(ctx, c)(10, 2)["out"])
    scaled = run_ex10(ctx, c, gamma)
    assert all(torch.equal(scaled[k], plain[k]) for k in ("out", "mr_out", "mu_out")), "gamma changed the stream or its statistics"
    want, B = gb.scaled_copy_reference(scaled["out"].cpu().double() - mu64[:, None], g64)
    w = gb._worst(scaled["out2"], want, B)
    print(f"GEMM_RATIO ring2 10 {family} scaled copy (hl 0) M {M} N {N} K {K}: worst |err| / B {w:.3f}")
    assert w <= 1.0
    # the stream as centre + hi + lo: three launches planned, stopped after 1, 2, 3
    x1, B1 = gb.reference(c, 10)
    for stop in (1, 2):
        hl, hl_g = run_ex10(ctx, c, None, 3, stop), run_ex10(ctx, c, gamma, 3, stop)
        assert all(torch.equal(hl_g[k], hl[k]) for k in ("out2", "mr_out", "mu_out")), f"launch {stop}: gamma changed the hi half or the statistics"
        assert torch.equal(hl["out"].cpu(), c["x0"][:M]), "the fp32 stream is not written while it travels as hi + lo"
        hi = hl_g["out2"].cpu().double()
        # out2 = fp16(d), out3 = fp16(fl(d gamma)) of the same fp32 d, |d| <= |hi| (1 + 2^-10): hi's own rounding times |gamma|, then out3's
        hg = (hi * g64[None]).abs()
        B3 = g64.abs()[None] * gb.f16_term(hi.abs() * (1 + 2.0 ** -10)) + gb.f16_term(hg * (1 + 2.0 ** -10)) + 2 * gb.U * hg
        w3 = gb._worst(hl_g["out3"], hi * g64[None], B3)
        print(f"GEMM_RATIO ring2 10 {family} scaled copy against hi (hl {stop}) M {M} N {N} K {K}: worst |err| / B {w3:.3f}")
        assert w3 <= 1.0
        if stop == 1:      # the first hi half against float64: the stream's bound, the subtraction, the fp16 rounding
            d1 = x1 - mu64[:, None]
            w1 = gb._worst(hl["out2"], d1, B1 + gb.U * d1.abs() + gb.f16_term(d1.abs() + B1))
            print(f"GEMM_RATIO ring2 10 {family} hi (hl 1) M {M} N {N} K {K}: worst |err| / B {w1:.3f}")
            assert w1 <= 1.0
    centre = hl["mu_out"].cpu().double()          # the mean after the second launch: what the third centres its copy on
    last, last_g = run_ex10(ctx, c, None, 3, 3), run_ex10(ctx, c, gamma, 3, 3)
    assert all(torch.equal(last_g[k], last[k]) for k in ("out", "mr_out", "mu_out")), "gamma changed the final stream or its statistics"
    d = last_g["out"].cpu().double() - centre[:, None]
    want, B = gb.scaled_copy_reference(d, g64)
    w = gb._worst(last_g["out2"], want, B)
    print(f"GEMM_RATIO ring2 10 {family} scaled copy (hl 3) M {M} N {N} K {K}: worst |err| / B {w:.3f}")
    assert w <= 1.0
    s = gb.stats_reference(last["out"], centre)
    assert gb._worst(last["out2"], s["copy"], s["B_copy"]) <= 1.0 and gb._worst(last["mu_out"], s["mean"], s["B_mean"]) <= 1.0
    assert gb._worst(last["mr_out"][:, 1], s["rstd"], s["B_rstd"]) <= 1.0
    # the final stream against float64: what the halves carry (test_residual_stream_as_centre_hi_lo: 2^-14 of the row's spread per update)
    x3 = c["x0"][:M].double() + 3 * (x1 - c["x0"][:M].double())
    spread = (x3 - x3.mean(1, keepdim=True)).abs().amax(1, keepdim=True)
    assert float(((last["out"].cpu().double() - x3).abs() / spread).max()) <= 3 * 2.0 ** -14 * 1.02
