// Test hooks: single kernels behind the C ABI, operands rounded to fp16 on the device (tests/test_gpu_gemm.py, test_gpu_attention*.py,
// test_gpu_qkv_attn_bound.py);
// hg_test_elem: one launcher of hg_elem.hip on the caller's own buffers, nothing converted (tests/test_gpu_elem.py).
#include "hg_host.h"

extern "C" {

// Test hook: out[M,N] (fp32) (+)= epilogue(A[M,K] x W[N,K]^T) with the operands rounded to fp16 on the device.
// kernel: 0 = dispatcher's choice, 1 = simple 128x128 kernel, 2 = persistent ring kernels, 3 = two-workgroups-per-CU (duo) kernel.
int hg_test_gemm(hg_ctx* c, const float* a, const float* w, const float* bias, float* out, int M, int N, int K,
                 int epi, int kernel, void* stream) {
    if (!c || !a || !w || !out || M <= 0) return HG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    int rc = ensure(c, c->h, rup(M, 256) * K * 2);
    if (!rc) rc = ensure(c, c->att, (size_t)N * K * 2);
    const bool f16out = (epi == EPI_BIAS_F16 || epi == EPI_BIAS_QGELU_F16 || epi == EPI_BIAS_RELU_F16);
    if (!rc && f16out) rc = ensure(c, c->qkv, rup(M, 256) * N * 2);
    // EPI_RESID_LN_F32 (timing only): centred fp16 copy into the qkv buffer, partial statistics + zero centres into cq
    const bool rln = (epi == EPI_RESID_LN_F32);
    const int sld = 4 * N / 256;
    if (!rc && rln) rc = ensure(c, c->qkv, rup(M, 256) * N * 2);
    if (!rc && rln) rc = ensure(c, c->cq, rup(M, 256) * (size_t)(2 * sld + 1) * 4);
    if (rc) return rc;
    HG_HIP(launch_f32_to_f16(a, (half_t*)c->h.p, (size_t)M * K, s));
    HG_HIP(launch_f32_to_f16(w, (half_t*)c->att.p, (size_t)N * K, s));
    GemmArgs g = gemm_args((half_t*)c->h.p, K, (half_t*)c->att.p, bias, f16out ? c->qkv.p : (void*)out, N, M, N, K);
    if (rln) {
        g.out2 = (half_t*)c->qkv.p; g.stats = (float*)c->cq.p; g.stats_ld = sld;
        g.mu = (float*)c->cq.p + (size_t)rup(M, 256) * 2 * sld;
        HG_HIP(hipMemsetAsync((void*)g.mu, 0, (size_t)M * 4, s));
    }
    hipError_t e;
    ProfScope ps(c, s, epi, M, N, K);
    if (kernel == 1) e = launch_gemm_simple(epi, g, s);
    else if (kernel == 2) e = gemm_ring_ok(g) ? launch_gemm_ring(epi, g, s) : hipErrorInvalidValue;
    else if (kernel == 3) e = gemm_duo_ok(epi, g) ? launch_gemm_duo(epi, g, s) : hipErrorInvalidValue;
    else e = launch_gemm(epi, g, s);
    ps.finish();
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "test gemm launch failed: %s", hipGetErrorString(e));
    if (f16out) HG_HIP(launch_f16_to_f32((const half_t*)c->qkv.p, out, (size_t)M * N, s));
    return HG_OK;
}

int hg_test_gemm_ln(hg_ctx* c, const float* a, const float* w, const float* bias, float* out, int M, int N, int K, int epi,
                    int kernel, const float* cs, const float* mr, const float* mu, const float* scale, float* out2,
                    float* mr_out, float* mu_out, void* stream) {
    if (!c || !a || !w || !out || M <= 0) return HG_ERR_INVALID;
    const bool lnc = (epi == EPI_LN_BIAS_F16 || epi == EPI_LN_BIAS_QGELU_F16);
    const bool rln = (epi == EPI_RESID_LN_F32 || epi == EPI_SCALE_RESID_LN_F32);
    if (!lnc && !rln) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ln: epi must be 8, 9, 10 or 12");
    if (lnc && (!cs || !mr)) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ln: epi 8/9 need cs and mr");
    if (rln && (!mu || !out2 || !mr_out || !mu_out || (epi == EPI_SCALE_RESID_LN_F32 && !scale)))
        return fail(c, HG_ERR_INVALID, "hg_test_gemm_ln: epi 10/12 need mu, out2, mr_out, mu_out (12: scale)");
    if (N % 256) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ln: N must be a multiple of 256");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t Mp = rup(M, 256);
    const int sld = 4 * (N / 256);
    int rc = ensure(c, c->h, Mp * K * 2);
    if (!rc) rc = ensure(c, c->att, (size_t)N * K * 2);
    if (!rc) rc = ensure(c, c->qkv, Mp * N * 2);
    if (!rc) rc = ensure(c, c->mr, Mp * 2 * 4);
    if (!rc) rc = ensure(c, c->mu, Mp * 4);
    if (!rc) rc = ensure(c, c->stats, Mp * (size_t)sld * 2 * 4);
    if (rc) return rc;
    HG_HIP(launch_f32_to_f16(a, (half_t*)c->h.p, (size_t)M * K, s));
    HG_HIP(launch_f32_to_f16(w, (half_t*)c->att.p, (size_t)N * K, s));
    GemmArgs g = gemm_args((half_t*)c->h.p, K, (half_t*)c->att.p, bias, nullptr, N, M, N, K);
    if (lnc) {
        HG_HIP(hipMemsetAsync(c->mr.p, 0, Mp * 2 * 4, s));                  // padded rows are read by the tile's DMA
        HG_HIP(hipMemcpyAsync(c->mr.p, mr, (size_t)M * 2 * 4, hipMemcpyDeviceToDevice, s));
        g.cs = cs; g.mr = (const float*)c->mr.p; g.out = c->qkv.p;
    } else {
        HG_HIP(hipMemcpyAsync(c->mu.p, mu, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
        g.out = out; g.out2 = (half_t*)c->qkv.p; g.stats = (float*)c->stats.p; g.stats_ld = sld; g.mu = (const float*)c->mu.p;
        g.pos = scale;
    }
    hipError_t e;
    if (kernel == 2) {
        ProfScope ps(c, s, epi, M, N, K);
        e = gemm_ln_ok(epi, g) ? launch_gemm_ring(epi, g, s) : hipErrorInvalidValue;
    } else if (kernel == 3) e = gemm_duo_ok(epi, g) ? launch_gemm_duo(epi, g, s) : hipErrorInvalidValue;
    else e = launch_gemm(epi, g, s);
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "test gemm (ln) launch failed: %s", hipGetErrorString(e));
    if (lnc) {
        HG_HIP(launch_f16_to_f32((const half_t*)c->qkv.p, out, (size_t)M * N, s));
    } else {
        HG_HIP(launch_f16_to_f32((const half_t*)c->qkv.p, out2, (size_t)M * N, s));
        HG_HIP(launch_finalize_stats((const float*)c->stats.p, (float*)c->mr.p, (float*)c->mu.p, M, sld, 64, s));
        HG_HIP(hipMemcpyAsync(mr_out, c->mr.p, (size_t)M * 2 * 4, hipMemcpyDeviceToDevice, s));
        HG_HIP(hipMemcpyAsync(mu_out, c->mu.p, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    }
    return HG_OK;
}

int hg_test_gemm_hilo(hg_ctx* c, const float* a, const float* w, const float* bias, float* x, int M, int N, int K, int steps,
                      int hilo, float* mu, float* out2, float* mr_out, void* stream) {
    if (!c || !a || !w || !x || !mu || M <= 0 || steps < 1 || steps > 16) return HG_ERR_INVALID;
    if (N % 256) return fail(c, HG_ERR_INVALID, "hg_test_gemm_hilo: N must be a multiple of 256");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t Mp = rup(M, 256);
    const int sld = 4 * (N / 256);
    int rc = ensure(c, c->h, Mp * K * 2);
    if (!rc) rc = ensure(c, c->att, (size_t)N * K * 2);
    if (!rc) rc = ensure(c, c->qkv, Mp * N * 2);
    if (!rc) rc = ensure(c, c->mr, Mp * 2 * 4);
    if (!rc) rc = ensure(c, c->mu, Mp * 4);
    if (!rc) rc = ensure(c, c->muc, Mp * 4);
    if (!rc) rc = ensure(c, c->stats, Mp * (size_t)sld * 2 * 4);
    if (!rc) rc = ensure(c, c->xlo, gemm_lo_bytes(M, N));
    if (rc) return rc;
    HG_HIP(launch_f32_to_f16(a, (half_t*)c->h.p, (size_t)M * K, s));
    HG_HIP(launch_f32_to_f16(w, (half_t*)c->att.p, (size_t)N * K, s));
    HG_HIP(hipMemcpyAsync(c->mu.p, mu, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    GemmArgs g = gemm_args((half_t*)c->h.p, K, (half_t*)c->att.p, bias, x, N, M, N, K);
    g.out2 = (half_t*)c->qkv.p; g.stats = (float*)c->stats.p; g.stats_ld = sld; g.mu = (const float*)c->mu.p;
    g.lo = (half_t*)c->xlo.p; g.muc = (const float*)c->muc.p;
    if (!gemm_ring2_ok(g)) return fail(c, HG_ERR_INVALID, "hg_test_gemm_hilo: shape not eligible for gemm_ring2");
    for (int i = 0; i < steps; ++i) {
        g.hl = (hilo && steps >= 2) ? (i == 0 ? 1 : (i == steps - 1 ? 3 : 2)) : 0;
        ProfScope ps(c, s, EPI_RESID_LN_F32, M, N, K);
        hipError_t e = launch_gemm_ring2(EPI_RESID_LN_F32, g, s);
        ps.finish();
        if (e != hipSuccess) return fail(c, HG_ERR_HIP, "test gemm (hi / lo) launch failed: %s", hipGetErrorString(e));
        HG_HIP(launch_finalize_stats((const float*)c->stats.p, (float*)c->mr.p, (float*)c->mu.p, M, sld, 64, s, (float*)c->muc.p));
    }
    if (out2) HG_HIP(launch_f16_to_f32((const half_t*)c->qkv.p, out2, (size_t)M * N, s));
    if (mr_out) HG_HIP(hipMemcpyAsync(mr_out, c->mr.p, (size_t)M * 2 * 4, hipMemcpyDeviceToDevice, s));
    HG_HIP(hipMemcpyAsync(mu, c->mu.p, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    return HG_OK;
}

// hg_test_gemm_ex, epi 10: gemm_ring2's residual epilogue with the copy's own row stride (ld2), the copy scaled by gamma (out3, ld3) and
// the stream as fp32 (chain = 0: one launch) or as centre + hi + lo (chain >= 2 launches planned, hl = 1, 2 .., 3; the first `stop` made).
// The fp16 buffers are filled with the byte 0x5A first, so that the columns behind N of a row come back as 203.25.
static int gemm_ex_resid_ln(hg_ctx* c, const hg_test_gemm_ex_args* x, hipStream_t s) {
    const int M = x->M, N = x->N, K = x->K, lda = x->lda, ldc = x->ldc;
    const int ld2 = x->ld2 ? x->ld2 : ldc, ld3 = x->ld3 ? x->ld3 : ldc;
    const int chain = x->chain, stop = chain ? x->stop : 1;
    if (x->kernel != 4) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: epi 10 runs on kernel 4 (ring2) here");
    if (!x->mu || !x->out2 || !x->mr_out || !x->mu_out) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: epi 10 needs mu, out2, mr_out, mu_out");
    if (N % 256 || ld2 < N || ld3 < N || ld2 % 8 || ld3 % 8) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: epi 10 needs N % 256 == 0, ld2 and ld3 >= N, multiples of 8");
    if (chain && (chain < 2 || chain > 16 || stop < 1 || stop > chain)) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: chain is 0 or 2 .. 16, 1 <= stop <= chain");
    if (x->out3 && !x->gamma) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: out3 goes with gamma");
    const size_t Mp = rup(M, 256);
    const int sld = 4 * (N / 256);
    GemmArgs g = gemm_args(nullptr, lda, nullptr, x->bias, x->out, ldc, M, N, K);
    if (!gemm_ring2_ok(g)) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: the shape is not eligible for kernel 4");
    int rc = ensure(c, c->h, Mp * lda * 2);
    if (!rc) rc = ensure(c, c->att, (size_t)N * K * 2);
    if (!rc) rc = ensure(c, c->qkv, Mp * ld2 * 2);
    if (!rc) rc = ensure(c, c->hg, Mp * ld3 * 2);
    if (!rc) rc = ensure(c, c->mr, Mp * 2 * 4);
    if (!rc) rc = ensure(c, c->mu, Mp * 4);
    if (!rc) rc = ensure(c, c->muc, Mp * 4);
    if (!rc) rc = ensure(c, c->stats, Mp * (size_t)sld * 2 * 4);
    if (!rc) rc = ensure(c, c->xlo, gemm_lo_bytes(M, N));
    if (rc) return rc;
    HG_HIP(launch_f32_to_f16(x->a, (half_t*)c->h.p, (size_t)M * lda, s));
    HG_HIP(launch_f32_to_f16(x->w, (half_t*)c->att.p, (size_t)N * K, s));
    HG_HIP(hipMemcpyAsync(c->mu.p, x->mu, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    HG_HIP(hipMemsetAsync(c->qkv.p, 0x5A, Mp * ld2 * 2, s));
    HG_HIP(hipMemsetAsync(c->hg.p, 0x5A, Mp * ld3 * 2, s));
    g.A = (const half_t*)c->h.p; g.W = (const half_t*)c->att.p;
    g.out2 = (half_t*)c->qkv.p; g.ld2 = ld2; g.stats = (float*)c->stats.p; g.stats_ld = sld; g.mu = (const float*)c->mu.p;
    g.lo = (half_t*)c->xlo.p; g.muc = (const float*)c->muc.p;
    g.gamma = x->gamma; g.out3 = (half_t*)c->hg.p; g.ld3 = ld3;
    for (int i = 0; i < stop; ++i) {
        g.hl = chain ? (i == 0 ? 1 : (i == chain - 1 ? 3 : 2)) : 0;
        ProfScope ps(c, s, EPI_RESID_LN_F32, M, N, K);
        hipError_t e = launch_gemm_ring2(EPI_RESID_LN_F32, g, s);
        ps.finish();
        if (e != hipSuccess) return fail(c, HG_ERR_HIP, "test gemm (ex, epi 10) launch failed: %s", hipGetErrorString(e));
        HG_HIP(launch_finalize_stats((const float*)c->stats.p, (float*)c->mr.p, (float*)c->mu.p, M, sld, 64, s, (float*)c->muc.p));
    }
    HG_HIP(launch_f16_to_f32((const half_t*)c->qkv.p, x->out2, (size_t)M * ld2, s));
    if (x->out3) HG_HIP(launch_f16_to_f32((const half_t*)c->hg.p, x->out3, (size_t)M * ld3, s));
    HG_HIP(hipMemcpyAsync(x->mr_out, c->mr.p, (size_t)M * 2 * 4, hipMemcpyDeviceToDevice, s));
    HG_HIP(hipMemcpyAsync(x->mu_out, c->mu.p, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    return HG_OK;
}

// One GEMM launch with the arguments the hooks above cannot set (include/hoigen_amd.h has the contract).  Nothing is launched unless the
// chosen kernel's own eligibility test accepts the call.
int hg_test_gemm_ex(hg_ctx* c, const hg_test_gemm_ex_args* x, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x || !x->a || !x->w || !x->out || x->M <= 0 || x->N <= 0 || x->K <= 0) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: a, w, out and M, N, K > 0 are required");
    const int M = x->M, N = x->N, K = x->K, lda = x->lda, ldc = x->ldc, epi = x->epi;
    const bool f16out = (epi == EPI_BIAS_F16 || epi == EPI_BIAS_QGELU_F16 || epi == EPI_BIAS_RELU_F16);
    const bool f32out = (epi == EPI_BIAS_RESID_F32 || epi == EPI_BIAS_F32 || epi == EPI_PATCH_F32 || epi == EPI_BIAS_RELU_F32 ||
                         epi == EPI_SCALE_RESID_F32 || epi == EPI_MU_BIAS_RELU_F32);
    if (epi == EPI_RESID_LN_F32) {
        if (lda < K || ldc < N || lda % 8 || ldc % 8) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: lda >= K, ldc >= N, both multiples of 8");
        HG_ON_DEVICE(c);
        return gemm_ex_resid_ln(c, x, (hipStream_t)stream);
    }
    if (!f16out && !f32out) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: epi must be 0 .. 7, 10 or 11");
    // (two destinations: a row of either holds its own half only)
    const int cols = x->out_hi ? (x->n_split > N - x->n_split ? x->n_split : N - x->n_split) : N;
    if (lda < K || ldc < cols || lda % 8 || ldc % 8) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: lda >= K, ldc >= N (with out_hi: the wider half), both multiples of 8");
    if (epi == EPI_PATCH_F32 && (x->G <= 0 || x->L <= x->G || M % x->G)) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: epi 5 needs 0 < G < L and M a multiple of G");
    if (epi == EPI_SCALE_RESID_F32 && !x->scale) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: epi 7 needs scale");
    if (epi == EPI_MU_BIAS_RELU_F32 && (!x->mu || !x->cs || x->n_split < 0 || x->n_split % 16)) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: epi 11 needs mu, cs and n_split a multiple of 16");
    if (x->out_hi && !((epi == EPI_BIAS_F32 || epi == EPI_BIAS_RELU_F32) && x->n_split > 0 && x->n_split < N && x->n_split % 16 == 0))
        return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: out_hi goes with epi 4 / 6 and 0 < n_split < N, a multiple of 16");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    GemmArgs g = gemm_args(nullptr, lda, nullptr, x->bias, x->out, ldc, M, N, K);
    g.G = x->G; g.L = x->L;
    g.pos = epi == EPI_PATCH_F32 ? x->pos : (epi == EPI_SCALE_RESID_F32 ? x->scale : nullptr);
    if (epi == EPI_MU_BIAS_RELU_F32) { g.mu = x->mu; g.cs = x->cs; g.n_split = x->n_split; }
    if (x->out_hi) { g.out_hi = x->out_hi; g.n_split = x->n_split; }
    const bool simple_ok = N % 128 == 0 && K % 64 == 0;
    bool ok;
    switch (x->kernel) {
        case 0: ok = simple_ok || (epi != EPI_MU_BIAS_RELU_F32 && gemm_ring_ok(g)); break;
        case 1: ok = simple_ok; break;
        case 2: ok = epi != EPI_MU_BIAS_RELU_F32 && gemm_ring_ok(g); break;
        case 3: ok = gemm_duo_ok(epi, g); break;
        case 4: ok = epi != EPI_MU_BIAS_RELU_F32 && gemm_ring2_ok(g); break;
        default: return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: kernel must be 0 .. 4");
    }
    if (!ok) return fail(c, HG_ERR_INVALID, "hg_test_gemm_ex: the shape or epilogue is not eligible for kernel %d", x->kernel);
    const size_t Mp = rup(M, 256);
    int rc = ensure(c, c->h, Mp * lda * 2);
    if (!rc) rc = ensure(c, c->att, (size_t)N * K * 2);
    if (!rc && f16out) rc = ensure(c, c->qkv, Mp * ldc * 2);
    if (!rc && f16out) rc = ensure(c, c->cq, (size_t)M * N * 2);
    if (!rc && f16out) rc = ensure(c, c->fc, (size_t)M * N * 4);
    if (rc) return rc;
    HG_HIP(launch_f32_to_f16(x->a, (half_t*)c->h.p, (size_t)M * lda, s));
    HG_HIP(launch_f32_to_f16(x->w, (half_t*)c->att.p, (size_t)N * K, s));
    g.A = (const half_t*)c->h.p; g.W = (const half_t*)c->att.p;
    if (f16out) g.out = c->qkv.p;
    hipError_t e;
    {
        ProfScope ps(c, s, epi, M, N, K);
        if (x->kernel == 1) e = launch_gemm_simple(epi, g, s);
        else if (x->kernel == 2) e = launch_gemm_ring(epi, g, s);
        else if (x->kernel == 3) e = launch_gemm_duo(epi, g, s);
        else if (x->kernel == 4) e = launch_gemm_ring2(epi, g, s);
        else e = launch_gemm(epi, g, s);
    }
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "test gemm (ex) launch failed: %s", hipGetErrorString(e));
    if (f16out) {      // the fp16 rows (stride ldc) -> dense -> fp32 -> the caller's rows (stride ldc): columns >= N of `out` stay untouched
        HG_HIP(hipMemcpy2DAsync(c->cq.p, (size_t)N * 2, c->qkv.p, (size_t)ldc * 2, (size_t)N * 2, M, hipMemcpyDeviceToDevice, s));
        HG_HIP(launch_f16_to_f32((const half_t*)c->cq.p, (float*)c->fc.p, (size_t)M * N, s));
        HG_HIP(hipMemcpy2DAsync(x->out, (size_t)ldc * 4, c->fc.p, (size_t)N * 4, (size_t)N * 4, M, hipMemcpyDeviceToDevice, s));
    }
    return HG_OK;
}

int hg_test_attention(hg_ctx* c, const float* qkv, const float* q0, const int32_t* sel, int n_seq, int L, int heads,
                      int causal, float* out, void* stream) {
    if (!c || !qkv || !out || n_seq <= 0 || L < 1 || L > ATTN_LONG_MAX_L || heads < 1) return HG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const int D = heads * 64;
    const size_t M = (size_t)n_seq * L;
    int rc = ensure(c, c->qkv, rup(M, 256) * 3 * D * 2);
    if (!rc) rc = ensure(c, c->att, rup(M, 256) * D * 2);
    if (!rc && q0) rc = ensure(c, c->cq, rup(n_seq, 256) * (size_t)D * 2);
    if (rc) return rc;
    HG_HIP(launch_f32_to_f16(qkv, (half_t*)c->qkv.p, M * 3 * D, s));
    if (q0) {      // one query row per sequence (row sel[seq], or 0): out [n_seq, D]
        HG_HIP(launch_f32_to_f16(q0, (half_t*)c->cq.p, (size_t)n_seq * D, s));
        HG_HIP(launch_attention_row0((const half_t*)c->qkv.p, (const half_t*)c->cq.p, sel, (half_t*)c->att.p, n_seq, L,
                                     heads, (causal & 1) != 0, s));
        HG_HIP(launch_f16_to_f32((const half_t*)c->att.p, out, (size_t)n_seq * D, s));
    } else {
        // (causal bit 1: the one-workgroup-per-item launch for L <= 32 instead of four items per workgroup - same bits: tests)
        ProfScope ps(c, s, HG_PROF_ATTENTION, n_seq, L, heads);      // the kernel alone, as attention() above (tools/bench_vitl336.py)
        HG_HIP(launch_attention((const half_t*)c->qkv.p, (half_t*)c->att.p, n_seq, L, heads, (causal & 1) != 0, s, 0, !(causal & 2)));
        ps.finish();
        HG_HIP(launch_f16_to_f32((const half_t*)c->att.p, out, M * D, s));
    }
    return HG_OK;
}

// The DETR attention kernel alone (hg_detr_attn.hip) on fp32 arrays that hold fp16 values (include/hoigen_amd.h has the contract;
// tests/test_gpu_detr_attention.py).  Every refusal is decided before anything is written.
int hg_test_detr_attention(hg_ctx* c, const float* q, const float* k, const float* v, const uint8_t* mask, int n_seq, int Lq, int Lk,
                           int heads, int chunk, int layout, int ldo, float* out, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!q || !k || !v || !out || n_seq < 1 || heads < 1) return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: q, k, v, out, n_seq >= 1 and heads >= 1 are required");
    if (Lq < 1 || Lk < 1 || Lq > DETR_ATTN_MAX_L || Lk > DETR_ATTN_MAX_L)
        return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: Lq and Lk must be 1 .. %d (got %d, %d)", DETR_ATTN_MAX_L, Lq, Lk);
    if (chunk < 0) chunk = c->opt_detr_attn_chunk;
    if (chunk % 32 || chunk > DETR_ATTN_RESIDENT_L) return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: chunk must be 0 or a multiple of 32 up to %d", DETR_ATTN_RESIDENT_L);
    if (layout < 0 || layout > 2 || (layout != 1 && Lq != Lk)) return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: layout 0 .. 2; 0 and 2 need Lq == Lk");
    const int D = heads * 32;
    if (!ldo) ldo = D;
    if (ldo < D || ldo % 8) return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: ldo >= heads * 32, a multiple of 8");
    if ((long long)n_seq * (Lq > Lk ? Lq : Lk) > (1LL << 20)) return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: at most 2^20 rows");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t Mq = (size_t)n_seq * Lq, Mk = (size_t)n_seq * Lk;
    int rc = ensure(c, c->qkv, (Mq + 2 * Mk) * D * 2);      // the three operands, dense, then interleaved into `h` as the layout asks
    if (!rc) rc = ensure(c, c->h, (Mq + 2 * Mk) * D * 2);
    if (!rc) rc = ensure(c, c->att, (Mq + 8) * ldo * 2);
    if (rc) return rc;
    HG_HIP(hipMemsetAsync(c->att.p, 0x5A, (Mq + 8) * ldo * 2, s));      // what the kernel does not write comes back as 203.25
    half_t* d16 = (half_t*)c->qkv.p;
    HG_HIP(launch_f32_to_f16(q, d16, Mq * D, s));
    HG_HIP(launch_f32_to_f16(k, d16 + Mq * D, Mk * D, s));
    HG_HIP(launch_f32_to_f16(v, d16 + (Mq + Mk) * D, Mk * D, s));
    DetrAttnArgs da{};
    half_t* b = (half_t*)c->h.p;
    if (layout == 1) {
        da.q = d16; da.k = d16 + Mq * D; da.v = d16 + (Mq + Mk) * D; da.ldq = da.ldk = da.ldv = D;
    } else {      // columns q | k (| v) of one buffer
        const int ld = layout == 0 ? 2 * D : 3 * D;
        HG_HIP(hipMemcpy2DAsync(b, (size_t)ld * 2, d16, (size_t)D * 2, (size_t)D * 2, Mq, hipMemcpyDeviceToDevice, s));
        HG_HIP(hipMemcpy2DAsync(b + D, (size_t)ld * 2, d16 + Mq * D, (size_t)D * 2, (size_t)D * 2, Mk, hipMemcpyDeviceToDevice, s));
        da.q = b; da.k = b + D; da.ldq = da.ldk = ld;
        if (layout == 2) {
            HG_HIP(hipMemcpy2DAsync(b + 2 * D, (size_t)ld * 2, d16 + (Mq + Mk) * D, (size_t)D * 2, (size_t)D * 2, Mk, hipMemcpyDeviceToDevice, s));
            da.v = b + 2 * D; da.ldv = ld;
        } else {
            da.v = d16 + (Mq + Mk) * D; da.ldv = D;
        }
    }
    da.mask = mask; da.out = (half_t*)c->att.p; da.ldo = ldo; da.n_seq = n_seq; da.Lq = Lq; da.Lk = Lk; da.heads = heads; da.chunk = chunk;
    da.waves = c->opt_detr_attn_waves;
    if (da.waves == 3) return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: option detr_attn_waves must be 0, 1, 2 or 4");
    hipError_t e;
    {
        ProfScope ps(c, s, HG_PROF_ATTENTION, n_seq, Lk, heads);
        e = launch_detr_attention(da, s);
    }
    if (e == hipErrorInvalidValue) return fail(c, HG_ERR_INVALID, "hg_test_detr_attention: refused by the launcher");
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_test_detr_attention: launch failed: %s", hipGetErrorString(e));
    HG_HIP(launch_f16_to_f32((const half_t*)c->att.p, out, (Mq + 8) * ldo, s));
    return HG_OK;
}

// The FFN of a DETR decoder layer with its tail (hg_detr_ffn.hip or the two GEMMs, then detr_dec_tail_kernel), as hg_detr_decoder runs
// it (include/hoigen_amd.h has the contract; tests/test_gpu_detr_ffn.py).  Every refusal is decided before anything is written.
int hg_test_detr_ffn(hg_ctx* c, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* norm_w,
                     const float* norm_b, int M, int D, int F, float* y, float* partials, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x || !w1 || !b1 || !w2 || !b2 || !norm_w || !norm_b || !y) return fail(c, HG_ERR_INVALID, "hg_test_detr_ffn: every input and y are required");
    if (M < 1 || M > (1 << 20) || D < 128 || D % 128 || D > 512 || F < 128 || F % 128)
        return fail(c, HG_ERR_INVALID, "hg_test_detr_ffn: 1 <= M <= 2^20, D a multiple of 128 up to 512, F a multiple of 128 (got %d, %d, %d)", M, D, F);
    const bool fits = detr_ffn_ok(M, D, F);
    if (c->opt_detr_ffn == 2 && !fits) return fail(c, HG_ERR_INVALID, "hg_test_detr_ffn: option detr_ffn = 2, and the split kernel does not cover this shape");
    const bool split = c->opt_detr_ffn == 2 || (c->opt_detr_ffn == 0 && fits && M <= c->opt_detr_ffn_max_m);
    if (partials && !split) return fail(c, HG_ERR_INVALID, "hg_test_detr_ffn: partials exist on the split kernel's path only");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t Mp = rup(M, 256), n_sl = F / DETR_FFN_SLICE;
    const size_t o_w1 = 0, o_w2 = o_w1 + (size_t)F * D * 2, o_x = o_w2 + (size_t)F * D * 2, o_x16 = o_x + Mp * D * 4, o_x16o = o_x16 + Mp * D * 2,
                 o_ff = o_x16o + Mp * D * 2, total = o_ff + std::max(Mp * F * 2, rup(detr_ffn_partial_bytes(M, D, F), 256));
    int rc = ensure(c, c->cx, total);
    if (rc) return rc;
    char* ws = (char*)c->cx.p;
    half_t *w1h = (half_t*)(ws + o_w1), *w2h = (half_t*)(ws + o_w2), *x16 = (half_t*)(ws + o_x16), *x16o = (half_t*)(ws + o_x16o), *ff = (half_t*)(ws + o_ff);
    float *xs = (float*)(ws + o_x), *part = (float*)(ws + o_ff);
    HG_HIP(launch_f32_to_f16(w1, w1h, (size_t)F * D, s));
    HG_HIP(launch_f32_to_f16(w2, w2h, (size_t)F * D, s));
    HG_HIP(launch_f32_to_f16(x, x16, (size_t)M * D, s));
    HG_HIP(hipMemcpyAsync(xs, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    if (split) {
        ProfScope ps(c, s, HG_PROF_DETR_FFN, M, F, D);
        HG_HIP(launch_detr_ffn(x16, w1h, b1, w2h, part, M, D, F, s));
        ps.finish();
        if (partials) HG_HIP(hipMemcpyAsync(partials, part, n_sl * M * D * 4, hipMemcpyDeviceToDevice, s));
    } else {
        HG_HIP(gemm(c, EPI_BIAS_RELU_F16, gemm_args(x16, D, w1h, b1, ff, F, M, F, D), s));
        HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(ff, F, w2h, b2, xs, D, M, D, F), s));
    }
    {
        ProfScope ps(c, s, HG_PROF_DETR_ROWS, M, D, split ? (int)n_sl : 0);
        HG_HIP(launch_detr_dec_tail(xs, split ? b2 : nullptr, split ? part : nullptr, split ? (int)n_sl : 0, norm_w, norm_b, nullptr, x16o, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, 0, 0, 1, M, D, s));
    }
    HG_HIP(hipMemcpyAsync(y, xs, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    return HG_OK;
}

// One call of the fused in_proj + attention kernels, or of the two launches they replace, with the arguments production sets
// (include/hoigen_amd.h has the contract; tests/test_gpu_qkv_attn_bound.py).  Every refusal is decided before anything is written.
int hg_test_qkv_attn_ex(hg_ctx* c, const hg_test_qkv_attn_ex_args* x, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x || !x->a || !x->w || !x->cs || !x->mr || !x->out || x->n_seq <= 0 || x->L <= 0 || x->heads < 1) return HG_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const int n_seq = x->n_seq, L = x->L, heads = x->heads;
    int fused = x->fused;
    const int D = heads * 64, M = n_seq * L;
    const int K = D + ((fused & 2) ? 64 : 0);      // (bit 1: a is [M, D + 64], w [3D, D + 64] - the shape of a block with a folded adapter)
    // bit 2: the causal mask - the text tower's kernel (hg_qkv_attn_text.hip, L <= 80) against the folded GEMM + the causal attention launch
    const bool causal = (fused & 4) != 0;
    if ((fused & ~7) || (causal && (fused & 2))) return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: fused must be 0 .. 5");
    fused &= 1;
    const int lda = x->lda ? x->lda : K, ldo = x->ldo ? x->ldo : D;
    if (lda < K || ldo < D || lda % 8 || ldo % 8) return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: lda >= K, ldo >= D, both multiples of 8");
    if (x->pad_fill != 0 && x->pad_fill != 1) return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: pad_fill is 0 or 1");
    if (x->qkv_out && fused) return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: qkv_out goes with the two launches (fused bit 0 clear)");
    // (the folded ring GEMM wants 512 rows: a shorter causal call runs it over the pad rows up to there - a row's result does not
    // depend on the rows beside it)
    const int Mg = causal && M < 512 ? 512 : M;
    const size_t Mp = rup(Mg, 256);
    if (fused && causal && !qkv_attn_text_ok(n_seq, L, D, heads, lda))
        return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: shape not eligible for the fused causal kernel");
    if (fused && !causal && !qkv_attn_ok(n_seq, L, D, heads, lda, K)) return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: shape not eligible for the fused kernel");
    if (!fused) {
        GemmArgs g = gemm_args(nullptr, lda, nullptr, x->bias, nullptr, 3 * D, Mg, 3 * D, K);
        g.cs = x->cs; g.mr = x->mr;
        if (!gemm_ln_ok(EPI_LN_BIAS_F16, g)) return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: shape not eligible for the folded GEMM");
    }
    int rc = ensure(c, c->h, Mp * lda * 2);
    if (!rc) rc = ensure(c, c->hg, (size_t)M * K * 2);
    if (!rc) rc = ensure(c, c->fc, (size_t)3 * D * K * 2 * 2 + (size_t)(heads / 2 + 1) * 768 * 4);
    if (!rc) rc = ensure(c, c->qkv, Mp * 3 * D * 2);
    if (!rc) rc = ensure(c, c->att, Mp * ldo * 2);
    if (!rc) rc = ensure(c, c->mr, Mp * 2 * 4);
    if (rc) return rc;
    half_t* w16 = (half_t*)c->fc.p;
    half_t* wp = w16 + (size_t)3 * D * K;
    float* bcs = (float*)(wp + (size_t)3 * D * K);
    // rows M .. Mp - 1 and columns K .. lda - 1 of the operand: zeros, or fp16 NaN (the byte 0x7E twice)
    HG_HIP(hipMemsetAsync(c->h.p, x->pad_fill ? 0x7E : 0, Mp * lda * 2, s));
    HG_HIP(launch_f32_to_f16(x->a, (half_t*)c->hg.p, (size_t)M * K, s));
    HG_HIP(hipMemcpy2DAsync(c->h.p, (size_t)lda * 2, c->hg.p, (size_t)K * 2, (size_t)K * 2, M, hipMemcpyDeviceToDevice, s));
    HG_HIP(launch_f32_to_f16(x->w, w16, (size_t)3 * D * K, s));
    HG_HIP(hipMemsetAsync(c->mr.p, 0, Mp * 2 * 4, s));
    HG_HIP(hipMemcpyAsync(c->mr.p, x->mr, (size_t)M * 2 * 4, hipMemcpyDeviceToDevice, s));
    HG_HIP(hipMemsetAsync(c->att.p, 0x5A, Mp * ldo * 2, s));      // what a kernel does not write comes back as 203.25
    if (fused) {
        HG_HIP(launch_pack_qkv(w16, x->bias, x->cs, wp, bcs, D, heads, s, K));
        QkvAttnArgs qa{};
        qa.x16 = (const half_t*)c->h.p; qa.lda = lda; qa.K = K; qa.wp = wp; qa.bcs = bcs; qa.mr = (const float*)c->mr.p;
        qa.out = (half_t*)c->att.p; qa.ldo = ldo; qa.n_seq = n_seq; qa.L = L; qa.D = D; qa.heads = heads;
        qa.gsz = c->opt_qkv_attn_gsz; qa.a_bytes = (unsigned)(Mp * (size_t)lda * 2);
#ifdef HG_STAMPS
        if (!(rc = ensure(c, c->cq, 256 * 8 * 16 * 8))) qa.dbg = (unsigned long long*)c->cq.p;      // read back by tools/qkv_attn_stamps.py
        else return rc;
        HG_HIP(hipMemsetAsync(c->cq.p, 0, 256 * 8 * 16 * 8, s));
#endif
        ProfScope ps(c, s, HG_PROF_QKV_ATTN, n_seq, L, heads);
        hipError_t e = causal ? launch_qkv_attn_text(qa, s) : launch_qkv_attn(qa, s);
        ps.finish();
        if (e == hipErrorInvalidValue) return fail(c, HG_ERR_INVALID, "hg_test_qkv_attn: refused by the launcher");
        if (e != hipSuccess) return fail(c, HG_ERR_HIP, "test qkv_attn launch failed: %s", hipGetErrorString(e));
#ifdef HG_STAMPS
        {      // diagnostic build: median over workgroups of the per-wave s_memtime totals of every phase (hg_qkv_attn.hip QA_ST)
            HG_HIP(hipStreamSynchronize(s));
            std::vector<unsigned long long> hd((size_t)256 * 8 * 16);
            HG_HIP(hipMemcpy(hd.data(), c->cq.p, hd.size() * 8, hipMemcpyDeviceToHost));
            static const char* nm[14] = {"K loop", "drain+barrier", "barrier behind head a", "attention a", "barrier", "head b -> LDS",
                                         "attention b", "barrier", "whole kernel", "LN fold", "head a -> LDS", "K loop: wait A", "K loop: barrier",
                                         "K loop: wait W"};
            for (int wv : {0, 3, 4, 6, 7}) {
                fprintf(stderr, "[stamps] wave %d:", wv);
                for (int k = 0; k < 14; ++k) {
                    std::vector<unsigned long long> v;
                    for (int b = 0; b < 256; ++b) if (hd[((size_t)b * 8 + wv) * 16 + 8]) v.push_back(hd[((size_t)b * 8 + wv) * 16 + k]);
                    if (v.empty()) continue;
                    std::sort(v.begin(), v.end());
                    fprintf(stderr, " %s %llu |", nm[k], v[v.size() / 2]);
                }
                fprintf(stderr, "\n");
            }
        }
#endif
    } else {
        GemmArgs g = gemm_args((const half_t*)c->h.p, lda, w16, x->bias, c->qkv.p, 3 * D, Mg, 3 * D, K);
        g.cs = x->cs; g.mr = (const float*)c->mr.p;
        HG_HIP(gemm(c, EPI_LN_BIAS_F16, g, s));
        HG_HIP(attention(c, (const half_t*)c->qkv.p, (half_t*)c->att.p, n_seq, L, heads, causal, s, ldo));
        if (x->qkv_out) HG_HIP(launch_f16_to_f32((const half_t*)c->qkv.p, x->qkv_out, (size_t)M * 3 * D, s));
    }
    HG_HIP(launch_f16_to_f32((const half_t*)c->att.p, x->out, (size_t)M * ldo, s));
    return HG_OK;
}

// (hg_test_qkv_attn_ex with dense rows and zeroed pad rows)
int hg_test_qkv_attn(hg_ctx* c, const float* a, const float* w, const float* bias, const float* cs, const float* mr, int n_seq,
                     int L, int heads, int fused, float* out, void* stream) {
    hg_test_qkv_attn_ex_args x{};
    x.a = a; x.w = w; x.bias = bias; x.cs = cs; x.mr = mr; x.out = out;
    x.n_seq = n_seq; x.L = L; x.heads = heads; x.fused = fused;
    return hg_test_qkv_attn_ex(c, &x, stream);
}

// One launcher of hg_elem.hip with the caller's own device buffers (include/hoigen_amd.h has the table of operands; tests/test_gpu_elem.py).
int hg_test_elem(hg_ctx* c, int op, const hg_test_elem_args* x, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x) return fail(c, HG_ERR_INVALID, "hg_test_elem: args are required");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    void* const* p = x->p;
    const int32_t* i = x->i;
    auto F = [&](int k) { return (float*)p[k]; };
    auto H = [&](int k) { return (half_t*)p[k]; };
    auto I = [&](int k) { return (int32_t*)p[k]; };
    hipError_t e;
    switch (op) {
        case 0: e = launch_layernorm_f16(F(0), F(1), F(2), H(3), i[0], i[1], I(4), i[2], i[3], s); break;
        case 1: e = launch_layernorm_f32(F(0), F(1), F(2), F(3), i[0], i[1], s, F(4), F(5), i[2]); break;
        case 2: e = launch_layernorm_rowstats(F(0), F(1), F(2), H(3), F(4), F(5), F(6), i[0], i[1], s, F(7), F(8), i[2], i[3]); break;
        case 3: e = launch_rowstats_cast(F(0), H(1), F(2), F(3), i[0], i[1], s, F(4), F(5)); break;
        case 4: e = launch_finalize_stats(F(0), F(1), F(2), i[0], i[1], i[2], s, F(3), i[3] != 0, (int*)p[4]); break;
        case 5: e = launch_fold_ln(H(0), F(1), F(2), F(3), H(4), F(5), F(6), i[0], i[1], s, F(7)); break;
        case 6: e = launch_copy_rows(F(0), F(1), i[0], i[1], i[2], s, I(2)); break;
        case 7: e = launch_copy_rows_hilo(H(0), H(1), F(2), F(3), i[0], i[1], i[2], s); break;
        case 8: e = launch_copy_cols(F(0), i[0], F(1), i[1], i[2], s); break;
        case 9: e = launch_im2col(F(0), H(1), i[0], i[1], i[2], s); break;
        case 10: e = launch_embed_tokens(I(0), i[0], F(1), F(2), F(3), i[1], i[2], i[3], i[4], s); break;
        case 11: e = launch_add_pos(F(0), i[0], F(1), F(2), i[1], i[2], i[3], s); break;
        case 12: e = launch_gather_rows(I(0), F(1), F(2), i[0], i[1], i[2], s); break;
        case 13: e = launch_eot_argmax(I(0), i[0], i[1], I(1), I(2), s); break;
        case 14: e = launch_clamp_eot(I(0), i[0], i[1], I(1), I(2), s, I(3)); break;
        case 15: e = launch_poison_if_flag(F(0), (size_t)x->n, I(1), s); break;
        case 16: e = launch_f32_to_f16(F(0), H(1), (size_t)x->n, s); break;
        case 17: e = launch_f16_to_f32(H(0), F(1), (size_t)x->n, s); break;
        case 18: e = launch_f16_remainder(F(0), H(1), (size_t)x->n, s); break;
        case 19: e = launch_transpose_to_f16(p[0], i[0], H(1), i[1], i[2], s); break;
        case 20: e = launch_l2_normalize(F(0), F(1), i[0], i[1], s); break;
        case 21: e = launch_assemble_prompts(F(0), F(1), F(2), F(3), I(4), i[0], i[1], i[2], i[3], i[4], F(5), s); break;
        case 22: e = launch_vae_loss(F(0), F(1), F(2), F(3), i[0], i[1], F(4), s); break;
        case 23: e = launch_split_global_local(F(0), F(1), F(2), i[0], i[1], i[2], s); break;
        default: return fail(c, HG_ERR_INVALID, "hg_test_elem: op must be 0 .. 23");
    }
    if (e == hipErrorInvalidValue) return fail(c, HG_ERR_INVALID, "hg_test_elem: op %d refused by its launcher: %s", op, hipGetErrorString(e));
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_test_elem: op %d failed: %s", op, hipGetErrorString(e));
    return HG_OK;
}

// One launcher of hg_text_grad.hip with the caller's own device buffers, or one block of the text tower's backward
// (include/hoigen_amd.h has the table of operands; tests/test_gpu_text_grad_kernels.py).
int hg_test_text_grad(hg_ctx* c, int op, const hg_test_elem_args* x, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x) return fail(c, HG_ERR_INVALID, "hg_test_text_grad: args are required");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    void* const* p = x->p;
    const int32_t* i = x->i;
    auto F = [&](int k) { return (float*)p[k]; };
    auto H = [&](int k) { return (half_t*)p[k]; };
    hipError_t e;
    switch (op) {
        case 0: e = launch_text_attn_bwd(H(0), H(1), H(2), i[0], i[1], i[2], s); break;
        case 1: e = launch_layernorm_bwd(F(0), F(1), F(2), F(3), i[0], i[1], (const int32_t*)p[4], i[2], s); break;
        case 2: e = launch_qgelu_bwd(H(0), H(1), H(2), (size_t)x->n, s); break;
        case 3: e = launch_grad_scale(F(0), H(1), F(2), i[0], i[1], s); break;
        case 4: e = launch_grad_unscale(F(0), F(1), F(2), i[0], i[1], i[2], i[3], s); break;
        case 5: e = launch_prompts_bwd(F(0), i[0], i[1], i[2], i[3], F(1), F(2), F(3), s); break;
        case 6: {
            if (!c->text.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_text has not been called");
            if (i[0] < 0 || i[0] >= (int)c->text.blocks.size() || i[1] < 1 || i[2] < 1 || i[2] > TEXT_GRAD_MAX_L || !p[0] || !p[1] ||
                (long long)i[1] * i[2] > c->text_rows_budget)
                return fail(c, HG_ERR_INVALID, "hg_test_text_grad: block, n_seq >= 1, 1 <= L <= %d, x_in and g are needed", TEXT_GRAD_MAX_L);
            if (int rc = ensure_text_grad(c)) return rc;
            if (int rc = text_grad_ws(c, i[1] * i[2], 0)) return rc;
            return text_block_backward(c, i[0], F(0), F(1), i[1], i[2], s);
        }
        default: return fail(c, HG_ERR_INVALID, "hg_test_text_grad: op must be 0 .. 6");
    }
    if (e == hipErrorInvalidValue) return fail(c, HG_ERR_INVALID, "hg_test_text_grad: op %d refused by its launcher: %s", op, hipGetErrorString(e));
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_test_text_grad: op %d failed: %s", op, hipGetErrorString(e));
    return HG_OK;
}

// One launcher of hg_detr_rows.hip with the caller's own device buffers (include/hoigen_amd.h has the table of operands;
// tests/test_gpu_detr_rows.py, tests/test_gpu_detr_wiring.py).
int hg_test_detr_rows(hg_ctx* c, int op, const hg_test_detr_rows_args* x, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x) return fail(c, HG_ERR_INVALID, "hg_test_detr_rows: args are required");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    void* const* p = x->p;
    const int64_t* st = x->s;
    const int32_t* i = x->i;
    auto F = [&](int k) { return (float*)p[k]; };
    auto H = [&](int k) { return (half_t*)p[k]; };
    hipError_t e;
    switch (op) {
        case 0: e = launch_detr_entry(F(0), F(1), st[0], st[1], st[2], st[3], i[0], i[1], i[2], F(2), H(3), H(4), F(5), s); break;
        case 1: e = launch_detr_postnorm(F(0), F(1), F(2), F(3), H(4), H(5), F(6), i[0], i[1], s); break;
        case 2: e = launch_detr_exit(F(0), F(1), st[0], st[1], i[0], i[1], i[2], s); break;
        case 3: e = launch_detr_dec_entry(F(0), st[0], st[1], F(1), st[2], st[3], i[0], i[1], i[2], F(2), H(3), H(4), F(5), s); break;
        case 4: e = launch_detr_dec_tail(F(0), F(1), F(2), i[0], F(3), F(4), F(5), H(6), H(7), F(8), F(9), F(10), F(11), st[0], st[1], i[1], i[2],
                                         i[3], s); break;
        default: return fail(c, HG_ERR_INVALID, "hg_test_detr_rows: op must be 0 .. 4");
    }
    if (e == hipErrorInvalidValue) return fail(c, HG_ERR_INVALID, "hg_test_detr_rows: op %d refused by its launcher: %s", op, hipGetErrorString(e));
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_test_detr_rows: op %d failed: %s", op, hipGetErrorString(e));
    return HG_OK;
}

// ONE launch of the bottleneck convolution (hg_resnet_conv.hip) from fp32 tensors, the loader's packing included (include/hoigen_amd.h;
// tests/test_gpu_resnet_conv.py).  x's fp16 copy is an allocation of exactly its size.
int hg_test_resnet_conv(hg_ctx* c, const hg_test_resnet_conv_args* x, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x || !x->x || !x->w || !x->scale || !x->bias) return fail(c, HG_ERR_INVALID, "hg_test_resnet_conv: x, w, scale and bias are required");
    ResnetConvArgs k{};
    k.B = x->B; k.H = x->H; k.W = x->W; k.Cin = x->cin; k.Cout = x->cout; k.R = x->k; k.stride = x->stride; k.epi = x->epi; k.tile = x->tile;
    if ((k.R != 1 && k.R != 3) || (k.stride != 1 && k.stride != 2) || k.H < 1 || k.W < 1 || k.B < 1)
        return fail(c, HG_ERR_INVALID, "hg_test_resnet_conv: k must be 1 or 3, stride 1 or 2, B, H, W at least 1");
    k.Ho = resnet_out_size(k.H, k.R, k.stride); k.Wo = resnet_out_size(k.W, k.R, k.stride);
    // placeholders for the pointers the check wants; replaced below
    k.x = (const half_t*)x->x; k.w = (const half_t*)x->w; k.scale = x->scale; k.bias = x->bias; k.identity = x->identity;
    k.out32 = x->out32; k.out16 = (half_t*)x->out16;
    if (!resnet_conv_ok(k)) return fail(c, HG_ERR_INVALID, "hg_test_resnet_conv: the launcher refuses this shape, epilogue or tile");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t nx = (size_t)k.B * k.H * k.W * k.Cin, nw = (size_t)k.Cout * k.Cin * k.R * k.R, no = (size_t)k.B * k.Ho * k.Wo * k.Cout;
    std::vector<void*> tmp;
    void *x16 = nullptr, *w16 = nullptr, *o16 = nullptr, *flag = nullptr;
    hipError_t e = hipMalloc(&x16, nx * 2);
    if (e == hipSuccess) { tmp.push_back(x16); e = hipMalloc(&w16, nw * 2); }
    if (e == hipSuccess) { tmp.push_back(w16); e = hipMalloc(&o16, no * 2); }
    if (e == hipSuccess) { tmp.push_back(o16); e = hipMalloc(&flag, 16); }
    if (e == hipSuccess) { tmp.push_back(flag); e = hipMemsetAsync(flag, 0, 16, s); }
    if (e == hipSuccess) e = launch_f32_to_f16(x->x, (half_t*)x16, nx, s);
    if (e == hipSuccess) e = launch_resnet_pack(x->w, (half_t*)w16, k.Cout, k.Cin, k.R, (int*)flag, s);
    if (e == hipSuccess) {
        k.x = (const half_t*)x16; k.w = (const half_t*)w16; k.out16 = (half_t*)o16;
        ProfScope ps(c, s, HG_PROF_RESNET_CONV, k.B * k.Ho * k.Wo, k.Cout, k.R * k.R * k.Cin);
        e = launch_resnet_conv(k, s);
    }
    if (e == hipSuccess && k.epi != 2) e = launch_f16_to_f32((const half_t*)o16, x->out16, no, s);
    hipError_t e2 = hipStreamSynchronize(s);
    free_all(tmp);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_test_resnet_conv: %s", hipGetErrorString(e));
    return HG_OK;
}

// ONE launch of the stem (hg_resnet_stem.hip) from fp32 tensors, the loader's packing included (include/hoigen_amd.h;
// tests/test_gpu_resnet_stem.py).  x is read where the caller put it.
int hg_test_resnet_stem(hg_ctx* c, const hg_test_resnet_stem_args* x, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x || !x->x || !x->w || !x->scale || !x->bias || !x->out32 || !x->out16)
        return fail(c, HG_ERR_INVALID, "hg_test_resnet_stem: x, w, scale, bias, out32 and out16 are required");
    ResnetStemArgs k{};
    k.B = x->B; k.Hi = x->Hi; k.Wi = x->Wi;
    if (k.B < 1 || k.Hi < 1 || k.Wi < 1 || k.Hi > 4 * RESNET_MAX_SIDE || k.Wi > 4 * RESNET_MAX_SIDE)
        return fail(c, HG_ERR_INVALID, "hg_test_resnet_stem: B, Hi, Wi at least 1, Hi and Wi at most %d", 4 * RESNET_MAX_SIDE);
    k.Hc = resnet_stem_conv_size(k.Hi); k.Wc = resnet_stem_conv_size(k.Wi);
    k.Hp = resnet_stem_pool_size(k.Hc); k.Wp = resnet_stem_pool_size(k.Wc);
    k.x = x->x; k.sb = 3LL * k.Hi * k.Wi; k.sc = (long long)k.Hi * k.Wi; k.sr = k.Wi;
    k.scale = x->scale; k.bias = x->bias; k.out32 = x->out32;
    // placeholders for the pointers the check wants; replaced below
    k.w = (const half_t*)x->scale; k.out16 = (half_t*)x->out32;
    if (((uintptr_t)x->scale & 15) || !resnet_stem_ok(k)) return fail(c, HG_ERR_INVALID, "hg_test_resnet_stem: the launcher refuses this shape or alignment");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t no = (size_t)k.B * k.Hp * k.Wp * 64;
    std::vector<void*> tmp;
    void *w16 = nullptr, *o16 = nullptr, *flag = nullptr;
    hipError_t e = hipMalloc(&w16, RESNET_STEM_W_HALFS * 2);
    if (e == hipSuccess) { tmp.push_back(w16); e = hipMalloc(&o16, no * 2); }
    if (e == hipSuccess) { tmp.push_back(o16); e = hipMalloc(&flag, 16); }
    if (e == hipSuccess) { tmp.push_back(flag); e = hipMemsetAsync(flag, 0, 16, s); }
    if (e == hipSuccess) e = launch_resnet_stem_pack(x->w, (half_t*)w16, (int*)flag, s);
    if (e == hipSuccess) {
        k.w = (const half_t*)w16; k.out16 = (half_t*)o16;
        ProfScope ps(c, s, HG_PROF_RESNET_STEM, k.B * k.Hp * k.Wp, 64, 147);
        e = launch_resnet_stem(k, s);
    }
    if (e == hipSuccess) e = launch_f16_to_f32((const half_t*)o16, x->out16, no, s);
    hipError_t e2 = hipStreamSynchronize(s);
    free_all(tmp);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_test_resnet_stem: %s", hipGetErrorString(e));
    return HG_OK;
}

// ONE launch of the pool + normalise kernel (hg_resnet_pool.hip) on the caller's NHWC map (include/hoigen_amd.h;
// tests/test_gpu_resnet_features.py)
int hg_test_resnet_pool(hg_ctx* c, const float* x_nhwc, int B, int HW, int C, float* pooled, float* features, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!resnet_pool_ok(x_nhwc, B, HW, C, pooled, features))
        return fail(c, HG_ERR_INVALID, "hg_test_resnet_pool: x and one of pooled / features are required; B 1 .. %d, C a multiple of 64 up to %d, HW 1 .. %d^2",
                    RESNET_MAX_B, RESNET_MAX_C, RESNET_MAX_SIDE);
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    hipError_t e;
    {
        ProfScope ps(c, s, HG_PROF_RESNET_POOL, B, C, HW);
        e = launch_resnet_pool(x_nhwc, B, HW, C, pooled, features, s);
    }
    hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_test_resnet_pool: %s", hipGetErrorString(e));
    return HG_OK;
}

}  // extern "C"
