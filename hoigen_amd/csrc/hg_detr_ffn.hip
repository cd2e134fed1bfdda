// The FFN of a short stream in one launch, split over d_ff (the DETR decoder: detr/models/transformer.py:231, linear2(relu(linear1(x)))
// on 100 x B rows).  The 128 x 128-tile GEMMs give linear2 (K = 2048, N = 256) one workgroup per 128 rows, each walking the whole K
// loop; here a work item is (32-row tile, 128-unit slice of d_ff), 64 items for one image instead of 2, and the hidden layer never
// reaches memory.
//
//   phase 1   h[r][u] = fp16(relu(sum_k x16[r][k] W1[u][k] + b1[u]))  for the slice's 128 units u: wave w owns units 32 w .. 32 w + 31 of
//             the slice; v_mfma_f32_16x16x32_f16 over k = 0 .. D - 1 in ascending blocks of 32, fp32 accumulate from zero; the bias is
//             added after the sum, then the ReLU, then ONE rounding to fp16 (round to nearest even) - as EPI_BIAS_RELU_F16 does.
//             h goes to LDS (32 x 128 fp16, rows padded to 272 B).
//   phase 2   partial[slice][r][n] = sum_u h[r][u] W2[n][slice * 128 + u]: wave w owns columns w D / 4 .. (w + 1) D / 4 - 1; the same
//             MFMA over u in four ascending blocks of 32, fp32 accumulate from zero; stored as fp32 with plain 16-byte vector stores.
//   reduce    not here: detr_dec_tail_kernel (hg_detr_rows.hip) computes ((x + b2) + partial[0]) + partial[1] + ... in ascending slice
//             order, one fp32 addition each, and the LayerNorm behind it.  No counters, no atomics, nothing waits inside the launch:
//             the bits do not depend on where or when an item runs.
//
// Operands come straight from global memory in MFMA fragment order (lane l: row l & 15, eight halfs at k = 8 (l >> 4)): the weights of
// a slice are read once per row tile and stay in L2 (2 MiB for the whole layer), x16 is 16 KiB a tile.  Rows at or beyond M are read
// from row M - 1 and never stored.  D in {128, 256}, d_ff a multiple of 128.
//
// Measured on an MI355X (profiles/detr_decoder.txt; D = 256, d_ff = 2048; this kernel + the tail that sums 16 slices against linear1 GEMM +
// linear2 GEMM + the tail without slices, per launch, median of 7 alternating rounds; the spread of repeats is up to 6 us):
//     M = 100: 11.4 + 9.2 = 20.7 us against 10.6 + 28.5 + 6.7 = 45.8 us      M = 800: 20.6 + 9.9 = 30.5 against 12.1 + 42.9 + 6.9 = 62.1
//     M = 950: 20.5 + 10.1 = 30.6 against 62.0                               M = 2 888: 44.1 + 12.8 = 56.9 against 64.2
// so option detr_ffn = 0 runs it up to 1 000 rows (detr_ffn_max_m) and the GEMMs beyond.
#include "hg_kernels.h"

namespace hg {

static constexpr int FFN_LDH = DETR_FFN_SLICE + 8;      // halfs per LDS row: 272 B, 16-byte aligned, rows 4 banks apart

template <int D>
__global__ __launch_bounds__(256) void detr_ffn_kernel(const half_t* __restrict__ x16, const half_t* __restrict__ W1,
                                                       const float* __restrict__ b1, const half_t* __restrict__ W2,
                                                       float* __restrict__ partial, int M, int F) {
    __shared__ __attribute__((aligned(16))) half_t hs[DETR_FFN_ROWS * FFN_LDH];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = blockIdx.x, m0 = (int)blockIdx.y * DETR_FFN_ROWS;
    const int r16 = lane & 15, cg = lane >> 4, kq = cg * 8;
    const int u0 = slice * DETR_FFN_SLICE;

    // ---- phase 1
    {
        const half_t* wp[2];
        const half_t* xp[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wp[i] = W1 + (size_t)(u0 + wave * 32 + i * 16 + r16) * D + kq;
            int m = m0 + i * 16 + r16;
            m = m < M ? m : M - 1;
            xp[i] = x16 + (size_t)m * D + kq;
        }
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks) {
            half8 wf[2], xf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                wf[i] = *reinterpret_cast<const half8*>(wp[i] + ks * 32);
                xf[i] = *reinterpret_cast<const half8*>(xp[i] + ks * 32);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], xf[j], acc[i][j], 0, 0, 0);
        }
        // acc[i][j][r] = unit wave * 32 + i * 16 + 4 cg + r of the slice, row j * 16 + r16 of the tile
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = wave * 32 + i * 16 + 4 * cg;
            const f32x4 b = *reinterpret_cast<const f32x4*>(b1 + u0 + u);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                half4 h;
#pragma unroll
                for (int r = 0; r < 4; ++r) h[r] = (half_t)fmaxf(acc[i][j][r] + b[r], 0.0f);
                *reinterpret_cast<half4*>(hs + (j * 16 + r16) * FFN_LDH + u) = h;
            }
        }
    }
    __syncthreads();

    // ---- phase 2
    constexpr int NF = D / 64;      // 16-column fragments per wave
    const int c0 = wave * (D / 4);
    f32x4 acc[NF][2];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < DETR_FFN_SLICE / 32; ++ks) {
        half8 wf[NF], hf[2];
#pragma unroll
        for (int i = 0; i < NF; ++i) wf[i] = *reinterpret_cast<const half8*>(W2 + (size_t)(c0 + i * 16 + r16) * F + u0 + ks * 32 + kq);
#pragma unroll
        for (int j = 0; j < 2; ++j) hf[j] = *reinterpret_cast<const half8*>(hs + (j * 16 + r16) * FFN_LDH + ks * 32 + kq);
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], hf[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = m0 + j * 16 + r16;
        if (m >= M) continue;
        float* prow = partial + ((size_t)slice * M + m) * D;
#pragma unroll
        for (int i = 0; i < NF; ++i) *reinterpret_cast<f32x4*>(prow + c0 + i * 16 + 4 * cg) = acc[i][j];
    }
}

bool detr_ffn_ok(int M, int D, int F) {
    return M >= 1 && M <= (1 << 20) && (D == 128 || D == 256) && F >= DETR_FFN_SLICE && F % DETR_FFN_SLICE == 0 && F <= 8192;
}

hipError_t launch_detr_ffn(const half_t* x16, const half_t* W1, const float* b1, const half_t* W2, float* partial, int M, int D, int F,
                           hipStream_t s) {
    if (!x16 || !W1 || !b1 || !W2 || !partial || !detr_ffn_ok(M, D, F)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(F / DETR_FFN_SLICE), (unsigned)((M + DETR_FFN_ROWS - 1) / DETR_FFN_ROWS));
    if (D == 128) hipLaunchKernelGGL(detr_ffn_kernel<128>, grid, dim3(256), 0, s, x16, W1, b1, W2, partial, M, F);
    else hipLaunchKernelGGL(detr_ffn_kernel<256>, grid, dim3(256), 0, s, x16, W1, b1, W2, partial, M, F);
    return hipGetLastError();
}

}  // namespace hg
