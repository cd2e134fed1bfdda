// DETR's heads and PostProcess on the decoder's output in one launch (upt_tip_cache_model_free_finetune_distill3.py:1598-1605:
// class_embed(hs), bbox_embed(hs).sigmoid() - detr/models/detr.py:37-38, MLP :293-305 - and PostProcess.forward, detr.py:269-282).
// A work item is a tile of 32 rows of hs, as in hg_detr_ffn.hip: 256 threads, v_mfma_f32_16x16x32_f16, the operands straight from global
// memory in MFMA fragment order (lane l: row l & 15, eight values at k = 8 (l >> 4)); everything between the phases stays in LDS.
//
//   input     x16 = fp16(hs), round to nearest even; rows are fp32 [L, B, Q, D] through element strides (channel stride 1).  Rows at or
//             beyond M are read from row M - 1 and never stored.
//   logits    logit[c] = (sum_k x16[k] Wc[c][k]) + bc[c]: fp32 from zero over k in ascending blocks of 32, the bias after the sum.  The
//             loader pads Wc and bc with zero rows to C1p = a multiple of 16; wave w owns the 16-column fragments w, w + 4, ..  Columns
//             at or beyond C1 never enter the softmax, the maximum or a store.
//   box MLP   h1 = fp16(relu(acc + b0)), h2 = fp16(relu(acc + b1)): one rounding each, as EPI_BIAS_RELU_F16 does; wave w owns D / 4
//             columns.  t = acc + b2 (W2 padded to 16 rows; waves 0 and 1 take 16 rows of the tile each), pred_box = 1 / (1 + expf(-t)).
//   PostProcess, rows of the last level only: eight threads a row, thread s takes columns s, s + 8, ..; m = max over all C1 logits,
//             label = the lowest index of the greatest logit among c < C1 - 1, s = sum expf(logit_c - m) (per thread in ascending c, then
//             the xor butterfly 1, 2, 4), score = expf(logit_label - m) / s; boxes = (cx - 0.5 w, cy - 0.5 h, cx + 0.5 w, cy + 0.5 h)
//             times (w_img, h_img, w_img, h_img), every operation rounded on its own (__fmul_rn / __fadd_rn: the build contracts).
//
// No counters, no atomics, nothing waits inside the launch: a row's outputs depend on that row and the weights alone.
// Measured on an MI355X: profiles/detr_heads.txt, DESIGN.md section 18.
#include <limits.h>

#include "hg_kernels.h"

namespace hg {

static constexpr int HEADS_LDL = DETR_HEADS_MAX_C + 4;      // floats per LDS row of logits: 1 040 B, 16-byte aligned

template <int D>
__global__ __launch_bounds__(256) void detr_heads_kernel(const DetrHeadsArgs a) {
    constexpr int LDH = D + 8;      // halfs per LDS row of a hidden layer: 16-byte aligned, rows 4 banks apart
    constexpr int NK = D / 32, NF = D / 64;
    __shared__ __attribute__((aligned(16))) float lg[DETR_HEADS_ROWS * HEADS_LDL];
    __shared__ __attribute__((aligned(16))) half_t hb[DETR_HEADS_ROWS * LDH];
    __shared__ __attribute__((aligned(16))) float pb[DETR_HEADS_ROWS * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, cg = lane >> 4, kq = cg * 8;
    const int BQ = a.B * a.Q, M = a.L * BQ, m0 = (int)blockIdx.x * DETR_HEADS_ROWS;

    // ---- x16 = fp16(hs) as fragments: xf[ks][j] = row j * 16 + r16 of the tile, k = 32 ks + kq .. + 7
    half8 xf[NK][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int m = m0 + j * 16 + r16;
        m = m < M ? m : M - 1;
        const int l = m / BQ, rem = m - l * BQ, b = rem / a.Q, q = rem - b * a.Q;
        const float* p = a.hs + (long long)(a.l0 + l) * a.s_l + (long long)b * a.s_b + (long long)q * a.s_q + kq;
        if (a.vec4) {
#pragma unroll
            for (int ks = 0; ks < NK; ++ks) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(p + ks * 32), hi = *reinterpret_cast<const f32x4*>(p + ks * 32 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xf[ks][j][e] = (half_t)lo[e];
                    xf[ks][j][4 + e] = (half_t)hi[e];
                }
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < NK; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) xf[ks][j][e] = (half_t)p[ks * 32 + e];
        }
    }

    // ---- class logits -> lg
    for (int f = wave; f < (a.C1p >> 4); f += 4) {
        const half_t* wp = a.wc + (size_t)(f * 16 + r16) * D + kq;
        f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            const half8 wf = *reinterpret_cast<const half8*>(wp + ks * 32);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[ks][j], acc[j], 0, 0, 0);
        }
        // acc[j][r] = column f * 16 + 4 cg + r, row j * 16 + r16 of the tile
        const int c = f * 16 + 4 * cg;
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.bc + c);
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(lg + (j * 16 + r16) * HEADS_LDL + c) = acc[j] + b;
    }

    // ---- box MLP, layers 0 and 1: hidden layer -> hb
    const int c0 = wave * (D / 4);
#pragma unroll
    for (int layer = 0; layer < 2; ++layer) {
        const half_t* W = layer ? a.w1 : a.w0;
        const float* bias = layer ? a.b1 : a.b0;
        if (layer) {      // h1 of the whole tile into registers, so that h2 can take its place
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < NK; ++ks)
#pragma unroll
                for (int j = 0; j < 2; ++j) xf[ks][j] = *reinterpret_cast<const half8*>(hb + (j * 16 + r16) * LDH + ks * 32 + kq);
            __syncthreads();
        }
        f32x4 acc[NF][2];
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            half8 wf[NF];
#pragma unroll
            for (int i = 0; i < NF; ++i) wf[i] = *reinterpret_cast<const half8*>(W + (size_t)(c0 + i * 16 + r16) * D + ks * 32 + kq);
#pragma unroll
            for (int i = 0; i < NF; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], xf[ks][j], acc[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int u = c0 + i * 16 + 4 * cg;
            const f32x4 b = *reinterpret_cast<const f32x4*>(bias + u);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                half4 h;
#pragma unroll
                for (int r = 0; r < 4; ++r) h[r] = (half_t)fmaxf(acc[i][j][r] + b[r], 0.0f);
                *reinterpret_cast<half4*>(hb + (j * 16 + r16) * LDH + u) = h;
            }
        }
    }
    __syncthreads();

    // ---- box MLP, layer 2 and the sigmoid -> pb: wave j takes rows 16 j .. 16 j + 15 of the tile
    if (wave < 2) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
            const half8 wf = *reinterpret_cast<const half8*>(a.w2 + (size_t)r16 * D + ks * 32 + kq);
            const half8 hf = *reinterpret_cast<const half8*>(hb + (wave * 16 + r16) * LDH + ks * 32 + kq);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, hf, acc, 0, 0, 0);
        }
        if (cg == 0) {      // outputs 0 .. 3 of row r16
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.b2);
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = 1.0f / (1.0f + expf(-(acc[r] + b[r])));
            *reinterpret_cast<f32x4*>(pb + (wave * 16 + r16) * 4) = o;
        }
    }
    __syncthreads();

    // ---- what leaves: the tile's rows are one contiguous span of every output
    const int nrows = M - m0 < DETR_HEADS_ROWS ? M - m0 : DETR_HEADS_ROWS;
    const int C1 = a.C1;
    if (a.pred_logits) {
        float* o = a.pred_logits + (size_t)m0 * C1;
        for (int i = tid; i < nrows * C1; i += 256) {
            const int r = i / C1;
            o[i] = lg[r * HEADS_LDL + (i - r * C1)];
        }
    }
    if (a.pred_boxes && tid < nrows * 4) a.pred_boxes[(size_t)m0 * 4 + tid] = pb[tid];

    // ---- PostProcess of the last level's rows
    const int pp0 = (a.L - 1) * BQ;
    if (m0 + DETR_HEADS_ROWS <= pp0) return;
    const int r = tid >> 3, s = tid & 7;
    const float* row = lg + r * HEADS_LDL;
    float mx = -INFINITY, bv = -INFINITY;
    int bi = INT_MAX;
    for (int c = s; c < C1; c += 8) {
        const float v = row[c];
        mx = fmaxf(mx, v);
        if (c < C1 - 1 && (bi == INT_MAX || v > bv)) {
            bv = v;
            bi = c;
        }
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o));
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    float se = 0.0f;
    for (int c = s; c < C1; c += 8) se += expf(row[c] - mx);
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) se += __shfl_xor(se, o);
    const int m = m0 + r;
    if (s == 0 && r < nrows && m >= pp0) {
        const int i = m - pp0, b = i / a.Q;
        const float h_img = a.sizes[2 * b], w_img = a.sizes[2 * b + 1];
        const f32x4 p = *reinterpret_cast<const f32x4*>(pb + r * 4);
        const float hw = __fmul_rn(0.5f, p[2]), hh = __fmul_rn(0.5f, p[3]);
        f32x4 o;
        o[0] = __fmul_rn(__fsub_rn(p[0], hw), w_img);
        o[1] = __fmul_rn(__fsub_rn(p[1], hh), h_img);
        o[2] = __fmul_rn(__fadd_rn(p[0], hw), w_img);
        o[3] = __fmul_rn(__fadd_rn(p[1], hh), h_img);
        a.scores[i] = expf(bv - mx) / se;
        a.labels[i] = bi;
        *reinterpret_cast<f32x4*>(a.boxes + (size_t)i * 4) = o;
    }
}

bool detr_heads_ok(int D, int C1, int L, int B, int Q) {
    return (D == 128 || D == 256) && C1 >= 2 && C1 <= DETR_HEADS_MAX_C && L >= 1 && L <= DETR_HEADS_MAX_L && B >= 1 && B <= DETR_HEADS_MAX_B &&
           Q >= 1 && Q <= DETR_HEADS_MAX_Q;
}

hipError_t launch_detr_heads(const DetrHeadsArgs& a, hipStream_t s) {
    if (!a.hs || !a.wc || !a.bc || !a.w0 || !a.b0 || !a.w1 || !a.b1 || !a.w2 || !a.b2 || !a.scores || !a.labels || !a.boxes ||
        !detr_heads_ok(a.D, a.C1, a.L, a.B, a.Q) || a.C1p != (a.C1 + 15) / 16 * 16 || a.l0 < 0)
        return hipErrorInvalidValue;
    const int M = a.L * a.B * a.Q;
    const dim3 grid((unsigned)((M + DETR_HEADS_ROWS - 1) / DETR_HEADS_ROWS));
    if (a.D == 128) hipLaunchKernelGGL(detr_heads_kernel<128>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(detr_heads_kernel<256>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hg
