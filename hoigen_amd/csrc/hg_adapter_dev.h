// Device pieces of the instance adapter's MFMA decoder layer (hg_adapter.hip: sequences of at most 224 tokens; hg_adapter_long.hip:
// 225 .. 640 tokens): the fp16 weight set, the LDS pitches, and the register-tile helpers - a 64-wide linear as D = W . X^T on
// v_mfma_f32_16x16x32_f16, bias, the fp16 hand-over through a wave's LDS rows, LayerNorm over the 64 features, the key order of V^T.
#pragma once
#include "hg_kernels.h"

namespace hg {

struct DecW16 {
    const half_t *Wq, *Wk, *Wv, *Wo, *W1, *W2;      // fp16 [out][in]: 64x64 (x4), 128x64, 64x128
    const float *bq, *bk, *bv, *bo, *b1, *b2, *norms;   // norms = {norm2.w, norm2.b, norm3.w, norm3.b}
};

static constexpr int XP = 136;      // halfs per row of a wave's activation buffer (64 or 128 features + pad)
static constexpr int KP = 72;       // halfs per row of K [key][64]
static constexpr int NKMAX = ADAPTER_MAX_L;   // keys: 14 tiles of 16 (L <= 224)
static constexpr int VP = NKMAX + 8;   // halfs per row of V^T [feature][key slot]

typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float max_rows(float x) {      // max over the four 16-lane rows
    x = fmaxf(x, __shfl_xor(x, 16, 64));
    return fmaxf(x, __shfl_xor(x, 32, 64));
}
__device__ __forceinline__ float sum_rows4(float x) {
    x += __shfl_xor(x, 16, 64);
    return x + __shfl_xor(x, 32, 64);
}

// t[f][g] (+)= W[16g.., :] . X[16f.., :]^T over K = 32 * KS features; W global fp16 [.][ldw], X = LDS rows of pitch XP
template <int G, int KS, int F>
__device__ __forceinline__ void linear_T(f32x4 (&t)[F][G], const half_t* __restrict__ W, int ldw, const half_t* X, int lane) {
    const int r = lane & 15, q = lane >> 4;
    half8 xf[F][KS];
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xf[f][ks] = *reinterpret_cast<const half8*>(X + (16 * f + r) * XP + 32 * ks + 8 * q);
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const half8 wf = *reinterpret_cast<const half8*>(W + (size_t)(16 * g + r) * ldw + 32 * ks + 8 * q);
#pragma unroll
            for (int f = 0; f < F; ++f) t[f][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[f][ks], t[f][g], 0, 0, 0);
        }
}
template <int G, int F>
__device__ __forceinline__ void init_bias(f32x4 (&t)[F][G], const float* __restrict__ b, int lane) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b + 16 * g + 4 * (lane >> 4));
#pragma unroll
        for (int f = 0; f < F; ++f) t[f][g] = bv;
    }
}
template <int G, int F>
__device__ __forceinline__ void store_T(const f32x4 (&t)[F][G], half_t* X, int lane) {
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            half4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)t[f][g][e];
            *reinterpret_cast<half4*>(X + (16 * f + r) * XP + 16 * g + 4 * q) = h;
        }
}
// LayerNorm over the 64 features of every token (eps 1e-5, biased variance), in place; AFFINE = false: normalised values only
template <bool AFFINE = true, int F>
__device__ __forceinline__ void layer_norm_T(f32x4 (&t)[F][4], const float* __restrict__ w, const float* __restrict__ b, int lane) {
    const int q = lane >> 4;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) s += (t[f][g][0] + t[f][g][1]) + (t[f][g][2] + t[f][g][3]);
        const float mean = sum_rows4(s) * (1.0f / 64.0f);
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = t[f][g][e] - mean;
                v = fmaf(d, d, v);
            }
        const float rstd = 1.0f / sqrtf(sum_rows4(v) * (1.0f / 64.0f) + 1e-5f);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if constexpr (AFFINE) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + 16 * g + 4 * q), bv = *reinterpret_cast<const f32x4*>(b + 16 * g + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[f][g][e] = (t[f][g][e] - mean) * rstd * wv[e] + bv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) t[f][g][e] = (t[f][g][e] - mean) * rstd;
            }
        }
    }
}

// key index -> slot inside the V^T rows: within a block of 32 keys, key 16*kt + 4*q + r sits at 8*q + 4*kt + r, which is
// where the score accumulators of key tiles (2b, 2b+1) put it when they are packed as the P.V B operand
__device__ __forceinline__ int key_slot(int key) {
    const int w = key & 31;
    return (key & ~31) + 8 * ((w & 15) >> 2) + 4 * (w >> 4) + (w & 3);
}

}  // namespace hg
