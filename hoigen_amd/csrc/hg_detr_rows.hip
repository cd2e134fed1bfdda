// Row kernels of the DETR encoder (detr/models/transformer.py:127-153, the post-norm layer): the entry that turns the caller's
// strided src / pos into the device layout, the post-norm LayerNorm that also emits the next GEMMs' fp16 operands, and the exit; and of
// the decoder (:187-233): its entry (tgt, query_pos) and the layer tail that sums the split FFN's partial sums, applies norm3 and
// writes the final norm of what leaves.
#include "hg_kernels.h"

namespace hg {

// one workgroup per row of [B * S, D] (one 32-bit division a workgroup), a thread per channel; src / pos element (b, t, ch) at
// b * sb + t * ss + ch.  Scalar accesses: the caller's src / pos need no alignment beyond a float's, and a row is read and written once
__global__ __launch_bounds__(256) void detr_entry_kernel(const float* __restrict__ src, const float* __restrict__ pos, long long sb,
                                                         long long ss, long long pb, long long ps, int S, int D,
                                                         float* __restrict__ x, half_t* __restrict__ x16, half_t* __restrict__ xp16,
                                                         float* __restrict__ posb) {
    const int row = (int)blockIdx.x;
    const int b = row / S, t = row - b * S;
    const float* sr = src + (long long)b * sb + (long long)t * ss;
    const float* pr = pos ? pos + (long long)b * pb + (long long)t * ps : nullptr;
    const size_t o = (size_t)row * D;
    for (int ch = threadIdx.x; ch < D; ch += 256) {
        const float v = sr[ch];
        const float p = pr ? pr[ch] : 0.f;
        x[o + ch] = v;
        x16[o + ch] = (half_t)v;
        xp16[o + ch] = (half_t)(v + p);
        posb[o + ch] = p;
    }
}

// one wave per row, four rows per workgroup; three passes over the row (mean, variance about the mean, output): the row is 1 KiB at
// D = 256 and stays in the cache
__global__ __launch_bounds__(256) void detr_postnorm_kernel(float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                            const float* __restrict__ posb, half_t* __restrict__ x16,
                                                            half_t* __restrict__ xp16, float* __restrict__ copy, int M, int D) {
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    float* xr = x + (size_t)row * D;
    const int n4 = D >> 2;
    float sum = 0.f;
    for (int i = lane; i < n4; i += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * i);
        sum += (v[0] + v[1]) + (v[2] + v[3]);
    }
    const float mean = wave_sum(sum) / (float)D;
    float sq = 0.f;
    for (int i = lane; i < n4; i += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) sq = fmaf(v[e] - mean, v[e] - mean, sq);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + 1e-5f);
    for (int i = lane; i < n4; i += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + 4 * i);
        const f32x4 g = *reinterpret_cast<const f32x4*>(w + 4 * i), be = *reinterpret_cast<const f32x4*>(b + 4 * i);
        f32x4 y;
        half4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = fmaf((v[e] - mean) * rstd, g[e], be[e]);
            h[e] = (half_t)y[e];
        }
        *reinterpret_cast<f32x4*>(xr + 4 * i) = y;
        *reinterpret_cast<half4*>(x16 + (size_t)row * D + 4 * i) = h;
        if (copy) {      // the caller's trace buffer: no alignment beyond a float's is asked of it
#pragma unroll
            for (int e = 0; e < 4; ++e) copy[(size_t)row * D + 4 * i + e] = y[e];
        }
        if (xp16) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(posb + (size_t)row * D + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)(y[e] + p[e]);
            *reinterpret_cast<half4*>(xp16 + (size_t)row * D + 4 * i) = h;
        }
    }
}

__global__ __launch_bounds__(256) void detr_exit_kernel(const float* __restrict__ x, float* __restrict__ out, long long ob, long long os,
                                                        int S, int D) {
    const int row = (int)blockIdx.x;
    const int b = row / S, t = row - b * S;
    float* orow = out + (long long)b * ob + (long long)t * os;
    for (int ch = threadIdx.x; ch < D; ch += 256) orow[ch] = x[(size_t)row * D + ch];
}

// the decoder's entry: one workgroup per row of [B * Q, D]; a null tgt writes zeros and reads nothing
__global__ __launch_bounds__(256) void detr_dec_entry_kernel(const float* __restrict__ tgt, long long tb, long long tq,
                                                             const float* __restrict__ qpos, long long qb, long long qq, int Q, int D,
                                                             float* __restrict__ x, half_t* __restrict__ x16, half_t* __restrict__ xp16,
                                                             float* __restrict__ qposb) {
    const int row = (int)blockIdx.x;
    const int b = row / Q, q = row - b * Q;
    const float* tr = tgt ? tgt + (long long)b * tb + (long long)q * tq : nullptr;
    const float* pr = qpos + (long long)b * qb + (long long)q * qq;
    const size_t o = (size_t)row * D;
    for (int ch = threadIdx.x; ch < D; ch += 256) {
        const float v = tr ? tr[ch] : 0.f;
        const float p = pr[ch];
        x[o + ch] = v;
        x16[o + ch] = (half_t)v;
        xp16[o + ch] = (half_t)(v + p);
        qposb[o + ch] = p;
    }
}

// the decoder layer's tail: one wave per row, four rows per workgroup, the row in registers (D <= 512: two 16-byte pieces a lane).
// Summation order: ((x + b2) + partial[0]) + partial[1] + ...; the LayerNorms are detr_postnorm_kernel's arithmetic
__global__ __launch_bounds__(256) void detr_dec_tail_kernel(float* __restrict__ x, const float* __restrict__ b2,
                                                            const float* __restrict__ partial, int n_slices, const float* __restrict__ w3,
                                                            const float* __restrict__ b3, const float* __restrict__ qposb,
                                                            half_t* __restrict__ x16, half_t* __restrict__ xp16, float* __restrict__ copy,
                                                            const float* __restrict__ wf, const float* __restrict__ bf,
                                                            float* __restrict__ out, long long ob, long long oq, int Q, int M, int D) {
    const int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const int n4 = D >> 2;
    const size_t o = (size_t)row * D;
    f32x4 v[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = lane + 64 * t;
        v[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n4) {
            v[t] = *reinterpret_cast<const f32x4*>(x + o + 4 * i);
            if (b2) v[t] += *reinterpret_cast<const f32x4*>(b2 + 4 * i);
            for (int sl = 0; sl < n_slices; ++sl) v[t] += *reinterpret_cast<const f32x4*>(partial + ((size_t)sl * M + row) * D + 4 * i);
        }
    }
    auto norm = [&](const float* __restrict__ g, const float* __restrict__ be) {
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (lane + 64 * t < n4) sum += (v[t][0] + v[t][1]) + (v[t][2] + v[t][3]);
        const float mean = wave_sum(sum) / (float)D;
        float sq = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (lane + 64 * t < n4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sq = fmaf(v[t][e] - mean, v[t][e] - mean, sq);
            }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + 1e-5f);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int i = lane + 64 * t;
            if (i < n4) {
                const f32x4 gg = *reinterpret_cast<const f32x4*>(g + 4 * i), bb = *reinterpret_cast<const f32x4*>(be + 4 * i);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[t][e] = fmaf((v[t][e] - mean) * rstd, gg[e], bb[e]);
            }
        }
    };
    norm(w3, b3);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = lane + 64 * t;
        if (i >= n4) continue;
        half4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (half_t)v[t][e];
        *reinterpret_cast<f32x4*>(x + o + 4 * i) = v[t];
        *reinterpret_cast<half4*>(x16 + o + 4 * i) = h;
        if (copy) {
#pragma unroll
            for (int e = 0; e < 4; ++e) copy[o + 4 * i + e] = v[t][e];
        }
        if (xp16) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(qposb + o + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)(v[t][e] + p[e]);
            *reinterpret_cast<half4*>(xp16 + o + 4 * i) = h;
        }
    }
    if (!out) return;
    norm(wf, bf);      // the decoder's final norm of this layer's output: to the caller only (transformer.py:112-113)
    const int b = row / Q, q = row - b * Q;
    float* orow = out + (long long)b * ob + (long long)q * oq;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = lane + 64 * t;
        if (i >= n4) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) orow[4 * i + e] = v[t][e];
    }
}

hipError_t launch_detr_dec_entry(const float* tgt, long long tb, long long tq, const float* qpos, long long qb, long long qq, int B, int Q,
                                 int D, float* x, half_t* x16, half_t* xp16, float* qposb, hipStream_t s) {
    if (!qpos || !x || !x16 || !xp16 || !qposb || B < 1 || Q < 1 || D < 1) return hipErrorInvalidValue;
    if ((long long)B * Q > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(detr_dec_entry_kernel, dim3((unsigned)(B * Q)), dim3(256), 0, s, tgt, tb, tq, qpos, qb, qq, Q, D, x, x16, xp16, qposb);
    return hipGetLastError();
}

hipError_t launch_detr_dec_tail(float* x, const float* b2, const float* partial, int n_slices, const float* w3, const float* b3,
                                const float* qposb, half_t* x16, half_t* xp16, float* copy, const float* wf, const float* bf, float* out,
                                long long ob, long long oq, int Q, int M, int D, hipStream_t s) {
    if (!x || !w3 || !b3 || !x16 || M < 1 || D < 4 || D % 4 || D > 512 || n_slices < 0 || (n_slices && !partial) || (xp16 && !qposb) ||
        (out && (!wf || !bf || Q < 1)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(detr_dec_tail_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, b2, partial, n_slices, w3, b3, qposb, x16,
                       xp16, copy, wf, bf, out, ob, oq, Q, M, D);
    return hipGetLastError();
}

hipError_t launch_detr_entry(const float* src, const float* pos, long long sb, long long ss, long long pb, long long ps, int B, int S, int D,
                             float* x, half_t* x16, half_t* xp16, float* posb, hipStream_t s) {
    if (!src || !x || !x16 || !xp16 || !posb || B < 1 || S < 1 || D < 1) return hipErrorInvalidValue;
    if ((long long)B * S > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(detr_entry_kernel, dim3((unsigned)(B * S)), dim3(256), 0, s, src, pos, sb, ss, pb, ps, S, D, x, x16, xp16, posb);
    return hipGetLastError();
}

hipError_t launch_detr_postnorm(float* x, const float* w, const float* b, const float* posb, half_t* x16, half_t* xp16, float* copy, int M,
                                int D, hipStream_t s) {
    if (!x || !w || !b || !x16 || M < 1 || D < 4 || D % 4 || (xp16 && !posb)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(detr_postnorm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, w, b, posb, x16, xp16, copy, M, D);
    return hipGetLastError();
}

hipError_t launch_detr_exit(const float* x, float* out, long long ob, long long os, int B, int S, int D, hipStream_t s) {
    if (!x || !out || B < 1 || S < 1 || D < 1) return hipErrorInvalidValue;
    if ((long long)B * S > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(detr_exit_kernel, dim3((unsigned)(B * S)), dim3(256), 0, s, x, out, ob, os, S, D);
    return hipGetLastError();
}

}  // namespace hg
