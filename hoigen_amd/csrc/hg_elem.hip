// Row / elementwise kernels (HBM-bound): LayerNorm, im2col, token embedding gather, prompt assembly,
// reparameterisation, L2 normalisation, layout permutations, dtype conversion.  One wave per row
// where a row reduction is needed; 16-byte accesses per lane.
#include <climits>
#include "hg_gemm_dev.h"

namespace hg {

static constexpr int LN_MAXC = 4;   // float4 chunks per lane -> D <= 1024

// ---- LayerNorm (clipnet/model.py:153-159: fp32 statistics, eps 1e-5, biased variance) ----------
template <typename OutT>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b, OutT* __restrict__ out, int M,
                                                        int D, const int32_t* __restrict__ gather, int rows_per_seq,
                                                        int in_row_mul, const float* __restrict__ pos = nullptr,
                                                        const float* __restrict__ cls = nullptr, int Lpos = 1) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    size_t in_row;
    if (gather) {
        int gidx = gather[r];
        gidx = gidx < 0 ? 0 : (gidx >= rows_per_seq ? rows_per_seq - 1 : gidx);   // caller error guard
        in_row = (size_t)r * rows_per_seq + gidx;
    }
    else in_row = (size_t)r * in_row_mul;
    // ln_pre of the vision tower (pos != nullptr): the row is [cls ; patch embedding] + pos[t] (clipnet/model.py:223-224) -
    // the class row (t = 0) comes from cls, the patch GEMM left the other rows without their positional embedding
    const int tpos = pos ? r % Lpos : 0;
    const f32x4* xp = reinterpret_cast<const f32x4*>((pos && tpos == 0) ? cls : x + in_row * D);
    const f32x4* pp = reinterpret_cast<const f32x4*>(pos ? pos + (size_t)tpos * D : nullptr);
    const int nc = D >> 2;
    f32x4 v[LN_MAXC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            v[i] = xp[c];
            if (pos) v[i] += pp[c];
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                q += d * d;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
    const f32x4* wp = reinterpret_cast<const f32x4*>(w);
    const f32x4* bp = reinterpret_cast<const f32x4*>(b);
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            const f32x4 g = wp[c], be = bp[c];
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * g[e] + be[e];
            if constexpr (sizeof(OutT) == 2) {
                half4 h;
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = (half_t)y[e];
                reinterpret_cast<half4*>(out + (size_t)r * D)[c] = h;
            } else {
                reinterpret_cast<f32x4*>(out + (size_t)r * D)[c] = y;
            }
        }
    }
}

hipError_t launch_layernorm_f16(const float* x, const float* w, const float* b, half_t* out, int M, int D,
                                const int32_t* gather, int rows_per_seq, int in_row_mul, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (D % 4 || D > 256 * LN_MAXC) return hipErrorInvalidValue;
    hipLaunchKernelGGL(layernorm_kernel<half_t>, dim3((M + 3) / 4), dim3(256), 0, s, x, w, b, out, M, D, gather,
                       rows_per_seq, in_row_mul);
    return hipGetLastError();
}
hipError_t launch_layernorm_f32(const float* x, const float* w, const float* b, float* out, int M, int D,
                                hipStream_t s, const float* pos, const float* cls, int L) {
    if (M <= 0) return hipSuccess;
    if (D % 4 || D > 256 * LN_MAXC || (pos && (!cls || L < 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(layernorm_kernel<float>, dim3((M + 3) / 4), dim3(256), 0, s, x, w, b, out, M, D,
                       (const int32_t*)nullptr, 0, 1, pos, cls, L);
    return hipGetLastError();
}

// ---- im2col: patch matrix of the stride-p conv (clipnet/model.py:220-222) -------------------------
// thread -> 8 consecutive pixels of one image row segment inside a patch (32 B read, 16 B write)
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ x, half_t* __restrict__ out, int B,
                                                     int R, int p) {
    const int g = R / p, pk = p / 8;
    const size_t total = (size_t)B * 3 * R * (R / 8);
    const int K = 3 * p * p;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int xs = (int)(i % (R / 8));          // 8-pixel segment along x
        size_t rest = i / (R / 8);
        const int y = (int)(rest % R);
        rest /= R;
        const int c = (int)(rest % 3);
        const int b = (int)(rest / 3);
        const f32x4* src = reinterpret_cast<const f32x4*>(x + (((size_t)b * 3 + c) * R + y) * R + xs * 8);
        const f32x4 a = src[0], d = src[1];
        const int gy = y / p, ky = y - gy * p, gx = xs / pk, kx = (xs - gx * pk) * 8;
        half8 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = (half_t)a[e];
            h[4 + e] = (half_t)d[e];
        }
        *reinterpret_cast<half8*>(out + ((size_t)b * g * g + gy * g + gx) * K + c * p * p + ky * p + kx) = h;
    }
}
// Any patch size (p = 14: rows of 14 floats = 56 B are 8-byte aligned in the image, 4-byte aligned in the fp16 matrix, so the 8-pixel
// mapping above does not apply): thread -> the p pixels of one image row inside one patch, neighbouring threads neighbouring patches
// of the same image row (the reads of a wave are one contiguous stretch).  Row stride of the matrix is Kp >= 3*p*p; the thread that
// holds a patch's first row (c = 0, ky = 0) also writes zeros into its pad columns 3*p*p .. Kp-1 - on every call, whatever the
// workspace held.  EVEN: p is even, two pixels per load / store.
template <bool EVEN>
__global__ __launch_bounds__(256) void im2col_pad_kernel(const float* __restrict__ x, half_t* __restrict__ out, int B, int R, int p,
                                                         int Kp) {
    const int g = R / p, K = 3 * p * p;
    const size_t total = (size_t)B * 3 * R * g;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int gx = (int)(i % g);
        size_t rest = i / g;
        const int y = (int)(rest % R);
        rest /= R;
        const int c = (int)(rest % 3);
        const int b = (int)(rest / 3);
        const int gy = y / p, ky = y - gy * p;
        const float* src = x + (((size_t)b * 3 + c) * R + y) * R + gx * p;
        half_t* row = out + ((size_t)b * g * g + gy * g + gx) * Kp;
        half_t* dst = row + c * p * p + ky * p;
        if constexpr (EVEN) {
            for (int e = 0; e < p; e += 2) {
                const float2 a = *reinterpret_cast<const float2*>(src + e);
                half2v h;
                h[0] = (half_t)a.x;
                h[1] = (half_t)a.y;
                *reinterpret_cast<half2v*>(dst + e) = h;
            }
        } else {
            for (int e = 0; e < p; ++e) dst[e] = (half_t)src[e];
        }
        if (c == 0 && ky == 0) {
            if constexpr (EVEN) {
                half2v z;
                z[0] = (half_t)0.f;
                z[1] = (half_t)0.f;
                for (int e = K; e < Kp; e += 2) *reinterpret_cast<half2v*>(row + e) = z;
            } else {
                for (int e = K; e < Kp; ++e) row[e] = (half_t)0.f;
            }
        }
    }
}
hipError_t launch_im2col(const float* x, half_t* out, int B, int R, int p, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (p <= 0 || R % p) return hipErrorInvalidValue;
    if (p % 8) {
        const size_t total = (size_t)B * 3 * R * (R / p);
        const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
        if (p % 2) hipLaunchKernelGGL(im2col_pad_kernel<false>, dim3(grid), dim3(256), 0, s, x, out, B, R, p, im2col_kp(p));
        else hipLaunchKernelGGL(im2col_pad_kernel<true>, dim3(grid), dim3(256), 0, s, x, out, B, R, p, im2col_kp(p));
        return hipGetLastError();
    }
    const size_t total = (size_t)B * 3 * R * (R / 8);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(im2col_kernel, dim3(grid), dim3(256), 0, s, x, out, B, R, p);
    return hipGetLastError();
}


// ---- text embedding: x = token_embedding[ids] + positional (clipnet/model.py:340-342) ------------
__global__ __launch_bounds__(256) void embed_tokens_kernel(const int32_t* __restrict__ ids, int ld_ids,
                                                           const float* __restrict__ table,
                                                           const float* __restrict__ pos, float* __restrict__ x,
                                                           int T, int L, int D, int vocab) {
    const int nc = D >> 2;
    const size_t total = (size_t)T * L * nc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % nc);
        const size_t r = i / nc;
        const int t = (int)(r / L), l = (int)(r - (size_t)t * L);
        int id = ids[(size_t)t * ld_ids + l];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        const f32x4 e = reinterpret_cast<const f32x4*>(table + (size_t)id * D)[c];
        const f32x4 pe = reinterpret_cast<const f32x4*>(pos + (size_t)l * D)[c];
        reinterpret_cast<f32x4*>(x + r * D)[c] = e + pe;
    }
}
hipError_t launch_embed_tokens(const int32_t* ids, int ld_ids, const float* table, const float* pos, float* x,
                               int T, int L, int D, int vocab, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    if (D % 4) return hipErrorInvalidValue;      // (16-byte chunks: the last D % 4 columns would stay unwritten)
    const size_t total = (size_t)T * L * (D / 4);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(embed_tokens_kernel, dim3(grid), dim3(256), 0, s, ids, ld_ids, table, pos, x, T, L, D, vocab);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void add_pos_kernel(const float* __restrict__ prompts, int Lfull,
                                                      const float* __restrict__ pos, float* __restrict__ x, int R,
                                                      int L, int D) {
    const int nc = D >> 2;
    const size_t total = (size_t)R * L * nc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % nc);
        const size_t r = i / nc;
        const int t = (int)(r / L), l = (int)(r - (size_t)t * L);
        const f32x4 e = reinterpret_cast<const f32x4*>(prompts + ((size_t)t * Lfull + l) * D)[c];
        const f32x4 pe = reinterpret_cast<const f32x4*>(pos + (size_t)l * D)[c];
        reinterpret_cast<f32x4*>(x + r * D)[c] = e + pe;
    }
}
hipError_t launch_add_pos(const float* prompts, int Lfull, const float* pos, float* x, int R, int L, int D,
                          hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (D % 4) return hipErrorInvalidValue;
    const size_t total = (size_t)R * L * (D / 4);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(add_pos_kernel, dim3(grid), dim3(256), 0, s, prompts, Lfull, pos, x, R, L, D);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const int32_t* __restrict__ ids,
                                                          const float* __restrict__ table, float* __restrict__ out,
                                                          int n, int D, int vocab) {
    const int nc = D >> 2;
    const size_t total = (size_t)n * nc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % nc);
        const size_t r = i / nc;
        int id = ids[r];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        reinterpret_cast<f32x4*>(out + r * D)[c] = reinterpret_cast<const f32x4*>(table + (size_t)id * D)[c];
    }
}
hipError_t launch_gather_rows(const int32_t* ids, const float* table, float* out, int n, int D, int vocab,
                              hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (D % 4) return hipErrorInvalidValue;
    const size_t total = (size_t)n * (D / 4);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, s, ids, table, out, n, D, vocab);
    return hipGetLastError();
}

// ---- EOT index = argmax over the row (first occurrence of the maximum, like torch.argmax;
// clipnet/model.py:350) and the batch maximum of those indices (for causal truncation) -------------
__global__ __launch_bounds__(64) void eot_argmax_kernel(const int32_t* __restrict__ ids, int T, int L,
                                                        int32_t* __restrict__ eot, int32_t* __restrict__ max_eot) {
    const int t = blockIdx.x, lane = threadIdx.x;
    int best = INT32_MIN, bi = 0x7fffffff;
    for (int l = lane; l < L; l += 64) {
        const int v = ids[(size_t)t * L + l];
        if (v > best) { best = v; bi = l; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ov = __shfl_xor(best, o, 64), oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) {
        eot[t] = bi;
        if (max_eot) atomicMax(max_eot, bi);
    }
}
hipError_t launch_eot_argmax(const int32_t* ids, int T, int L, int32_t* eot, int32_t* max_eot, hipStream_t s) {
    if (T <= 0) return hipSuccess;
    hipLaunchKernelGGL(eot_argmax_kernel, dim3(T), dim3(64), 0, s, ids, T, L, eot, max_eot);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void clamp_eot_kernel(const int32_t* in, int n, int Leff, int32_t* out, int32_t* flag,
                                                        int32_t* flag_dev) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int v = in[i];
    if (v >= Leff) {
        if (flag) *flag = 1;
        if (flag_dev) *flag_dev = 1;
        v = Leff - 1;
    }
    out[i] = v < 0 ? 0 : v;
}
hipError_t launch_clamp_eot(const int32_t* in, int n, int Leff, int32_t* out, int32_t* flag, hipStream_t s, int32_t* flag_dev) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(clamp_eot_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, n, Leff, out, flag, flag_dev);
    return hipGetLastError();
}

// A truncation length that did not cover every EOT row (flag set by clamp_eot_kernel earlier in the same call): the call's
// whole output becomes NaN - the stale call itself is loud, not only the next one (it cannot be failed without a sync)
// (flag: DEVICE memory - a quarter of a million lanes polling a host-mapped word over PCIe cost 0.7 ms per call)
__global__ __launch_bounds__(256) void poison_if_flag_kernel(float* out, size_t n, const int32_t* flag) {
    if (*(const volatile int32_t*)flag == 0) return;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = __builtin_nanf("");
}
hipError_t launch_poison_if_flag(float* out, size_t n, const int32_t* flag, hipStream_t s) {
    if (n == 0 || !flag) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(poison_if_flag_kernel, dim3((unsigned)blocks), dim3(256), 0, s, out, n, flag);
    return hipGetLastError();
}

// ---- dtype conversion / transposition (weight loading) ------------------------------------------------
// dtype conversions, HBM-bound: 8 elements per lane (2 x 16-byte loads -> one 16-byte store, and back) when the
// pointers are 16-byte aligned, scalar otherwise and for the tail
__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float* __restrict__ in, half_t* __restrict__ out, size_t n,
                                                         int vec) {
    const size_t n8 = vec ? n / 8 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const f32x4 a = reinterpret_cast<const f32x4*>(in)[2 * i], b = reinterpret_cast<const f32x4*>(in)[2 * i + 1];
        half8 h;
#pragma unroll
        for (int k = 0; k < 4; ++k) { h[k] = (half_t)a[k]; h[4 + k] = (half_t)b[k]; }
        reinterpret_cast<half8*>(out)[i] = h;
    }
    for (size_t i = n8 * 8 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (half_t)in[i];
}
__global__ __launch_bounds__(256) void f16_to_f32_kernel(const half_t* __restrict__ in, float* __restrict__ out, size_t n,
                                                         int vec) {
    const size_t n8 = vec ? n / 8 : 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const half8 h = reinterpret_cast<const half8*>(in)[i];
        f32x4 a, b;
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = (float)h[k]; b[k] = (float)h[4 + k]; }
        reinterpret_cast<f32x4*>(out)[2 * i] = a;
        reinterpret_cast<f32x4*>(out)[2 * i + 1] = b;
    }
    for (size_t i = n8 * 8 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (float)in[i];
}
hipError_t launch_f32_to_f16(const float* in, half_t* out, size_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    const int vec = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const size_t work = vec ? (n + 7) / 8 : n;
    const int grid = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3(grid), dim3(256), 0, s, in, out, n, vec);
    return hipGetLastError();
}
// lo of a weight held as hi + lo: 2^11 x fp16(w - fp16(w)) (weight-load time; the remainder itself would sit in fp16's subnormals)
__global__ __launch_bounds__(256) void f16_remainder_kernel(const float* __restrict__ in, half_t* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float x = in[i];
        out[i] = (half_t)((x - (float)(half_t)x) * 2048.0f);
    }
}
hipError_t launch_f16_remainder(const float* in, half_t* out, size_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(f16_remainder_kernel, dim3(grid), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}
hipError_t launch_f16_to_f32(const half_t* in, float* out, size_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    const int vec = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const size_t work = vec ? (n + 7) / 8 : n;
    const int grid = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(grid), dim3(256), 0, s, in, out, n, vec);
    return hipGetLastError();
}
__global__ void transpose_to_f16_kernel(const void* __restrict__ in, int in_dtype, half_t* __restrict__ out,
                                        int rows, int cols) {
    const size_t n = (size_t)rows * cols;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i / rows), r = (int)(i - (size_t)c * rows);   // out[c][r]
        const size_t src = (size_t)r * cols + c;
        out[i] = in_dtype == 0 ? (half_t) reinterpret_cast<const float*>(in)[src]
                               : reinterpret_cast<const half_t*>(in)[src];
    }
}
hipError_t launch_transpose_to_f16(const void* in, int in_dtype, half_t* out, int rows, int cols, hipStream_t s) {
    const size_t n = (size_t)rows * cols;
    if (!n) return hipSuccess;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(transpose_to_f16_kernel, dim3(grid), dim3(256), 0, s, in, in_dtype, out, rows, cols);
    return hipGetLastError();
}

// ---- x / ||x||_2 per row (main_coop_vae.py:438,466) ----------------------------------------------
__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                           int R, int D) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float v = x[(size_t)r * D + d];
        q += v * v;
    }
    const float inv = 1.0f / sqrtf(wave_sum(q));
    for (int d = lane; d < D; d += 64) out[(size_t)r * D + d] = x[(size_t)r * D + d] * inv;
}
hipError_t launch_l2_normalize(const float* x, float* out, int R, int D, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((R + 3) / 4), dim3(256), 0, s, x, out, R, D);
    return hipGetLastError();
}

// ---- PromptLearner_*.forward (main_coop_vae.py:119-128) -------------------------------------------
__global__ __launch_bounds__(256) void assemble_prompts_kernel(const float* __restrict__ prefix,
                                                               const float* __restrict__ suffix,
                                                               const float* __restrict__ ctx,
                                                               const float* __restrict__ bias,
                                                               const int32_t* __restrict__ target, int R, int C, int L,
                                                               int n_ctx, int D, float* __restrict__ prompts) {
    const int nc = D >> 2;
    const size_t total = (size_t)R * L * nc;
    const int ls = L - 1 - n_ctx;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % nc);
        const size_t rl = i / nc;
        const int r = (int)(rl / L), l = (int)(rl - (size_t)r * L);
        int t = target[r];
        t = t < 0 ? 0 : (t >= C ? C - 1 : t);
        f32x4 v;
        if (l == 0) v = reinterpret_cast<const f32x4*>(prefix + (size_t)t * D)[c];
        else if (l <= n_ctx)
            v = reinterpret_cast<const f32x4*>(ctx + (size_t)(l - 1) * D)[c] +
                reinterpret_cast<const f32x4*>(bias + (size_t)r * D)[c];
        else v = reinterpret_cast<const f32x4*>(suffix + ((size_t)t * ls + (l - 1 - n_ctx)) * D)[c];
        reinterpret_cast<f32x4*>(prompts + rl * D)[c] = v;
    }
}
hipError_t launch_assemble_prompts(const float* prefix, const float* suffix, const float* ctx, const float* bias,
                                   const int32_t* target, int R, int C, int L, int n_ctx, int D, float* prompts,
                                   hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (D % 4 || n_ctx < 0 || n_ctx >= L) return hipErrorInvalidValue;
    const size_t total = (size_t)R * L * (D / 4);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(assemble_prompts_kernel, dim3(grid), dim3(256), 0, s, prefix, suffix, ctx, bias, target, R, C,
                       L, n_ctx, D, prompts);
    return hipGetLastError();
}

// ---- reparameterise (main_coop_vae.py:445-447): z = exp(0.5 * log_var) * eps + mean ------------------------------
// HBM-bound: 12 B read + 4 (+2) B written per element, 16-byte accesses.
__global__ __launch_bounds__(256) void reparam_kernel(const f32x4* __restrict__ mean, const f32x4* __restrict__ logvar,
                                                      const f32x4* __restrict__ eps, size_t total4, int D4,
                                                      f32x4* __restrict__ z, half_t* __restrict__ z16, int ld16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        const f32x4 m = mean[i], lv = logvar[i], e = eps[i];
        f32x4 zz;
#pragma unroll
        for (int k = 0; k < 4; ++k) zz[k] = reparam1(m[k], lv[k], e[k]);
        if (z) z[i] = zz;
        const size_t r = i / D4;
        const int d4 = (int)(i - r * D4);
        half4 h;
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = (half_t)zz[k];
        *reinterpret_cast<half4*>(z16 + r * ld16 + 4 * d4) = h;
    }
}
hipError_t launch_reparam(const float* mean, const float* logvar, const float* eps, int R, int D, float* z, half_t* z16,
                          int ld16, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (D % 4 || ld16 % 4) return hipErrorInvalidValue;
    const size_t total4 = (size_t)R * (D / 4);
    const int grid = (int)((total4 + 255) / 256 < 4096 ? (total4 + 255) / 256 : 4096);
    hipLaunchKernelGGL(reparam_kernel, dim3(grid), dim3(256), 0, s, (const f32x4*)mean, (const f32x4*)logvar,
                       (const f32x4*)eps, total4, D / 4, (f32x4*)z, z16, ld16);
    return hipGetLastError();
}

// ---- vae_loss forward (main_coop_vae.py:300-303) ---------------------------------------------------
__global__ __launch_bounds__(256) void vae_loss_kernel(const float* __restrict__ recon, const float* __restrict__ x,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ logvar, int R, int D,
                                                       float* __restrict__ loss) {
    __shared__ float part[4];
    const size_t total = (size_t)R * D;
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const float d = recon[i] - x[i];
        const float m = mean[i], lv = logvar[i];
        acc += d * d - 0.5f * (1.0f + lv - m * m - expf(lv));
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss, (part[0] + part[1] + part[2] + part[3]) / (float)R);
}
hipError_t launch_vae_loss(const float* recon, const float* x, const float* mean, const float* logvar, int R,
                           int D, float* loss, hipStream_t s) {
    hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), s);
    if (e != hipSuccess || R <= 0) return e;
    const size_t total = (size_t)R * D;
    const int grid = (int)((total + 255) / 256 < 256 ? (total + 255) / 256 : 256);
    hipLaunchKernelGGL(vae_loss_kernel, dim3(grid), dim3(256), 0, s, recon, x, mean, logvar, R, D, loss);
    return hipGetLastError();
}

// ---- variant C output split (CLIP_models_adapter_prior2.py:506): tokens [B*L,E] ->
//      global [B,E] = token 0; local [B,E,g,g] = tokens 1.. permuted to NCHW --------------------------
__global__ __launch_bounds__(256) void split_global_local_kernel(const float* __restrict__ tok,
                                                                 float* __restrict__ glob,
                                                                 float* __restrict__ local, int B, int L, int E) {
    // block = one image x 32 channels; stage [G, 32] through LDS so both sides are coalesced
    __shared__ float tile[32][33];
    const int G = L - 1;
    const int b = blockIdx.y, e0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    if (ty == 0 && glob) glob[(size_t)b * E + e0 + tx] = tok[((size_t)b * L) * E + e0 + tx];
    for (int t0 = 0; t0 < G; t0 += 32) {
        for (int r = ty; r < 32; r += 8) {
            const int t = t0 + r;
            tile[r][tx] = t < G ? tok[((size_t)b * L + 1 + t) * E + e0 + tx] : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int t = t0 + tx;
            if (t < G) local[((size_t)b * E + e0 + r) * G + t] = tile[tx][r];
        }
        __syncthreads();
    }
}
hipError_t launch_split_global_local(const float* tok, float* glob, float* local, int B, int L, int E,
                                     hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (E % 32 || !local) return hipErrorInvalidValue;      // (glob may be null, local is always written)
    hipLaunchKernelGGL(split_global_local_kernel, dim3(E / 32, B), dim3(256), 0, s, tok, glob, local, B, L, E);
    return hipGetLastError();
}

__global__ void copy_rows_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int row_stride, int D,
                                 const int32_t* __restrict__ gather) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, d = i - b * D;
    int g = gather ? gather[b] : 0;
    g = g < 0 ? 0 : (g >= row_stride ? row_stride - 1 : g);      // caller error guard, as in layernorm_kernel
    out[i] = x[((size_t)b * row_stride + g) * D + d];
}
hipError_t launch_copy_rows(const float* x, float* out, int B, int row_stride, int D, hipStream_t s,
                            const int32_t* gather) {
    if (B <= 0) return hipSuccess;
    if (D <= 0 || (size_t)B * D > (size_t)INT_MAX - 255) return hipErrorInvalidValue;      // (the kernel's element index is an int)
    hipLaunchKernelGGL(copy_rows_kernel, dim3((B * D + 255) / 256), dim3(256), 0, s, x, out, B, row_stride, D, gather);
    return hipGetLastError();
}
// row b * row_stride of a stream held as centre + hi + lo (GemmArgs::hl): hi row-major [*, D], lo in gemm_ring2's tile-fragment
// order (tile 128 x 256; wave = (row % 64) / 32 * 4 + (col % 128) / 32; piece = (row / 64 % 2, col / 128 % 2, col / 16 % 2);
// lane = (col % 16) / 4 * 16 + row % 16; inside the lane's 8 bytes: row tile (row % 32) / 16, then col % 4)
__global__ void copy_rows_hilo_kernel(const half_t* __restrict__ hi, const half_t* __restrict__ lo, const float* __restrict__ muc,
                                      float* __restrict__ out, int B, int row_stride, int D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * D) return;
    const int b = i / D, n = i - b * D;
    const size_t m = (size_t)b * row_stride;
    const int r = (int)(m & 127), cc = n & 255;
    const size_t tile = (m >> 7) * (size_t)(D >> 8) + (n >> 8);
    const int wave = ((r & 63) >> 5) * 4 + ((cc & 127) >> 5);
    const int piece = (r >> 6) * 4 + (cc >> 7) * 2 + ((cc >> 4) & 1);
    const int lane = ((cc & 15) >> 2) * 16 + (r & 15);
    const size_t lo_i = (((tile * 8 + wave) * 8 + piece) * 64 + lane) * 8 + ((r & 31) >> 4) * 4 + (cc & 3);
    const unsigned short b8 = reinterpret_cast<const unsigned char*>(lo)[lo_i];      // bf8 (e5m2) = the top byte of an fp16
    const float lof = (float)__builtin_bit_cast(half_t, (unsigned short)(b8 << 8)) * (1.0f / HG_LO_SCALE);
    out[i] = (muc[m] + (float)hi[m * D + n]) + lof;
}
hipError_t launch_copy_rows_hilo(const half_t* hi, const half_t* lo, const float* muc, float* out, int B, int row_stride, int D,
                                 hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (D <= 0 || D % 256 || (size_t)B * D > (size_t)INT_MAX - 255) return hipErrorInvalidValue;      // (int element index, as copy_rows)
    hipLaunchKernelGGL(copy_rows_hilo_kernel, dim3((B * D + 255) / 256), dim3(256), 0, s, hi, lo, muc, out, B, row_stride, D);
    return hipGetLastError();
}
// first N columns of a [R, ld] matrix -> dense [R, N]
__global__ void copy_cols_kernel(const float* __restrict__ x, int ld, float* __restrict__ out, int R, int N) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)R * N) return;
    const int r = (int)(i / N), j = (int)(i - (size_t)r * N);
    out[i] = x[(size_t)r * ld + j];
}
hipError_t launch_copy_cols(const float* x, int ld, float* out, int R, int N, hipStream_t s) {
    if (R <= 0 || N <= 0) return hipSuccess;
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)(((size_t)R * N + 255) / 256)), dim3(256), 0, s, x, ld, out, R, N);
    return hipGetLastError();
}

// ---- LayerNorm folding support ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_ln_kernel(const half_t* __restrict__ w16, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ bias,
                                                      half_t* __restrict__ wf16, float* __restrict__ cs,
                                                      float* __restrict__ bf, int N, int K, float* __restrict__ csg) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float c = 0.f, b = 0.f, cg = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = (float)w16[(size_t)n * K + k];
        // fp16(fl(w gamma)): the product is rounded to fp32 FIRST.  Left to -ffp-contract the multiply and the conversion became one
        // mixed-precision instruction that rounds the exact product once, and about 1 weight in 30 000 was another fp16 number than
        // the one this line and hg_kernels.h state (tests/test_gpu_elem.py::test_fold_ln); the empty asm keeps the two apart
        float wg = w * gamma[k];
        asm volatile("" : "+v"(wg));
        const half_t wf = (half_t)wg;
        wf16[(size_t)n * K + k] = wf;
        c += (float)wf;
        b += w * beta[k];
        cg += w * gamma[k];
    }
    c = wave_sum(c);
    b = wave_sum(b);
    cg = wave_sum(cg);
    if (lane == 0) {
        cs[n] = c;
        bf[n] = (bias ? bias[n] : 0.f) + b;
        // column sums for the form that keeps gamma in the ACTIVATION copy and W unrounded (GemmArgs::gamma): sum_k gamma[k] W[n][k]
        if (csg) csg[n] = cg;
    }
}
hipError_t launch_fold_ln(const half_t* w16, const float* gamma, const float* beta, const float* bias, half_t* wf16,
                          float* cs, float* bf, int N, int K, hipStream_t s, float* csg) {
    if (N <= 0) return hipSuccess;
    if (K <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fold_ln_kernel, dim3((N + 3) / 4), dim3(256), 0, s, w16, gamma, beta, bias, wf16, cs, bf, N, K, csg);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void rowstats_cast_kernel(const float* __restrict__ x, half_t* __restrict__ x16,
                                                            float* __restrict__ mr, float* __restrict__ mu, int M, int D,
                                                            float* __restrict__ muc, const float* __restrict__ gamma) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const f32x4* xp = reinterpret_cast<const f32x4*>(x + (size_t)r * D);
    const int nc = D >> 2;
    f32x4 v[LN_MAXC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            v[i] = xp[c];
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            half4 h;
            const f32x4 gm = gamma ? reinterpret_cast<const f32x4*>(gamma)[c] : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                q += d * d;
                h[e] = gamma ? (half_t)(d * gm[e]) : (half_t)d;      // (gamma: the copy carries the next LayerNorm's weight, GemmArgs::gamma)
            }
            reinterpret_cast<half4*>(x16 + (size_t)r * D)[c] = h;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
    if (lane == 0) {
        mr[2 * (size_t)r] = 0.f;
        mr[2 * (size_t)r + 1] = rstd;
        mu[r] = mean;
        if (muc) muc[r] = mean;
    }
}
// ln_pre and the first block's folding statistics in one pass (vision tower, LayerNorm folding on): y = LN(x) written in
// place as fp32, then exactly rowstats_cast's arithmetic on the y values still in registers (same bits as the two kernels)
__global__ __launch_bounds__(256) void layernorm_rowstats_kernel(float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ b, half_t* __restrict__ x16,
                                                                 float* __restrict__ mr, float* __restrict__ mu,
                                                                 float* __restrict__ muc, int M, int D,
                                                                 const float* __restrict__ pos, const float* __restrict__ cls,
                                                                 int Lpos, int ld16) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    f32x4* xp = reinterpret_cast<f32x4*>(x + (size_t)r * D);
    // pos != nullptr: the row is [cls ; patch embedding] + pos[t] first (see layernorm_kernel)
    const int tpos = pos ? r % Lpos : 0;
    const f32x4* xin = (pos && tpos == 0) ? reinterpret_cast<const f32x4*>(cls) : xp;
    const f32x4* pp = reinterpret_cast<const f32x4*>(pos ? pos + (size_t)tpos * D : nullptr);
    const int nc = D >> 2;
    f32x4 v[LN_MAXC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            v[i] = xin[c];
            if (pos) v[i] += pp[c];
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean;
                q += d * d;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
    const f32x4* wp = reinterpret_cast<const f32x4*>(w);
    const f32x4* bp = reinterpret_cast<const f32x4*>(b);
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            const f32x4 g = wp[c], be = bp[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = (v[i][e] - mean) * rstd * g[e] + be[e];
            xp[c] = v[i];
            s2 += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean2 = wave_sum(s2) / (float)D;
    float q2 = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            half4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[i][e] - mean2;
                q2 += d * d;
                h[e] = (half_t)d;
            }
            reinterpret_cast<half4*>(x16 + (size_t)r * ld16)[c] = h;
        }
    }
    const float rstd2 = 1.0f / sqrtf(wave_sum(q2) / (float)D + 1e-5f);
    if (lane == 0) {
        mr[2 * (size_t)r] = 0.f;
        mr[2 * (size_t)r + 1] = rstd2;
        mu[r] = mean2;
        if (muc) muc[r] = mean2;
    }
}
hipError_t launch_layernorm_rowstats(float* x, const float* w, const float* b, half_t* x16, float* mr, float* mu, float* muc,
                                     int M, int D, hipStream_t s, const float* pos, const float* cls, int L, int ld16) {
    if (M <= 0) return hipSuccess;
    if (!ld16) ld16 = D;
    if (D % 4 || D > 256 * LN_MAXC || (pos && (!cls || L < 1)) || ld16 < D || ld16 % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(layernorm_rowstats_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, w, b, x16, mr, mu, muc, M, D, pos, cls, L,
                       ld16);
    return hipGetLastError();
}
hipError_t launch_rowstats_cast(const float* x, half_t* x16, float* mr, float* mu, int M, int D, hipStream_t s, float* muc,
                                const float* gamma) {
    if (M <= 0) return hipSuccess;
    if (D % 4 || D > 256 * LN_MAXC) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rowstats_cast_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, x16, mr, mu, M, D, muc, gamma);
    return hipGetLastError();
}

// The copy and statistics rowstats_cast left (centre = the row's own mean) moved to the centre c[m] a preceding residual GEMM would have
// used (its previous mean): x16 = fp16(x - c) with row stride ld16, mr[m][0] = mean - c, muc[m] = c; mu (the mean) and rstd stay.
// Test hook only (hg_test_adapter).
__global__ __launch_bounds__(256) void recentre_cast_kernel(const float* __restrict__ x, const float* __restrict__ c,
                                                            half_t* __restrict__ x16, int ld16, float* __restrict__ mr,
                                                            const float* __restrict__ mu, float* __restrict__ muc, int M, int D) {
    const int r = blockIdx.x;
    if (r >= M) return;
    const float cr = c[r];
    for (int k = threadIdx.x; k < D; k += 256) x16[(size_t)r * ld16 + k] = (half_t)(x[(size_t)r * D + k] - cr);
    if (threadIdx.x == 0) {
        mr[2 * (size_t)r] = mu[r] - cr;
        muc[r] = cr;
    }
}
hipError_t launch_recentre_cast(const float* x, const float* c, half_t* x16, int ld16, float* mr, const float* mu, float* muc, int M,
                                int D, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (ld16 < D) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recentre_cast_kernel, dim3(M), dim3(256), 0, s, x, c, x16, ld16, mr, mu, muc, M, D);
    return hipGetLastError();
}

// partial statistics of row m over nt column groups of `gw` columns each: (sum_k, M2_k = sum (x - mean_k)^2);
// combined with Chan's parallel-variance formula (no E[x^2] - mean^2 cancellation)
__global__ void finalize_stats_kernel(const float* __restrict__ stats, float* __restrict__ mr, float* __restrict__ mu,
                                      int M, int nt, int gw, float* __restrict__ muc, int centred, int* __restrict__ range_flag) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    finalize_stats_row<false>(stats + (size_t)m * nt * 2, mr, mu, muc, m, nt, gw, centred, range_flag);      // (hg_gemm_dev.h)
}
hipError_t launch_finalize_stats(const float* stats, float* mr, float* mu, int M, int nt, int gw, hipStream_t s, float* muc,
                                 bool centred, int* range_flag) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(finalize_stats_kernel, dim3((M + 255) / 256), dim3(256), 0, s, stats, mr, mu, M, nt, gw, muc,
                       centred ? 1 : 0, range_flag);
    return hipGetLastError();
}

// [w_out | fp16(scale * up_w)] and b_out + scale * up_b (weight-load time)
__global__ __launch_bounds__(256) void concat_upproj_kernel(const half_t* __restrict__ w_out, const float* __restrict__ b_out,
                                                            const half_t* __restrict__ up_w, const float* __restrict__ up_b,
                                                            const float* __restrict__ scale, half_t* __restrict__ wk,
                                                            float* __restrict__ bk, int N, int K, int d) {
    const int n = blockIdx.x;
    const float sc = scale[n];
    for (int k = threadIdx.x; k < K + d; k += 256)
        wk[(size_t)n * (K + d) + k] = k < K ? w_out[(size_t)n * K + k] : (half_t)(sc * (float)up_w[(size_t)n * d + (k - K)]);
    if (threadIdx.x == 0) bk[n] = b_out[n] + sc * up_b[n];
}
hipError_t launch_concat_upproj(const half_t* w_out, const float* b_out, const half_t* up_w, const float* up_b,
                                const float* scale, half_t* wk, float* bk, int N, int K, int d, hipStream_t s) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(concat_upproj_kernel, dim3(N), dim3(256), 0, s, w_out, b_out, up_w, up_b, scale, wk, bk, N, K, d);
    return hipGetLastError();
}

// ---- adapter folded into the block's own GEMMs (weight-load time; DESIGN.md §4 "variant C") -------------------------
// The decoder's last LayerNorm gives d = g3 * z + b3 with sum_i z_i = 0, so the adapter's update of row x is
//   a = scale * (W_up d + b_up) = Q e,   e = [z_0 .. z_62, 1],
//   Q[:, i] = g3_i P[:, i] - g3_63 P[:, 63]  (i < 63),   Q[:, 63] = P b3 + scale * b_up,   P = diag(scale) W_up
// - no bias term left, which is what lets every consumer take `a` as 64 more K columns.
__global__ __launch_bounds__(64) void adapter_q_kernel(const half_t* __restrict__ up_w, const float* __restrict__ up_b,
                                                       const float* __restrict__ scale, const float* __restrict__ norms,
                                                       float* __restrict__ q32, int D) {
    const int j = blockIdx.x, i = threadIdx.x;
    const float sc = scale[j];
    const float* g3 = norms + 128;
    const float* b3 = norms + 192;
    __shared__ float P[64];
    P[i] = sc * (float)up_w[(size_t)j * 64 + i];
    __syncthreads();
    float v;
    if (i < 63) v = g3[i] * P[i] - g3[63] * P[63];
    else {
        v = sc * up_b[j];
        for (int k = 0; k < 64; ++k) v = fmaf(b3[k], P[k], v);
    }
    q32[(size_t)j * 64 + i] = v;
}
// down2 [128, D]: rows 0..63 = down_w, rows 64+i = fp16(Q[:, i]);  wk [D, D+64] = [w_out | fp16(Q)];
// wq [N3, D+64] = [wf_qkv | fp16(wf_qkv Q)]
__global__ __launch_bounds__(256) void adapter_fold_down_kernel(const half_t* __restrict__ down_w, const float* __restrict__ q32,
                                                                half_t* __restrict__ down2, int D) {
    const int n = blockIdx.x;
    for (int k = threadIdx.x; k < D; k += 256)
        down2[(size_t)n * D + k] = n < 64 ? down_w[(size_t)n * D + k] : (half_t)q32[(size_t)k * 64 + (n - 64)];
}
__global__ __launch_bounds__(256) void adapter_fold_w_kernel(const half_t* __restrict__ w, const float* __restrict__ q32,
                                                             half_t* __restrict__ wk, int K, int identity) {
    const int n = blockIdx.x;
    for (int k = threadIdx.x; k < K; k += 256) wk[(size_t)n * (K + 64) + k] = w[(size_t)n * K + k];
    if (identity) {      // K == D, rows of w are rows of the stream: the update itself
        if (threadIdx.x < 64) wk[(size_t)n * (K + 64) + K + threadIdx.x] = (half_t)q32[(size_t)n * 64 + threadIdx.x];
        return;
    }
    __shared__ float part[4][64];
    const int i = threadIdx.x & 63, c = threadIdx.x >> 6;
    float acc = 0.f;
    for (int j = c; j < K; j += 4) acc = fmaf((float)w[(size_t)n * K + j], q32[(size_t)j * 64 + i], acc);
    part[c][i] = acc;
    __syncthreads();
    if (threadIdx.x < 64) wk[(size_t)n * (K + 64) + K + i] = (half_t)((part[0][i] + part[1][i]) + (part[2][i] + part[3][i]));
}
// statistics operands from the fp16-rounded Q the GEMMs really use: qm[i] = sum_j Q[j][i], G = Q^T Q (fp16 [64][64])
__global__ __launch_bounds__(64) void adapter_fold_g_kernel(const float* __restrict__ q32, float* __restrict__ qm,
                                                            half_t* __restrict__ g16, int D) {
    const int i = blockIdx.x, k = threadIdx.x;
    float g = 0.f, m = 0.f;
    for (int j = 0; j < D; ++j) {
        const float a = (float)(half_t)q32[(size_t)j * 64 + i], b = (float)(half_t)q32[(size_t)j * 64 + k];
        g = fmaf(a, b, g);
        m += a;
    }
    g16[i * 64 + k] = (half_t)g;
    if (k == 0) qm[i] = m;
}
hipError_t launch_adapter_fold(const half_t* up_w, const float* up_b, const float* scale, const float* norms,
                               const half_t* down_w, const half_t* w_out, const half_t* wf_qkv, int D, float* q32,
                               half_t* down2, half_t* wk_out, half_t* wq_cat, float* qm, half_t* g16, hipStream_t s) {
    hipLaunchKernelGGL(adapter_q_kernel, dim3(D), dim3(64), 0, s, up_w, up_b, scale, norms, q32, D);
    hipLaunchKernelGGL(adapter_fold_down_kernel, dim3(128), dim3(256), 0, s, down_w, q32, down2, D);
    hipLaunchKernelGGL(adapter_fold_w_kernel, dim3(D), dim3(256), 0, s, w_out, q32, wk_out, D, 1);
    hipLaunchKernelGGL(adapter_fold_w_kernel, dim3(3 * D), dim3(256), 0, s, wf_qkv, q32, wq_cat, D, 0);
    hipLaunchKernelGGL(adapter_fold_g_kernel, dim3(64), dim3(64), 0, s, q32, qm, g16, D);
    return hipGetLastError();
}

}  // namespace hg
