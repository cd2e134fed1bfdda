// Backward kernels of the frozen CLIP text tower (gfx950): the gradient of TextEncoder.forward (main_coop_vae.py:54-63) with respect to
// its `prompts` input, which the CoOp-VAE training loop (main_coop_vae.py:452-468) back-propagates through.  No weight gradients.
//   text_attn_bwd_kernel    causal attention backward of one (prompt, head): dQ, dK, dV from Q, K, V, dO (L <= 80, head dim 64)
//   layernorm_bwd_kernel    g += LayerNorm_backward(x, gamma, dy), a row per wave, optionally scattered to one row per prompt
//   qgelu_bwd_kernel        du = df * quickgelu'(u)
//   grad_scale / unscale    the per-prompt power-of-two scale that keeps the fp16 gradient operands inside fp16's normal range
//   prompts_bwd_*           PromptLearner_*.forward backward (main_coop_vae.py:119-128): grad_ctx (two stages, fixed order), grad_bias
// The host sequence is hg_text_bwd.hip; DESIGN.md section 23 has the derivation and the rounding sites.
#include <climits>
#include "hg_kernels.h"

namespace hg {

// ---- attention backward -------------------------------------------------------------------------------------------------------------
// One workgroup of four waves per (prompt, head).  Lp = L rounded up to 16.  LDS (dynamic):
//   Q, K, V, dO   fp16 [Lp][TG_LDH]    rows >= L are zeros (0 x NaN of a neighbour's rows must not reach this prompt)
//   P, dS         fp16 [Lp][Lp + 8]    the MFMA operands; zero above the diagonal and in rows >= L
//   S, dP         fp32 [Lp][Lp + 1]    tiles on and below the diagonal only; the row pass masks everything else
// Every product is 16 x 16 tiles of v_mfma_f32_16x16x16_f16 issued "swapped" (hg_gemm.hip): the first operand holds 16 output
// COLUMNS n, the second 16 output ROWS m, and lane l receives C[m = l % 16][n = 4 (l / 16) + 0 .. 3] - four consecutive columns of a
// row, one 8-byte store.  Operand element e of lane l is k = 4 (l / 16) + e.  Each tile is summed over k in ascending order by one
// wave, the row sums are xor-shuffle trees over fixed lanes: nothing depends on the batch size or on where the workgroup runs.
static constexpr int TG_LDH = 72;      // halfs per Q / K / V / dO row in LDS: 144 B, 16-byte aligned rows, 8-byte aligned k quads

__device__ __forceinline__ half4 ld_quad(const half_t* p) { return *reinterpret_cast<const half4*>(p); }
__device__ __forceinline__ half4 ld_col(const half_t* p, int stride) {      // four elements `stride` halfs apart
    half4 v;
    v[0] = p[0]; v[1] = p[stride]; v[2] = p[2 * stride]; v[3] = p[3 * stride];
    return v;
}

__global__ __launch_bounds__(256) void text_attn_bwd_kernel(const half_t* __restrict__ qkv, const half_t* __restrict__ dout,
                                                            half_t* __restrict__ dqkv, int L, int heads, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int D = heads * 64, Lp = (L + 15) & ~15, nt = Lp >> 4, ldp = Lp + 8, lds = Lp + 1;
    half_t* q_s = reinterpret_cast<half_t*>(smem);
    half_t* k_s = q_s + Lp * TG_LDH;
    half_t* v_s = k_s + Lp * TG_LDH;
    half_t* o_s = v_s + Lp * TG_LDH;
    half_t* p_s = o_s + Lp * TG_LDH;
    half_t* d_s = p_s + Lp * ldp;
    float* s_s = reinterpret_cast<float*>(d_s + Lp * ldp);
    float* dp_s = s_s + Lp * lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seq = blockIdx.x / heads, head = blockIdx.x - seq * heads;
    const size_t row0 = (size_t)seq * L;

    // ---- stage Q, K, V, dO of the head: 16-byte chunks, zeros behind row L - 1
    for (int i = tid; i < Lp * 32; i += 256) {
        const int which = i & 3, c = (i >> 2) & 7, r = i >> 5;
        half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < L) {
            const half_t* src = which < 3 ? qkv + (row0 + r) * (size_t)(3 * D) + which * D + head * 64 + c * 8
                                          : dout + (row0 + r) * (size_t)D + head * 64 + c * 8;
            v = *reinterpret_cast<const half8*>(src);
        }
        *reinterpret_cast<half8*>(q_s + (which * Lp + r) * TG_LDH + c * 8) = v;
    }
    __syncthreads();

    const int lr = lane & 15, kq = (lane >> 4) * 4;
    // ---- S = scale Q K^T and dP = dO V^T on and below the diagonal
    const int ntri = nt * (nt + 1) / 2;
    for (int w = wave; w < 2 * ntri; w += 4) {
        int t = w >> 1, ti = 0;
        while (t > ti) { t -= ti + 1; ++ti; }      // tile t of row ti
        const int tj = t;
        const half_t* a = (w & 1) ? o_s : q_s;     // rows m = i
        const half_t* b = (w & 1) ? v_s : k_s;     // columns n = j
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            acc = __builtin_amdgcn_mfma_f32_16x16x16f16(ld_quad(b + (tj * 16 + lr) * TG_LDH + ks * 16 + kq),
                                                        ld_quad(a + (ti * 16 + lr) * TG_LDH + ks * 16 + kq), acc, 0, 0, 0);
        float* dst = ((w & 1) ? dp_s : s_s) + (ti * 16 + lr) * lds + tj * 16 + kq;
        const float f = (w & 1) ? 1.0f : scale;
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[r] = acc[r] * f;
    }
    __syncthreads();

    // ---- rows: P = softmax(S), delta = sum_j P dP, dS = P (dP - delta) in fp32; P and dS rounded to fp16 for the products below
    for (int i = wave; i < Lp; i += 4) {
        float sv[2], dv[2], e[2];
        float mx = -INFINITY;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            const bool ok = i < L && j <= i;
            sv[h] = ok ? s_s[i * lds + j] : -INFINITY;
            dv[h] = ok ? dp_s[i * lds + j] : 0.f;
            mx = fmaxf(mx, sv[h]);
        }
        mx = wave_max(mx);
#pragma unroll
        for (int h = 0; h < 2; ++h) e[h] = (i < L && lane + 64 * h <= i) ? __builtin_amdgcn_exp2f((sv[h] - mx) * 1.4426950408889634f) : 0.f;
        const float sum = wave_sum(e[0] + e[1]);
        const float inv = i < L ? 1.0f / sum : 0.f;
        const float p0 = e[0] * inv, p1 = e[1] * inv;
        const float delta = wave_sum(p0 * dv[0] + p1 * dv[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            if (j < Lp) {
                const bool ok = i < L && j <= i;
                const float p = h ? p1 : p0;
                p_s[i * ldp + j] = ok ? (half_t)p : (half_t)0.f;
                d_s[i * ldp + j] = ok ? (half_t)(p * (dv[h] - delta)) : (half_t)0.f;
            }
        }
    }
    __syncthreads();

    // ---- dV = P^T dO, dK = scale dS^T Q (sums over the rows i >= j), dQ = scale dS K (sums over the keys j <= i)
    for (int w = wave; w < 3 * nt * 4; w += 4) {
        const int which = w / (nt * 4), rem = w - which * nt * 4, tm = rem >> 2, tn = rem & 3;      // 0 dV, 1 dK, 2 dQ; row tile; d tile
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (which < 2) {
            const half_t* a = which == 0 ? p_s : d_s;      // [i][j]: rows m = j, k = i
            const half_t* b = which == 0 ? o_s : q_s;      // [i][d]: columns n = d, k = i
            for (int kt = tm; kt < nt; ++kt)
                acc = __builtin_amdgcn_mfma_f32_16x16x16f16(ld_col(b + (kt * 16 + kq) * TG_LDH + tn * 16 + lr, TG_LDH),
                                                            ld_col(a + (kt * 16 + kq) * ldp + tm * 16 + lr, ldp), acc, 0, 0, 0);
        } else {
            for (int kt = 0; kt <= tm; ++kt)
                acc = __builtin_amdgcn_mfma_f32_16x16x16f16(ld_col(k_s + (kt * 16 + kq) * TG_LDH + tn * 16 + lr, TG_LDH),
                                                            ld_quad(d_s + (tm * 16 + lr) * ldp + kt * 16 + kq), acc, 0, 0, 0);
        }
        const int row = tm * 16 + lr;
        if (row < L) {
            const float f = which == 0 ? 1.0f : scale;
            half4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (half_t)(acc[r] * f);
            const int col = (which == 0 ? 2 : which == 1 ? 1 : 0) * D + head * 64 + tn * 16 + kq;
            *reinterpret_cast<half4*>(dqkv + (row0 + row) * (size_t)(3 * D) + col) = o;
        }
    }
}

size_t text_attn_bwd_lds(int L) {
    const size_t Lp = (size_t)((L + 15) & ~15);
    return 4 * Lp * TG_LDH * 2 + 2 * Lp * (Lp + 8) * 2 + 2 * Lp * (Lp + 1) * 4;
}

hipError_t launch_text_attn_bwd(const half_t* qkv, const half_t* dout, half_t* dqkv, int n_seq, int L, int heads, hipStream_t s) {
    if (n_seq <= 0) return hipSuccess;
    if (L < 1 || L > TEXT_GRAD_MAX_L || heads < 1 || !qkv || !dout || !dqkv) return hipErrorInvalidValue;
    if ((long long)n_seq * heads > INT32_MAX) return hipErrorInvalidValue;
    static bool attr_set_d[HG_MAX_DEVICES] = {};
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&text_attn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)text_attn_bwd_lds(TEXT_GRAD_MAX_L));
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(text_attn_bwd_kernel, dim3(n_seq * heads), dim3(256), text_attn_bwd_lds(L), s, qkv, dout, dqkv, L, heads, 0.125f);
    return hipGetLastError();
}

// ---- LayerNorm backward (eps 1e-5, biased variance, statistics recomputed from x in fp32 as layernorm_kernel does) -------------------
//   g[row] += rstd * (dyg - mean(dyg) - xhat * mean(dyg * xhat)),  dyg = dy * gamma,  xhat = (x - mean) * rstd
// x, dy dense [M, D]; row = r, or with sel: r * rows_per_seq + sel[r] (ln_final: the EOT row of prompt r)
static constexpr int LNB_MAXC = 4;      // float4 chunks per lane -> D <= 1024

__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ dy, float* __restrict__ g, int M, int D,
                                                            const int32_t* __restrict__ sel, int rows_per_seq) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    size_t grow = (size_t)r;
    if (sel) {
        int gi = sel[r];
        gi = gi < 0 ? 0 : (gi >= rows_per_seq ? rows_per_seq - 1 : gi);
        grow = (size_t)r * rows_per_seq + gi;
    }
    const f32x4* xp = reinterpret_cast<const f32x4*>(x + (size_t)r * D);
    const f32x4* dp = reinterpret_cast<const f32x4*>(dy + (size_t)r * D);
    const f32x4* wp = reinterpret_cast<const f32x4*>(gamma);
    f32x4* gp = reinterpret_cast<f32x4*>(g + grow * D);
    const int nc = D >> 2;
    f32x4 v[LNB_MAXC], w[LNB_MAXC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LNB_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            v[i] = xp[c];
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LNB_MAXC; ++i) {
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
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < LNB_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            const f32x4 d = dp[c], gm = wp[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[i][e] = (v[i][e] - mean) * rstd;
                w[i][e] = d[e] * gm[e];
                s1 += w[i][e];
                s2 += w[i][e] * v[i][e];
            }
        }
    }
    const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
#pragma unroll
    for (int i = 0; i < LNB_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nc) {
            f32x4 o = gp[c];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] += rstd * ((w[i][e] - m1) - v[i][e] * m2);
            gp[c] = o;
        }
    }
}

hipError_t launch_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* g, int M, int D, const int32_t* sel,
                                int rows_per_seq, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (D % 4 || D > 256 * LNB_MAXC || D < 4 || (sel && rows_per_seq < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, gamma, dy, g, M, D, sel, rows_per_seq);
    return hipGetLastError();
}

// ---- QuickGELU backward: du = df * (sig + 1.702 u sig (1 - sig)), sig = sigmoid(1.702 u); fp16 in, fp32 arithmetic, fp16 out (du may be df)
__global__ __launch_bounds__(256) void qgelu_bwd_kernel(const half_t* df, const half_t* __restrict__ u, half_t* du, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const half8 a = reinterpret_cast<const half8*>(df)[i], b = reinterpret_cast<const half8*>(u)[i];
        half8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float uu = (float)b[e];
            const float sig = 1.0f / (1.0f + __builtin_amdgcn_exp2f(uu * -2.4554669595930157f));
            o[e] = (half_t)((float)a[e] * (sig + 1.702f * uu * sig * (1.0f - sig)));
        }
        reinterpret_cast<half8*>(du)[i] = o;
    }
}

hipError_t launch_qgelu_bwd(const half_t* df, const half_t* u, half_t* du, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (n % 8) return hipErrorInvalidValue;
    const size_t n8 = n / 8, blocks = (n8 + 255) / 256;
    hipLaunchKernelGGL(qgelu_bwd_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, df, u, du, n8);
    return hipGetLastError();
}

// ---- the per-prompt scale: s_r = 2^-floor(log2(max_e |go[r][e]|)) (1 for an all-zero row; the exponent clamped to +-126 so that s and
// 1 / s are normal); go16 = fp16(s_r go), sinv[r] = 1 / s_r.  A wave per row.  No saturation: Inf / NaN stay what they are.
__global__ __launch_bounds__(256) void grad_scale_kernel(const float* __restrict__ go, half_t* __restrict__ go16, float* __restrict__ sinv,
                                                         int R, int E) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    float mx = 0.f;
    for (int e = lane; e < E; e += 64) mx = fmaxf(mx, fabsf(go[(size_t)r * E + e]));
    mx = wave_max(mx);
    int ex = 0;
    if (mx > 0.f) {
        ex = mx < INFINITY ? ilogbf(mx) : 126;
        ex = ex < -126 ? -126 : (ex > 126 ? 126 : ex);
    }
    const float sc = ldexpf(1.0f, -ex);
    for (int e = lane; e < E; e += 64) go16[(size_t)r * E + e] = (half_t)(go[(size_t)r * E + e] * sc);
    if (lane == 0) sinv[r] = ldexpf(1.0f, ex);
}

hipError_t launch_grad_scale(const float* go, half_t* go16, float* sinv, int R, int E, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (E < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grad_scale_kernel, dim3((R + 3) / 4), dim3(256), 0, s, go, go16, sinv, R, E);
    return hipGetLastError();
}

// out [R, L, D] = g [R, Leff, D] * sinv[r] for the first Leff positions, zeros behind them
__global__ __launch_bounds__(256) void grad_unscale_kernel(const float* __restrict__ g, const float* __restrict__ sinv,
                                                           float* __restrict__ out, int R, int L, int Leff, int D) {
    const int nc = D >> 2;
    const size_t total = (size_t)R * L * nc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % nc);
        const size_t rl = i / nc;
        const int r = (int)(rl / L), l = (int)(rl - (size_t)r * L);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (l < Leff) {
            v = reinterpret_cast<const f32x4*>(g + ((size_t)r * Leff + l) * D)[c];
            const float f = sinv[r];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= f;
        }
        reinterpret_cast<f32x4*>(out + rl * D)[c] = v;
    }
}

hipError_t launch_grad_unscale(const float* g, const float* sinv, float* out, int R, int L, int Leff, int D, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (D % 4 || Leff < 1 || Leff > L) return hipErrorInvalidValue;
    const size_t total = (size_t)R * L * (D / 4), blocks = (total + 255) / 256;
    hipLaunchKernelGGL(grad_unscale_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, g, sinv, out, R, L, Leff, D);
    return hipGetLastError();
}

// ---- PromptLearner_*.forward backward: g [R, L, D] -> grad_bias[r] = sum_j g[r][1 + j], grad_ctx[j] = sum_r g[r][1 + j] -----------------
// grad_ctx in two stages: partial[p][j] = the rows r of chunk p (PROMPTS_BWD_CHUNK rows) in ascending order, then the chunks in ascending
// order.  No atomics: the same bits on every run.
__global__ __launch_bounds__(256) void prompts_bwd_bias_kernel(const float* __restrict__ g, float* __restrict__ gb, int R, int L, int n_ctx,
                                                               int D) {
    const size_t total = (size_t)R * D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / D;
        const int d = (int)(i - r * D);
        float acc = 0.f;
        for (int j = 0; j < n_ctx; ++j) acc += g[(r * L + 1 + j) * D + d];
        gb[i] = acc;
    }
}
__global__ __launch_bounds__(256) void prompts_bwd_partial_kernel(const float* __restrict__ g, float* __restrict__ partial, int R, int L,
                                                                  int n_ctx, int D) {
    const int jd = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (jd >= n_ctx * D) return;
    const int j = jd / D, d = jd - j * D;
    const int r0 = p * PROMPTS_BWD_CHUNK, r1 = r0 + PROMPTS_BWD_CHUNK < R ? r0 + PROMPTS_BWD_CHUNK : R;
    float acc = 0.f;
    for (int r = r0; r < r1; ++r) acc += g[((size_t)r * L + 1 + j) * D + d];
    partial[(size_t)p * n_ctx * D + jd] = acc;
}
__global__ __launch_bounds__(256) void prompts_bwd_final_kernel(const float* __restrict__ partial, float* __restrict__ gc, int n_part,
                                                                int n) {
    const int jd = blockIdx.x * 256 + threadIdx.x;
    if (jd >= n) return;
    float acc = 0.f;
    for (int p = 0; p < n_part; ++p) acc += partial[(size_t)p * n + jd];
    gc[jd] = acc;
}

hipError_t launch_prompts_bwd(const float* g, int R, int L, int n_ctx, int D, float* partial, float* grad_ctx, float* grad_bias,
                              hipStream_t s) {
    if (R <= 0 || n_ctx < 1 || n_ctx >= L || D < 1) return hipErrorInvalidValue;
    const int n = n_ctx * D, n_part = (R + PROMPTS_BWD_CHUNK - 1) / PROMPTS_BWD_CHUNK;
    if (grad_bias) {
        const size_t blocks = ((size_t)R * D + 255) / 256;
        hipLaunchKernelGGL(prompts_bwd_bias_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, g, grad_bias, R, L,
                           n_ctx, D);
    }
    if (grad_ctx) {
        hipLaunchKernelGGL(prompts_bwd_partial_kernel, dim3((n + 255) / 256, n_part), dim3(256), 0, s, g, partial, R, L, n_ctx, D);
        hipLaunchKernelGGL(prompts_bwd_final_kernel, dim3((n + 255) / 256), dim3(256), 0, s, partial, grad_ctx, n_part, n);
    }
    return hipGetLastError();
}

}  // namespace hg
