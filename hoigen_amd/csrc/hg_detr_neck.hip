// DETR's neck between the ResNet body and the transformer encoder in one call (upt_tip_cache_model_free_finetune_distill3.py:1594-1597:
// the padding mask on the feature grid, detr/models/backbone.py:78; PositionEmbeddingSine.forward, detr/models/position_encoding.py:28-48;
// input_proj, the 1 x 1 Conv2d of detr/models/detr.py:40, :65; and the flatten(2).permute of detr/models/transformer.py:50-51).  The
// outputs are the three buffers hg_detr_encoder and hg_detr_decoder take: batch-first src and pos, and the uint8 key-padding mask.
//
// detr_neck_kernel: a work item is (a tile of 32 tokens of ONE image, a slice of Cin), 256 threads, v_mfma_f32_16x16x32_f16 with W as the A
// operand (fragments straight from global memory: lane l holds row l & 15, k = 8 (l >> 4) .. + 7) and tokens on the lane index.
//   x       fp32 [B, Cin, S] through element strides (image, channel), token stride 1, read where it lies: a 64-channel x 32-token block
//           goes global -> registers -> fp16 (round to nearest even) -> LDS as xs[token][k], two blocks in flight ahead of the MFMAs (four, and W's fragments a block ahead, measured no faster).
//           vec4 (base and both strides on 16 bytes, S a multiple of 4): a thread loads four tokens of two channels as two 16-byte
//           loads; otherwise one token of eight channel pairs as 4-byte loads.  The values are the same, so are the bits that leave.
//           Tokens at or beyond S are read from the image's last token(s) and never stored.
//   src     acc from zero over k in ascending blocks of 32.  One slice: src[b, s, :] = acc + bias.  n slices: slice z writes
//           partial[z][b S + s][:] = acc, and detr_neck_sum_kernel writes src = (((p0 + p1) + p2) + ..) + bias, ascending.
//   slice 0 also writes the tile's mask and pos rows:
//   mask    the image's whole grid, m[y][x] = image_mask[b][min((int)floorf(y * ((float)Hi / (float)H)), Hi - 1)][likewise x] != 0
//           (legacy `nearest`), in LDS - at most DETR_ATTN_MAX_L bytes.
//   pos     counts of unpadded cells: down the token's column up to its row (cy) and over the whole column (ly), along its row up to
//           its column (cx) and over the whole row (lx) - integers, so the order of the sum does not matter and the masks may be
//           arbitrary.  normalize: e = count / (last + 1e-6f) * scale; a = e / dim_t[i]; sinf(a) for even i, cosf(a) for odd i, each
//           operation rounded once in fp32 (the __f*_rn forms, and build.sh compiles this file without contraction).  The y half goes to
//           channels [0, D / 2), the x half to [D / 2, D).
//
// No counters, no atomics, nothing waits inside a launch: a row's outputs depend on its own image's x column and mask and on the weights.
// Measured on an MI355X: profiles/detr_neck.txt, DESIGN.md section 19.
#include "hg_kernels.h"

namespace hg {

static constexpr int NECK_KB = 64;                // channels per staged block
static constexpr int NECK_LDK = NECK_KB + 8;      // halfs per LDS row of a block: 144 B, 16-byte aligned, rows 4 banks apart

struct NeckRegs {
    float v[8];
};

// the 64-channel x 32-token block at channel k0 of image row `xb` into registers
__device__ __forceinline__ void neck_load(NeckRegs& r, const float* __restrict__ xb, long long sc, int k0, int s0, int S, int vec4, int tid) {
    if (vec4) {
        int t0 = s0 + 4 * (tid & 7);
        t0 = t0 + 4 <= S ? t0 : S - 4;
        const float* p = xb + (long long)(k0 + 2 * (tid >> 3)) * sc + t0;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + sc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r.v[e] = lo[e];
            r.v[4 + e] = hi[e];
        }
    } else {
        int t = s0 + (tid & 31);
        t = t < S ? t : S - 1;
        const float* p = xb + (long long)(k0 + 2 * (tid >> 5)) * sc + t;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            r.v[2 * q] = p[(long long)(16 * q) * sc];
            r.v[2 * q + 1] = p[(long long)(16 * q + 1) * sc];
        }
    }
}

__device__ __forceinline__ void neck_store(const NeckRegs& r, half_t* xs, int vec4, int tid) {
    if (vec4) {
        half_t* d = xs + (4 * (tid & 7)) * NECK_LDK + 2 * (tid >> 3);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            half2v h;
            h[0] = (half_t)r.v[e];
            h[1] = (half_t)r.v[4 + e];
            *reinterpret_cast<half2v*>(d + e * NECK_LDK) = h;
        }
    } else {
        half_t* d = xs + (tid & 31) * NECK_LDK + 2 * (tid >> 5);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            half2v h;
            h[0] = (half_t)r.v[2 * q];
            h[1] = (half_t)r.v[2 * q + 1];
            *reinterpret_cast<half2v*>(d + 16 * q) = h;
        }
    }
}

template <int D>
__global__ __launch_bounds__(256) void detr_neck_kernel(const DetrNeckArgs a) {
    constexpr int NF = D / 64;      // 16-channel fragments of W a wave owns
    __shared__ __attribute__((aligned(16))) half_t xs[2][DETR_NECK_TOKENS * NECK_LDK];
    __shared__ unsigned char grid[DETR_ATTN_MAX_L];
    __shared__ float emb[DETR_NECK_TOKENS][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, cg = lane >> 4, kq = cg * 8;
    const int S = a.H * a.W, b = blockIdx.y, s0 = (int)blockIdx.x * DETR_NECK_TOKENS, z = blockIdx.z;
    const int nrows = S - s0 < DETR_NECK_TOKENS ? S - s0 : DETR_NECK_TOKENS;

    // ---- mask and pos of the tile's tokens
    if (z == 0 && (a.mask || a.pos)) {
        const float fy = __fdiv_rn((float)a.Hi, (float)a.H), fx = __fdiv_rn((float)a.Wi, (float)a.W);
        const unsigned char* im = a.image_mask + (size_t)b * a.Hi * a.Wi;
        for (int s = tid; s < S; s += 256) {
            const int y = s / a.W, x = s - y * a.W;
            int iy = (int)floorf(__fmul_rn((float)y, fy)), ix = (int)floorf(__fmul_rn((float)x, fx));
            iy = iy < a.Hi - 1 ? iy : a.Hi - 1;
            ix = ix < a.Wi - 1 ? ix : a.Wi - 1;
            grid[s] = im[(size_t)iy * a.Wi + ix] != 0;
        }
        __syncthreads();
        if (a.mask && tid < nrows) a.mask[(size_t)b * S + s0 + tid] = grid[s0 + tid];
        if (a.pos) {
            // eight threads a token: thread u takes rows / columns u, u + 8, ..
            const int r = tid >> 3, u = tid & 7;
            int s = s0 + r;
            s = s < S ? s : S - 1;
            const int y = s / a.W, x = s - y * a.W;
            int cy = 0, ly = 0, cx = 0, lx = 0;
            for (int i = u; i < a.H; i += 8) {
                const int v = !grid[i * a.W + x];
                ly += v;
                cy += i <= y ? v : 0;
            }
            for (int j = u; j < a.W; j += 8) {
                const int v = !grid[y * a.W + j];
                lx += v;
                cx += j <= x ? v : 0;
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                cy += __shfl_xor(cy, o);
                ly += __shfl_xor(ly, o);
                cx += __shfl_xor(cx, o);
                lx += __shfl_xor(lx, o);
            }
            if (u == 0) {
                float ey = (float)cy, ex = (float)cx;
                if (a.normalize) {
                    ey = __fmul_rn(__fdiv_rn(ey, __fadd_rn((float)ly, 1e-6f)), a.scale);
                    ex = __fmul_rn(__fdiv_rn(ex, __fadd_rn((float)lx, 1e-6f)), a.scale);
                }
                emb[r][0] = ey;
                emb[r][1] = ex;
            }
            __syncthreads();
            constexpr int HALF = D / 2;
            for (int i = tid; i < nrows * D; i += 256) {
                const int r2 = i / D, ch = i - r2 * D;
                const int hx = ch >= HALF, f = ch - hx * HALF;
                const float arg = __fdiv_rn(emb[r2][hx], a.dim_t[f]);
                a.pos[(long long)b * a.pos_sb + (long long)(s0 + r2) * a.pos_ss + ch] = (f & 1) ? cosf(arg) : sinf(arg);
            }
        }
    }

    // ---- the projection: this slice's channels in blocks of 64
    const float* xb = a.x + (long long)b * a.x_sb;
    const int kbeg = z * a.kslice, nkb = a.kslice / NECK_KB;
    const int c0 = wave * (D / 4);
    const half_t* wp = a.w + (size_t)(c0 + r16) * a.Cin + kbeg + kq;
    f32x4 acc[NF][2];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    NeckRegs ra, rb;      // two blocks of x in flight
    neck_load(ra, xb, a.x_sc, kbeg, s0, S, a.vec4, tid);
    if (nkb > 1) neck_load(rb, xb, a.x_sc, kbeg + NECK_KB, s0, S, a.vec4, tid);

    auto compute = [&](const half_t* xt, int kb) {
#pragma unroll
        for (int ks = 0; ks < NECK_KB / 32; ++ks) {
            half8 xf[2], wf[NF];
#pragma unroll
            for (int j = 0; j < 2; ++j) xf[j] = *reinterpret_cast<const half8*>(xt + (j * 16 + r16) * NECK_LDK + ks * 32 + kq);
#pragma unroll
            for (int i = 0; i < NF; ++i) wf[i] = *reinterpret_cast<const half8*>(wp + (size_t)(i * 16) * a.Cin + kb * NECK_KB + ks * 32);
#pragma unroll
            for (int i = 0; i < NF; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], xf[j], acc[i][j], 0, 0, 0);
        }
    };

    // the barrier behind a store is also what lets the next step overwrite the other buffer: every wave has left the step before
    for (int kb = 0; kb < nkb; kb += 2) {
        neck_store(ra, xs[0], a.vec4, tid);
        __syncthreads();
        if (kb + 2 < nkb) neck_load(ra, xb, a.x_sc, kbeg + (kb + 2) * NECK_KB, s0, S, a.vec4, tid);
        compute(xs[0], kb);
        if (kb + 1 < nkb) {
            neck_store(rb, xs[1], a.vec4, tid);
            __syncthreads();
            if (kb + 3 < nkb) neck_load(rb, xb, a.x_sc, kbeg + (kb + 3) * NECK_KB, s0, S, a.vec4, tid);
            compute(xs[1], kb + 1);
        }
    }

    // ---- acc[i][j][r] = channel c0 + 16 i + 4 cg + r of token j * 16 + r16 of the tile
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int s = s0 + j * 16 + r16;
        if (s >= S) continue;
        if (a.nsplit > 1) {
            float* o = a.partial + ((size_t)z * a.B * S + (size_t)b * S + s) * D + c0 + 4 * cg;
#pragma unroll
            for (int i = 0; i < NF; ++i) *reinterpret_cast<f32x4*>(o + i * 16) = acc[i][j];
        } else {
            float* o = a.src + (long long)b * a.src_sb + (long long)s * a.src_ss + c0 + 4 * cg;
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const f32x4 v = acc[i][j] + *reinterpret_cast<const f32x4*>(a.bias + c0 + i * 16 + 4 * cg);
                if (a.ovec4) *reinterpret_cast<f32x4*>(o + i * 16) = v;
                else
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[i * 16 + r] = v[r];
            }
        }
    }
}

// src[b, s, c] = (((p0 + p1) + p2) + ..) + bias[c]: a thread per element, the slices in ascending order
__global__ __launch_bounds__(256) void detr_neck_sum_kernel(const DetrNeckArgs a) {
    const int S = a.H * a.W, D = a.D;
    const size_t n = (size_t)a.B * S * D, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % D);
    const size_t row = i / D;
    const int b = (int)(row / S), s = (int)(row - (size_t)b * S);
    float v = a.partial[i];
    for (int zz = 1; zz < a.nsplit; ++zz) v = __fadd_rn(v, a.partial[(size_t)zz * n + i]);
    a.src[(long long)b * a.src_sb + (long long)s * a.src_ss + c] = __fadd_rn(v, a.bias[c]);
}

bool detr_neck_ok(int Cin, int D, int B, int H, int W, int Hi, int Wi) {
    return Cin >= 64 && Cin % 64 == 0 && Cin <= DETR_NECK_MAX_CIN && (D == 128 || D == 256) && B >= 1 && B <= DETR_NECK_MAX_B && H >= 1 && W >= 1 &&
           (long long)H * W <= DETR_ATTN_MAX_L && Hi >= 1 && Wi >= 1 && Hi <= DETR_NECK_MAX_IMG && Wi <= DETR_NECK_MAX_IMG;
}

hipError_t launch_detr_neck(const DetrNeckArgs& a, hipStream_t s) {
    if (!a.x || !a.w || !a.bias || !a.src || !detr_neck_ok(a.Cin, a.D, a.B, a.H, a.W, a.Hi, a.Wi) || a.nsplit < 1 ||
        a.kslice * a.nsplit != a.Cin || a.kslice % NECK_KB || (a.nsplit > 1 && !a.partial) || ((a.pos || a.mask) && !a.image_mask) ||
        (a.pos && !a.dim_t))
        return hipErrorInvalidValue;
    const int S = a.H * a.W;
    const dim3 grid((unsigned)((S + DETR_NECK_TOKENS - 1) / DETR_NECK_TOKENS), (unsigned)a.B, (unsigned)a.nsplit);
    if (a.D == 128) hipLaunchKernelGGL(detr_neck_kernel<128>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(detr_neck_kernel<256>, grid, dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.nsplit == 1) return e;
    const size_t n = (size_t)a.B * S * a.D;
    hipLaunchKernelGGL(detr_neck_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace hg
