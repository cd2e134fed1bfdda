// The stem of a ResNet - conv1 7 x 7 / 2 pad 3 (3 -> 64), the frozen norm, ReLU, max-pool 3 x 3 / 2 pad 1 - as ONE launch (torchvision's
// ResNet under the reference's FrozenBatchNorm2d: detr/models/backbone.py:45-55, :83-93).  DESIGN.md section 21.
//
// resnet_stem_kernel:  out[b][ph][pw][n] = max over the conv pixels (ch, cw), ch in 2 ph - 1 .. 2 ph + 1, cw in 2 pw - 1 .. 2 pw + 1, that
// lie inside [0, Hc) x [0, Wc), of relu(fmaf(acc[b][ch][cw][n], scale[n], bias[n])), Hc = (Hi - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1 (the same
// for W).  A position outside the conv map takes no part (it is NOT a conv pixel made of zero padding).  relu(v) = v < 0 ? 0 : v; the max
// keeps a NaN (m = (v > m || v != v) ? v : m), as torch's max_pool2d does.  The fp32 output is that max, the fp16 output its RNE rounding;
// both NHWC [B, Hp, Wp, 64]: the pair the stages read.  The conv map never reaches global memory.
//   acc     fp32 from zero on v_mfma_f32_16x16x32_f16, weights as the A operand, pixels on the lane index (as hg_resnet_conv.hip).  Every
//           image value and every weight is rounded once to fp16 (RNE).  K = 147 is laid out as k = (c 7 + r) 8 + s over 192 = 6 k-steps,
//           ascending: c the input channel, r the tap row, s the tap column 0 .. 7.  s = 7 and (c 7 + r) = 21 .. 23 are padding: their
//           weights are zero AND their pixel operands are zero (s = 7 would otherwise be the neighbouring pixel's value, whose NaN or Inf
//           times zero would leak out of its window), so each adds an exact +0.  No split over K, no atomics, nothing between workgroups:
//           a conv pixel is a fixed function of its own window, the same bits in every tile whose halo holds it.
//   x       fp32 [B, 3, Hi, Wi] through element strides (image, channel, row), column stride 1, 64-bit offsets, read with 4-byte loads
//           where it lies: any Wi, any row stride, any 4-byte aligned base, nothing read beyond the last element.
//   item    a rectangle of 4 x 8 pooled pixels of one image x all 64 channels, 256 threads.  It needs 9 x 17 conv pixels (153, the halo's
//           recompute factor is 153 / 128 = 1.20) and 23 x 39 input pixels of each channel, staged once in LDS as fp16 (rows of 40);
//           a pad position forms no address and is a real zero.  A lane's operand of one k-step is 8 consecutive halfs of one patch row
//           (4-byte aligned: four LDS dword reads), its eighth zeroed.  The conv tile goes to LDS as relu(fmaf) fp32 [153][68], then every
//           thread pools 4 channels of 2 pooled pixels: 16-byte fp32 and 8-byte fp16 NHWC stores.
//   waves   2 (channels: 32 each, two fragments, their 12 weight fragments in registers) x 2 (conv pixels: 80 each, five fragments; the
//           rows 153 .. 159 repeat pixel 152 and are never stored).
//   w       fp16 in fragment order (resnet_stem_pack_kernel): [4][6][64 lanes][8], 24 KiB, read from global memory (L2-resident).
#include "hg_kernels.h"

namespace hg {

static constexpr int ST_TPH = RESNET_STEM_TILE_H, ST_TPW = RESNET_STEM_TILE_W;      // pooled pixels of a work item
static constexpr int ST_CH = 2 * ST_TPH + 1, ST_CW = 2 * ST_TPW + 1;                // conv pixels: 9 x 17
static constexpr int ST_PH = 4 * ST_TPH + 7, ST_PW = 4 * ST_TPW + 7;                // input pixels: 23 x 39
static constexpr int ST_PLD = ST_PW + 1;                                            // halfs per LDS patch row (40)
static constexpr int ST_M = ST_CH * ST_CW;                                          // 153 conv pixels
static constexpr int ST_MF = (ST_M + 15) / 16;                                      // 10 fragments
static constexpr int ST_CLD = 68;                                                   // floats per LDS conv row
static constexpr int ST_KS = 6;                                                     // k-steps of 32
static_assert(ST_MF % 2 == 0, "two pixel waves share the fragments evenly");
static_assert((ST_TPH * ST_TPW) % 16 == 0, "the pool phase gives every thread whole pixels");

__global__ __launch_bounds__(256) void resnet_stem_kernel(const ResnetStemArgs a) {
    constexpr int NJ = ST_MF / 2;
    __shared__ __attribute__((aligned(16))) half_t xs[3 * ST_PH * ST_PLD];
    __shared__ __attribute__((aligned(16))) float cs[ST_M * ST_CLD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int r16 = lane & 15, cg = lane >> 4;
    const int ntw = (a.Wp + ST_TPW - 1) / ST_TPW, nth = (a.Hp + ST_TPH - 1) / ST_TPH;
    const unsigned per = (unsigned)(ntw * nth);
    const int b = (int)(blockIdx.x / per), t = (int)(blockIdx.x % per);
    const int ph0 = (t / ntw) * ST_TPH, pw0 = (t % ntw) * ST_TPW;
    const int ch0 = 2 * ph0 - 1, cw0 = 2 * pw0 - 1;          // first conv pixel of the tile
    const int ih0 = 2 * ch0 - 3, iw0 = 2 * cw0 - 3;          // first input pixel of the patch

    // ---- the patch: fp32 -> fp16 (RNE), zeros outside the image
    const float* xb = a.x + (long long)b * a.sb;
    for (int i = tid; i < 3 * ST_PH * ST_PLD; i += 256) {
        const int c = i / (ST_PH * ST_PLD), rem = i - c * (ST_PH * ST_PLD);
        const int y = rem / ST_PLD, x = rem - y * ST_PLD;
        const int hi = ih0 + y, wi = iw0 + x;
        float v = 0.f;
        if ((unsigned)hi < (unsigned)a.Hi && (unsigned)wi < (unsigned)a.Wi && x < ST_PW) v = xb[(long long)c * a.sc + (long long)hi * a.sr + wi];
        xs[i] = (half_t)v;
    }

    // ---- this wave's weight fragments: channel fragments 2 wn, 2 wn + 1, all six k-steps
    half8 wf[2][ST_KS];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int kk = 0; kk < ST_KS; ++kk) wf[i][kk] = *reinterpret_cast<const half8*>(a.w + ((size_t)((wn * 2 + i) * ST_KS + kk) * 64 + lane) * 8);

    // pixel offsets of this lane's five fragments (halfs into a channel's patch): conv pixel (cy, cx) reads rows 2 cy .., columns 2 cx ..
    int poff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        int p = wm * (NJ * 16) + j * 16 + r16;
        p = p < ST_M ? p : ST_M - 1;
        const int cy = p / ST_CW, cx = p - cy * ST_CW;
        poff[j] = 2 * cy * ST_PLD + 2 * cx;
    }
    f32x4 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

#pragma unroll
    for (int kk = 0; kk < ST_KS; ++kk) {
        const int q = 4 * kk + cg;                 // (channel, tap row) of this lane's eight k: q = c 7 + r; 21 .. 23 are padding
        const bool live = q < 21;
        const int c = q / 7, r = q - c * 7;
        const int qoff = live ? (c * ST_PH + r) * ST_PLD : 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const unsigned* src = reinterpret_cast<const unsigned*>(xs + qoff + poff[j]);      // even offsets: 4-byte aligned
            union {
                unsigned u[4];
                half8 h;
            } v;
            v.u[0] = src[0]; v.u[1] = src[1]; v.u[2] = src[2];
            v.u[3] = src[3] & 0xffffu;             // s = 7 is the neighbouring pixel: zero
            if (!live) v.u[0] = v.u[1] = v.u[2] = v.u[3] = 0u;
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i][kk], v.h, acc[i][j], 0, 0, 0);
        }
    }

    // ---- acc[i][j][e] = channel wn 32 + 16 i + 4 cg + e of conv pixel wm 80 + 16 j + r16: relu(fmaf) -> cs
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int p = wm * (NJ * 16) + j * 16 + r16;
        if (p >= ST_M) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ch = wn * 32 + i * 16 + 4 * cg;
            f32x4 v = fma4(acc[i][j], *reinterpret_cast<const f32x4*>(a.scale + ch), *reinterpret_cast<const f32x4*>(a.bias + ch));
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
            *reinterpret_cast<f32x4*>(cs + p * ST_CLD + ch) = v;
        }
    }
    __syncthreads();

    // ---- the pool: thread -> channels 4 (tid & 15) .. + 3 of pooled pixels (tid >> 4) + 16 k
    const int ch = (tid & 15) * 4;
#pragma unroll
    for (int k = 0; k < ST_TPH * ST_TPW / 16; ++k) {
        const int pp = (tid >> 4) + 16 * k;
        const int py = pp / ST_TPW, px = pp - py * ST_TPW;
        const int ph = ph0 + py, pw = pw0 + px;
        if (ph >= a.Hp || pw >= a.Wp) continue;
        const float ninf = -__builtin_inff();
        f32x4 m = {ninf, ninf, ninf, ninf};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ty = 2 * py + dy, tx = 2 * px + dx;      // tile coordinates of conv pixel (2 ph - 1 + dy, 2 pw - 1 + dx)
                if ((unsigned)(ch0 + ty) >= (unsigned)a.Hc || (unsigned)(cw0 + tx) >= (unsigned)a.Wc) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(cs + (ty * ST_CW + tx) * ST_CLD + ch);
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] = (v[e] > m[e] || v[e] != v[e]) ? v[e] : m[e];
            }
        }
        const long long o = (((long long)b * a.Hp + ph) * a.Wp + pw) * 64 + ch;
        *reinterpret_cast<f32x4*>(a.out32 + o) = m;
        half4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (half_t)m[e];
        *reinterpret_cast<half4*>(a.out16 + o) = h;
    }
}

// w fp32 [64, 3, 7, 7] (torch's order) -> fp16 fragments [4][6][64][8]: element (nf, kk, lane, j) is channel 16 nf + (lane & 15) at
// k = 32 kk + 8 (lane >> 4) + j = (c 7 + r) 8 + s; zero for s = 7 and c 7 + r >= 21.  A thread an element.  flag[0] becomes 1 where a
// weight is not finite or rounds beyond fp16's range.
__global__ __launch_bounds__(256) void resnet_stem_pack_kernel(const float* __restrict__ w, half_t* __restrict__ out, int* flag) {
    const int idx = (int)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 4 * ST_KS * 512) return;
    const int j = idx & 7, lane = (idx >> 3) & 63, f = idx >> 9;
    const int kk = f % ST_KS, nf = f / ST_KS;
    const int ch = nf * 16 + (lane & 15), q = 4 * kk + (lane >> 4);
    half_t h = (half_t)0.f;
    if (q < 21 && j < 7) {
        const int c = q / 7, r = q - c * 7;
        h = (half_t)w[((ch * 3 + c) * 7 + r) * 7 + j];
        if (!(fabsf((float)h) <= 65504.f)) *flag = 1;
    }
    out[idx] = h;
}

bool resnet_stem_ok(const ResnetStemArgs& a) {
    if (!a.x || !a.w || !a.scale || !a.bias || !a.out32 || !a.out16) return false;
    if (a.B < 1 || a.B > RESNET_MAX_B || a.Hi < 1 || a.Wi < 1) return false;
    if (a.Hc != resnet_stem_conv_size(a.Hi) || a.Wc != resnet_stem_conv_size(a.Wi)) return false;
    if (a.Hp != resnet_stem_pool_size(a.Hc) || a.Wp != resnet_stem_pool_size(a.Wc)) return false;
    if (a.Hp > RESNET_MAX_SIDE || a.Wp > RESNET_MAX_SIDE) return false;
    return ((uintptr_t)a.x & 3) == 0 && ((uintptr_t)a.out32 & 15) == 0 && ((uintptr_t)a.out16 & 7) == 0 && ((uintptr_t)a.w & 15) == 0;
}

hipError_t launch_resnet_stem(const ResnetStemArgs& a, hipStream_t s) {
    if (!resnet_stem_ok(a)) return hipErrorInvalidValue;
    const long long blocks = (long long)a.B * ((a.Hp + ST_TPH - 1) / ST_TPH) * ((a.Wp + ST_TPW - 1) / ST_TPW);
    if (blocks > (1LL << 23)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resnet_stem_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_resnet_stem_pack(const float* w, half_t* out, int* flag, hipStream_t s) {
    if (!w || !out || !flag) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resnet_stem_pack_kernel, dim3(4 * ST_KS * 512 / 256), dim3(256), 0, s, w, out, flag);
    return hipGetLastError();
}

}  // namespace hg
