// The bottleneck convolutions of a ResNet's layer1 .. layer4 as ONE implicit-GEMM kernel (torchvision's Bottleneck under the reference's
// FrozenBatchNorm2d: detr/models/backbone.py:45-55, :83-93), and the two layout kernels around the stages.  DESIGN.md section 20.
//
// resnet_conv_kernel<TM, EPI>: out[m][n] = epilogue(sum over taps (r, s) ascending, then input channels ascending, of x[pixel(m, r, s)][c] *
// w[n][r][s][c]), M = B Ho Wo output pixels, N = Cout, K = R R Cin, R in {1, 3}, stride in {1, 2}, pad = (R - 1) / 2.  fp16 operands,
// fp32 accumulation from zero on v_mfma_f32_16x16x32_f16 with the WEIGHTS as the A operand and the pixels on the lane index (as
// hg_detr_neck.hip), so a lane ends with four consecutive channels of one pixel: 16-byte fp32 and 8-byte fp16 NHWC stores.
//   x       fp16 NHWC [B, H, W, Cin].  A work item is a tile of TM output pixels (they may belong to different images: every row carries
//           its own address) x 64 output channels, 256 threads.  A K step is one tap and one block of 64 channels: row m's operand is
//           the 128 contiguous bytes of pixel (b, ho stride + r - pad, wo stride + s - pad), or zeros - a pad position and a row at or
//           beyond M form no address and load nothing; the zeros are written to LDS.  Global -> registers (16 bytes a thread and row) ->
//           LDS as xs[row][k] (rows of 72 halfs), the next step's rows in flight in registers ahead of the MFMAs, two LDS buffers,
//           one barrier a step.  Offsets into x are 64-bit.
//   w       fp16 in MFMA fragment order (resnet_pack_kernel): [Cout / 16][K / 32][64 lanes][8], k = (r R + s) Cin + c; a wave reads a
//           fragment as one contiguous KiB straight from global memory (L2-resident), a step ahead of its use.
//   waves   2 (channels: 32 each, two fragments) x 2 (pixels: TM / 2 each, TM / 32 fragments).
//   EPI 1   relu(fmaf(acc, scale[n], bias[n]))                  -> fp16 NHWC
//   EPI 2   fmaf(acc, scale[n], bias[n])                        -> fp32 NHWC                (downsample)
//   EPI 3   relu(fmaf(acc, scale[n], bias[n]) + identity[m][n]) -> fp32 NHWC and fp16 NHWC  (identity fp32 NHWC)
//           relu(v) = v < 0 ? 0 : v, which keeps a NaN as torch's does.
// No split over K, no atomics, no counters or waits between workgroups: an output element is a fixed function of its own window.
//
// resnet_entry_kernel: fp32 [B, C, H, W] through element strides (image, channel, row), column stride 1 -> the fp32 + fp16 NHWC pair.
// resnet_exit_kernel:  fp32 NHWC -> fp32 [B, C, H W] through element strides (image, channel), token stride 1 (what hg_detr_neck reads).
// Both move a 64-pixel x 64-channel tile through LDS so that reads and writes run along the contiguous axis of their side.
#include "hg_kernels.h"

namespace hg {

static constexpr int RC_KB = 64;               // channels per K step
static constexpr int RC_LDK = RC_KB + 8;       // halfs per LDS row: 144 B, 16-byte aligned, rows 4 banks apart
static constexpr int RC_TN = 64;               // output channels of a tile

template <int TM, int EPI>
__global__ __launch_bounds__(256) void resnet_conv_kernel(const ResnetConvArgs a) {
    constexpr int NJ = TM / 32;      // 16-pixel fragments a wave owns = rows a thread stages per step
    __shared__ __attribute__((aligned(16))) half_t xs[2][TM * RC_LDK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int r16 = lane & 15, cg = lane >> 4, kq = cg * 8;
    const int NT = a.Cout / RC_TN;
    const int nt = (int)(blockIdx.x % (unsigned)NT);
    const long long m0 = (long long)(blockIdx.x / (unsigned)NT) * TM;
    const long long M = (long long)a.B * a.Ho * a.Wo;
    const int pad = (a.R - 1) / 2, ncb = a.Cin / RC_KB, nsteps = a.R * a.R * ncb;

    // the rows this thread stages: row (tid >> 3) + 32 i of the tile, bytes 16 (tid & 7) .. + 15 of its 128
    const int chunk = (tid & 7) * 8;
    long long rpix[NJ];      // first pixel of the row's image
    int rh[NJ], rw[NJ];      // input coordinates of tap (0, 0); a row at or beyond M: far outside, so no tap is ever valid
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const long long m = m0 + (tid >> 3) + 32 * i;
        if (m < M) {
            const int hw = a.Ho * a.Wo;
            const int b = (int)(m / hw), rem = (int)(m - (long long)b * hw);
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            rpix[i] = (long long)b * a.H * a.W;
            rh[i] = ho * a.stride - pad;
            rw[i] = wo * a.stride - pad;
        } else {
            rpix[i] = 0;
            rh[i] = -(1 << 20);
            rw[i] = 0;
        }
    }
    half8 ra[NJ];
    auto load = [&](int tr, int ts, int cb) {
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
            const int hi = rh[i] + tr, wi = rw[i] + ts;
            half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if ((unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W)
                v = *reinterpret_cast<const half8*>(a.x + ((rpix[i] + (long long)hi * a.W + wi) * a.Cin + cb * RC_KB + chunk));
            ra[i] = v;
        }
    };
    auto store = [&](half_t* xt) {
#pragma unroll
        for (int i = 0; i < NJ; ++i) *reinterpret_cast<half8*>(xt + ((tid >> 3) + 32 * i) * RC_LDK + chunk) = ra[i];
    };

    // fragment (nf, kk) of w: 512 halfs at ((nf K / 32) + kk) 512; this wave's two channel fragments
    const int K32 = a.R * a.R * a.Cin / 32;
    const half_t* wp = a.w + ((size_t)(nt * 4 + wn * 2) * K32 * 64 + lane) * 8;
    f32x4 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int tr = 0, ts = 0, cb = 0;      // the step in flight: tap (tr, ts), channel block cb
    load(tr, ts, cb);
    for (int t = 0; t < nsteps; ++t) {
        half8 wf[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) wf[i][ks] = *reinterpret_cast<const half8*>(wp + ((size_t)i * K32 + 2 * t + ks) * 512);
        half_t* xt = xs[t & 1];
        store(xt);
        // the barrier behind a store is also what lets the next step overwrite the other buffer: every wave has left the step before
        __syncthreads();
        if (t + 1 < nsteps) {
            if (++cb == ncb) {
                cb = 0;
                if (++ts == a.R) {
                    ts = 0;
                    ++tr;
                }
            }
            load(tr, ts, cb);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            half8 xf[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) xf[j] = *reinterpret_cast<const half8*>(xt + (wm * (TM / 2) + j * 16 + r16) * RC_LDK + ks * 32 + kq);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i][ks], xf[j], acc[i][j], 0, 0, 0);
        }
    }

    // ---- acc[i][j][r] = channel nt 64 + wn 32 + 16 i + 4 cg + r of pixel m0 + wm TM / 2 + 16 j + r16
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const long long m = m0 + wm * (TM / 2) + j * 16 + r16;
        if (m >= M) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ch = nt * RC_TN + wn * 32 + i * 16 + 4 * cg;
            const long long o = m * a.Cout + ch;
            f32x4 v = fma4(acc[i][j], *reinterpret_cast<const f32x4*>(a.scale + ch), *reinterpret_cast<const f32x4*>(a.bias + ch));
            if (EPI == 3) v = v + *reinterpret_cast<const f32x4*>(a.identity + o);
            if (EPI != 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] < 0.f ? 0.f : v[r];
            }
            if (EPI != 1) *reinterpret_cast<f32x4*>(a.out32 + o) = v;
            if (EPI != 2) {
                half4 h;
#pragma unroll
                for (int r = 0; r < 4; ++r) h[r] = (half_t)v[r];
                *reinterpret_cast<half4*>(a.out16 + o) = h;
            }
        }
    }
}

// w fp32 [Cout, Cin, R, R] (torch's order) -> fp16 fragments [Cout / 16][K / 32][64][8], k = (r R + s) Cin + c.  A thread an element.
// flag[0] becomes 1 where a weight is not finite or rounds beyond fp16's range.
__global__ __launch_bounds__(256) void resnet_pack_kernel(const float* __restrict__ w, half_t* __restrict__ out, int Cout, int Cin, int R, int* flag) {
    const int K = R * R * Cin;
    const size_t n = (size_t)Cout * K, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    const size_t f = idx >> 9;
    const int K32 = K / 32, kk = (int)(f % K32), nf = (int)(f / K32);
    const int ch = nf * 16 + (lane & 15), k = kk * 32 + 8 * (lane >> 4) + j;
    const int tap = k / Cin, c = k - tap * Cin, r = tap / R, s = tap - r * R;
    const float v = w[(((size_t)ch * Cin + c) * R + r) * R + s];
    const half_t h = (half_t)v;
    if (!(fabsf((float)h) <= 65504.f)) *flag = 1;
    out[idx] = h;
}

__global__ __launch_bounds__(256) void resnet_entry_kernel(const float* __restrict__ x, long long sb, long long sc, long long sr, int C, int H, int W,
                                                            float* __restrict__ o32, half_t* __restrict__ o16) {
    __shared__ float t[64][65];
    const int S = H * W, p0 = (int)blockIdx.x * 64, c0 = (int)blockIdx.y * 64, b = blockIdx.z;
    const int tid = threadIdx.x, lo = tid & 63, hi = tid >> 6;
    const int p = p0 + lo;
    if (p < S) {
        const int h = p / W, w = p - h * W;
        const float* src = x + (long long)b * sb + (long long)h * sr + w;
#pragma unroll 4
        for (int k = 0; k < 16; ++k) t[hi + 4 * k][lo] = src[(long long)(c0 + hi + 4 * k) * sc];
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int q = p0 + hi + 4 * k;
        if (q >= S) break;
        const float v = t[lo][hi + 4 * k];
        const long long o = ((long long)b * S + q) * C + c0 + lo;
        o32[o] = v;
        o16[o] = (half_t)v;
    }
}

__global__ __launch_bounds__(256) void resnet_exit_kernel(const float* __restrict__ x, int C, int S, float* __restrict__ out, long long sb, long long sc) {
    __shared__ float t[64][65];
    const int p0 = (int)blockIdx.x * 64, c0 = (int)blockIdx.y * 64, b = blockIdx.z;
    const int tid = threadIdx.x, lo = tid & 63, hi = tid >> 6;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int q = p0 + hi + 4 * k;
        if (q >= S) break;
        t[hi + 4 * k][lo] = x[((long long)b * S + q) * C + c0 + lo];
    }
    __syncthreads();
    const int p = p0 + lo;
    if (p < S) {
        float* dst = out + (long long)b * sb + p;
#pragma unroll 4
        for (int k = 0; k < 16; ++k) dst[(long long)(c0 + hi + 4 * k) * sc] = t[lo][hi + 4 * k];
    }
}

bool resnet_conv_ok(const ResnetConvArgs& a) {
    if (!a.x || !a.w || !a.scale || !a.bias) return false;
    if (a.B < 1 || a.H < 1 || a.W < 1 || a.H > RESNET_MAX_SIDE || a.W > RESNET_MAX_SIDE) return false;
    if (a.Cin < 64 || a.Cin % 64 || a.Cin > RESNET_MAX_C || a.Cout < 64 || a.Cout % 64 || a.Cout > RESNET_MAX_C) return false;
    if ((a.R != 1 && a.R != 3) || (a.R == 3 && a.Cin > RESNET_MAX_C3) || (a.stride != 1 && a.stride != 2)) return false;
    if (a.Ho != resnet_out_size(a.H, a.R, a.stride) || a.Wo != resnet_out_size(a.W, a.R, a.stride)) return false;
    if ((long long)a.B * a.Ho * a.Wo >= (1LL << 31)) return false;
    if (a.epi < 1 || a.epi > 3 || (a.epi != 1 && !a.out32) || (a.epi != 2 && !a.out16) || (a.epi == 3 && !a.identity)) return false;
    return a.tile == 0 || a.tile == 32 || a.tile == 128;
}

// 128-pixel tiles where they fill the compute units at least once, 32-pixel tiles below (layer3 and layer4 of one image: M = 4 200 and
// 1 050 pixels are 33 and 9 tiles of 128)
int resnet_conv_tile(long long M, int Cout) { return ((M + 127) / 128) * (Cout / RC_TN) >= 256 ? 128 : 32; }

template <int TM>
static hipError_t launch_conv_tm(const ResnetConvArgs& a, hipStream_t s) {
    const long long M = (long long)a.B * a.Ho * a.Wo, blocks = ((M + TM - 1) / TM) * (a.Cout / RC_TN);
    if (blocks > (1LL << 23)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (a.epi == 1) hipLaunchKernelGGL((resnet_conv_kernel<TM, 1>), grid, dim3(256), 0, s, a);
    else if (a.epi == 2) hipLaunchKernelGGL((resnet_conv_kernel<TM, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((resnet_conv_kernel<TM, 3>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_resnet_conv(const ResnetConvArgs& a, hipStream_t s) {
    if (!resnet_conv_ok(a)) return hipErrorInvalidValue;
    const int tile = a.tile ? a.tile : resnet_conv_tile((long long)a.B * a.Ho * a.Wo, a.Cout);
    return tile == 128 ? launch_conv_tm<128>(a, s) : launch_conv_tm<32>(a, s);
}

hipError_t launch_resnet_pack(const float* w, half_t* out, int Cout, int Cin, int R, int* flag, hipStream_t s) {
    if (!w || !out || !flag || Cout % 16 || Cin % 64 || (R != 1 && R != 3)) return hipErrorInvalidValue;
    const size_t n = (size_t)Cout * Cin * R * R;
    hipLaunchKernelGGL(resnet_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, out, Cout, Cin, R, flag);
    return hipGetLastError();
}

hipError_t launch_resnet_entry(const float* x, long long sb, long long sc, long long sr, int B, int C, int H, int W, float* o32, half_t* o16,
                               hipStream_t s) {
    if (!x || !o32 || !o16 || B < 1 || B > 65535 || C % 64 || C < 64 || H < 1 || W < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resnet_entry_kernel, dim3((unsigned)((H * W + 63) / 64), (unsigned)(C / 64), (unsigned)B), dim3(256), 0, s, x, sb, sc, sr, C, H,
                       W, o32, o16);
    return hipGetLastError();
}

hipError_t launch_resnet_exit(const float* x, int B, int C, int S, float* out, long long sb, long long sc, hipStream_t s) {
    if (!x || !out || B < 1 || B > 65535 || C % 64 || C < 64 || S < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resnet_exit_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)(C / 64), (unsigned)B), dim3(256), 0, s, x, C, S, out, sb, sc);
    return hipGetLastError();
}

}  // namespace hg
