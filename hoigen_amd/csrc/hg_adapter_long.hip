// Instance adapter (hg_adapter.hip) on sequences of 225 .. 640 tokens: the decoder layer of ViT-L/14@336px's 577 tokens per image.
// Option adapter_long (default 0) admits such towers at hg_load_vit / hg_update_adapters; launch_adapter_decoder sends L > 224 here.
//
// The short kernel (adapter_decoder_mfma) keeps one sequence per workgroup and K / V of all its keys (at most 224) in LDS.  Beyond that:
//   * a sequence is cut into n_qc = ceil(L / 224) QUERY chunks of 32 ceil(ceil(L / n_qc) / 32) tokens (577: 224 + 224 + 129), one
//     workgroup each, 32 tokens per wave, at most seven waves: the LDS map, the register tiles and every stage behind the attention are
//     the short kernel's (hg_adapter_dev.h);
//   * with priors (SELF = false) a token attends only to the N <= 32 prior tokens, so the chunks share nothing: every workgroup
//     projects the priors as the short kernel does and a token's arithmetic is the short kernel's, bit for bit;
//   * without priors (SELF = true) the memory is the sequence's own L rows.  adapter_kv16_kernel projects them once per sequence into
//     the adkv workspace (fp16, in the layouts the LDS area holds), and the decoder streams them through that area in KEY chunks of at
//     most 224 with a running maximum: per chunk the short kernel's pass 1 (chunk maximum), the rescale of l, o0, o1 by
//     exp(m - m_new), the short kernel's pass 2 against m_new.
// No down_proj inside the kernel, no folded mode, no wait on another workgroup; every loop is bounded by L <= 640.
#include "hg_adapter_dev.h"

namespace hg {

namespace {

constexpr int LF = 2;                       // 16-token tiles per wave
constexpr int KCH = NKMAX;                  // keys per chunk (the K / V area of the short kernel)
constexpr int LONG_LDS = (4 * 64 * XP + NKMAX * KP + 64 * VP + 64 * XP) * 2;      // the short kernel's map: 148 992 B
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

inline int pad32(int n) { return (n + 31) & ~31; }

}  // namespace

// the dynamic LDS size the decoder is launched with, as data of the code object (tests/test_adapter_long_resources.py reads it there)
extern "C" __device__ __attribute__((used)) const int hg_adapter_long_lds_bytes = LONG_LDS;

// K and V of every `down` row of a sequence (memory = the sequence itself) with the roundings of the short kernel's emit_kv: fp16 row,
// fp16 weights, fp32 accumulation on top of the bias, fp16 result.  Lp = L rounded up to 32; key slots L .. Lp - 1 carry row L - 1
// (the short kernel's clamped rows), so the P . V MFMA never multiplies p = 0 into stale bits.
//   k16 [n_seq][Lp][64]      row-major
//   vt16 [n_seq][64][Lp]     V^T, inside every block of 32 keys in key_slot order
// A wave owns 32 keys = one key block; a workgroup of four waves 128 keys of one sequence.  V goes through the wave's own LDS tile
// so that it leaves in 16-byte pieces.
__global__ __launch_bounds__(256) void adapter_kv16_kernel(const float* __restrict__ down, int ld_down, const half_t* __restrict__ Wk,
                                                           const half_t* __restrict__ Wv, const float* __restrict__ bk,
                                                           const float* __restrict__ bv, int L, int Lp, int blocks_per_seq,
                                                           half_t* __restrict__ k16, half_t* __restrict__ vt16) {
    constexpr int TP = 40;                                  // halfs per row of the V^T tile (32 slots + pad; 80 B: 16-byte aligned)
    __shared__ __attribute__((aligned(16))) half_t Xs[4][32 * XP];
    __shared__ __attribute__((aligned(16))) half_t Vs[4][64 * TP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int seq = blockIdx.x / blocks_per_seq, kb = blockIdx.x - seq * blocks_per_seq;
    const int key0 = kb * 128 + wave * 32;
    if (key0 >= Lp) return;                                 // (no barrier below: a wave works on its own LDS rows only)
    half_t* X = Xs[wave];
    half_t* V = Vs[wave];
    f32x4 t[LF][4];
#pragma unroll
    for (int f = 0; f < LF; ++f) {
        const int key = key0 + 16 * f + r;
        const size_t m = (size_t)seq * L + (key < L ? key : L - 1);
#pragma unroll
        for (int g = 0; g < 4; ++g) t[f][g] = *reinterpret_cast<const f32x4*>(down + m * ld_down + 16 * g + 4 * q);
    }
    store_T<4>(t, X, lane);
    f32x4 kk[LF][4], vv[LF][4];
    init_bias<4>(kk, bk, lane);
    init_bias<4>(vv, bv, lane);
    linear_T<4, 2>(kk, Wk, 64, X, lane);
    linear_T<4, 2>(vv, Wv, 64, X, lane);
#pragma unroll
    for (int f = 0; f < LF; ++f) {
        const int key = key0 + 16 * f + r;                  // < Lp: key0 < Lp, both multiples of 32
        const int slot = key_slot(16 * f + r);
        half_t* kdst = k16 + ((size_t)seq * Lp + key) * 64;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)kk[f][g][e];
            *reinterpret_cast<half4*>(kdst + 16 * g + 4 * q) = h;
#pragma unroll
            for (int e = 0; e < 4; ++e) V[(16 * g + 4 * q + e) * TP + slot] = (half_t)vv[f][g][e];
        }
    }
    // the wave's V^T tile [64 features][32 slots] -> global, 64 B per feature row = four 16-byte pieces
    half_t* vdst = vt16 + (size_t)seq * 64 * Lp + key0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int pc = lane + 64 * j, feat = pc >> 2, part = pc & 3;
        *reinterpret_cast<u32x4*>(vdst + (size_t)feat * Lp + 8 * part) = *reinterpret_cast<const u32x4*>(V + feat * TP + 8 * part);
    }
}

// One workgroup per (sequence, query chunk of QC tokens); blockDim.x = 64 * QC / 32 <= 448.  `down` is not __restrict__: a chained
// layer (adapter_num_layers > 1, priors only) writes chain32 == down in place - every workgroup reads and writes its own tokens' rows.
template <bool SELF>
__global__ __launch_bounds__(512) void adapter_decoder_long(const float* down, int ld_down, DecW16 W, const float* __restrict__ priors,
                                                            const uint8_t* __restrict__ mask, int L, int N, int n_qc, int QC,
                                                            const half_t* __restrict__ k16, const half_t* __restrict__ vt16,
                                                            half_t* __restrict__ out16, float* chain32, int ld16) {
    constexpr int F = LF;
    extern __shared__ __attribute__((aligned(16))) char smem_adl[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int seq = blockIdx.x / n_qc, qc = blockIdx.x - seq * n_qc;
    const int nkeys = SELF ? L : N;
    const int Lp = (L + 31) & ~31;
    half_t* Xw = reinterpret_cast<half_t*>(smem_adl) + wave * 16 * F * XP;       // this wave's activation rows
    half_t* Ks = reinterpret_cast<half_t*>(smem_adl) + 4 * 64 * XP;              // K [key][KP]
    half_t* VT = Ks + NKMAX * KP;                                                // V^T [feature][VP]
    half_t* Mem = VT + 64 * VP;                                                  // prior tokens fp16 [32][XP] (prior case)

    // ---- this wave's 32 tokens (rows behind L - 1 repeat it and are never stored): fp32 residual in registers, fp16 copy in LDS
    f32x4 tgt[F][4];
    int tok[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        tok[f] = qc * QC + wave * 16 * F + 16 * f + r;
        const size_t m = (size_t)seq * L + (tok[f] < L ? tok[f] : L - 1);
#pragma unroll
        for (int g = 0; g < 4; ++g) tgt[f][g] = *reinterpret_cast<const f32x4*>(down + m * ld_down + 16 * g + 4 * q);
    }
    store_T<4>(tgt, Xw, lane);
    if constexpr (!SELF) {
        // prior tokens [N <= 32][64] fp32 -> fp16 rows (rows >= N zero), then wave 0 projects them: the short kernel's emit_kv
        for (int i = tid; i < 32 * 16; i += (int)blockDim.x) {
            const int row = i >> 4, c4 = (i & 15) * 4;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row < N) v = *reinterpret_cast<const f32x4*>(priors + ((size_t)seq * N + row) * 64 + c4);
            half4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)v[e];
            *reinterpret_cast<half4*>(Mem + row * XP + c4) = h;
        }
        __syncthreads();
        if (wave == 0) {
            f32x4 kk[F][4], vv[F][4];
            init_bias<4>(kk, W.bk, lane);
            init_bias<4>(vv, W.bv, lane);
            linear_T<4, 2>(kk, W.Wk, 64, Mem, lane);
            linear_T<4, 2>(vv, W.Wv, 64, Mem, lane);
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const int key = 16 * f + r;
                const int slot = key_slot(key);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    half4 h;
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[e] = (half_t)kk[f][g][e];
                    *reinterpret_cast<half4*>(Ks + key * KP + 16 * g + 4 * q) = h;
#pragma unroll
                    for (int e = 0; e < 4; ++e) VT[(16 * g + 4 * q + e) * VP + slot] = (half_t)vv[f][g][e];
                }
            }
        }
        __syncthreads();
    }

    // ---- q = (Wq x + bq) / sqrt(32)
    f32x4 t[F][4];
    init_bias<4>(t, W.bq, lane);
    linear_T<4, 2>(t, W.Wq, 64, Xw, lane);
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) t[f][g] *= 0.17677669529663687f;
    store_T<4>(t, Xw, lane);                                  // (the fp16 copy of the input is no longer needed)

    // ---- cross attention, 2 heads of 32, over key chunks of at most KCH keys: running maximum m, sum l and output o0 / o1 per
    // (head, token tile)
    float mrun[2][F], lsum[2][F];
    f32x4 o0[2][F], o1[2][F];
#pragma unroll
    for (int hd = 0; hd < 2; ++hd)
#pragma unroll
        for (int f = 0; f < F; ++f) {
            mrun[hd][f] = -INFINITY;
            lsum[hd][f] = 0.f;
            o0[hd][f] = f32x4{0.f, 0.f, 0.f, 0.f};
            o1[hd][f] = o0[hd][f];
        }
    const int n_kc = SELF ? (L + KCH - 1) / KCH : 1;
    for (int kc = 0; kc < n_kc; ++kc) {
        const int key0 = kc * KCH;
        const int nk = nkeys - key0 < KCH ? nkeys - key0 : KCH;     // keys of this chunk (>= 1)
        const int nkt = (nk + 15) >> 4;                     // key tiles of 16
        const int nkb = (nkt + 1) >> 1;                     // key blocks of 32
        if constexpr (SELF) {
            if (kc > 0) __syncthreads();                    // every wave is done with the previous chunk
            // K rows and V^T columns key0 .. key0 + 32 nkb - 1 (<= Lp) -> LDS, 16 bytes a piece
            const half_t* kg = k16 + ((size_t)seq * Lp + key0) * 64;
            for (int i = tid; i < 32 * nkb * 8; i += (int)blockDim.x)
                *reinterpret_cast<u32x4*>(Ks + (i >> 3) * KP + (i & 7) * 8) = *reinterpret_cast<const u32x4*>(kg + (size_t)i * 8);
            const half_t* vg = vt16 + (size_t)seq * 64 * Lp + key0;
            const int per = 4 * nkb;                        // pieces per feature row
            for (int i = tid; i < 64 * per; i += (int)blockDim.x) {
                const int feat = i / per, pc = i - feat * per;
                *reinterpret_cast<u32x4*>(VT + feat * VP + pc * 8) = *reinterpret_cast<const u32x4*>(vg + (size_t)feat * Lp + pc * 8);
            }
            __syncthreads();
        }
        // masked keys of the chunk as a bit set (wave-uniform): bit k of word k >> 5; keys behind the last one never enter a maximum
        unsigned mbits[NKMAX / 32];
#pragma unroll
        for (int b = 0; b < NKMAX / 32; ++b) {
            unsigned m = 0u;
            if (b < nkb) {
                const int key = 32 * b + (lane & 31);
                bool dead = key >= nk;
                if (!SELF && !dead && mask) dead = mask[(size_t)seq * N + key] != 0;
                const unsigned long long bal = __ballot(dead);
                m = (unsigned)bal;                           // lanes 0..31 carry keys 32b .. 32b+31
            }
            mbits[b] = __builtin_amdgcn_readfirstlane(m);
        }
#pragma unroll
        for (int hd = 0; hd < 2; ++hd) {
#pragma unroll
            for (int f = 0; f < F; ++f) {
                const half8 qf = *reinterpret_cast<const half8*>(Xw + (16 * f + r) * XP + 32 * hd + 8 * q);
                // pass 1: scores of every key tile of the chunk -> its maximum (scores are recomputed in pass 2: one MFMA per tile)
                float mx = -INFINITY;
                for (int kt = 0; kt < nkt; ++kt) {
                    const half8 kf = *reinterpret_cast<const half8*>(Ks + (16 * kt + r) * KP + 32 * hd + 8 * q);
                    f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    const unsigned mb = mbits[kt >> 1] >> (16 * (kt & 1) + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (!((mb >> e) & 1u)) mx = fmaxf(mx, s[e]);
                }
                mx = fmaxf(mrun[hd][f], max_rows(mx));
                if (kc > 0) {                                // the first chunk has nothing to rescale (and no exp(-inf - ..) to take)
                    const float alpha = __expf(mrun[hd][f] - mx);
                    lsum[hd][f] *= alpha;
                    o0[hd][f] *= alpha;
                    o1[hd][f] *= alpha;
                }
                mrun[hd][f] = mx;
                float ls = lsum[hd][f];
                f32x4 a0 = o0[hd][f], a1 = o1[hd][f];
                for (int b = 0; b < nkb; ++b) {
                    half8 pf;
#pragma unroll
                    for (int k2 = 0; k2 < 2; ++k2) {
                        const int kt = 2 * b + k2;
                        f32x4 s = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                        unsigned mb = 0xFu;
                        if (kt < nkt) {
                            const half8 kf = *reinterpret_cast<const half8*>(Ks + (16 * kt + r) * KP + 32 * hd + 8 * q);
                            s = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                            mb = mbits[b] >> (16 * k2 + 4 * q);
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float pe = ((mb >> e) & 1u) ? 0.f : __expf(s[e] - mx);
                            ls += pe;
                            pf[4 * k2 + e] = (half_t)pe;
                        }
                    }
                    const half8 v0 = *reinterpret_cast<const half8*>(VT + (32 * hd + r) * VP + 32 * b + 8 * q);
                    const half8 v1 = *reinterpret_cast<const half8*>(VT + (32 * hd + 16 + r) * VP + 32 * b + 8 * q);
                    a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v0, pf, a0, 0, 0, 0);
                    a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(v1, pf, a1, 0, 0, 0);
                }
                lsum[hd][f] = ls;
                o0[hd][f] = a0;
                o1[hd][f] = a1;
            }
        }
    }
    f32x4 att[F][4];
#pragma unroll
    for (int hd = 0; hd < 2; ++hd)
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float inv = 1.0f / sum_rows4(lsum[hd][f]);
            att[f][2 * hd] = o0[hd][f] * inv;
            att[f][2 * hd + 1] = o1[hd][f] * inv;
        }
    // ---- out_proj, residual, norm2
    store_T<4>(att, Xw, lane);
    init_bias<4>(t, W.bo, lane);
    linear_T<4, 2>(t, W.Wo, 64, Xw, lane);
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) tgt[f][g] += t[f][g];
    layer_norm_T(tgt, W.norms, W.norms + 64, lane);
    // ---- FFN 64 -> 128 (relu) -> 64, residual, norm3
    store_T<4>(tgt, Xw, lane);
    {
        f32x4 hid[F][8];
        init_bias<8>(hid, W.b1, lane);
        linear_T<8, 2>(hid, W.W1, 64, Xw, lane);
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int g = 0; g < 8; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) hid[f][g][e] = fmaxf(hid[f][g][e], 0.f);
        store_T<8>(hid, Xw, lane);
    }
    init_bias<4>(t, W.b2, lane);
    linear_T<4, 4>(t, W.W2, 128, Xw, lane);
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) tgt[f][g] += t[f][g];
    layer_norm_T(tgt, W.norms + 128, W.norms + 192, lane);
    if (chain32) {      // adapter_num_layers > 1: fp32, in the layout the next layer of the chain reads (rows of ld_down)
#pragma unroll
        for (int f = 0; f < F; ++f)
            if (tok[f] < L) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<f32x4*>(chain32 + ((size_t)seq * L + tok[f]) * ld_down + 16 * g + 4 * q) = tgt[f][g];
            }
        return;
    }
#pragma unroll
    for (int f = 0; f < F; ++f)
        if (tok[f] < L) {
            half_t* dst = out16 + ((size_t)seq * L + tok[f]) * ld16;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 h;
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = (half_t)tgt[f][g][e];
                *reinterpret_cast<half4*>(dst + 16 * g + 4 * q) = h;
            }
        }
}

// the long MFMA decoder serves 225 .. 640 tokens with fp16 weights present and, with priors, at most 32 prior tokens
bool adapter_decoder_long_ok(const AdapterDev& ad, bool priors, int L, int N) {
    return ad.w16[priors ? 0 : 1][0] && L > ADAPTER_MAX_L && L <= ADAPTER_LONG_MAX_L && (priors ? N >= 1 && N <= 32 : true);
}

// kv16: the adkv workspace, at least B * L * 512 bytes (self memory: K and V^T of the padded sequences take B * pad32(L) * 256)
hipError_t launch_adapter_decoder_long(const float* down32, const AdapterDev& ad, const float* priors, const uint8_t* mask, int B, int L,
                                       int N, void* kv16, half_t* out16, hipStream_t s, float* chain32, int ld16) {
    if (!adapter_decoder_long_ok(ad, priors != nullptr, L, N) || ld16 < 64 || ld16 % 8 || B < 1) return hipErrorInvalidValue;
    if (!priors && (!kv16 || chain32)) return hipErrorInvalidValue;
    const int which = priors ? 0 : 1;
    const float* const* dl = ad.dl[which];
    const half_t* const* w = ad.w16[which];
    const DecW16 Wd{w[0], w[1], w[2], w[3], w[4], w[5], dl[3], dl[4], dl[5], dl[7], dl[10], dl[11] + (size_t)2 * 64 * 64, dl[8]};
    static bool attr_set_d[HG_MAX_DEVICES] = {};
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        const void* fns[2] = {reinterpret_cast<const void*>(&adapter_decoder_long<true>),
                              reinterpret_cast<const void*>(&adapter_decoder_long<false>)};
        for (const void* fn : fns) {
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, LONG_LDS);
            if (e != hipSuccess) return e;
        }
        attr_set = true;
    }
    const int n_qc = (L + ADAPTER_MAX_L - 1) / ADAPTER_MAX_L;
    const int QC = pad32((L + n_qc - 1) / n_qc);            // <= 224: ceil(L / n_qc) <= 224
    const unsigned threads = 64u * (unsigned)(QC / 32);
    const int Lp = pad32(L);
    half_t* k16 = (half_t*)kv16;
    half_t* vt16 = k16 ? k16 + (size_t)B * Lp * 64 : nullptr;
    if (priors) {
        hipLaunchKernelGGL(adapter_decoder_long<false>, dim3((unsigned)(B * n_qc)), dim3(threads), LONG_LDS, s, down32, 128, Wd, priors,
                           mask, L, N, n_qc, QC, (const half_t*)nullptr, (const half_t*)nullptr, out16, chain32, ld16);
    } else {
        const int bps = (Lp + 127) / 128;
        hipLaunchKernelGGL(adapter_kv16_kernel, dim3((unsigned)(B * bps)), dim3(256), 0, s, down32, 128, Wd.Wk, Wd.Wv, Wd.bk, Wd.bv, L, Lp,
                           bps, k16, vt16);
        hipLaunchKernelGGL(adapter_decoder_long<true>, dim3((unsigned)(B * n_qc)), dim3(threads), LONG_LDS, s, down32, 128, Wd, priors,
                           mask, L, 0, n_qc, QC, (const half_t*)k16, (const half_t*)vt16, out16, chain32, ld16);
    }
    return hipGetLastError();
}

}  // namespace hg
