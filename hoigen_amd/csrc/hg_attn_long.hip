// Fused scaled-dot-product attention for gfx950, head_dim 64, for sequences of 225 .. ATTN_LONG_MAX_L tokens (the 577 tokens of
// ViT-L/14@336px, the 257 of ViT-L/14 at 224 px).  Same data layout, same per-tile arithmetic (tile_scores / tile_softmax_pv of
// hg_attn_dev.h) as attention_kernel (hg_attn.hip), which keeps every L <= 224.
//
// Structure: K and V of the whole (sequence, head) stay LDS resident (2 x 592 rows x 128 B = 151 552 B at L = 577: one workgroup per
// CU; two at L = 257), staged once by all waves with the same LDS-DMA and swizzles.  A workgroup has min(query tiles, 16) waves and a
// wave WALKS query tiles wave, wave + 16 (at most ATTN_LONG_TPW = 2: 20 tiles at the maximum length).  19 tiles over 16 waves
// land 5 / 5 / 5 / 4 on the four SIMDs, so the second round costs no SIMD more than a quarter of a tile over the even split.
// The LDS has no room left for the 4 KiB per wave that turn a tile's row-per-lane results into whole 128-byte rows while K and V are
// live, so a wave keeps its finished tiles as packed fp16 (16 registers per tile) until every wave has left the key loop; then the
// K/V rows are dead and the tiles leave through them exactly as in attention_kernel.
// The maximum length is what the LDS holds: 2 x 640 rows x 128 B = 163 840 B, all of a CU's 160 KiB.
#include "hg_attn_dev.h"

namespace hg {

// Waves per workgroup at most: 16 (128 registers a lane, which the non-causal kernel fills exactly); the causal instance needs 136
// for the diagonal tile's mask and runs 12 waves (170 a lane) rather than spill - 19 tiles over 12 waves are 5 / 5 / 5 / 4 a SIMD too
template <bool CAUSAL> static constexpr int ATTN_LONG_NW = CAUSAL ? 12 : 16;
static constexpr int ATTN_LONG_TPW = 2;      // query tiles per wave at most (20 tiles at the maximum length over >= 12 waves)
static_assert((ATTN_LONG_MAX_L / 32 + ATTN_LONG_NW<true> - 1) / ATTN_LONG_NW<true> <= ATTN_LONG_TPW, "tiles per wave");
static_assert(2 * ATTN_LONG_MAX_L * ROWB <= 160 * 1024, "K and V of the longest sequence fill the LDS");

// ROW0: as in attention_kernel - every wave helps to stage, wave 0 runs the one query row sel[seq] (row 0 when sel is null) with all
// 32 lanes of the tile aliasing it, through the same instruction sequence as the full kernel: its row is the full kernel's row bit
// for bit.  q0 / out are dense [n_seq, D].
template <bool CAUSAL, bool ROW0>
__global__ __launch_bounds__(64 * ATTN_LONG_NW<CAUSAL>) void attention_long_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ out,
                                                                          int L, int heads, int nkt, const half_t* __restrict__ q0,
                                                                          const int32_t* __restrict__ sel, const int ldo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // K and V rows 0 .. rs-1 are staged, rs = L rounded up to 16 (the last key tile may be half present: its second 16-key step is
    // skipped in P V, its missing K rows read into the V region and are masked); rows L .. rs-1 repeat row L-1 and are masked
    const int rs = (L + 15) & ~15;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = (int)(blockDim.x >> 6);
    char* Ks = smem;
    char* Vs = smem + rs * ROWB;
    const int D = heads * HD;
    const int item = (int)blockIdx.x;
    const int seq = item / heads, head = item - seq * heads;
    const size_t ld = (size_t)3 * D;
    const half_t* base = qkv + (size_t)seq * L * ld + head * HD;

    // ---- stage K and V: piece = 8 rows x 128 B; lane -> (row = l>>3, chunk' = l&7)
    for (int piece = wave; piece < rs / 8; piece += nwaves) {
        const int row = piece * 8 + (lane >> 3);
        const int src_row = row < L ? row : L - 1;
        const half_t* rp = base + (size_t)src_row * ld;
        const int cp = lane & 7;
        glds16(rp + D + ((cp ^ swz_k(row)) << 3), Ks + piece * 1024);
        glds16(rp + 2 * D + ((cp ^ swz_v(row)) << 3), Vs + piece * 1024);
    }

    const int qcol = lane & 31, hh = lane >> 5;
    // lane-constant LDS offsets
    int k_off[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) k_off[ks] = qcol * ROWB + (((2 * ks + hh) ^ swz_k(qcol)) << 4);
    const int gi = lane >> 4, l16 = lane & 15;
    const int vq = l16 >> 2, vp = l16 & 3;   // tr-read role: row vq of the 4x16 block, columns 4*vp..4*vp+3
    int v_off[2];
    {
        const int key0 = 4 * (gi >> 1) + vq;   // + kt*32 + 16*sstep (+8 for the second read)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            const int chunk = dt * 4 + (gi & 1) * 2 + (vp >> 1);
            v_off[dt] = key0 * ROWB + ((chunk ^ swz_v(key0)) << 4) + (vp & 1) * 8;
        }
    }
    int qsel = ROW0 && sel ? __builtin_amdgcn_readfirstlane(sel[seq]) : 0;
    qsel = qsel < 0 ? 0 : (qsel >= L ? L - 1 : qsel);      // caller error guard, as in layernorm_kernel

    __syncthreads();   // K/V landed (the barrier's fence waits for the LDS-DMA: vmcnt(0))
    if constexpr (ROW0) {
        if (wave != 0) return;
    }

    const float c = 0.125f * 1.4426950408889634f;   // head_dim^-0.5 * log2(e)
    // (held[t] stays in registers because the t loops below unroll completely, `break` included: tests/test_build_resources.py fails on
    // a byte of scratch)
    half4 held[ROW0 ? 1 : ATTN_LONG_TPW][8];         // finished tiles: d = dt*32 + 8*g + 4*hh + e of query qcol in [dt*4 + g][e]
#pragma unroll
    for (int t = 0; t < (ROW0 ? 1 : ATTN_LONG_TPW); ++t) {
        const int qt = ROW0 ? (qsel >> 5) : wave + t * nwaves;      // wave-uniform
        if (qt >= nkt) break;
        const int q = ROW0 ? qsel : qt * 32 + qcol;
        // Q fragments straight from global (B operand: lane = query, k = d)
        const half_t* qp = ROW0 ? q0 + (size_t)seq * D + head * HD + hh * 8 : base + (size_t)(q < L ? q : L - 1) * ld + hh * 8;
        half8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const half8*>(qp + ks * 16);
        float m = -1.0e30f, lsum = 0.f;
        f32x16 o[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
        const int kt_end = CAUSAL ? (qt + 1 < nkt ? qt + 1 : nkt) : nkt;
        for (int kt = 0; kt < kt_end; ++kt) {
            f32x16 sc;
            tile_scores(Ks + kt * TILEB, k_off, qf, sc);
            tile_softmax_pv<CAUSAL>(Vs + kt * TILEB, v_off, sc, kt, qt, q, L, rs, hh, c, m, lsum, o);
        }
        lsum += __shfl_xor(lsum, 32, 64);
        const float inv = 1.0f / lsum;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) held[t][dt * 4 + g][e] = (half_t)(o[dt][g * 4 + e] * inv);
    }
    if constexpr (ROW0) {
        if (qcol == 0) {
            half_t* op = out + (size_t)seq * D + head * HD;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) *reinterpret_cast<half4*>(op + dt * 32 + 8 * g + 4 * hh) = held[0][dt * 4 + g];
        }
    } else {
        // every wave has left the key loop: the K/V rows are dead, a wave's 32 x 64 tile goes through 4 KiB of them (16-byte chunks
        // XOR-swizzled by row) and leaves as whole 128-byte rows: lane -> (row = l >> 3, chunk = l & 7)
        __syncthreads();
        char* ot = smem + wave * 4096;
        const int cr = lane >> 3, cc = lane & 7;
#pragma unroll
        for (int t = 0; t < ATTN_LONG_TPW; ++t) {
            const int qt = wave + t * nwaves;
            if (qt >= nkt) break;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                *reinterpret_cast<half4*>(ot + qcol * 128 + ((j ^ (qcol & 7)) << 4) + hh * 8) = held[t][j];
#pragma unroll
            for (int rb = 0; rb < 32; rb += 8) {
                const int row = rb + cr, qq = qt * 32 + row;
                const half8 v = *reinterpret_cast<const half8*>(ot + row * 128 + ((cc ^ (row & 7)) << 4));
                if (qq < L) *reinterpret_cast<half8*>(out + ((size_t)seq * L + qq) * ldo + head * HD + cc * 8) = v;
            }
        }
    }
}

template <bool CAUSAL, bool ROW0>
static hipError_t launch_long_t(const half_t* qkv, half_t* out, int n_seq, int L, int heads, hipStream_t s, const half_t* q0,
                                const int32_t* sel, int ldo) {
    if (ldo <= 0) ldo = heads * HD;
    const int nkt = (L + 31) / 32;
    const int nwaves = nkt < ATTN_LONG_NW<CAUSAL> ? nkt : ATTN_LONG_NW<CAUSAL>;
    const int lds_kv = 2 * ((L + 15) & ~15) * ROWB, lds_out = nwaves * 4096;
    const int lds = lds_kv > lds_out ? lds_kv : lds_out;
    static bool attr_set_d[HG_MAX_DEVICES] = {};      // function attributes are per device
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_long_kernel<CAUSAL, ROW0>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 2 * ATTN_LONG_MAX_L * ROWB);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((attention_long_kernel<CAUSAL, ROW0>), dim3(n_seq * heads), dim3(64 * nwaves), lds, s, qkv, out, L, heads, nkt,
                       q0, sel, ldo);
    return hipGetLastError();
}

hipError_t launch_attention_long(const half_t* qkv, half_t* out, int n_seq, int L, int heads, bool causal, hipStream_t s, int ldo) {
    if (L <= ATTN_MAX_L_RESIDENT || L > ATTN_LONG_MAX_L) return hipErrorInvalidValue;
    return causal ? launch_long_t<true, false>(qkv, out, n_seq, L, heads, s, nullptr, nullptr, ldo)
                  : launch_long_t<false, false>(qkv, out, n_seq, L, heads, s, nullptr, nullptr, ldo);
}

hipError_t launch_attention_long_row0(const half_t* qkv, const half_t* q0, const int32_t* sel, half_t* out, int n_seq, int L, int heads,
                                      bool causal, hipStream_t s) {
    if (L <= ATTN_MAX_L_RESIDENT || L > ATTN_LONG_MAX_L || !q0) return hipErrorInvalidValue;
    return causal ? launch_long_t<true, true>(qkv, out, n_seq, L, heads, s, q0, sel, 0)
                  : launch_long_t<false, true>(qkv, out, n_seq, L, heads, s, q0, sel, 0);
}

}  // namespace hg
