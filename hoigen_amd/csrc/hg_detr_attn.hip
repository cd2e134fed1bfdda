// Masked scaled-dot-product attention for gfx950 with head_dim 32 and separate query and key lengths: the DETR transformer's attention
// (detr/models/transformer.py:137-140 self-attention of the encoder with src_key_padding_mask; the decoder's cross-attention is the
// same kernel with Lq = 100).  out = softmax(q k^T / sqrt(32) + key_padding_mask) v per (sequence, head).
//
// Rounding points are those of tile_softmax_pv (hg_attn_dev.h): scores in fp32 from exact fp16 products, a running maximum with
// rescale, P rounded to fp16, the row sum in fp32 from the unrounded exponentials, P V in fp32, one fp16 rounding of the output.
// With head dim 32 the 32 x 32 x 16 MFMA needs two k-steps for a score tile and ONE accumulator for O^T.
//
// Work item = (sequence, head, slab of nw query tiles): a workgroup of nw waves, one 32-query tile a wave.  nw = DETR_ATTN_NW = 4
// (128-query slabs) unless the launch fixes 1 or 2: measured on an MI355X (profiles/detr_encoder.txt), ONE image of 25 x 38 tokens takes
// 25 us with 32-, 64- and 128-query slabs alike (240, 120 and 64 workgroups: what a wider grid gains it pays in staging K and V again),
// and a batch never gains from smaller slabs (4 images: 85 / 48 / 29 us).  K and V of the (sequence, head) go through
// the LDS in CHUNKS of `chunk_rows` keys (a multiple of 32; 64-byte rows: 128 B a key for both): one chunk = all keys while they fit
// (Lk <= 1 280: 160 KiB), 512 keys (64 KiB: two workgroups a CU) beyond.  Running maximum, sum and accumulator are carried from chunk
// to chunk, and the 32-key tiles are walked in the same order whatever the chunk size: every chunk size gives the same bits.
//
// The key padding mask is not staged: per tile, lane i reads the byte of key 32 kt + i (one tile ahead of its use) and the wave's
// ballot is the tile's 32 mask bits in a scalar register; keys >= Lk count as masked.  A tile whose 32 keys are all masked is skipped
// (its probabilities are zero: the running maximum starts at -1e30, not -inf, so neither the rescale exp2((m_old - m_new) c) nor the
// exponentials meet inf - inf); a sequence without a visible key ends with a zero row sum and 0 * inf = NaN in its own rows.
// LDS rows >= Lk repeat row Lk - 1 of the same sequence and their V values are read as zeros.
#include "hg_kernels.h"

namespace hg {

static constexpr int DA_ROWB = 64;              // bytes per K / V row in LDS (head dim 32)
static constexpr int DA_TILEB = 32 * DA_ROWB;   // bytes per 32-key tile
static_assert(2 * DETR_ATTN_RESIDENT_L * DA_ROWB <= 160 * 1024, "K and V of the longest resident sequence fill the LDS");
static_assert(DETR_ATTN_RESIDENT_L % 32 == 0 && DETR_ATTN_CHUNK_L % 32 == 0 && DETR_ATTN_MAX_L % 32 == 0, "whole key tiles");

// 16-byte chunk c of K row `row` sits at chunk c ^ swz: the 16 lanes of a b128 read (16 rows, one chunk) then cover all 64 banks
__device__ __forceinline__ int da_swz_k(int row) { return (row >> 2) & 3; }

__global__ __launch_bounds__(64 * DETR_ATTN_NW) void detr_attn_kernel(const DetrAttnArgs a, const int chunk_rows, const int nslab) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Lq = a.Lq, Lk = a.Lk;
    const int item = (int)blockIdx.x;
    const int slab = item % nslab, sh = item / nslab;
    const int seq = sh / a.heads, head = sh - seq * a.heads;
    char* Ks = smem;
    char* Vs = smem + chunk_rows * DA_ROWB;
    const half_t* kbase = a.k + (size_t)seq * Lk * a.ldk + head * 32;
    const half_t* vbase = a.v + (size_t)seq * Lk * a.ldv + head * 32;
    const uint8_t* mrow = a.mask ? a.mask + (size_t)seq * Lk : nullptr;

    const int qcol = lane & 31, hh = lane >> 5;
    const int nw = (int)(blockDim.x >> 6);                 // waves of this workgroup = query tiles of a slab
    const int qt = slab * nw + wave;                       // this wave's query tile (wave-uniform)
    const bool active = qt * 32 < Lq;                      // the last slab's spare waves only help to stage
    const int q = qt * 32 + qcol;
    // lane-constant LDS offsets: K row = key qcol, 16-byte chunk 2 ks + hh; V through the transposing read (4 keys x 16 channels per
    // group of 16 lanes: lane -> key vq of the four, channels 4 vp .. 4 vp + 3 of the group's 16)
    int k_off[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) k_off[ks] = qcol * DA_ROWB + (((2 * ks + hh) ^ da_swz_k(qcol)) << 4);
    const int gi = lane >> 4, l16 = lane & 15;
    const int vq = l16 >> 2, vp = l16 & 3;
    const int v_off = (4 * (gi >> 1) + vq) * DA_ROWB + (((gi & 1) * 2 + (vp >> 1)) << 4) + (vp & 1) * 8;

    half8 qf[2];
    {      // Q fragments straight from global (B operand: lane = query, k = d); rows >= Lq repeat the last row and are never stored
        const int qr = active ? (q < Lq ? q : Lq - 1) : 0;
        const half_t* qp = a.q + ((size_t)seq * Lq + qr) * a.ldq + head * 32 + hh * 8;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const half8*>(qp + ks * 16);
    }
    const float c = 0.17677669529663689f * 1.4426950408889634f;      // head_dim^-0.5 * log2(e)
    float m = -1.0e30f, lsum = 0.f;
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;

    // the mask byte of key 32 kt + qcol, read one tile ahead (keys >= Lk: masked, nothing read)
    auto mask_byte = [&](int kt) -> int {
        const int key = kt * 32 + qcol;
        if (key >= Lk) return 1;
        return mrow ? (int)mrow[key] : 0;
    };
    int mb = active ? mask_byte(0) : 1;

    for (int c0 = 0; c0 < Lk; c0 += chunk_rows) {
        const int left = (Lk - c0 + 31) & ~31;
        const int rows = left < chunk_rows ? left : chunk_rows;      // staged rows of this chunk: whole 32-key tiles
        if (c0) __syncthreads();                                     // every wave has left the previous chunk
        // ---- stage K and V: piece = 16 rows x 64 B; lane -> (row = l >> 2, chunk = l & 3)
        for (int piece = wave; piece < rows / 16; piece += nw) {
            const int row = c0 + piece * 16 + (lane >> 2);
            const int src_row = row < Lk ? row : Lk - 1;
            const int cp = lane & 3;
            glds16(kbase + (size_t)src_row * a.ldk + ((cp ^ da_swz_k(row)) << 3), Ks + piece * 1024);
            glds16(vbase + (size_t)src_row * a.ldv + (cp << 3), Vs + piece * 1024);
        }
        __syncthreads();   // K/V landed (the barrier's fence waits for the LDS-DMA: vmcnt(0))
        if (!active) continue;
        for (int t = 0; t < rows / 32; ++t) {
            const int kt = c0 / 32 + t;
            const unsigned bits = (unsigned)__ballot(mb != 0);      // lanes 0 .. 31: keys 32 kt .. 32 kt + 31 (wave-uniform)
            mb = mask_byte(kt + 1);
            if (bits == 0xffffffffu) continue;                       // no visible key in this tile
            const char* kb = Ks + t * DA_TILEB;
            const char* vb = Vs + t * DA_TILEB;
            // ---- S^T tile: lane holds keys kt*32 + (r&3) + 8*(r>>2) + 4*hh of query q
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const half8 kf = *reinterpret_cast<const half8*>(kb + k_off[ks]);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s, 0, 0, 0);
            }
            if (bits) {
                const unsigned mine = bits >> (4 * hh);
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = ((mine >> ((r & 3) + 8 * (r >> 2))) & 1u) ? -INFINITY : s[r];
            }
            float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
#pragma unroll
            for (int r = 4; r < 16; r += 4) mx = fmaxf(mx, fmaxf(fmaxf(s[r], s[r + 1]), fmaxf(s[r + 2], s[r + 3])));
            {      // the other half of the query's keys sits in lane ^ 32
                const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, mx), __builtin_bit_cast(unsigned, mx),
                                                                 false, false);
                mx = fmaxf(__builtin_bit_cast(float, (unsigned)sw[0]), __builtin_bit_cast(float, (unsigned)sw[1]));
            }
            if (__any(mx > m)) {                 // some query's running max grew: rescale (wave-uniform branch)
                const float mn = fmaxf(m, mx);
                const float alpha = __builtin_amdgcn_exp2f((m - mn) * c);
                m = mn;
                lsum *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) o[r] *= alpha;
            }
            const float mc = m * c;
            half8 pf[2];
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = __builtin_amdgcn_exp2f(fmaf(s[r], c, -mc));
                ps += e;
                pf[r >> 3][r & 7] = (half_t)e;
            }
            lsum += ps;
            // ---- O^T[d][q] += sum_key V[key][d] P[q][key]; element j of lane half hh is key 16s + 8(j>>2) + 4hh + (j&3)
            // (transposing reads as in tile_softmax_pv: inline asm loads, lgkmcnt waited here)
#pragma unroll
            for (int sstep = 0; sstep < 2; ++sstep) {
                fp16x4_t vr[2];
                const unsigned va = (unsigned)(size_t)(HG_LDS const char*)(vb + sstep * (16 * DA_ROWB) + v_off);
                asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %2 offset:512"
                             : "=&v"(vr[0]), "=&v"(vr[1])
                             : "v"(va)
                             : "memory");
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[0]), "+v"(vr[1])::"memory");
                half8 vf;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vf[e] = (half_t)vr[0][e];
                    vf[4 + e] = (half_t)vr[1][e];
                }
                if (kt * 32 + 32 > Lk) {      // rows behind Lk: zeros, whatever the LDS holds
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (kt * 32 + 16 * sstep + 8 * (j >> 2) + 4 * hh + (j & 3) >= Lk) vf[j] = (half_t)0.f;
                }
                o = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[sstep], o, 0, 0, 0);
            }
        }
    }
    if (!active) return;
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / lsum;
    if (q < Lq) {      // lane holds channels 8 g + 4 hh + e of query q
        half_t* op = a.out + ((size_t)seq * Lq + q) * a.ldo + head * 32 + 4 * hh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half4 h4;
#pragma unroll
            for (int e = 0; e < 4; ++e) h4[e] = (half_t)(o[g * 4 + e] * inv);
            *reinterpret_cast<half4*>(op + 8 * g) = h4;
        }
    }
}

int detr_attn_chunk_rows(int Lk, int chunk) {
    const int lk32 = (Lk + 31) & ~31;
    if (chunk > 0) return chunk < lk32 ? chunk : lk32;
    return lk32 <= DETR_ATTN_RESIDENT_L ? lk32 : DETR_ATTN_CHUNK_L;
}

hipError_t launch_detr_attention(const DetrAttnArgs& a, hipStream_t s) {
    if (!a.q || !a.k || !a.v || !a.out || a.n_seq < 1 || a.heads < 1) return hipErrorInvalidValue;
    if (a.Lq < 1 || a.Lk < 1 || a.Lq > DETR_ATTN_MAX_L || a.Lk > DETR_ATTN_MAX_L) return hipErrorInvalidValue;
    if (a.chunk < 0 || a.chunk % 32 || a.chunk > DETR_ATTN_RESIDENT_L) return hipErrorInvalidValue;
    const int D = a.heads * 32;
    // 16-byte row reads of q / k / v (LDS-DMA and b128 loads), 8-byte stores of out
    if (a.ldq < D || a.ldk < D || a.ldv < D || a.ldo < D || a.ldq % 8 || a.ldk % 8 || a.ldv % 8 || a.ldo % 4) return hipErrorInvalidValue;
    if (((size_t)a.q | (size_t)a.k | (size_t)a.v) & 15 || ((size_t)a.out & 7)) return hipErrorInvalidValue;
    if (a.waves < 0 || a.waves == 3 || a.waves > DETR_ATTN_NW) return hipErrorInvalidValue;
    const int nw = a.waves ? a.waves : DETR_ATTN_NW;
    const int nslab = (a.Lq + 32 * nw - 1) / (32 * nw);
    const long long grid = (long long)a.n_seq * a.heads * nslab;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    const int chunk_rows = detr_attn_chunk_rows(a.Lk, a.chunk);
    const int lds = 2 * chunk_rows * DA_ROWB;
    static bool attr_set_d[HG_MAX_DEVICES] = {};      // function attributes are per device
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&detr_attn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           2 * DETR_ATTN_RESIDENT_L * DA_ROWB);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(detr_attn_kernel, dim3((unsigned)grid), dim3(64 * nw), lds, s, a, chunk_rows, nslab);
    return hipGetLastError();
}

}  // namespace hg
