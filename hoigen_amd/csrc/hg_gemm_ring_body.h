// Body of the persistent ring GEMM (hg_gemm_ring.hip holds the kernel's description, the stand-alone kernel and its launchers) as a
// device function over a tile schedule, so that the MLP pair kernel (hg_mlp_pair.hip: c_fc -> QuickGELU -> c_proj in ONE launch) runs
// the very same K loop and epilogues on its own tile order.  SCHED: n_items(), tile(r, tm, tn), slack(), PUBLISH (+ publish(tm, lane)).
#pragma once
#include <type_traits>

#include "hg_gemm_dev.h"

namespace hg {

// Diagnostic build (HG_EXTRA_FLAGS="-DHG_STAMPS -DHG_STAMP_MASK=<bits>"): per-wave s_memtime totals of the
// selected segment kinds (0 vmcnt waits, 1 lgkmcnt waits, 2 fetch barriers, 3 MFMA segments, 4 MFMA barriers,
// 5 DMA issue, 6 ds_read issue, 7 epilogue) and of the whole tile loop, written to GemmArgs::dbg.
#ifdef HG_STAMPS
#ifndef HG_STAMP_MASK
#define HG_STAMP_MASK 0xFF
#endif
#define SEG_B(k) do { if constexpr ((HG_STAMP_MASK >> (k)) & 1) t_beg = __builtin_amdgcn_s_memtime(); } while (0)
#define SEG_E(k) do { if constexpr ((HG_STAMP_MASK >> (k)) & 1) tacc[k] += __builtin_amdgcn_s_memtime() - t_beg; } while (0)
#else
#define SEG_B(k) do {} while (0)
#define SEG_E(k) do {} while (0)
#endif

// Fragment I of 16 (8 of A, 8 of W) of the one-tile two-phase loop, read from LDS into a FIXED register tuple, v[192 + 4 I : 195 + 4 I].
// Left to the register allocator, values that live across the loop in ones and twos (a zero for the panel poll's address, the lane
// number, hoisted epilogue addresses) end up between the fragment tuples and push them to 2 (mod 4), where MFMAs issue slower.  The
// ds_read itself is the asm statement: an empty asm that only names the tuple reads the register the ds_read is filling, and the
// compiler then waits for every ds_read on its own (measured: profiles/mlp_pair256_ph2.txt).  The compiler does not know of these
// reads: the fetch segment ends in an explicit lgkmcnt(0) (sync_fetch) before anything uses them.
template <int I, int OFF, class T>
__device__ __forceinline__ void ds_read_fixed(T& x, int addr) {
    static_assert(sizeof(T) == 16 && I >= 0 && I < 16 && OFF >= 0 && OFF < 65536, "a 4-register fragment, 16 tuples, a 16-bit offset");
#define HG_DS_READ_FIXED(n, r) if constexpr (I == n) asm volatile("ds_read_b128 %0, %1 offset:%2" : "={" r "}"(x) : "v"(addr), "n"(OFF) : "memory")
    HG_DS_READ_FIXED(0, "v[192:195]"); HG_DS_READ_FIXED(1, "v[196:199]"); HG_DS_READ_FIXED(2, "v[200:203]"); HG_DS_READ_FIXED(3, "v[204:207]");
    HG_DS_READ_FIXED(4, "v[208:211]"); HG_DS_READ_FIXED(5, "v[212:215]"); HG_DS_READ_FIXED(6, "v[216:219]"); HG_DS_READ_FIXED(7, "v[220:223]");
    HG_DS_READ_FIXED(8, "v[224:227]"); HG_DS_READ_FIXED(9, "v[228:231]"); HG_DS_READ_FIXED(10, "v[232:235]"); HG_DS_READ_FIXED(11, "v[236:239]");
    HG_DS_READ_FIXED(12, "v[240:243]"); HG_DS_READ_FIXED(13, "v[244:247]"); HG_DS_READ_FIXED(14, "v[248:251]"); HG_DS_READ_FIXED(15, "v[252:255]");
#undef HG_DS_READ_FIXED
}
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// HL (EPI_RESID_LN_F32 at MF = 4; GemmArgs::hl): the residual stream as centre + hi + lo, in the very bytes the 128 x 256
// kernel reads and writes (hg_gemm_ring2_body.h): 2 = hi + lo in, hi + lo out; 3 = hi + lo in, fp32 out.  SCHED::CONSUME: the A operand
// is written by other workgroups of this launch on the same XCD (hg_mlp_pair256.hip): it is fetched past this CU's vector L1 (sc1); the
// caller has waited for the row panel and runs the body on ONE tile per call, so the operand ring never reaches into a panel early.
// The two-phase loop (PH2) under EPI_RESID_LN_F32 exists for such one-tile calls only: no tile follows and no stores are pending at the
// start, so its K-tile kinds are decided at compile time and only the last one carries the residual prefetch (hg_mlp_pair256p.hip).
template <int MF, int EPI, bool PH2, int HL = 0, class SCHED>
__device__ __forceinline__ void gemm_ring_body(const GemmArgs& p, const unsigned a_bytes, const int mode, const SCHED& sc) {
#if defined(__HIP_DEVICE_COMPILE__)   // device-only builtins (buffer resources, LDS DMA): host sees just the stub
    // mode >> 8: the start stagger's estimated cycles per K-tile (0 = off)
    constexpr int BM = 64 * MF, BK = 64;
    constexpr int AH = MF * 4096, BH = 16384;          // bytes per A / W half-tile slot
    constexpr int STAGE = 2 * AH + 2 * BH;
    constexpr int GA = MF / 2, GB = 2;
    static_assert(GA <= 2, "DMA piece helpers cover two pieces per half-tile");
    constexpr int N1 = 2 * GA + 3 * GB, N2 = 3 * GA + 2 * GB;
    constexpr bool RLN = (EPI == EPI_RESID_LN_F32);    // residual + centred fp16 copy + LayerNorm statistics (MF = 4)
    constexpr bool RESID = (EPI == EPI_BIAS_RESID_F32 || EPI == EPI_SCALE_RESID_F32 || RLN);
    // epilogue store instructions per wave (vmcnt immediates are 6 bits: anything above is clamped, i.e. stricter)
    // (fp16 outputs leave as paired 16-byte stores: half as many; counting too many here would let the first waits of
    // the next tile pass before its operands have landed)
    constexpr bool F16_STORES = (EPI == EPI_BIAS_F16 || EPI == EPI_BIAS_QGELU_F16 || EPI == EPI_BIAS_RELU_F16 ||
                                 EPI == EPI_LN_BIAS_F16 || EPI == EPI_LN_BIAS_QGELU_F16);
    constexpr bool IN_HL = (HL == 2 || HL == 3), OUT_HL = (HL == 2);
    static_assert(HL == 0 || (IN_HL && RLN && MF == 4), "hi / lo stream: EPI_RESID_LN_F32 on 256 rows, hl 2 or 3");
    // ONE: PH2 on a one-tile call (SCHED::CONSUME).  The stream ends with the tile, the bias staging above the prologue has drained
    // every older store: `more` and `post` are constants, and the waits of the last two K-tiles count what is really behind them
    constexpr bool ONE = PH2 && SCHED::CONSUME;
    static_assert(!(PH2 && RLN) || (ONE && MF == 4), "two-phase loop under EPI_RESID_LN_F32: one tile per call, 256 rows");
    // (HL: per pair of row tiles 4 copy + 2 statistics stores and 4 lo or 16 fp32 stores, four pairs)
    constexpr int E_RAW = IN_HL ? (OUT_HL ? 40 : 88) : RLN ? 8 * MF + 4 * MF + 2 * MF : (F16_STORES ? 4 * MF : 8 * MF);
    constexpr int E = E_RAW > 52 ? 52 : E_RAW;
    // RESID at MF = 2: the residual rows are fetched one K-tile before the epilogue (64 spare VGPRs)
    constexpr bool XPRE = RESID && MF == 2;
    // folded LayerNorm (EPI_LN_*): (mean, rstd) of this lane's 2*MF rows are fetched one K-tile ahead as well
    constexpr bool LNC = (EPI == EPI_LN_BIAS_F16 || EPI == EPI_LN_BIAS_QGELU_F16);
    // RESID at MF = 4: no room for all 32 residual chunks; a rolling window of ROLL_W chunks (f32x4 per lane) is
    // filled one K-tile before the epilogue and refilled as the epilogue consumes it (the fragment registers are
    // dead by then, the accumulators die chunk by chunk)
    constexpr bool ROLL = RESID && MF == 4;
    constexpr int ROLL_W = RLN ? 6 : 8;               // 8 with the LayerNorm extras spills 3 VGPRs
    // (HL: the first pair of row tiles' 4 hi + 4 lo pieces and their 2 + 2 centres)
    constexpr int R = XPRE ? E : (IN_HL ? 12 : ROLL ? ROLL_W + (RLN ? 1 : 0) : 0);   // prefetch loads per wave in the last K-tile
    // PUB (SCHED::PUBLISH, the MLP pair kernel's c_fc): the output tile is handed to OTHER workgroups of this launch, all of them ON THE
    // SAME XCD (the schedule deals a row panel's producers and consumers to one hardware XCC id, hg_mlp_pair.hip): plain stores.  Every
    // wave's stores of tile r have retired, i.e. are in that XCD's L2, once it has passed the counted wait of the first phase of the
    // second K-tile of tile r + 1 (ten operations issued behind the stores, at most eight outstanding); the two barriers of that phase
    // tell wave 0 that all eight waves have (waves 4-7 run one barrier behind), and wave 0 then adds 1 to the row panel's ready counter
    // (sc.publish) - no drain of the operand ring, one atomic per tile.  Behind the last tile of a segment: drain, barrier, publish.
    // The atomic is one more operation in wave 0's vmcnt stream: K-tile kinds 4 / 5 (the second and third K-tile of a tile) run the two
    // waits it is younger than with one more allowed.  (Per-wave atomics - 96 per panel - cost 14 us per launch; stored write-through
    // (sc1) for consumers behind another L2 the epilogue costs 50 us per launch: profiles/r06_mlp_pair.txt.)
    constexpr bool PUB = SCHED::PUBLISH;
    static_assert(!PUB || (PH2 && (EPI == EPI_LN_BIAS_F16 || EPI == EPI_LN_BIAS_QGELU_F16)), "hand-off: two-phase loop, fp16 LayerNorm-fold epilogues");
    constexpr int BIAS_OFF = 2 * STAGE;                // bias[N] (and cs[N] for EPI_LN_*) staged in LDS behind the ring
    const int MR_OFF = BIAS_OFF + 2 * p.N * 4;         // EPI_LN_*: (mean, rstd) of the tile's BM rows, 8 B each
    extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef HG_STAMPS
    unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_beg = 0, t_all = 0;
#endif
    // (the MLP pair kernel's schedules rebuild the thread id from the wave index and v_mbcnt, behind an opaque move: threadIdx.x itself
    // would have to stay in v0 across the other body, and with v0 / v1 taken every register tuple of this body - accumulators, fragments -
    // starts at 2 (mod 4) instead of 0: the same K loop then runs 6 % slower (profiles/r06_mlp_pair.txt))
    const int tid = sc.thread_id();
    int lane = tid & 63;      // (ONE: rebuilt behind the steady-state loop, see there)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int nk = p.K / BK;

    // ---- this workgroup's tiles come from the schedule `sc`: RingTileList (hg_gemm_dev.h) for the stand-alone kernels - XCD-contiguous
    // chunks of an n-group-major list, tiles slot, slot + cpx, ... -; the MLP pair kernel (hg_mlp_pair.hip) deals row-panel-progressive
    // lists and hands finished row panels to its c_proj tiles (SCHED::PUBLISH)
    const int bid = blockIdx.x;
    const int n_items = sc.n_items();
    const int my_tiles = n_items;
    const int tiles_m_all = (p.M + BM - 1) / BM;
    // item e of this workgroup: its tile (every item sweeps all of K)
    auto item_get = [&](int e, int& tm, int& tn, int& kb, int& ke) {
        kb = 0;
        ke = nk;
        sc.tile(e, tm, tn);
    };
    // De-synchronised epilogues: all tiles take the same time, so every CU would store (and, for the residual
    // epilogue, load) its output tile at the same moment - HBM idles during the K loops and saturates during
    // the epilogues.  Workgroups that own one tile fewer than the fullest ones have a tile time of slack; they
    // spend a pseudo-random fraction of it BEFORE their first tile instead of after their last.
    {
        const int dunit = mode >> 8;                               // estimated cycles per K-tile, 0 = off
        const int slack = sc.slack();                              // tiles fewer than the fullest workgroups own
        if (dunit > 0 && slack > 0) {
            const unsigned h = ((unsigned)bid * 2654435761u) >> 24;   // 0..255
            const long long d = ((long long)slack * nk * dunit * h) >> 8;
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            while ((long long)(__builtin_amdgcn_s_memtime() - t0) < d) __builtin_amdgcn_s_sleep(32);
        }
    }
    const int S = my_tiles * nk;                   // K-tiles in this workgroup's stream

    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, (unsigned)((size_t)p.N * p.K * 2), 0x00020000);

    const __amdgpu_buffer_rsrc_t rsM = __builtin_amdgcn_make_buffer_rsrc(
        (void*)p.mr, 0, LNC ? (unsigned)((size_t)tiles_m_all * BM * 8) : 0u, 0x00020000);
    // ---- DMA source offsets (bytes, per lane; identical for every tile and K-step)
    int voffA[2][GA], voffW[2][GB];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < GA; ++i) {
            const int row = (wave * GA + i) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            voffA[h][i] = (h * (BM / 2) + row) * p.lda * 2 + c * 16 - i * 1024;
        }
#pragma unroll
        for (int i = 0; i < GB; ++i) {
            const int row = (wave * GB + i) * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            // fp16-output kernels: LDS row `row` of W half h holds output column (row/32)*64 + 16*((row%16)/4) +
            // 4*(2h + (row%32)/16) + row%4 of the tile, so that wave wn owns the 64 CONSECUTIVE columns wn*64.. and a
            // lane's four MFMA blocks (hb, g2) hold 16 consecutive ones: rows leave as whole 128-byte lines (epilogue)
            const int src = F16_STORES ? (row >> 5) * 64 + 16 * ((row & 15) >> 2) + 4 * (2 * h + ((row & 31) >> 4)) + (row & 3)
                                       : h * 128 + row;
            voffW[h][i] = src * p.K * 2 + c * 16 - i * 1024;
        }
    }
    // ---- load-stream state (wave-uniform): position ld_g, its tile origin and K offset
    int ld_g = -1, ld_kt = nk - 1, ld_ke = nk, ld_r = -1, ld_sA = 0, ld_sW = 0, ld_buf = 0;
    // WRAP: 0 = the stream stays inside its tile, 1 = it moves to the next tile, 2 = decide at run time.  In the
    // two-phase loop the stream (two K-tiles ahead) wraps exactly when K-tile nk-2 is consumed.
    auto ld_advance = [&](auto WRAP_T) {
        constexpr int WRAP = decltype(WRAP_T)::value;
        ++ld_g;
        ++ld_kt;
        if (WRAP == 1 || (WRAP == 2 && ld_kt == ld_ke)) {
            ++ld_r;
            int tm, tn;
            item_get(ld_r, tm, tn, ld_kt, ld_ke);
            ld_sA = tm * BM * p.lda * 2;
            ld_sW = tn * 256 * p.K * 2;
        }
        ld_buf = (ld_g & 1) * STAGE;
    };
    // pieces [i0, i1) of a half-tile (interleaving the pieces with the segment's LDS reads was measured: no
    // gain).  All pieces of a half-tile share one M0 (LDS base): piece i adds its
    // 1 KiB through the instruction's immediate offset, which the hardware also adds to the global address,
    // so voff*[h][i] carry -1024 * i
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    auto dma_A = [&](int h, auto I) {
        constexpr int i = decltype(I)::value;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (HG_LDS void*)(smem + ld_buf + h * AH + wave * GA * 1024), 16,
                                                 voffA[h][i], ld_sA + ld_kt * (BK * 2), i * 1024, SCHED::CONSUME ? 16 /* sc1 */ : 0);
    };
    auto dma_W = [&](int h, auto I) {
        constexpr int i = decltype(I)::value;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (HG_LDS void*)(smem + ld_buf + 2 * AH + h * BH + wave * GB * 1024),
                                                 16, voffW[h][i], ld_sW + ld_kt * (BK * 2), i * 1024, 0);
    };
    auto issue_A = [&](int h, int i0, int i1) {
        if (i0 <= 0 && 0 < i1) dma_A(h, P0{});
        if constexpr (GA > 1) {
            if (i0 <= 1 && 1 < i1) dma_A(h, P1{});
        }
    };
    auto issue_W = [&](int h, int i0, int i1) {
        if (i0 <= 0 && 0 < i1) dma_W(h, P0{});
        if (i0 <= 1 && 1 < i1) dma_W(h, P1{});
    };

    // ---- fragment read offsets
    const int sw = (lane >> 1) & 7;
    int coff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) coff[ks] = ((ks * 4 + (lane >> 4)) ^ sw) << 4;
    const int a_row = (wm * MF * 16 + (lane & 15)) * 128;
    const int w_row = 2 * AH + (wn * 32 + (lane & 15)) * 128;

    // Fragment registers: one A set (half 0 in P1-P2, half 1 in P3-P4) and both W halves.
    half8 xa[MF][2], wb[2][2][2];
    auto read_A = [&](int h, int buf) {
#pragma unroll
        for (int f = 0; f < MF; ++f)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                xa[f][ks] = *reinterpret_cast<const half8*>(smem + buf + h * AH + a_row + f * 2048 + coff[ks]);
    };
    auto read_W = [&](auto H, int buf) {
        constexpr int h = decltype(H)::value;
#pragma unroll
        for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
                wb[h][g2][ks] = *reinterpret_cast<const half8*>(smem + buf + h * BH + w_row + g2 * 2048 + coff[ks]);
    };

    // (ONE) the same reads into fixed tuples (ds_read_fixed): LDS addresses, the ring's base included
    auto read_A_fixed = [&](auto H, int buf) {
        constexpr int h = decltype(H)::value;
        const int base = (int)(unsigned)(__SIZE_TYPE__)(HG_LDS char*)smem + buf + a_row;
        static_for<2 * MF>([&](auto I) {
            constexpr int f = decltype(I)::value >> 1, ks = decltype(I)::value & 1;
            if constexpr (MF == 4) ds_read_fixed<f * 2 + ks, h * AH + f * 2048>(xa[f][ks], base + coff[ks]);
        });
    };
    auto read_W_fixed = [&](auto H, int buf) {
        constexpr int h = decltype(H)::value;
        const int base = (int)(unsigned)(__SIZE_TYPE__)(HG_LDS char*)smem + buf + w_row;
        static_for<4>([&](auto I) {
            constexpr int g2 = decltype(I)::value >> 1, ks = decltype(I)::value & 1;
            ds_read_fixed<8 + h * 4 + g2 * 2 + ks, h * BH + g2 * 2048>(wb[h][g2][ks], base + coff[ks]);
        });
    };

    f32x4 acc[2][2][MF][2];
    auto zero_acc = [&]() {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int f = 0; f < MF; ++f)
#pragma unroll
                    for (int g2 = 0; g2 < 2; ++g2) acc[a][b][f][g2] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto mma = [&](auto HA, auto HB) {
        constexpr int ha = decltype(HA)::value, hb = decltype(HB)::value;
        // (A branch that is never taken, kept on purpose: without it clang allocates the two-phase 256 x 256 instances' registers
        // differently, and the MLP pair kernel, which holds this body, spills 2 VGPRs to scratch.  It is the last trace of a timing
        // experiment that ran without MFMAs; leave it until the pair kernel no longer depends on it.)
        constexpr int no_mfma = 0;
        if (no_mfma) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int f = 0; f < MF; ++f) asm volatile("" ::"v"(xa[f][ks]));
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) asm volatile("" ::"v"(wb[hb][g2][ks]));
            }
            return;
        }
        SEG_B(3);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2)
                    acc[ha][hb][f][g2] =
                        __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[hb][g2][ks], xa[f][ks], acc[ha][hb][f][g2], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        SEG_E(3);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    // end of a fetch segment: this wave's fragment reads are complete, then the workgroup barrier; the
    // sched_barrier keeps the compiler from hoisting the (register-only) MFMAs into the fetch segment
    auto sync_fetch = [&]() {
        // the builtin (not inline asm) so that the compiler's waitcnt pass knows the LDS reads have returned:
        // with an opaque asm it keeps them on its scoreboard and throttles the next segment's ds_reads
        SEG_B(1);
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
        SEG_E(1);
        SEG_B(2);
        barrier_raw();
        SEG_E(2);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto sync_mma = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        SEG_B(4);
        barrier_raw();
        SEG_E(4);
    };

    // ---- bias -> LDS once per workgroup (epilogue reads must not touch vmcnt: a register-returning
    // global load would wait for every older DMA of the ring)
    {
        const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < p.N / 4; i += 512) {
            *reinterpret_cast<f32x4*>(smem + BIAS_OFF + i * 16) = p.bias ? reinterpret_cast<const f32x4*>(p.bias)[i] : z;
            if constexpr (LNC)
                *reinterpret_cast<f32x4*>(smem + BIAS_OFF + p.N * 4 + i * 16) = reinterpret_cast<const f32x4*>(p.cs)[i];
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    }
    // ---- prologue: stream positions 0 and 1 (A1 of position 1 is issued in the first P1)
    ld_advance(std::integral_constant<int, 2>{});
    issue_A(0, 0, GA); issue_W(0, 0, GB); issue_W(1, 0, GB); issue_A(1, 0, GA);
    if (S > 1) {
        ld_advance(std::integral_constant<int, 2>{});
        issue_A(0, 0, GA); issue_W(0, 0, GB); issue_W(1, 0, GB);
        if constexpr (PH2) wait_vm<2 * GA + 2 * GB>();   // A0, W0, W1 of position 0 landed
        else wait_vm<N1>();                // A0, W0 of position 0 landed
    } else {
        if constexpr (PH2) wait_vm<GA>();
        else wait_vm<GA + GB>();
    }
    barrier_raw();
    // Stagger: waves 4-7 (the second wave of every SIMD) run one barrier interval behind waves 0-3, so a
    // SIMD always has one wave in a fetch segment (LDS reads, DMA issue, waits) and one in an MFMA segment.
    const bool late = wave >= 4;
    if (late) barrier_raw();

#ifdef HG_STAMPS
    t_all = __builtin_amdgcn_s_memtime();
#endif
    int g = 0;
    // the previous tile lay inside M, i.e. issued every one of its E epilogue stores (a ragged tile may skip store
    // instructions whose rows are all masked: the waits that follow it then do not allow for any)
    bool prev_full = false;
    int tm_prev = 0;                               // (PUB) row panel of the previous tile: published in this tile's second K-tile
    (void)tm_prev;
    for (int r = 0; r < n_items; ++r) {
        int tm, tn, kb_r, ke_r;
        item_get(r, tm, tn, kb_r, ke_r);
        const int klen = nk;
        const int m0 = tm * BM, n0 = tn * 256;
        const bool post_ok = prev_full;
        prev_full = m0 + BM <= p.M;
        zero_acc();
        f32x4 xres[XPRE ? 2 : 1][XPRE ? 2 : 1][XPRE ? MF : 1][XPRE ? 2 : 1];
        // rolling residual window (ROLL): chunk c = ((ha * MF + f) * 2 + hb) * 2 + g2 is this lane's f32x4 of row
        // m0 + ha*BM/2 + wm*MF*16 + f*16 + (lane&15), columns n0 + hb*128 + wn*32 + g2*16 + 4*(lane>>4)
        f32x4 xw[ROLL && !IN_HL ? ROLL_W : 1];
        float muw[RLN ? 2 : 1];
        // (HL) the stream comes in as in the 128 x 256 kernel, whose tile (2 tm + ha, tn) a half ha of this tile is: a pair of row tiles
        // f = 2 fp, 2 fp + 1 of this wave is what that kernel's wave fp * 4 + wn holds in its half wm.  Unit u = ha * 2 + fp: hi as
        // paired 16-byte pieces of the row-major copy, lo as that wave's own pieces, the rows' old and new centres.  One unit is held
        // at a time: the first is fetched in the last K-tile, the next one while a unit is worked on.
        typedef unsigned u32x4_hl __attribute__((ext_vector_type(4)));
        typedef unsigned u32x2_hl __attribute__((ext_vector_type(2)));
        u32x4_hl xhi[IN_HL ? 2 : 1][IN_HL ? 2 : 1];      // [hb][g2]
        u32x2_hl xlo[IN_HL ? 2 : 1][IN_HL ? 2 : 1];
        float muv[IN_HL ? 2 : 1], mucv[IN_HL ? 2 : 1];  // [f & 1]
        const int tiles_n = p.N / 256;
        auto lo_ptr = [&](int u, int hb, int g2) {
            return p.lo + ((((size_t)(2 * tm + (u >> 1)) * tiles_n + tn) * 8 + ((u & 1) * 4 + wn)) * 8 + (wm * 4 + hb * 2 + g2)) * 256 + lane * 4;
        };
        auto unit_load = [&](int u) {
            const int qq = lane >> 4;
            const int mb = m0 + (u >> 1) * (BM / 2) + wm * MF * 16 + (u & 1) * 32 + (lane & 15);
            int mp = mb + ((qq & 1) ? 16 : 0);
            mp = mp < p.M ? mp : p.M - 1;
#pragma unroll
            for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) {
                    xhi[hb][g2] = *reinterpret_cast<const u32x4_hl*>(p.out2 + (size_t)mp * p.ld2 + n0 + hb * 128 + wn * 32 + g2 * 16 + 4 * (qq & ~1));
                    xlo[hb][g2] = *reinterpret_cast<const u32x2_hl*>(lo_ptr(u, hb, g2));
                }
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                int m = mb + f * 16;
                m = m < p.M ? m : p.M - 1;
                muv[f] = p.mu[m];
                mucv[f] = p.muc[m];
            }
        };
        auto chunk_row = [&](int rg) {
            int m = m0 + (rg / MF) * (BM / 2) + wm * MF * 16 + (rg % MF) * 16 + (lane & 15);
            return m < p.M ? m : p.M - 1;
        };
        auto chunk_load = [&](int c) {
            const int rg = c >> 2, hb = (c >> 1) & 1, g2 = c & 1;
            const int n = n0 + hb * 128 + wn * 32 + g2 * 16 + 4 * (lane >> 4);
            return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.out) + (size_t)chunk_row(rg) * p.ldc + n);
        };
        // One K-tile of the two-phase schedule.  KIND: 0 middle, 1 first of a tile (the previous epilogue's stores may be
        // pending), 2 second to last (LayerNorm statistics DMA), 3 last (residual prefetch).  K >= 256 makes the four
        // kinds distinct K-tiles, and every K-tile before the last two of a tile has two successors in the stream, so
        // the middle of the loop carries no run-time conditions at all.
        // (PUB) 4 / 5: the second / third K-tile of a tile - middle K-tiles that publish the previous tile (`pub`: there is one) / still
        // have its atomic among the NP + 1 youngest operations of the stream
        auto ph2_ktile = [&](auto KIND_T) {
            constexpr int KINDX = decltype(KIND_T)::value;
            constexpr int KIND = KINDX >= 4 ? 0 : KINDX;
            const int buf = (g & 1) * STAGE;
            const bool post = !ONE && post_ok;
            const bool more = KIND < 2 || (!ONE && r + 1 < n_items);       // a K-tile two positions ahead exists
            const bool pub = PUB && r > 0 && wave == 0;      // this wave publishes the previous tile
            (void)post; (void)more; (void)pub;
            // Two phases per K-tile (32 MFMAs per segment, half the barriers):
            //   PA: fetch A0 W0 W1 (t); refill A1(t+1);               wait -> A1(t) landed;        quadrants (0,0) (0,1)
            //   PB: fetch A1 (t);       refill A0 W0 W1 (t+2);         wait -> A0 W0 W1 (t+1) landed; quadrants (1,1) (1,0)
            // both waits leave NP = 2GA+2GB DMA instructions (64 KiB per CU) in flight
            constexpr int NP = 2 * GA + 2 * GB;
            if constexpr (ONE) {
                read_A_fixed(I0{}, buf);
                read_W_fixed(I0{}, buf);
                read_W_fixed(I1{}, buf);
            } else {
                read_A(0, buf);
                read_W(I0{}, buf);
                read_W(I1{}, buf);
            }
            if constexpr (LNC && KIND == 2) {
                if (lane < BM / 16)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsM, (HG_LDS void*)(smem + MR_OFF + wave * BM), 16, lane * 16,
                                                             (m0 + wave * (BM / 8)) * 8, 0, 0);
            }
            if (KIND < 3 || more) issue_A(1, 0, GA);      // A1 of position g+1 exists unless the stream ends here
            if constexpr (IN_HL && KIND == 3) unit_load(0);      // (xa, both W halves and this unit fit: 256 VGPRs, none spilled)
            if constexpr (ROLL && !IN_HL && KIND == 3) {
                {      // first ROLL_W residual chunks (+ the first row group's centre) of this tile
#pragma unroll
                    for (int c = 0; c < ROLL_W; ++c) xw[c] = chunk_load(c);
                    if constexpr (RLN) muw[0] = p.mu[chunk_row(0)];
                }
            }
            if constexpr (XPRE && KIND == 3) {
                {
#pragma unroll
                    for (int ha = 0; ha < 2; ++ha)
#pragma unroll
                        for (int f = 0; f < MF; ++f) {
                            int m = m0 + ha * (BM / 2) + wm * MF * 16 + f * 16 + (lane & 15);
                            m = m < p.M ? m : p.M - 1;
#pragma unroll
                            for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                                for (int g2 = 0; g2 < 2; ++g2) {
                                    const int n = n0 + hb * 128 + wn * 32 + g2 * 16 + 4 * (lane >> 4);
                                    xres[ha][hb][f][g2] = *reinterpret_cast<const f32x4*>(
                                        reinterpret_cast<const float*>(p.out) + (size_t)m * p.ldc + n);
                                }
                        }
                }
            }
            SEG_B(0);
            if constexpr (KINDX == 5) { if (pub) wait_vm<NP + 1>(); else wait_vm<NP>(); }
            else if constexpr (KIND == 0) wait_vm<NP>();
            else if constexpr (KIND == 1) { if (post) wait_vm<NP + E>(); else wait_vm<NP>(); }
            else if constexpr (KIND == 2) { if (more) wait_vm<NP>(); else wait_vm<ONE ? NP : 0>(); }      // (ONE: A1 of the last K-tile is behind it)
            else { if (more) wait_vm<NP + R>(); else wait_vm<ONE ? R : 0>(); }      // (ONE: only the prefetch is younger)
            SEG_E(0);
            sync_fetch();
            mma(I0{}, I0{});
            mma(I0{}, I1{});
            sync_mma();
            if constexpr (KINDX == 4) {
                // every wave has passed this phase's wait: the previous tile's stores have all retired
                if (pub) sc.publish(tm_prev, lane);
            }
            if constexpr (ONE) read_A_fixed(I1{}, buf);
            else read_A(1, buf);
            if (KIND < 2 || more) { ld_advance(std::integral_constant<int, KIND == 2 ? 1 : 0>{}); issue_A(0, 0, GA); issue_W(0, 0, GB); issue_W(1, 0, GB); }
            SEG_B(0);
            if constexpr (KINDX == 4) { if (pub) wait_vm<NP + 1>(); else wait_vm<NP>(); }
            else if constexpr (KIND == 0) wait_vm<NP>();
            else if constexpr (KIND == 1) { if (post) wait_vm<NP + E>(); else wait_vm<NP>(); }
            else if constexpr (KIND == 2) { if (more) wait_vm<NP>(); else wait_vm<ONE ? GA : 0>(); }      // (ONE: A1 of the last K-tile may still fly)
            else { if (more) wait_vm<NP + R>(); else if constexpr (!ONE) wait_vm<0>(); }      // (ONE: every operand has landed, the prefetch flies on)
            SEG_E(0);
            sync_fetch();
            mma(I1{}, I1{});
            mma(I1{}, I0{});
            sync_mma();
            ++g;
        };
        if constexpr (PH2) {
            using K0 = std::integral_constant<int, 0>;
            using K1 = std::integral_constant<int, 1>;
            using K2 = std::integral_constant<int, 2>;
            using K3 = std::integral_constant<int, 3>;
            ph2_ktile(K1{});
            if constexpr (PUB) {
                ph2_ktile(std::integral_constant<int, 4>{});
                ph2_ktile(std::integral_constant<int, 5>{});
            }
            for (int kt = PUB ? 3 : 1; kt < klen - 2; ++kt) {
                ph2_ktile(K0{});
            }
            // (ONE) the lane number again, from an opaque thread id (Pair256ProjSchedT<true>): what the prefetch and the epilogue derive from
            // it - row and column offsets, 64-bit addresses - is then worked out HERE and not held in VGPRs across the loop, which has
            // 64 of them fewer with the fragments in fixed tuples (the hi / lo -> fp32 instance spilled one)
            if constexpr (ONE) lane = sc.thread_id() & 63;
            ph2_ktile(K2{});
            ph2_ktile(K3{});
            if constexpr (ONE) asm volatile("" : "+v"(lane));      // (and once more: the epilogue's own addresses are not held across the last K-tiles)
        } else {
        for (int kt = 0; kt < klen; ++kt, ++g) {
            const int buf = (g & 1) * STAGE;
            const bool more = g + 2 < S;          // a K-tile two positions ahead exists
            const bool post = post_ok;             // epilogue stores of the previous tile may still be pending
            const bool xl = (XPRE || ROLL) && kt == klen - 1;  // residual rows are fetched during the last K-tile
            // ---------------- P1: fetch A0(t), W0(t); refill A1(t+1); then quadrant (0,0)
            read_A(0, buf);
            read_W(I0{}, buf);
            if constexpr (LNC) {
                // (mean, rstd) of this tile's rows -> LDS, one small DMA per wave (BM/8 rows x 8 B), a K-tile
                // ahead of the last one: by the last P4's counted wait it is more than N1 operations old, and that
                // phase's barriers publish it to every wave before the epilogue (the waits run one operation
                // stricter until it has retired)
                if (kt == klen - 2 && lane < BM / 16)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsM, (HG_LDS void*)(smem + MR_OFF + wave * BM), 16, lane * 16,
                                                             (m0 + wave * (BM / 8)) * 8, 0, 0);
            }
            if (g + 1 < S) issue_A(1, 0, GA);     // A1 of position g+1 (ld state already at g+1)
            if constexpr (IN_HL) {
                if (xl) unit_load(0);
            } else if constexpr (ROLL) {
                if (xl) {      // first ROLL_W residual chunks (+ the first row group's centre) of this tile
#pragma unroll
                    for (int c = 0; c < ROLL_W; ++c) xw[c] = chunk_load(c);
                    if constexpr (RLN) muw[0] = p.mu[chunk_row(0)];
                }
            }
            if constexpr (XPRE) {
                if (xl) {
#pragma unroll
                    for (int ha = 0; ha < 2; ++ha)
#pragma unroll
                        for (int f = 0; f < MF; ++f) {
                            int m = m0 + ha * (BM / 2) + wm * MF * 16 + f * 16 + (lane & 15);
                            m = m < p.M ? m : p.M - 1;
#pragma unroll
                            for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                                for (int g2 = 0; g2 < 2; ++g2) {
                                    const int n = n0 + hb * 128 + wn * 32 + g2 * 16 + 4 * (lane >> 4);
                                    xres[ha][hb][f][g2] = *reinterpret_cast<const f32x4*>(
                                        reinterpret_cast<const float*>(p.out) + (size_t)m * p.ldc + n);
                                }
                        }
                }
            }
            SEG_B(0);
            if (!more) wait_vm<0>();              // -> W1(t) landed (read in P2)
            else if (xl) wait_vm<N2 + R>();
            else if (post && kt <= 1) wait_vm<N2 + E>();
            else wait_vm<N2>();
            SEG_E(0);
            sync_fetch();
            mma(I0{}, I0{});
            sync_mma();
            // ---------------- P2: fetch W1(t); slot A0(t) is free -> A0(t+2); quadrant (0,1)
            read_W(I1{}, buf);
            if (more) { ld_advance(std::integral_constant<int, 2>{}); issue_A(0, 0, GA); }
            SEG_B(0);
            if (!more) wait_vm<0>();              // -> A1(t) landed (read in P3)
            else if (xl) wait_vm<N2 + R>();
            else if (post && kt == 0) wait_vm<N2 + E>();
            else wait_vm<N2>();
            SEG_E(0);
            sync_fetch();
            mma(I0{}, I1{});
            sync_mma();
            // ---------------- P3: fetch A1(t); slot W0(t) free -> W0(t+2); quadrant (1,1)
            read_A(1, buf);
            if (more) issue_W(0, 0, GB);
            sync_fetch();
            mma(I1{}, I1{});
            sync_mma();
            // ---------------- P4: slot W1(t) free -> W1(t+2); quadrant (1,0)
            if (more) issue_W(1, 0, GB);
            SEG_B(0);
            if (!more) wait_vm<0>();              // -> A0(t+1), W0(t+1) landed (read in the next P1)
            else if (xl) wait_vm<N1 + R>();
            else if (post && kt == 0) wait_vm<N1 + E>();
            else wait_vm<N1>();
            SEG_E(0);
            sync_fetch();
            mma(I1{}, I0{});
            sync_mma();
                            }
        }
        // ---------------- epilogue of tile r (the ring keeps prefetching the next tile meanwhile)
        SEG_B(7);
        constexpr bool F16OUT = (EPI == EPI_BIAS_F16 || EPI == EPI_BIAS_QGELU_F16 || EPI == EPI_BIAS_RELU_F16 || LNC);
        if constexpr (F16OUT) {
            // fp16 outputs: a lane holds 4 consecutive columns (8 B) of one row.  v_permlane16_swap pairs the
            // accumulator tiles f, f+1 (same columns, rows 16 apart) so that even 16-lane groups end up with 8
            // consecutive columns of tile f's row and odd groups with 8 of tile f+1's row: 16-byte stores,
            // half the store instructions (the tail is store-issue bound).
            // tiles that lie entirely inside M (all of them at M = 197 * 256) skip the per-store row masks
            auto f16_epilogue = [&](auto INTERIOR_T) {
            constexpr bool INTERIOR = decltype(INTERIOR_T)::value;
            const int q = lane >> 4, r16 = lane & 15;
            half_t* outp = reinterpret_cast<half_t*>(p.out);
            f32x4 gk = {0.f, 0.f, 0.f, 0.f};
            if constexpr (EPI == EPI_BIAS_QGELU_F16 || EPI == EPI_LN_BIAS_QGELU_F16) gk = quick_gelu_consts();
            (void)gk;
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            // Column map (see voffW): acc[ha][hb][f][g2] of lane (r16, q) = row ha*BM/2 + wm*MF*16 + f*16 + r16, columns
            // wn*64 + 16q + 4(2hb + g2) + 0..3: the lane's four blocks are 16 consecutive columns = 32 bytes of fp16,
            // a row's 64 columns sit in its four q lanes.  A store instruction that touches 32 partial lines holds the
            // CU's store path for 72 cycles, one that writes 8 whole lines for 17 (tools/ubench/store_path.hip), so rows
            // r16 and r16 ^ 8 trade halves through a row_ror:8 DPP move: lanes r16 < 8 keep columns +0..7 and receive
            // +0..7 of row r16 + 8, lanes r16 >= 8 receive +8..15 of row r16 - 8 and keep their own +8..15; the first
            // store then writes rows 0..7 of the 16-row block and the second rows 8..15, eight lanes (128 B) per row.
            // Bias (and folded-weight column sums) of the lane's 16 columns are read once per tile.
            f32x4 bv[4], cv[4];
            const int nq = n0 + wn * 64 + 16 * q;
#pragma unroll
            for (int b4 = 0; b4 < 4; ++b4) {
                bv[b4] = *reinterpret_cast<const f32x4*>(smem + BIAS_OFF + (nq + 4 * b4) * 4);
                if constexpr (LNC) cv[b4] = *reinterpret_cast<const f32x4*>(smem + BIAS_OFF + p.N * 4 + (nq + 4 * b4) * 4);
                else cv[b4] = bv[b4];
            }
            auto cvt2 = [](float a, float b) {      // RNE, one v_cvt_pk_f16_f32
                const half2v h = __builtin_convertvector(f32x2{a, b}, half2v);
                return __builtin_bit_cast(unsigned, h);
            };
            const bool low = r16 < 8;
            // byte offset of this lane's 16-byte piece inside a row: columns wn*64 + 8 * (2q + (r16 >> 3))
            half_t* colp = outp + n0 + wn * 64 + 8 * (2 * q + (r16 >> 3));
#pragma unroll
            for (int ha = 0; ha < 2; ++ha)
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    const int mb = m0 + ha * (BM / 2) + wm * MF * 16 + f * 16;      // first row of the 16-row block
                    f32x2 mr = {0.f, 1.f};                                           // (mean, rstd) of row mb + r16
                    if constexpr (LNC) mr = *reinterpret_cast<const f32x2*>(smem + MR_OFF + (mb + r16 - m0) * 8);
                    unsigned d[8];
#pragma unroll
                    for (int b4 = 0; b4 < 4; ++b4) {
                        f32x4 v;
                        if constexpr (LNC) v = (acc[ha][b4 >> 1][f][b4 & 1] - cv[b4] * mr[0]) * mr[1] + bv[b4];   // rstd * (acc - mean * cs) + bias'
                        else v = acc[ha][b4 >> 1][f][b4 & 1] + bv[b4];
                        if constexpr (EPI == EPI_BIAS_QGELU_F16 || EPI == EPI_LN_BIAS_QGELU_F16) v = quick_gelu4(v, gk);
                        if constexpr (EPI == EPI_BIAS_RELU_F16) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                        }
                        d[2 * b4] = cvt2(v[0], v[1]);
                        d[2 * b4 + 1] = cvt2(v[2], v[3]);
                    }
                    u32x4 st0, st1;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned send = low ? d[4 + j] : d[j];
                        const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0x128, 0xF, 0xF, false);   // row_ror:8
                        st0[j] = low ? d[j] : recv;
                        st1[j] = low ? recv : d[4 + j];
                    }
                    const int row0 = mb + (r16 & 7);
                    if (INTERIOR || row0 < p.M) *reinterpret_cast<u32x4*>(colp + (size_t)row0 * p.ldc) = st0;
                    if (INTERIOR || row0 + 8 < p.M) *reinterpret_cast<u32x4*>(colp + (size_t)(row0 + 8) * p.ldc) = st1;
                }
            };
            if (m0 + BM <= p.M) f16_epilogue(std::true_type{});
            else f16_epilogue(std::false_type{});
        } else if constexpr (IN_HL) {
            // the 128 x 256 kernel's epilogue (hg_gemm_ring2_body.h), unit by unit: the same expressions in the same order on the same
            // accumulator bits, so a row leaves with the bits that kernel gives it - stream, copy, partial statistics and lo bytes
            const int q = lane >> 4;
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            const int sg = tn * 4 + wn;                     // column group of this wave
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ha = u >> 1, fp = u & 1;
                if (m0 + ha * (BM / 2) >= p.M) break;      // (the chip's last panel may have one 128-row half only: no such tile, no lo bytes)
                half4 hin[2][2][2];                        // [f][hb][g2]
                u32x2 lraw[2][2];
                float mu_u[2], muc_u[2];
#pragma unroll
                for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                    for (int g2 = 0; g2 < 2; ++g2) {
                        const u32x4 o = xhi[hb][g2];
                        const auto s0 = __builtin_amdgcn_permlane16_swap(o[0], o[2], false, false);
                        const auto s1 = __builtin_amdgcn_permlane16_swap(o[1], o[3], false, false);
                        hin[0][hb][g2] = __builtin_bit_cast(half4, u32x2{(unsigned)s0[0], (unsigned)s1[0]});
                        hin[1][hb][g2] = __builtin_bit_cast(half4, u32x2{(unsigned)s0[1], (unsigned)s1[1]});
                        lraw[hb][g2] = xlo[hb][g2];
                    }
#pragma unroll
                for (int f = 0; f < 2; ++f) { mu_u[f] = muv[f]; muc_u[f] = mucv[f]; }
                __builtin_amdgcn_sched_barrier(0);
                if (u + 1 < 4 && m0 + ((u + 1) >> 1) * (BM / 2) < p.M) unit_load(u + 1);
                __builtin_amdgcn_sched_barrier(0);
                half4 h16[2][2][2];                         // [f][hb][g2]: the new copy (hi)
                unsigned l8[OUT_HL ? 2 : 1][OUT_HL ? 2 : 1][OUT_HL ? 2 : 1];      // the remainder as four bf8 (e5m2)
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    const int m = m0 + ha * (BM / 2) + wm * MF * 16 + fp * 32 + f * 16 + (lane & 15);
                    f32x4 v[2][2];
                    float sum = 0.f;
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                        for (int g2 = 0; g2 < 2; ++g2) {
                            const int n = n0 + hb * 128 + wn * 32 + g2 * 16 + 4 * q;
                            f32x4 xin, lin;
                            {
                                const auto a = __builtin_amdgcn_cvt_pk_f32_bf8((int)lraw[hb][g2][f], false);
                                const auto b = __builtin_amdgcn_cvt_pk_f32_bf8((int)lraw[hb][g2][f], true);
                                lin = f32x4{a[0], a[1], b[0], b[1]};
                            }
                            const f32x2 mc2 = {muc_u[f], muc_u[f]};
#pragma unroll
                            for (int e2 = 0; e2 < 2; ++e2) {      // (centre + hi) + lo, two elements per instruction
                                const half2v h2 = {hin[f][hb][g2][2 * e2], hin[f][hb][g2][2 * e2 + 1]};
                                const f32x2 ls2 = {1.0f / HG_LO_SCALE, 1.0f / HG_LO_SCALE};
                                const f32x2 x2 = f32x2{lin[2 * e2], lin[2 * e2 + 1]} * ls2 + (mc2 + __builtin_convertvector(h2, f32x2));
                                xin[2 * e2] = x2[0];
                                xin[2 * e2 + 1] = x2[1];
                            }
                            v[hb][g2] = xin + (acc[ha][hb][2 * fp + f][g2] + *reinterpret_cast<const f32x4*>(smem + BIAS_OFF + n * 4));
                            sum += (v[hb][g2][0] + v[hb][g2][1]) + (v[hb][g2][2] + v[hb][g2][3]);
                            if constexpr (!OUT_HL) {
                                if (m < p.M)
                                    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n) = v[hb][g2];
                            }
                            const f32x2 mu2 = {mu_u[f], mu_u[f]};
                            float rem[4];
#pragma unroll
                            for (int e2 = 0; e2 < 2; ++e2) {
                                const f32x2 d = f32x2{v[hb][g2][2 * e2], v[hb][g2][2 * e2 + 1]} - mu2;
                                const half2v hh = __builtin_convertvector(d, half2v);
                                h16[f][hb][g2][2 * e2] = hh[0];
                                h16[f][hb][g2][2 * e2 + 1] = hh[1];
                                if constexpr (OUT_HL) {
                                    const f32x2 r = d - __builtin_convertvector(hh, f32x2);
                                    const f32x2 rs = r * f32x2{HG_LO_SCALE, HG_LO_SCALE};
                                    rem[2 * e2] = rs[0];
                                    rem[2 * e2 + 1] = rs[1];
                                }
                            }
                            if constexpr (OUT_HL) {
                                int w8 = __builtin_amdgcn_cvt_pk_bf8_f32(rem[0], rem[1], 0, false);
                                w8 = __builtin_amdgcn_cvt_pk_bf8_f32(rem[2], rem[3], w8, true);
                                l8[f][hb][g2] = (unsigned)w8;
                            }
                        }
                    sum = sum_rows(sum);
                    const float gm = sum * (1.0f / 64.0f);
                    float m2 = 0.f;
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                        for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
                            for (int e2 = 0; e2 < 2; ++e2) {
                                const f32x2 d = f32x2{v[hb][g2][2 * e2], v[hb][g2][2 * e2 + 1]} - f32x2{gm, gm};
                                m2 = fmaf(d[0], d[0], m2);
                                m2 = fmaf(d[1], d[1], m2);
                            }
                    m2 = sum_rows(m2);
                    if (q == 0 && m < p.M) *reinterpret_cast<f32x2*>(p.stats + ((size_t)m * p.stats_ld + sg) * 2) = f32x2{sum, m2};
                }
                // fp16 copy: pair the row tiles f = 0, 1 through v_permlane16_swap -> 16-byte stores
                const int m = m0 + ha * (BM / 2) + wm * MF * 16 + fp * 32 + (lane & 15) + ((q & 1) ? 16 : 0);
#pragma unroll
                for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                    for (int g2 = 0; g2 < 2; ++g2) {
                        const int nb = n0 + hb * 128 + wn * 32 + g2 * 16;
                        const u32x2 ux = __builtin_bit_cast(u32x2, h16[0][hb][g2]), uy = __builtin_bit_cast(u32x2, h16[1][hb][g2]);
                        const auto s0 = __builtin_amdgcn_permlane16_swap(ux[0], uy[0], false, false);
                        const auto s1 = __builtin_amdgcn_permlane16_swap(ux[1], uy[1], false, false);
                        const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
                        if (m < p.M) *reinterpret_cast<u32x4*>(p.out2 + (size_t)m * p.ld2 + nb + 4 * (q & ~1)) = o;
                        if constexpr (OUT_HL) *reinterpret_cast<u32x2*>(lo_ptr(u, hb, g2)) = u32x2{l8[0][hb][g2], l8[1][hb][g2]};
                    }
            }
        } else if constexpr (ROLL) {
            // residual epilogue through the rolling window: chunk c is consumed, stored, and its window slot is
            // refilled with chunk c + ROLL_W (the sched_barrier keeps the compiler from hoisting the refills)
            const int q = lane >> 4;
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int rg = 0; rg < 2 * MF; ++rg) {
                const int ha = rg / MF, f = rg % MF;
                const int m = m0 + ha * (BM / 2) + wm * MF * 16 + f * 16 + (lane & 15);
                f32x4 v[2][2];
                float mu_r = 0.f;
                if constexpr (RLN) {
                    mu_r = muw[rg & 1];
                    if (rg + 1 < 2 * MF) muw[(rg + 1) & 1] = p.mu[chunk_row(rg + 1)];
                }
#pragma unroll
                for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                    for (int g2 = 0; g2 < 2; ++g2) {
                        const int c = (rg * 2 + hb) * 2 + g2;
                        const int n = n0 + hb * 128 + wn * 32 + g2 * 16 + 4 * q;
                        f32x4 a = acc[ha][hb][f][g2] + *reinterpret_cast<const f32x4*>(smem + BIAS_OFF + n * 4);
                        if constexpr (EPI == EPI_SCALE_RESID_F32) v[hb][g2] = fma4(a, *reinterpret_cast<const f32x4*>(p.pos + n), xw[c % ROLL_W]);
                        else v[hb][g2] = xw[c % ROLL_W] + a;
                        if (m < p.M)
                            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n) = v[hb][g2];
                        if (c + ROLL_W < 8 * MF) xw[c % ROLL_W] = chunk_load(c + ROLL_W);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                if constexpr (RLN) {
                    // per row and per wave column group (64 columns): (sum, sum of squared deviations from the group
                    // mean); fp16 copy centred on the row's previous mean
                    float sum = 0.f;
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                        for (int g2 = 0; g2 < 2; ++g2) sum += (v[hb][g2][0] + v[hb][g2][1]) + (v[hb][g2][2] + v[hb][g2][3]);
                    sum = sum_rows(sum);
                    const float gm = sum * (1.0f / 64.0f);
                    float m2 = 0.f;
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                        for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float d = v[hb][g2][e] - gm;
                                m2 = fmaf(d, d, m2);
                            }
                    m2 = sum_rows(m2);
                    if (q == 0 && m < p.M) {
                        typedef float f32x2 __attribute__((ext_vector_type(2)));
                        *reinterpret_cast<f32x2*>(p.stats + ((size_t)m * p.stats_ld + (n0 / 256) * 4 + wn) * 2) = f32x2{sum, m2};
                    }
                    // fp16 copy: the column blocks g2 = 0, 1 of this row are paired through v_permlane16_swap
                    // (even 16-lane groups end up with 8 consecutive columns of block 0, odd groups of block 1)
#pragma unroll
                    for (int hb = 0; hb < 2; ++hb) {
                        half4 h0, h1;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            h0[e] = (half_t)(v[hb][0][e] - mu_r);
                            h1[e] = (half_t)(v[hb][1][e] - mu_r);
                        }
                        const u32x2 ux = __builtin_bit_cast(u32x2, h0), uy = __builtin_bit_cast(u32x2, h1);
                        const auto s0 = __builtin_amdgcn_permlane16_swap(ux[0], uy[0], false, false);
                        const auto s1 = __builtin_amdgcn_permlane16_swap(ux[1], uy[1], false, false);
                        const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
                        const int nc = n0 + hb * 128 + wn * 32 + ((q & 1) ? 16 : 0) + 4 * (q & ~1);
                        if (m < p.M) *reinterpret_cast<u32x4*>(p.out2 + (size_t)m * p.ld2 + nc) = o;
                    }
                }
            }
        } else {
#pragma unroll
        for (int ha = 0; ha < 2; ++ha)
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const int m = m0 + ha * (BM / 2) + wm * MF * 16 + f * 16 + (lane & 15);
#pragma unroll
                for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                    for (int g2 = 0; g2 < 2; ++g2) {
                        const int n = n0 + hb * 128 + wn * 32 + g2 * 16 + 4 * (lane >> 4);
                        f32x4 v = acc[ha][hb][f][g2] + *reinterpret_cast<const f32x4*>(smem + BIAS_OFF + n * 4);
                        if constexpr (RESID) {
                            if (m < p.M) {
                                f32x4* dst = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.out) + (size_t)m * p.ldc + n);
                                f32x4 x;
                                if constexpr (XPRE) x = xres[ha][hb][f][g2];
                                else x = *dst;
                                if constexpr (EPI == EPI_SCALE_RESID_F32) *dst = fma4(v, *reinterpret_cast<const f32x4*>(p.pos + n), x);
                                else *dst = x + v;
                            }
                        } else {
                            epilogue_ring<EPI>(p, m, n, v);
                        }
                    }
            }
        }
        SEG_E(7);
        if constexpr (PUB) tm_prev = tm;
    }
    if constexpr (PUB) {      // the last tile: every wave drains its stores and meets the others before wave 0 publishes
        wait_vm<0>();
        barrier_raw();
    }
#ifdef HG_STAMPS
    if (p.dbg && lane == 0) {
        unsigned long long* d = p.dbg + (size_t)(blockIdx.x * 8 + wave) * 16;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = tacc[k];
        d[8] = __builtin_amdgcn_s_memtime() - t_all;
        d[9] = (unsigned long long)my_tiles * nk;
    }
#endif
    if (!late) barrier_raw();   // balances the extra barrier of the late waves
    if constexpr (PUB) {      // (waves 0-3 are here once waves 4-7 have passed the barrier behind their drain)
        if (wave == 0) sc.publish(tm_prev, lane);
    }
#endif
}

}  // namespace hg
