// The MLP of a transformer block as one persistent launch with c_proj on 256 x 256 TILES (gfx950).  hg_mlp_pair.hip describes the launch
// and its hand-off - c_fc tiles publish per 256-row panel of `fc`, c_proj tiles wait for their panel, producers and consumers of a
// panel on one XCD by HW_REG_XCC_ID and the census - and all of that holds here unchanged.  What differs:
//
//   * c_proj runs the 256 x 256 ring body (hg_gemm_ring_body.h, four phases, EPI_RESID_LN_F32 with the residual stream as fp32 or as
//     centre + hi + lo) instead of ring2's 128 x 256 body.  On the global -> LDS path, which bounds both K loops, the bigger tile moves
//     7.6 KB per MFLOP instead of 11.4.  A row leaves with the bits ring2 gives it: same K order, same MFMA, the same epilogue
//     expressions, the same partial statistics per 64 columns; lo is read and written in ring2's tile order - a 256-row tile is ring2's
//     tiles (2 k, n) and (2 k + 1, n) -, so out_proj, which stays on ring2, consumes it as before.
//   * A c_proj tile is a whole panel high, so its wait is simple: wave 0 polls ready[panel] in front of the tile (bounded, *err as in
//     hg_mlp_pair.hip: never a hang), a barrier publishes the answer, then the body runs that ONE tile - prologue, 48 K-tiles,
//     epilogue.  The operand ring therefore never reaches into a panel that is not complete; the price is one refill of the ring per
//     tile (~2 % of a tile).
//   * The slots of an XCD share its tiles by WORK (hg_mlp_pair256_deal.h): a c_proj tile weighs `ratio` c_fc tiles (option mlp_pair256_ratio), the slots
//     that own one c_proj tile more own that many c_fc tiles fewer, reach c_proj first and take the XCD's earliest panels.  Every slot
//     runs all of its c_fc tiles before any of its c_proj tiles, so resident workgroups always progress.
//
// The text tower's form (gamma in the activation copy) has no instance here: it stays on hg_mlp_pair.hip.
#include <stdio.h>
#include <stdlib.h>

#include "hg_gemm_ring_body.h"
#include "hg_mlp_pair_dev.h"
#include "hg_mlp_pair256_deal.h"

namespace hg {

static_assert(PAIR256_NX == MLP_NX, "one census geometry");

// ---- c_fc: the XCD's list is hg_mlp_pair.hip's (its chunks of `ch` panels one after the other; inside a chunk: column group, panel,
// column in the group); which positions a slot owns: Pair256Deal
struct Pair256FcSched {
    static constexpr bool PUBLISH = true, CONSUME = false;
    int x, ch, tn, wave, npx, total, slack_t;
    Pair256Deal deal;
    unsigned* ready;
    __device__ __forceinline__ Pair256FcSched(const MlpGeom& g, int M, int N, int proj_tn, int ratio, unsigned* ready_)
        : deal(pair256_panels((M + 255) / 256, g.xcd) * (N / 256), pair256_panels((M + 255) / 256, g.xcd) * proj_tn, g.cpx, g.cu, ratio) {
        x = g.xcd; ch = g.ch; wave = g.wave; ready = ready_;
        tn = N / 256;
        npx = pair256_panels((M + 255) / 256, x);
        total = deal.n_fc();
        slack_t = deal.slack();
    }
    __device__ __forceinline__ int n_items() const { return total; }
    __device__ __forceinline__ int slack() const { return slack_t; }
    __device__ __forceinline__ void tile(int r, int& tm, int& tn_) const {
        pair256_fc_tile(deal.fc_pos(r), x, ch, tn, npx, tm, tn_);
    }
    __device__ __forceinline__ int thread_id() const { return mlp_thread_id(wave); }
    __device__ __forceinline__ void publish(int tm, int lane) const {
        if (lane == 0) __hip_atomic_fetch_add(ready + tm, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ---- c_proj: ONE tile per call of the body; the kernel walks this slot's items, waits for each one's panel and sets (tm, tn).  (Only
// what the body reads lives here: the dealing's numbers kept alive across the body cost it scalar registers.)
struct Pair256ProjSched {
    static constexpr bool PUBLISH = false, CONSUME = true;
    int tm, tn, wave;
    __device__ __forceinline__ int n_items() const { return 1; }
    __device__ __forceinline__ int slack() const { return 0; }
    __device__ __forceinline__ void tile(int, int& tm_, int& tn_) const { tm_ = tm; tn_ = tn; }
    __device__ __forceinline__ int thread_id() const { return mlp_thread_id(wave); }
    __device__ __forceinline__ void publish(int, int) const {}
};
// bounded wait for a panel's counter (hg_mlp_pair.hip, MlpProjSched::spin)
__device__ __forceinline__ void pair256_wait_panel(const unsigned* ctr, unsigned target, int* err) {
    for (int it = 0; it < MLP_SPIN_LIMIT; ++it) {
        if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return;
        __builtin_amdgcn_s_sleep(16);
        // (a wait of this launch or an earlier one has already given up: the call is lost, do not sit out the bound tile after tile)
        if ((it & 1023) == 1023 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) return;
    }
    __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // never a hang: flag it and go on
}

struct Pair256Args {
    MlpFcArgs fc;
    MlpProjArgs proj;
    unsigned* ready;      // [mlp_pair_ready_words(M)] zeroed before the launch: the census words, a counter per 256-row panel
    int* err;             // host-mapped
    int ch;               // 256-row panels of an XCD per chunk of the c_fc order
    int proj_tn;          // column tiles of c_proj (the c_fc dealing balances against the c_proj list; c_proj's arguments are read late)
    int ratio;            // c_fc tile times a c_proj tile takes: what the dealing balances with (any value computes the same bits)
    int census_off;       // byte offset in dynamic LDS of the word through which a workgroup's waves learn their slot
    unsigned long long* dbg;   // diagnostics (HG_STAMPS build): s_memtime stamps per workgroup, normally null
};

// Straight-line: c_fc body, then c_proj's arguments from the kernel-argument segment, then the c_proj body once per tile - the lessons
// of hg_mlp_pair.hip's kernel note (scalar registers; address spaces; the thread id rebuilt per body).
template <int HL>
__global__ __launch_bounds__(512, 2) void mlp_pair256_kernel(const Pair256Args P_in) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Pair256Args& P = P_in;
    MlpGeom geo;
    geo.xcd = (int)(__builtin_amdgcn_s_getreg(20 /* HW_REG_XCC_ID */ | (0 << 6) | ((4 - 1) << 11)) & (MLP_NX - 1));
    geo.cpx = (gridDim.x + MLP_NX - 1) / MLP_NX;      // (slots per XCD; a grid launched short - the API's fault-injection option - leaves a slot untaken)
    geo.wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    geo.ch = P.ch;
    geo.fcs = geo.cpx;
    if (threadIdx.x == 0)
        *reinterpret_cast<int*>(smem + P.census_off) =
            (int)__hip_atomic_fetch_add(P.ready + geo.xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    geo.cu = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(smem + P.census_off));
    if (geo.cu >= geo.cpx) return;      // more workgroups on this XCD than it has slots: the others own all of its work
#ifdef HG_STAMPS
    unsigned long long t_stamp[4] = {__builtin_amdgcn_s_memtime(), 0, 0, 0};
#endif
    {
        Pair256FcSched sf(geo, P.fc.M, P.fc.N, P.proj_tn, P.ratio, P.ready + MLP_CENSUS);
        if (sf.total > 0) {
            GemmArgs a{};
            a.A = P.fc.A; a.W = P.fc.W; a.bias = P.fc.bias; a.out = P.fc.out; a.cs = P.fc.cs; a.mr = P.fc.mr;
            a.lda = P.fc.lda; a.ldc = P.fc.ldc; a.M = P.fc.M; a.N = P.fc.N; a.K = P.fc.K;
            gemm_ring_body<4, EPI_LN_BIAS_QGELU_F16, true>(a, P.fc.a_bytes, 3000 << 8, sf);
        }
#ifdef HG_STAMPS
        t_stamp[1] = __builtin_amdgcn_s_memtime();
        t_stamp[3] = (unsigned long long)sf.total;
#endif
    }
    {
        // (c_proj's geometry from the c_fc arguments, which are here already: M the same, K = c_fc's N)
        const int tnp = P.proj_tn, npx = pair256_panels((P.fc.M + 255) / 256, geo.xcd);
        const Pair256Deal deal(npx * (P.fc.N / 256), npx * tnp, geo.cpx, geo.cu, P.ratio);
        const int n_proj = deal.n_proj(), item0 = deal.proj_item(0);
        for (int j = 0; j < n_proj; ++j) {
            // c_proj's arguments: from the kernel-argument segment, here and not at the kernel's entry, and again for every tile - what the
            // body derives from them would otherwise be hoisted out of this loop and held in scalar registers across it (seven spilled)
            const MlpProjArgs Q = load_kernarg<MlpProjArgs>((unsigned)__builtin_offsetof(Pair256Args, proj));
            GemmArgs a{};
            a.A = global_bits(Q.A); a.W = global_bits(Q.W); a.bias = global_bits(Q.bias); a.out = global_bits(Q.out); a.mu = global_bits(Q.mu);
            a.out2 = global_bits(Q.out2); a.stats = global_bits(Q.stats); a.lo = global_bits(Q.lo); a.muc = global_bits(Q.muc);
            a.lda = Q.lda; a.ldc = Q.ldc; a.ld2 = Q.ld2; a.M = Q.M; a.N = Q.N; a.K = Q.K;
            a.stats_ld = Q.stats_ld;
            const int i = item0 + j * geo.cpx;      // (Pair256Deal::proj_item(j))
            Pair256ProjSched sp;
            sp.wave = geo.wave;
            pair256_proj_tile(i, geo.xcd, tnp, sp.tm, sp.tn);
            // one publish per c_fc tile of the panel
            if (geo.wave == 0) pair256_wait_panel(P.ready + MLP_CENSUS + sp.tm, (unsigned)(P.fc.N / 256), P.err);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            barrier_raw();      // the panel is complete; every wave has left the previous body (its LDS image is dead)
            gemm_ring_body<4, EPI_RESID_LN_F32, false, HL>(a, Q.a_bytes, 0, sp);
        }
#ifdef HG_STAMPS
        t_stamp[2] = __builtin_amdgcn_s_memtime();
        if (P.dbg && threadIdx.x == 0) {
            unsigned long long* d = P.dbg + (size_t)blockIdx.x * 8;
            d[0] = t_stamp[0]; d[1] = t_stamp[1]; d[2] = t_stamp[2]; d[3] = t_stamp[3]; d[4] = (unsigned long long)n_proj;
            d[5] = (unsigned long long)(geo.xcd * 256 + geo.cu);
        }
#endif
    }
#endif
}

// what hg_mlp_pair.hip's launch takes, without the text tower's gamma form and from min_m rows on (hg_tower.hip: option mlp_pair256_min_m)
bool mlp_pair256_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu, int min_m) {
    if (!mlp_pair_ok(fc, proj, n_cu) || proj.gamma) return false;
    if (fc.M < min_m) return false;
    // c_proj's A and lo through 32-bit offsets of whole 256-row tiles
    if ((size_t)((proj.M + 255) / 256) * 256 * proj.lda * 2 >= (1ull << 31)) return false;
    return proj.hl == 0 || proj.hl == 2 || proj.hl == 3;
}

template <int HL>
static hipError_t launch_pair256_t(const Pair256Args& a, int grid, int lds, hipStream_t s) {
    static bool attr_set_d[HG_MAX_DEVICES] = {};
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_pair256_kernel<HL>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL((mlp_pair256_kernel<HL>), dim3(grid), dim3(512), lds, s, a);
    return hipGetLastError();
}

static hipError_t launch_pair256_hl(const Pair256Args& a, int hl, int grid, int lds, hipStream_t s) {
    switch (hl) {
        case 0: return launch_pair256_t<0>(a, grid, lds, s);
        case 2: return launch_pair256_t<2>(a, grid, lds, s);
        case 3: return launch_pair256_t<3>(a, grid, lds, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_mlp_pair256(const GemmArgs& fc, const GemmArgs& proj_in, unsigned* ready, int* err, int ch, int ratio, int n_cu,
                              hipStream_t s, int grid_short) {
    GemmArgs proj = proj_in;
    if (!proj.ld2) proj.ld2 = proj.ldc;
    if (!mlp_pair256_ok(fc, proj, n_cu, 0) || !ready || !err || proj.ld2 % 8) return hipErrorInvalidValue;
    if (proj.hl && (!proj.lo || !proj.mu || !proj.muc)) return hipErrorInvalidValue;
    Pair256Args a{};
    a.fc = MlpFcArgs{fc.A, fc.W, fc.bias, (half_t*)fc.out, fc.cs, fc.mr, fc.lda, fc.ldc, fc.M, fc.N, fc.K,
                     (unsigned)((size_t)((fc.M + 255) / 256) * 256 * fc.lda * 2)};
    a.proj = MlpProjArgs{proj.A, proj.W, proj.bias, (float*)proj.out, proj.mu, proj.out2, proj.stats, proj.lo, proj.muc,
                         proj.lda, proj.ldc, proj.ld2, proj.M, proj.N, proj.K, proj.stats_ld,
                         (unsigned)((size_t)((proj.M + 255) / 256) * 256 * proj.lda * 2), nullptr, nullptr, 0};
    a.ready = ready; a.err = err;
    a.ch = ch < 1 ? 1 : (ch > 64 ? 64 : ch);
    a.proj_tn = proj.N / 256;
    a.ratio = ratio < 1 ? 1 : (ratio > 8 ? 8 : ratio);
    const int lds_fc = 2 * (2 * 4 * 4096 + 2 * 16384) + fc.N * 4 * 2 + 256 * 8;
    const int lds_proj = 2 * (2 * 4 * 4096 + 2 * 16384) + proj.N * 4;
    a.census_off = lds_fc > lds_proj ? lds_fc : lds_proj;      // (behind both bodies' LDS images: never overwritten)
    const int lds = a.census_off + 16;
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const int grid = n_cu - (grid_short > 0 && grid_short < MLP_NX ? grid_short : 0);
#ifdef HG_STAMPS
    if (getenv("HG_STAMPS")) {
        unsigned long long* d = nullptr;
        if (hipMalloc(&d, (size_t)grid * 64) != hipSuccess) return hipErrorOutOfMemory;
        hipMemsetAsync(d, 0, (size_t)grid * 64, s);
        a.dbg = d;
        hipError_t e = launch_pair256_hl(a, proj.hl, grid, lds, s);
        hipStreamSynchronize(s);
        unsigned long long* h = (unsigned long long*)malloc((size_t)grid * 64);
        hipMemcpy(h, d, (size_t)grid * 64, hipMemcpyDeviceToHost);
        // s_memtime is not synchronised across CUs: only differences inside a workgroup mean anything.  Group by (c_fc tiles, c_proj tiles).
        for (int nf = 0; nf <= 16; ++nf)
            for (int np = 0; np <= 8; ++np) {
                double f = 0, q = 0, tmax = 0; int n = 0;
                for (int b = 0; b < grid; ++b) {
                    if (!h[b * 8] || (int)h[b * 8 + 3] != nf || (int)h[b * 8 + 4] != np) continue;
                    const double d1 = (double)(h[b * 8 + 1] - h[b * 8]), d2 = (double)(h[b * 8 + 2] - h[b * 8 + 1]);
                    f += d1; q += d2; ++n;
                    tmax = d1 + d2 > tmax ? d1 + d2 : tmax;
                }
                if (n) fprintf(stderr, "[pair256-dbg] %3d workgroups with %2d c_fc + %d c_proj tiles: c_fc phase mean %.0f = %.0f per tile | c_proj phase mean %.0f = %.0f per tile | whole mean %.0f max %.0f [s_memtime ticks]\n",
                               n, nf, np, f / n, nf ? f / n / nf : 0.0, q / n, np ? q / n / np : 0.0, (f + q) / n, tmax);
            }
        free(h);
        hipFree(d);
        return e;
    }
#endif
    return launch_pair256_hl(a, proj.hl, grid, lds, s);
}

}  // namespace hg
