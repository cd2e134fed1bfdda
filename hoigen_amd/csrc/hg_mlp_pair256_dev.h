// What the two forms of the MLP pair launch with c_proj on 256 x 256 tiles share (hg_mlp_pair256.hip: c_proj on the four-phase K loop;
// hg_mlp_pair256p.hip: on the two-phase one): the schedules of the two bodies, the kernel arguments, the kernel's code with the c_proj
// loop form as a parameter, and the host side of a launch.  hg_mlp_pair256.hip holds the description.
#pragma once
#include <limits.h>

#include "hg_gemm_ring_body.h"
#include "hg_mlp_pair_dev.h"

namespace hg {

// ---- c_fc: the XCD's list is hg_mlp_pair.hip's (MlpFcList); which positions a slot owns: Pair256Deal
struct Pair256FcSched {
    static constexpr bool PUBLISH = true, CONSUME = false;
    int x, ch, tn, wave, npx, total, slack_t;
    Pair256Deal deal;
    unsigned* ready;
    __device__ __forceinline__ Pair256FcSched(const MlpGeom& g, int M, int N, int proj_tn, int ratio, unsigned* ready_)
        : deal(mlp_panels((M + 255) / 256, g.xcd) * (N / 256), mlp_panels((M + 255) / 256, g.xcd) * proj_tn, g.cpx, g.cu, ratio) {
        x = g.xcd; ch = g.ch; wave = g.wave; ready = ready_;
        tn = N / 256;
        npx = mlp_panels((M + 255) / 256, x);
        total = deal.n_fc();
        slack_t = deal.slack();
    }
    __device__ __forceinline__ int n_items() const { return total; }
    __device__ __forceinline__ int slack() const { return slack_t; }
    __device__ __forceinline__ void tile(int r, int& tm, int& tn_) const {
        const int L = deal.fc_pos(r);
        MlpFcList(x, ch, tn, npx).tile(L, tm, tn_);      // (built here: as a member its derived numbers live in scalar registers across the body)
    }
    __device__ __forceinline__ int thread_id() const { return mlp_thread_id(wave); }
    __device__ __forceinline__ void publish(int tm, int lane) const {
        if (lane == 0) __hip_atomic_fetch_add(ready + tm, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ---- c_proj: ONE tile per call of the body; the kernel walks this slot's items, waits for each one's panel and sets (tm, tn).  (Only
// what the body reads lives here: the dealing's numbers kept alive across the body cost it scalar registers.)
// FRESH_TID (the two-phase form): the lane number is rebuilt behind an opaque zero in every call.  Left to itself the compiler computes
// v_mbcnt once in front of the tile loop and keeps it in a VGPR across the body, which has none to spare (the hi / lo -> fp32 instance
// spilled it to scratch).
template <bool FRESH_TID>
struct Pair256ProjSchedT {
    static constexpr bool PUBLISH = false, CONSUME = true;
    int tm, tn, wave;
    __device__ __forceinline__ int n_items() const { return 1; }
    __device__ __forceinline__ int slack() const { return 0; }
    __device__ __forceinline__ void tile(int, int& tm_, int& tn_) const { tm_ = tm; tn_ = tn; }
    __device__ __forceinline__ int thread_id() const {
        if constexpr (FRESH_TID) {
            unsigned z = 0;
            asm volatile("" : "+v"(z));
            int t = wave * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
            asm volatile("" : "+v"(t));
            return t;
        } else {
            return mlp_thread_id(wave);
        }
    }
    __device__ __forceinline__ void publish(int, int) const {}
};
using Pair256ProjSched = Pair256ProjSchedT<false>;

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
// of hg_mlp_pair.hip's kernel note (scalar registers; address spaces; the thread id rebuilt per body).  PROJ_PH2: c_proj's K loop.
template <int HL, bool PROJ_PH2>
__device__ __forceinline__ void mlp_pair256_run(const Pair256Args& P) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MlpGeom geo;
    if (!mlp_take_slot(geo, smem, P.ready, P.census_off, P.ch, INT_MAX)) return;      // (every slot runs c_fc tiles)
#ifdef HG_STAMPS
    unsigned long long t_stamp[4] = {__builtin_amdgcn_s_memtime(), 0, 0, 0};
#endif
    {
        Pair256FcSched sf(geo, P.fc.M, P.fc.N, P.proj_tn, P.ratio, P.ready + MLP_CENSUS);
        if (sf.total > 0) {
            const GemmArgs a = mlp_fc_gemm_args(P.fc);
            gemm_ring_body<4, EPI_LN_BIAS_QGELU_F16, true>(a, P.fc.a_bytes, 3000 << 8, sf);
        }
#ifdef HG_STAMPS
        t_stamp[1] = __builtin_amdgcn_s_memtime();
        t_stamp[3] = (unsigned long long)sf.total;
#endif
    }
    {
        // (c_proj's geometry from the c_fc arguments, which are here already: M the same, K = c_fc's N)
        const int tnp = P.proj_tn, npx = mlp_panels((P.fc.M + 255) / 256, geo.xcd);
        const Pair256Deal deal(npx * (P.fc.N / 256), npx * tnp, geo.cpx, geo.cu, P.ratio);
        const int n_proj = deal.n_proj(), item0 = deal.proj_item(0);
        for (int j = 0; j < n_proj; ++j) {
            // c_proj's arguments: from the kernel-argument segment, here and not at the kernel's entry, and again for every tile - what the
            // body derives from them would otherwise be hoisted out of this loop and held in scalar registers across it (seven spilled)
            const MlpProjArgs Q = load_kernarg<MlpProjArgs>((unsigned)__builtin_offsetof(Pair256Args, proj));
            const GemmArgs a = mlp_proj_gemm_args<false>(Q);
            const int i = item0 + j * geo.cpx;      // (Pair256Deal::proj_item(j))
            Pair256ProjSchedT<PROJ_PH2> sp;
            sp.wave = geo.wave;
            pair256_proj_tile(i, geo.xcd, tnp, sp.tm, sp.tn);
            // one publish per c_fc tile of the panel
            if (geo.wave == 0) mlp_wait_panel(P.ready + MLP_CENSUS + sp.tm, (unsigned)(P.fc.N / 256), P.err);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            barrier_raw();      // the panel is complete; every wave has left the previous body (its LDS image is dead)
            gemm_ring_body<4, EPI_RESID_LN_F32, PROJ_PH2, HL>(a, Q.a_bytes, 0, sp);
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

// host side of a launch: the checks, the packed arguments, LDS and grid; launch_hl(args, hl, grid, lds, stream) launches the instance
bool mlp_pair256_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu, int min_m);
template <class LAUNCH_HL>
hipError_t mlp_pair256_launch(const char* tag, const GemmArgs& fc, const GemmArgs& proj_in, unsigned* ready, int* err, int ch, int ratio,
                              int n_cu, hipStream_t s, int grid_short, LAUNCH_HL launch_hl) {
    GemmArgs proj = proj_in;
    if (!proj.ld2) proj.ld2 = proj.ldc;
    if (!mlp_pair256_ok(fc, proj, n_cu, 0) || !ready || !err || proj.ld2 % 8) return hipErrorInvalidValue;
    if (proj.hl && (!proj.lo || !proj.mu || !proj.muc)) return hipErrorInvalidValue;
    Pair256Args a{};
    mlp_pack_args(fc, proj, 256, a.fc, a.proj);
    a.ready = ready; a.err = err;
    a.ch = ch < 1 ? 1 : (ch > 64 ? 64 : ch);
    a.proj_tn = proj.N / 256;
    a.ratio = ratio < 1 ? 1 : (ratio > 8 ? 8 : ratio);
    const int lds = mlp_pair_lds(fc.N, 2 * (2 * 4 * 4096 + 2 * 16384) + proj.N * 4, a.census_off);
    if (!lds) return hipErrorInvalidValue;
    const int grid = mlp_pair_grid(n_cu, grid_short);
    auto launch = [&](unsigned long long* dbg) {
        a.dbg = dbg;
        return launch_hl(a, proj.hl, grid, lds, s);
    };
#ifdef HG_STAMPS
    if (getenv("HG_STAMPS")) return mlp_launch_stamped(tag, grid, s, launch);
#endif
    (void)tag;
    return launch(nullptr);
}

}  // namespace hg
