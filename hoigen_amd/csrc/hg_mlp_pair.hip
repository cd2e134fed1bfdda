// The MLP of a transformer block as ONE persistent launch (gfx950): c_fc (LayerNorm-folded, + QuickGELU) -> c_proj (+ residual, emits
// the next LayerNorm's operand and statistics), clipnet/model.py:173-177,185-188 (reference: x = x + mlp(ln_2(x))).
//
// One workgroup per CU runs BOTH GEMMs' tiles: the 256 x 256 two-phase ring body (hg_gemm_ring_body.h, epilogue EPI_LN_BIAS_QGELU_F16) on
// its c_fc tiles and the 128 x 256 ring2 body (hg_gemm_ring2_body.h, EPI_RESID_LN_F32 on the hi / lo stream) on its c_proj tiles - the
// same K loops, epilogues and bits as the two stand-alone launches.  What the launch boundary used to order is ordered per 256-row panel
// of the intermediate activation `fc` instead:
//
//   producer  a c_fc tile is stored with plain stores; once all eight waves' stores have retired - they are in the XCD's L2 then - wave 0
//             adds 1 to ready[panel] (deferred into the second K-tile of the workgroup's next tile, where a counted vmcnt wait and the
//             phase's barriers prove it: no drain of the operand ring);
//   consumer  a c_proj tile (128 rows: half a panel) starts only when ready[panel] == N_fc / 256 column tiles; wave 0 issues
//             the counter load six K-tiles before the previous tile ends and looks at it three K-tiles later, a barrier publishes the
//             answer; its A operand is fetched with sc1 loads (past this CU's vector L1, from the XCD's L2).
//
// Producers and consumers of a row panel run ON THE SAME XCD, and that is what makes plain stores a valid hand-off: an XCD's L2 is
// coherent for all its CUs, the L2s of different XCDs are not with each other (MI355X_MICROARCH.md "Correctness boundaries"; measured
// here: the same kernel with the consumers on other XCDs reads stale lines, and storing write-through for them costs 50 us per launch,
// profiles/r06_mlp_pair.txt).  "Same XCD" is not an assumption about placement: a workgroup reads its XCD from the hardware register
// (HW_REG_XCC_ID) and takes the next free work slot OF THAT XCD from a census counter; XCD x's slots own the row panels p = x (mod 8),
// their c_fc tiles and their c_proj tiles.  So results do not depend on where or when workgroups land.  Progress needs every slot
// taken, i.e. gridDim / 8 workgroups on each XCD - what one workgroup per CU on the whole chip gives (the launcher refuses other
// devices); a workgroup beyond its XCD's slots exits, and a wait that outlasts its bound (~0.6 s: a slot nobody took) sets *err - a
// host-mapped word the API turns into HG_ERR_HIP - and goes on with whatever is there: wrong results behind an error, never a hang.
// Within a workgroup every c_fc tile precedes the c_proj tiles that could wait for it, so resident workgroups always progress.
// (The launch wants the GPU to itself: two such launches that each hold part of the CUs wait for each other until the bound expires.
// Across the streams of one process hg_api.hip orders them (PairGate); across processes INTEGRATION.md says so, option mlp_pair = 0.)
//
// Tile order.  XCD x walks its panels p = x + 8 k in CHUNKS of `ch` panels: inside a chunk the c_fc tiles run column group by column
// group (4 column tiles: their W slices stay in the XCD's L2 while the chunk's A panels stream, as in the stand-alone kernel's list);
// all XCDs finish their k-th panels at about the same time.  c_proj: the two 128-row halves of a panel, the column tiles of a half side
// by side (they share the A panel through L2).  A workgroup runs all its c_fc tiles, then its c_proj tiles - the launch boundary's order
// minus the boundary: a workgroup with one c_fc tile fewer starts its c_proj tiles a tile time earlier, its first panels are long
// complete.  (c_fc in two or three segments with the c_proj tiles of a segment's panels behind the next segment's c_fc - `fc` read back
// sooner after it was written - was built and measured no faster in any chunking: profiles/r06_mlp_pair.txt.)
#include "hg_gemm_ring_body.h"
#include "hg_gemm_ring2_body.h"
#include "hg_mlp_pair_dev.h"

namespace hg {

// ---- c_fc: the XCD's list (MlpFcList), dealt among its first `fcs` slots (MlpFcDeal; hg_mlp_pair_deal.h).  fcs < the number of slots
// leaves the other workgroups of the XCD idle (polling, asleep) until the first panels are complete: as in the stand-alone kernel,
// 2364 tiles take ten rounds on 240 or on 256 workgroups, and the idle CUs' power buys clock for the others.
struct MlpFcSched {
    static constexpr bool PUBLISH = true, CONSUME = false;
    MlpFcList list;
    MlpFcDeal deal;
    int wave;
    unsigned* ready;
    __device__ __forceinline__ MlpFcSched(const MlpGeom& g, int M, int N, unsigned* ready_)
        : list(g.xcd, g.ch, N / 256, mlp_panels((M + 255) / 256, g.xcd)), deal(list.size(), g.cu, g.fcs) {
        wave = g.wave; ready = ready_;
    }
    __device__ __forceinline__ int n_items() const { return deal.total; }
    // start stagger, as in the stand-alone kernel: slots that own one tile fewer than the fullest ones spend a pseudo-random fraction
    // of a tile time before their first tile (de-phased epilogue bursts: -11 us per launch)
    __device__ __forceinline__ int slack() const { return deal.slack(); }
    __device__ __forceinline__ void tile(int r, int& tm, int& tn_) const { list.tile(deal.pos(r), tm, tn_); }
    __device__ __forceinline__ int thread_id() const { return mlp_thread_id(wave); }
    __device__ __forceinline__ void publish(int tm, int lane) const {
        if (lane == 0) __hip_atomic_fetch_add(ready + tm, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ---- c_proj: this slot's items of the XCD's list (MlpProjDeal), each behind a wait for its panel
struct MlpProjSched {
    static constexpr bool PUBLISH = false, CONSUME = true;
    MlpProjDeal deal;
    int wave;
    unsigned target;
    const unsigned* ready;
    int* err;
    __device__ __forceinline__ MlpProjSched(const MlpGeom& g, int M, int N, int n_fc, const unsigned* ready_, int* err_)
        : deal(M, N / 256, g.xcd, g.cu, g.cpx) {
        wave = g.wave; ready = ready_; err = err_;
        target = (unsigned)(n_fc / 256);      // one publish per c_fc tile of the panel
    }
    __device__ __forceinline__ int n_items() const { return deal.total; }
    __device__ __forceinline__ int slack() const { return 0; }      // (the slots reach their c_proj tiles de-phased by their c_fc tiles)
    __device__ __forceinline__ void tile(int r, int& tm, int& tn_) const { deal.tile(deal.item(r), tm, tn_); }
    __device__ __forceinline__ int thread_id() const { return mlp_thread_id(wave); }
    __device__ __forceinline__ const unsigned* counter(int r) const {
        int tm, t2;
        tile(r, tm, t2);
        return ready + (tm >> 1);
    }
    // one relaxed agent-scope load (global_load_dword sc1): the value is looked at K-tiles later
    __device__ __forceinline__ unsigned poll_issue(int r) const {
        return __hip_atomic_load(counter(r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void poll_finish(int r, unsigned v) const {
        if ((unsigned)__builtin_amdgcn_readfirstlane((int)v) < target) mlp_wait_panel(counter(r), target, err);
    }
    __device__ __forceinline__ void poll_blocking(int r) const { mlp_wait_panel(counter(r), target, err); }
};

struct MlpPairArgs {
    MlpFcArgs fc;
    MlpProjArgs proj;
    unsigned* ready;      // [mlp_pair_ready_words(M)] zeroed before the launch: the census words, a counter per 256-row panel (c_fc tiles
                          // stored)
    int* err;             // host-mapped
    int ch;               // 256-row panels of an XCD per chunk
    int fc_slots;         // slots per XCD that run c_fc tiles (the others start with c_proj, i.e. wait)
    int census_off;       // byte offset in dynamic LDS of the word through which a workgroup's waves learn their slot
    unsigned long long* dbg;   // diagnostics (HG_STAMPS build): s_memtime stamps per workgroup, normally null
};

// Scalar registers are the scarce resource of this kernel.  With a whole GemmArgs per body as kernel arguments (2 x 47 dwords) the
// allocator spills scalars, and once it has to spill more than a dozen the scheduler minimises register pressure in EVERY region: the
// c_fc epilogue came out as ONE dependent chain through a single pair of temporaries (242 s_nop against 69 in the stand-alone kernel,
// +30 us per launch).  Reading the arguments back through an opaque pointer instead loses their address space (flat_ instead of
// global_ accesses, which also count in lgkmcnt: every fetch segment behind an epilogue then waits for the tile's stores, +19 us), and
// a loop around the two bodies (c_fc in several segments with c_proj between them - built, and no faster in any order:
// profiles/r06_mlp_pair.txt) makes both problems worse.  Hence: compact by-value arguments, straight-line code, c_fc then c_proj.
// c_proj's arguments are read from the kernel-argument segment BEHIND the c_fc body (as kernel arguments proper they are loaded at the
// kernel's entry and sit in 30 scalar registers all through c_fc: with the text tower's three more - gamma, out3, ld3 - that is what
// tips the allocator over, see above).  Read back as integers the pointers have lost their address space; a cast of the BITS to an
// address-space-1 pointer gives it back (a cast of the generic pointer there and back is folded away and leaves flat_ accesses):
// load_kernarg, global_bits (hg_mlp_pair_dev.h).
template <int HL, bool GS>
__global__ __launch_bounds__(512, 2) void mlp_pair_kernel(const MlpPairArgs P_in) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const MlpPairArgs& P = P_in;
    MlpGeom geo;
    if (!mlp_take_slot(geo, smem, P.ready, P.census_off, P.ch, P.fc_slots)) return;
#ifdef HG_STAMPS
    unsigned long long t_stamp[4] = {__builtin_amdgcn_s_memtime(), 0, 0, 0};
#endif
    {
        MlpFcSched sf(geo, P.fc.M, P.fc.N, P.ready + MLP_CENSUS);
        if (sf.deal.total > 0) {
            const GemmArgs a = mlp_fc_gemm_args(P.fc);
            gemm_ring_body<4, EPI_LN_BIAS_QGELU_F16, true>(a, P.fc.a_bytes, 3000 << 8, sf);
        }
#ifdef HG_STAMPS
        t_stamp[1] = __builtin_amdgcn_s_memtime();
        t_stamp[3] = (unsigned long long)sf.deal.total;
#endif
    }
    {
        const MlpProjArgs Q = load_kernarg<MlpProjArgs>((unsigned)__builtin_offsetof(MlpPairArgs, proj));      // (here, not at the kernel's entry)
        MlpProjSched sp(geo, Q.M, Q.N, Q.K, P.ready + MLP_CENSUS, P.err);
        if (sp.deal.total > 0) {
            const GemmArgs a = mlp_proj_gemm_args<GS>(Q);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            barrier_raw();      // every wave has left the c_fc body (its LDS image is dead)
            gemm_ring2_body<EPI_RESID_LN_F32, HL, GS>(a, a.N / 256, Q.a_bytes, 0, sp);
        }
#ifdef HG_STAMPS
        t_stamp[2] = __builtin_amdgcn_s_memtime();
        if (P.dbg && threadIdx.x == 0) {
            unsigned long long* d = P.dbg + (size_t)blockIdx.x * 8;
            d[0] = t_stamp[0]; d[1] = t_stamp[1]; d[2] = t_stamp[2]; d[3] = t_stamp[3]; d[4] = (unsigned long long)sp.deal.total;
            d[5] = (unsigned long long)(geo.xcd * 256 + geo.cu);
        }
#endif
    }
#endif
}

// c_fc: a LayerNorm-folded QuickGELU GEMM the 256 x 256 ring kernel takes; c_proj: the LayerNorm-emitting residual GEMM on fc
bool mlp_pair_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu) { return fc.M >= 8 * 256 && mlp_pair_shapes_ok(fc, proj, n_cu); }
// (without the row bound: the 256-row launch deals whatever panels there are - XCDs without a panel own no tile - and has a bound of its own)
bool mlp_pair_shapes_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu) {
    if (n_cu != 32 * MLP_NX) return false;      // one workgroup per CU must put gridDim / 8 workgroups on each of the 8 XCDs (MI355X: 8 x 32 CUs)
    if (!gemm_ln_ok(EPI_LN_BIAS_QGELU_F16, fc) || !gemm_ln_ok(EPI_RESID_LN_F32, proj)) return false;
    if (fc.M != proj.M || proj.K != fc.N || proj.lda != fc.ldc || (const void*)proj.A != fc.out) return false;
    if (fc.K < 5 * 64 || proj.K < 8 * 64) return false;                    // K-tile kinds of the two hand-off protocols
    if ((size_t)((fc.M + 255) / 256) * 256 * fc.ldc * 2 >= (1ull << 32)) return false;      // fc through one buffer descriptor
    // (the text tower: the next LayerNorm's weight in the activation copy - beside the stream's hi half where the stream leaves as hi / lo)
    if (proj.gamma && proj.hl == 2 && (!proj.out3 || proj.ld3 < proj.N || (proj.ld3 % 8))) return false;
    return proj.hl == 0 || proj.hl == 2 || proj.hl == 3;
}

static hipError_t launch_pair_hl(const MlpPairArgs& a, int hl, bool gs, int grid, int lds, hipStream_t s) {
    if (gs) {
        switch (hl) {
            case 2: return mlp_launch_instance<mlp_pair_kernel<2, true>>(a, grid, lds, s);
            case 3: return mlp_launch_instance<mlp_pair_kernel<3, true>>(a, grid, lds, s);
            default: return hipErrorInvalidValue;
        }
    }
    switch (hl) {
        case 0: return mlp_launch_instance<mlp_pair_kernel<0, false>>(a, grid, lds, s);
        case 2: return mlp_launch_instance<mlp_pair_kernel<2, false>>(a, grid, lds, s);
        case 3: return mlp_launch_instance<mlp_pair_kernel<3, false>>(a, grid, lds, s);
        default: return hipErrorInvalidValue;
    }
}

size_t mlp_pair_ready_words(int M) { return (size_t)MLP_CENSUS + (size_t)((M + 255) / 256); }

hipError_t launch_mlp_pair(const GemmArgs& fc, const GemmArgs& proj_in, unsigned* ready, int* err, int ch, int fc_slots, int n_cu,
                           hipStream_t s, int grid_short) {
    GemmArgs proj = proj_in;
    if (!proj.ld2) proj.ld2 = proj.ldc;
    if (!mlp_pair_ok(fc, proj, n_cu) || !ready || !err || proj.ld2 % 8) return hipErrorInvalidValue;
    if (proj.hl && (!proj.lo || !proj.mu || ((proj.hl == 2 || proj.hl == 3) && !proj.muc))) return hipErrorInvalidValue;
    MlpPairArgs a{};
    mlp_pack_args(fc, proj, 128, a.fc, a.proj);
    a.ready = ready; a.err = err;
    a.ch = ch < 1 ? 1 : (ch > 64 ? 64 : ch);
    a.fc_slots = fc_slots < 1 ? 1 : fc_slots;
    const int lds = mlp_pair_lds(fc.N, 3 * 49152 + proj.N * 4 * (proj.gamma ? 2 : 1), a.census_off);
    if (!lds) return hipErrorInvalidValue;
    const int grid = mlp_pair_grid(n_cu, grid_short);
    auto launch = [&](unsigned long long* dbg) {
        a.dbg = dbg;
        return launch_pair_hl(a, proj.hl, proj.gamma != nullptr, grid, lds, s);
    };
#ifdef HG_STAMPS
    if (getenv("HG_STAMPS")) return mlp_launch_stamped("pair", grid, s, launch);
#endif
    return launch(nullptr);
}

}  // namespace hg
