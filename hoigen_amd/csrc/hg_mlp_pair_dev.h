// What the two persistent MLP launches share (hg_mlp_pair.hip: c_proj on ring2's 128-row tiles; hg_mlp_pair256.hip: c_proj on 256-row
// tiles): the census geometry and how a workgroup takes its slot, the bounded wait for a panel, the compact kernel arguments of the two
// bodies, how c_proj's are read late, and the host side of a launch (argument packing, LDS layout, grid, instance launcher, the
// HG_STAMPS report).  hg_mlp_pair.hip holds the description of the hand-off, hg_mlp_pair_deal.h the list arithmetic.
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "hg_gemm_dev.h"
#include "hg_mlp_pair_deal.h"

namespace hg {

constexpr int MLP_SPIN_LIMIT = 1 << 20;    // polls of a ready counter (~0.5 us each: s_sleep 16) before giving up
constexpr int MLP_CENSUS = 16;             // words in front of the ready counters: [0, 8) work slots taken per XCD

struct MlpGeom {      // where this workgroup works: its XCD (hardware id), its work slot there, slots per XCD (all / those that run c_fc), panels per chunk
    int xcd, cu, cpx, fcs, ch;
    int wave;         // this wave's index in the workgroup (the bodies rebuild their thread id from it: see thread_id())
};
// threadIdx.x without keeping v0 alive: wave index (scalar) * 64 + lane (v_mbcnt), opaque so that nothing derived from it outlives a segment
__device__ __forceinline__ int mlp_thread_id(int wave) {
    int t = wave * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(t));
    return t;
}

// Kernel arguments: only what the two bodies read (a GemmArgs each would be 2 x 47 dwords of scalar registers: see the kernels' notes)
struct MlpFcArgs {
    const half_t* A; const half_t* W; const float* bias; half_t* out; const float* cs; const float* mr;
    int lda, ldc, M, N, K;
    unsigned a_bytes;
};
struct MlpProjArgs {
    const half_t* A; const half_t* W; const float* bias; float* out; const float* mu; half_t* out2; float* stats; half_t* lo;
    const float* muc;
    int lda, ldc, ld2, M, N, K, stats_ld;
    unsigned a_bytes;
    // GS instances (the text tower: the next LayerNorm's weight rides in the activation copy, GemmArgs::gamma)
    const float* gamma;
    half_t* out3;
    int ld3;
};

// c_proj's arguments are read from the kernel-argument segment BEHIND the c_fc body (hg_mlp_pair.hip, the kernel's note).  Read back as
// integers the pointers have lost their address space; a cast of the BITS to an address-space-1 pointer gives it back (a cast of the
// generic pointer there and back is folded away and leaves flat_ accesses).
template <class T>
__device__ __forceinline__ T load_kernarg(unsigned offset) {
    static_assert(sizeof(T) % 4 == 0, "dword-sized arguments");
    const __attribute__((address_space(4))) char* ka = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    const __attribute__((address_space(4))) unsigned* w = reinterpret_cast<const __attribute__((address_space(4))) unsigned*>(ka + offset);
    unsigned t[sizeof(T) / 4];
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) t[i] = w[i];
    T o;
    __builtin_memcpy(&o, t, sizeof(T));
    return o;
}
template <class T>
__device__ __forceinline__ T* global_bits(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(unsigned long long)p;
}

// This workgroup's XCD (the hardware's word, not blockIdx's) and its work slot there: the next free one of that XCD's census counter,
// which the waves learn through the LDS word at census_off.  False: more workgroups on this XCD than it has slots - the others own all
// of its work, this one exits.
__device__ __forceinline__ bool mlp_take_slot(MlpGeom& geo, char* smem, unsigned* ready, int census_off, int ch, int fc_slots) {
    geo.xcd = (int)(__builtin_amdgcn_s_getreg(20 /* HW_REG_XCC_ID */ | (0 << 6) | ((4 - 1) << 11)) & (MLP_NX - 1));
    geo.cpx = (gridDim.x + MLP_NX - 1) / MLP_NX;      // (slots per XCD; a grid launched short - the API's fault-injection option - leaves a slot untaken)
    geo.wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    geo.ch = ch;
    geo.fcs = fc_slots < geo.cpx ? fc_slots : geo.cpx;
    if (threadIdx.x == 0)
        *reinterpret_cast<int*>(smem + census_off) =
            (int)__hip_atomic_fetch_add(ready + geo.xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    geo.cu = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(smem + census_off));
    return geo.cu < geo.cpx;
}

// bounded wait for a panel's counter to reach `target` (one publish per c_fc tile of the panel)
__device__ __forceinline__ void mlp_wait_panel(const unsigned* ctr, unsigned target, int* err) {
    for (int it = 0; it < MLP_SPIN_LIMIT; ++it) {
        if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) return;
        __builtin_amdgcn_s_sleep(16);
        // (a wait of this launch or an earlier one has already given up: the call is lost, do not sit out the bound tile after tile)
        if ((it & 1023) == 1023 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) return;
    }
    __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // never a hang: flag it and go on
}

// the bodies' GemmArgs from the compact arguments (c_proj's: read late, so every pointer gets its address space back)
__device__ __forceinline__ GemmArgs mlp_fc_gemm_args(const MlpFcArgs& F) {
    GemmArgs a{};
    a.A = F.A; a.W = F.W; a.bias = F.bias; a.out = F.out; a.cs = F.cs; a.mr = F.mr;
    a.lda = F.lda; a.ldc = F.ldc; a.M = F.M; a.N = F.N; a.K = F.K;
    return a;
}
template <bool GS>
__device__ __forceinline__ GemmArgs mlp_proj_gemm_args(const MlpProjArgs& Q) {
    GemmArgs a{};
    a.A = global_bits(Q.A); a.W = global_bits(Q.W); a.bias = global_bits(Q.bias); a.out = global_bits(Q.out); a.mu = global_bits(Q.mu);
    a.out2 = global_bits(Q.out2); a.stats = global_bits(Q.stats); a.lo = global_bits(Q.lo); a.muc = global_bits(Q.muc);
    a.lda = Q.lda; a.ldc = Q.ldc; a.ld2 = Q.ld2; a.M = Q.M; a.N = Q.N; a.K = Q.K;
    a.stats_ld = Q.stats_ld;
    if constexpr (GS) { a.gamma = global_bits(Q.gamma); a.out3 = global_bits(Q.out3); a.ld3 = Q.ld3; }
    return a;
}

// ---- host side of a launch

// the compact arguments from the two GemmArgs; a_rows: the row rounding of c_proj's A operand (its tile height, 128 or 256)
inline void mlp_pack_args(const GemmArgs& fc, const GemmArgs& proj, int a_rows, MlpFcArgs& f, MlpProjArgs& p) {
    f = MlpFcArgs{fc.A, fc.W, fc.bias, (half_t*)fc.out, fc.cs, fc.mr, fc.lda, fc.ldc, fc.M, fc.N, fc.K,
                  (unsigned)((size_t)((fc.M + 255) / 256) * 256 * fc.lda * 2)};
    p = MlpProjArgs{proj.A, proj.W, proj.bias, (float*)proj.out, proj.mu, proj.out2, proj.stats, proj.lo, proj.muc,
                    proj.lda, proj.ldc, proj.ld2, proj.M, proj.N, proj.K, proj.stats_ld,
                    (unsigned)((size_t)((proj.M + a_rows - 1) / a_rows) * a_rows * proj.lda * 2), proj.gamma, proj.out3, proj.ld3};
}
constexpr int MLP_LDS_MAX = 160 * 1024;
// dynamic LDS of a launch whose c_proj body takes lds_proj bytes, and where in it the census word lies (behind both bodies' LDS
// images: never overwritten); 0: more than the CU has
inline int mlp_pair_lds(int fc_N, int lds_proj, int& census_off) {
    const int lds_fc = 2 * (2 * 4 * 4096 + 2 * 16384) + fc_N * 4 * 2 + 256 * 8;
    census_off = lds_fc > lds_proj ? lds_fc : lds_proj;
    return census_off + 16 <= MLP_LDS_MAX ? census_off + 16 : 0;
}
// one workgroup per CU, less grid_short (fault injection: hg_api.hip option mlp_pair_fault)
inline int mlp_pair_grid(int n_cu, int grid_short) { return n_cu - (grid_short > 0 && grid_short < MLP_NX ? grid_short : 0); }

// one kernel instance: its dynamic-LDS attribute once per device, then the launch
template <auto KERNEL, class ARGS>
hipError_t mlp_launch_instance(const ARGS& a, int grid, int lds, hipStream_t s) {
    static bool attr_set_d[HG_MAX_DEVICES] = {};
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, MLP_LDS_MAX);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(512), lds, s, a);
    return hipGetLastError();
}

#ifdef HG_STAMPS
// Diagnostic build: launch(dbg) with a buffer of 8 words per workgroup - the kernels fill s_memtime stamps (entry, end of c_fc, end of
// c_proj), the c_fc and c_proj tile counts and xcd * 256 + slot into dbg[0..5] -, wait, and report per (c_fc tiles, c_proj tiles) group.
template <class LAUNCH>
hipError_t mlp_launch_stamped(const char* tag, int grid, hipStream_t s, LAUNCH launch) {
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, (size_t)grid * 64) != hipSuccess) return hipErrorOutOfMemory;
    (void)hipMemsetAsync(d, 0, (size_t)grid * 64, s);
    hipError_t e = launch(d);
    (void)hipStreamSynchronize(s);
    unsigned long long* h = (unsigned long long*)malloc((size_t)grid * 64);
    (void)hipMemcpy(h, d, (size_t)grid * 64, hipMemcpyDeviceToHost);
    // s_memtime is not synchronised across CUs: only differences inside a workgroup mean anything.  Group by (c_fc tiles, c_proj tiles).
    for (int nf = 0; nf <= 16; ++nf)
        for (int np = 0; np <= 8; ++np) {
            double f = 0, q = 0, fmin = 1e30, fmax = 0, qmin = 1e30, qmax = 0, tmax = 0; int n = 0;
            for (int b = 0; b < grid; ++b) {
                if (!h[b * 8] || (int)h[b * 8 + 3] != nf || (int)h[b * 8 + 4] != np) continue;
                const double d1 = (double)(h[b * 8 + 1] - h[b * 8]), d2 = (double)(h[b * 8 + 2] - h[b * 8 + 1]);
                f += d1; q += d2; ++n;
                fmin = d1 < fmin ? d1 : fmin; fmax = d1 > fmax ? d1 : fmax; qmin = d2 < qmin ? d2 : qmin; qmax = d2 > qmax ? d2 : qmax;
                tmax = d1 + d2 > tmax ? d1 + d2 : tmax;
            }
            if (n) fprintf(stderr, "[%s-dbg] %3d workgroups with %2d c_fc + %d c_proj tiles: c_fc phase mean %.0f (min %.0f max %.0f) = %.0f per tile | c_proj phase mean %.0f (min %.0f max %.0f) = %.0f per tile | whole mean %.0f max %.0f [s_memtime ticks]\n",
                           tag, n, nf, np, f / n, fmin, fmax, nf ? f / n / nf : 0.0, q / n, qmin, qmax, np ? q / n / np : 0.0, (f + q) / n, tmax);
        }
    free(h);
    (void)hipFree(d);
    return e;
}
#endif

}  // namespace hg
