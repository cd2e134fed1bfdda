// What the two persistent MLP launches share (hg_mlp_pair.hip: c_proj on ring2's 128-row tiles; hg_mlp_pair256.hip: c_proj on 256-row
// tiles): the census geometry, the compact kernel arguments of the two bodies and how c_proj's are read late.  hg_mlp_pair.hip holds
// the description of the hand-off.
#pragma once
#include "hg_gemm_dev.h"

namespace hg {

constexpr int MLP_SPIN_LIMIT = 1 << 20;    // polls of a ready counter (~0.5 us each: s_sleep 16) before giving up
constexpr int MLP_NX = 8;                  // XCDs (HW_REG_XCC_ID 0 .. 7)
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

}  // namespace hg
