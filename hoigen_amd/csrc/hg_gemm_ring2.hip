// Persistent fp16 MFMA GEMM, 128 x 256 x 64 tiles, two phases per K-tile, three-stage LDS ring (gfx950).
//
// Used where 256x256 tiles would quantise badly over the 256 CUs: the N = 768 GEMMs of the ViT block
// (attention out-projection, MLP c_proj; 1182 tiles = 4.6 rounds instead of 591 = 2.3) and mid-sized
// problems.  Same conventions as hg_gemm_ring.hip (W rows as the MFMA A operand, activations as B, so a
// lane holds 4 consecutive output columns of one row; XOR-swizzled LDS images written by buffer_load...lds;
// bias staged in LDS; persistent workgroups walking their tiles as one K-tile stream).
//
// 512 threads = 8 waves as 2(M) x 4(N); a wave owns 32 rows of each A half (64 rows) and 32 columns of
// each W half (128 columns): acc[ha][hb] = 2 x 2 MFMA tiles of 16x16, 64 accumulator VGPRs.  LDS stage =
// A (16 KiB: half 0 | half 1) + W0 (16 KiB) + W1 (16 KiB) = 48 KiB, three stages.
//
//   phase   fetch segment: LDS reads -> regs   DMA refill issued      vmcnt before its barrier     MFMA segment
//   PA(t)   A0(t) W0(t) W1(t)                  A(t+2)  [2 DMA/wave]   -                            (A0,W0) (A0,W1)
//   PB(t)   A1(t)                              W(t+3)  [4 DMA/wave]   vmcnt(10) -> A,W(t+1) landed  (A1,W0) (A1,W1)
//
// Stage t%3 is refilled with tile t+3: its W halves as soon as PA(t) has read them (issued in PB(t)), its A
// once PB(t) has read half 1 (issued in PA(t+1)).  Two K-tiles (96 KiB) are in flight across the barriers.
// Every phase is [fetch] barrier [16 MFMAs] barrier, waves 4-7 one barrier interval behind waves 0-3.
#include <stdio.h>
#include <stdlib.h>

#include "hg_gemm_ring2_body.h"

namespace hg {

// the stand-alone kernel: the body over the XCD-chunked, n-group-major tile list
template <int EPI, int HL = 0, bool GS = false>
__global__ __launch_bounds__(512, 2) void gemm_ring2(const GemmArgs p, const int tiles_n, const int n_tiles,
                                                     const unsigned a_bytes, const int mode, const int gsz) {
#if defined(__HIP_DEVICE_COMPILE__)
    const RingTileList sc(n_tiles, tiles_n, gsz);
    if (sc.n_items() <= 0) return;
    gemm_ring2_body<EPI, HL, GS>(p, tiles_n, a_bytes, mode, sc);
#endif
}

template <int EPI, int HL = 0, bool GS = false>
static hipError_t launch_ring2_t(const GemmArgs& a, hipStream_t s) {
    constexpr int RING = 3 * 49152;
    const int LDS = RING + a.N * 4 * (GS ? 2 : 1);
    if (LDS > 160 * 1024) return hipErrorInvalidValue;
    static bool attr_set_d[HG_MAX_DEVICES] = {};      // function attributes and CU counts are per device
    static int n_cu_d[HG_MAX_DEVICES];
    const int dev_i = current_device_index();
    bool& attr_set = attr_set_d[dev_i];
    int& n_cu = n_cu_d[dev_i];
    if (!attr_set) {
        n_cu = 256;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_ring2<EPI, HL, GS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            n_cu = prop.multiProcessorCount;
        attr_set = true;
    }
    const int tiles_m = (a.M + 127) / 128, tiles_n = a.N / 256;
    const int n_tiles = tiles_m * tiles_n;
    const int grid = n_tiles < n_cu ? n_tiles : n_cu;
    const size_t a_bytes = (size_t)tiles_m * 128 * a.lda * 2;
    // start stagger: estimated cycles per K-tile (a deliberate under-estimate), in the kernel's `mode` >> 8
    constexpr int mode = 2200 << 8;
    // column tiles per L2 group: W slices of one group (gsz * 256 rows * K * 2 B) should fit ~1.5 MiB, but
    // never fewer than 3: an A panel that is not shared by neighbouring column tiles is re-read from HBM once
    // per column tile (c_proj, K = 3072: 310 MB of activations x 3)
    int gsz = (int)((1536 * 1024) / ((size_t)512 * a.K));
    if (gsz < 3) gsz = 3;
    if (gsz > tiles_n) gsz = tiles_n;
    {                                                    // equal groups: 9 column tiles -> 3 + 3 + 3, not 4 + 4 + 1
        const int ngroups = (tiles_n + gsz - 1) / gsz;
        gsz = (tiles_n + ngroups - 1) / ngroups;
    }
#ifdef HG_STAMPS
    if (getenv("HG_STAMPS")) {
        const size_t n = (size_t)grid * 8 * 16;
        unsigned long long* d = nullptr;
        if (hipMalloc(&d, n * 8) != hipSuccess) return hipErrorOutOfMemory;
        hipMemsetAsync(d, 0, n * 8, s);
        GemmArgs b = a;
        b.dbg = d;
        hipLaunchKernelGGL((gemm_ring2<EPI, HL, GS>), dim3(grid), dim3(512), LDS, s, b, tiles_n, n_tiles, (unsigned)a_bytes, mode, gsz);
        hipStreamSynchronize(s);
        unsigned long long* h = (unsigned long long*)malloc(n * 8);
        hipMemcpy(h, d, n * 8, hipMemcpyDeviceToHost);
        static const char* names[8] = {"vmcnt", "lgkmcnt", "fetch-barrier", "MFMA", "mfma-barrier", "-", "-", "epilogue"};
        for (int w = 0; w < 8; w += 4) {
            double acc[10] = {0};
            for (int blk = 0; blk < grid; ++blk)
                for (int k = 0; k < 10; ++k) acc[k] += (double)h[(size_t)(blk * 8 + w) * 16 + k];
            const double kts = acc[9] > 0 ? acc[9] : 1;
            fprintf(stderr, "[stamps] ring2<%d> N=%d K=%d wave %d: loop %.0f cycles/K-tile;", EPI, a.N, a.K, w, acc[8] / kts);
            for (int k = 0; k < 8; ++k)
                if (((HG_STAMP_MASK >> k) & 1) && names[k][0] != '-') fprintf(stderr, " %s %.0f", names[k], acc[k] / kts);
            fprintf(stderr, "\n");
        }
        free(h);
        hipFree(d);
        return hipGetLastError();
    }
#endif
    hipLaunchKernelGGL((gemm_ring2<EPI, HL, GS>), dim3(grid), dim3(512), LDS, s, a, tiles_n, n_tiles, (unsigned)a_bytes, mode, gsz);
    return hipGetLastError();
}

// N*4 bytes of bias must fit behind the 144 KiB ring
bool gemm_ring2_ok(const GemmArgs& a) { return gemm_ring_ok(a) && a.N <= 3072; }

hipError_t launch_gemm_ring2(int epi, const GemmArgs& a_in, hipStream_t s) {
    GemmArgs a = a_in;
    if (!a.ld2) a.ld2 = a.ldc;
    if (a.ld2 % 8) return hipErrorInvalidValue;
    switch (epi) {
        case EPI_BIAS_F16: return launch_ring2_t<EPI_BIAS_F16>(a, s);
        case EPI_BIAS_QGELU_F16: return launch_ring2_t<EPI_BIAS_QGELU_F16>(a, s);
        case EPI_BIAS_RELU_F16: return launch_ring2_t<EPI_BIAS_RELU_F16>(a, s);
        case EPI_BIAS_RESID_F32: return launch_ring2_t<EPI_BIAS_RESID_F32>(a, s);
        case EPI_BIAS_F32: return launch_ring2_t<EPI_BIAS_F32>(a, s);
        case EPI_PATCH_F32: return launch_ring2_t<EPI_PATCH_F32>(a, s);
        case EPI_BIAS_RELU_F32: return launch_ring2_t<EPI_BIAS_RELU_F32>(a, s);
        case EPI_SCALE_RESID_F32: return launch_ring2_t<EPI_SCALE_RESID_F32>(a, s);
        case EPI_RESID_LN_F32:
            if (a.hl && (!a.lo || !a.mu || ((a.hl == 2 || a.hl == 3) && !a.muc))) return hipErrorInvalidValue;      // (the hi half lives at out2 with row stride ld2: any)
            if (a.gamma) {      // the copy scaled by the next LayerNorm's weight (hl 1, 2: in out3 beside the stream's hi half in out2)
                if ((a.hl == 1 || a.hl == 2) && (!a.out3 || a.ld3 < a.N || (a.ld3 % 8))) return hipErrorInvalidValue;
                switch (a.hl) {
                    case 0: return launch_ring2_t<EPI_RESID_LN_F32, 0, true>(a, s);
                    case 1: return launch_ring2_t<EPI_RESID_LN_F32, 1, true>(a, s);
                    case 2: return launch_ring2_t<EPI_RESID_LN_F32, 2, true>(a, s);
                    case 3: return launch_ring2_t<EPI_RESID_LN_F32, 3, true>(a, s);
                    default: return hipErrorInvalidValue;
                }
            }
            switch (a.hl) {
                case 0: return launch_ring2_t<EPI_RESID_LN_F32, 0>(a, s);
                case 1: return launch_ring2_t<EPI_RESID_LN_F32, 1>(a, s);
                case 2: return launch_ring2_t<EPI_RESID_LN_F32, 2>(a, s);
                case 3: return launch_ring2_t<EPI_RESID_LN_F32, 3>(a, s);
                default: return hipErrorInvalidValue;
            }
        default: return hipErrorInvalidValue;
    }
}

}  // namespace hg
