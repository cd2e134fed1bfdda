// Fused in_proj (QKV projection, LayerNorm folded in) + CAUSAL scaled-dot-product attention for the text tower on gfx950: the
// short-sequence member of the hg_qkv_attn.hip family.  Replaces the pair  gemm_ring<EPI_LN_BIAS_F16> -> attention_kernel<causal>
// of a text-tower block (clipnet/model.py:171,181-183) for L <= 80: q, k and v never reach HBM (600 prompts x 77 tokens, D = 512:
// 142 MB written and read back per block by the separate kernels).
//
// Work item = (PACK of G = floor(160 / L) whole sequences, head PAIR): a 160 x 384 output tile [q_a | k_a | v_a | q_b | k_b | v_b]
// (10 row blocks x 24 column blocks of 16), K = D.  Two sequences per pack at L = 77, ten at L = 16, 160 at L = 1; the sequences sit
// back to back (tile row L g), the last pack of a call may hold fewer.  Items are dealt XCD-wise so that the head pairs of a pack
// run side by side on one XCD.
//
// GEMM phase: the K loop of hg_qkv_attn.hip (hg_seq_dev.h, hg_seq_kloop*.inc) with 10 row blocks: 8 waves along N, 10 x 3
// accumulator blocks = 120 VGPRs per wave, the A ring fed by buffer_load ... lds (20 pieces of 8 rows per K-tile: two per wave, a
// third from waves 0-3), wave-private W rings of packed fragments (pack_qkv_kernel), counted vmcnt.  K-tile schedules: 3 m
// (D = 768: the text tower of ViT-L/14@336) and 3 m + 2 (D = 512: eight K-tiles; the last one sits in stage 1 and K-tile nk - 2
// holds stage 0 to the end, so the next item's first K-tile is fetched behind the loop, as in the 3 m + 1 schedule).
// Epilogue: rstd * (acc - (mean - c) * cs) + b', the expression and the rounding of EPI_LN_BIAS_F16, written to LDS as Q, K, V rows
//   of 128 B, swizzled by the row's index in its own sequence.
// Attention phase: per sequence of the pack, attention_kernel's tile functions (hg_attn_dev.h) with the causal mask: the pack's
//   (sequence, 32-query tile) pairs go round-robin to the waves, a wave walks the key tiles up to its diagonal.  A sequence never
//   attends to a pack neighbour, and a neighbour's non-finite values never reach it: keys >= L are masked in the scores and their
//   V values are read as zeros (tile_softmax_pv<.., VMASK>).  Bit-identical to the separate kernels (tests/test_gpu_qkv_attn_text.py).
//
// LDS (151 808 B): W rings 48 KiB | A stage 0 20 KiB | 76 KiB: A stages 1 and 2 during the K loop (40 KiB); Q, K, V of one head
// (3 x 20 KiB) and the waves' output staging (8 x 2 KiB) during the attention phases | bias' and column sums of the pair (3 KiB) |
// (mean - c, rstd) of the 160 rows (1 280 B).
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "hg_attn_dev.h"
#define SQ_RB_BLOCKS 10
#define SQ_S12_KIB 76
#include "hg_seq_dev.h"

namespace hg {

namespace {
constexpr int QT_RB = SQ_RB;                       // 16-row blocks of a pack tile: 160 rows
[[maybe_unused]] constexpr int QT_NCB = SQ_NCB;                     // 16-column blocks per wave
constexpr int QT_ASTG = SQ_ASTG;                   // one A stage = one Q / K / V matrix: 160 rows x 128 B
[[maybe_unused]] constexpr int QT_ATT = SQ_S12;    // stages 1 and 2 of the K loop = the attention operands
[[maybe_unused]] constexpr int QT_OT_BYTES = 8 * 2048;              // output staging, 2 KiB per wave, behind V (whose last tile reads up to 15 rows on: masked)
[[maybe_unused]] constexpr int QT_OT = QT_ATT + 3 * QT_ASTG;
constexpr int QT_BCS = SQ_END;                     // bias'[384] | cs[384] in tile column order
constexpr int QT_MR = QT_BCS + 2 * 384 * 4;
constexpr int QT_LDS = QT_MR + QT_RB * 16 * 8;
constexpr int QT_MAX_L = 80;
static_assert(QT_LDS <= 160 * 1024, "LDS budget");
static_assert(QT_RB * 16 >= 2 * QT_MAX_L, "a pack holds two of the longest sequences");
}  // namespace

// the dynamic LDS size both instances are launched with, as data of the code object (tests/test_qkv_attn_text_resources.py reads it there)
extern "C" __device__ __attribute__((used)) const int hg_qkv_attn_text_lds_bytes = QT_LDS;

#define QT_KERNEL qkv_attn_kernel_text
#define SQ_NKMOD 0
#include "hg_qkv_attn_text_body.inc"
#undef QT_KERNEL
#undef SQ_NKMOD
// D = 512 (8 K-tiles): the text tower of ViT-B
#define QT_KERNEL qkv_attn_kernel_text_k2
#define SQ_NKMOD 2
#include "hg_qkv_attn_text_body.inc"
#undef QT_KERNEL
#undef SQ_NKMOD

bool qkv_attn_text_ok(int n_seq, int L, int D, int heads, int lda) {
    if (n_seq < 1 || heads < 2 || (heads & 1) || D != heads * 64) return false;
    if (L < 1 || L > QT_MAX_L) return false;
    const int nk = D / 64;
    if (nk < 6 || nk % 3 == 1) return false;                      // K-tile schedules: 3 m and 3 m + 2
    if (lda < D || (lda & 7)) return false;
    const size_t Mp = (size_t)(((size_t)n_seq * L + 255) / 256) * 256;
    if (Mp * lda * 2 >= (1ull << 31) || (size_t)3 * D * D * 2 >= (1ull << 31)) return false;
    return true;
}

int qkv_attn_text_items(int n_seq, int L, int heads) {
    const int G = QT_RB * 16 / L;
    return ((n_seq + G - 1) / G) * (heads / 2);
}

// Option qkv_attn_text = 1: whether the one kernel beats the two it replaces at this shape.  Measured per launch, fused / separate
// (profiles/qkv_attn_text.txt section 1; items = packs x head pairs, rounds = items / 256 CUs):
//   below one round it depends on the item: 64 x 77 (0.50 rounds) 0.90, but 600 x 13 (0.78 rounds: twelve sequences per pack, 45 us
//   per item against a 30 us GEMM) 1.12;  one round and more with the last round well filled: 1.00 rounds 0.68, 2.56: 0.96, 4.00: 0.92,
//   4.69: 0.96, 10.23: 0.90;  a third round a third full: 2.32 rounds 1.02, 2.34: 0.99.
// So: at least one full round of items, and at most a fifth of the launch's CU-rounds idle in the tail (0.227 and 0.22 in the two
// cases that do not pay, <= 0.15 in every case that does).  Results are bit-identical either way.
bool qkv_attn_text_pays(int n_seq, int L, int heads, int n_cu) {
    if (n_cu <= 0) n_cu = 256;
    const long items = qkv_attn_text_items(n_seq, L, heads);
    const long rounds = (items + n_cu - 1) / n_cu;
    return items >= n_cu && items * 100 >= rounds * n_cu * 80;
}

hipError_t launch_qkv_attn_text(const QkvAttnArgs& a_in, hipStream_t s) {
    QkvAttnArgs a = a_in;
    if (a.K <= 0) a.K = a.D;
    if (a.K != a.D || !qkv_attn_text_ok(a.n_seq, a.L, a.D, a.heads, a.lda) || !a.x16 || !a.wp || !a.bcs || !a.mr || !a.out)
        return hipErrorInvalidValue;
    if (a.ldo <= 0) a.ldo = a.D;
    if (a.ldo < a.D || (a.ldo & 7)) return hipErrorInvalidValue;
    const int HP = a.heads / 2;
    if (a.gsz <= 0 || HP % a.gsz) a.gsz = HP;
    static bool attr_set_d[HG_MAX_DEVICES] = {};
    static int n_cu_d[HG_MAX_DEVICES];
    const int dev_i = current_device_index();
    if (!attr_set_d[dev_i]) {
        n_cu_d[dev_i] = 256;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qkv_attn_kernel_text), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        if (e != hipSuccess) return e;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&qkv_attn_kernel_text_k2), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
        if (e != hipSuccess) return e;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu_d[dev_i] = prop.multiProcessorCount;
        attr_set_d[dev_i] = true;
    }
    const int n_items = qkv_attn_text_items(a.n_seq, a.L, a.heads);
    int grid = n_cu_d[dev_i] & ~7;                 // XCD-wise dealing wants a multiple of 8
    if (grid < 8) grid = n_cu_d[dev_i];
    if (n_items < grid) grid = n_items;            // (not a multiple of 8: plain dealing)
    if (!a.a_bytes) a.a_bytes = (unsigned)((size_t)(((size_t)a.n_seq * a.L + 255) / 256) * 256 * a.lda * 2);
    if ((a.K / 64) % 3 == 0) hipLaunchKernelGGL(qkv_attn_kernel_text, dim3(grid), dim3(512), QT_LDS, s, a);
    else hipLaunchKernelGGL(qkv_attn_kernel_text_k2, dim3(grid), dim3(512), QT_LDS, s, a);      // (K / 64 = 3 m + 2)
    return hipGetLastError();
}

}  // namespace hg
