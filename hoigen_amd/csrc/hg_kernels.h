// Host-callable launchers of the gfx950 kernels (internal; the public ABI is include/hoigen_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hg_common.h"

namespace hg {

// ---- GEMM:  D[m][n] = sum_k A[m][k] * W[n][k]  (fp16 operands, fp32 accumulate) ---------------
enum Epilogue : int {
    EPI_BIAS_F16 = 0,        // out fp16 [M,ldc] = acc + bias
    EPI_BIAS_QGELU_F16 = 1,  // out fp16 = quickgelu(acc + bias)        (clipnet/model.py:162-164)
    EPI_BIAS_RELU_F16 = 2,   // out fp16 = relu(acc + bias)
    EPI_BIAS_RESID_F32 = 3,  // out fp32 += acc + bias   (residual stream, in place)
    EPI_BIAS_F32 = 4,        // out fp32 = acc + bias (bias may be null)
    EPI_PATCH_F32 = 5,       // patch embedding: row m=(b,t) -> out row b*L+1+t (+ pos[1+t] when GemmArgs::pos is given)
    EPI_BIAS_RELU_F32 = 6,   // out fp32 = relu(acc + bias)
    EPI_SCALE_RESID_F32 = 7, // out fp32 += (acc + bias) * pos[n]   (adapter up_proj * scale, residual)
    // LayerNorm folded into the GEMM (ring kernels only): A = raw fp16 copy of the residual rows, W = gamma-folded
    // weight, cs[n] = sum_k W'[n][k], bias' = bias + W beta, mr[m] = (mean, rstd) of row m:
    //     out = rstd[m] * (acc - mean[m] * cs[n]) + bias'[n]
    EPI_LN_BIAS_F16 = 8,
    EPI_LN_BIAS_QGELU_F16 = 9,
    // residual update that also emits what the next folded-LN GEMM needs (ring2 kernel only):
    //     out fp32 += acc + bias;  out2 fp16 = the updated rows;  stats[m][tile_n] = (sum, sum of squares) over the tile's columns
    EPI_RESID_LN_F32 = 10,
    // A = centred fp16 copy of the stream (x - mu[m]): out fp32 = relu(acc + mu[m] * cs[n] + bias[n]) = relu(W x + b)
    // (adapter down_proj on the copy the residual GEMMs emit; simple kernel only)
    EPI_MU_BIAS_RELU_F32 = 11,
    // EPI_RESID_LN_F32 with the update scaled per column: out fp32 += (acc + bias) * pos[n]; fp16 copy + statistics
    // (adapter up_proj: LayerNorm folding stays on behind the adapter; duo kernel only)
    EPI_SCALE_RESID_LN_F32 = 12
};

// Low half of a residual stream held as centre + hi + lo (GemmArgs::hl): bf8 (e5m2: the top byte of the fp16 remainder, rounded to
// nearest even by v_cvt_pk_bf8_f32; 13-14 bits of x - centre, 6 bytes per element through a residual epilogue).
// The bf8 low half holds the remainder TIMES 2^10: the remainder of an fp16 rounding is <= 2^-11 of the element, so unscaled it sits
// 11 binades below hi and - e5m2 has fp16's exponent range - flushes to zero once the element is below ~0.25 (a stream whose rows
// spread by 0.02 would travel as fp16 alone); scaled it is normal wherever |x - centre| >= 2.4e-4 (hi: 6.1e-5) and cannot overflow
// (<= half of |hi|).  One packed multiply on the way out, the add on the way in becomes a packed fma.
#ifndef HG_LO_SCALE
#define HG_LO_SCALE 1024.0f
#endif

struct GemmArgs {
    const half_t* A;   // [M, lda] (K contiguous)
    const half_t* W;   // [N, K]
    const float* bias; // [N] or nullptr
    void* out;
    const float* pos;  // EPI_PATCH: positional embedding [L, N]
    int lda, ldc;
    int M, N, K;
    int G, L;          // EPI_PATCH: patches per image, tokens per image
    const float* cs = nullptr;   // EPI_LN_*: [N] column sums of the folded weight
    const float* mr = nullptr;   // EPI_LN_*: [M][2] (row mean minus the centre of the fp16 copy, rstd)
    const float* mu = nullptr;   // EPI_RESID_LN: [M] centre subtracted from the fp16 copy (the row's previous mean)
    half_t* out2 = nullptr;      // EPI_RESID_LN: fp16 copy of the updated rows, leading dimension ld2 (0 = ldc)
    int ld2 = 0;                 //   a stride other than ldc exists in gemm_ring2 only (the dispatcher routes it there)
    float* stats = nullptr;      // EPI_RESID_LN: [M][stats_ld][2] partial (sum, sumsq) per row and wave column group
    int stats_ld = 0;            //   = 4 * N / 256
    // EPI_BIAS_F32 / EPI_BIAS_RELU_F32 with two destinations: columns >= n_split go to out_hi[m * ldc + (n - n_split)]
    // (the stacked mean | log_var GEMM of the VAE encoder writes its two halves straight into the caller's tensors)
    void* out_hi = nullptr;
    int n_split = 0;                     // multiple of 16
    unsigned long long* dbg = nullptr;   // diagnostics: s_memtime totals (HG_STAMPS build), normally null
    // EPI_RESID_LN with the residual stream held as TWO fp16 halves instead of fp32 (gemm_ring2 only; DESIGN.md 4 "hi / lo"):
    //   x = centre + hi + lo,   hi = fp16(x - centre) = the centred copy `out2` the next GEMM reads anyway,
    //   lo = fp16((x - centre) - hi) in `lo` (tile-fragment order: only this kernel family reads it, 16 B per lane, whole lines)
    // hl: 0 fp32 in / fp32 out (`out`), 1 fp32 in / hi+lo out, 2 hi+lo in / hi+lo out, 3 hi+lo in / fp32 out (+ copy as always).
    // muc [M] = the centre the hi / lo being READ were written with (finalize_stats' muc); mu = the centre to write with.
    int hl = 0;
    half_t* lo = nullptr;
    const float* muc = nullptr;
    // EPI_RESID_LN_F32 (gemm_ring2): gamma [N] = the NEXT LayerNorm's weight, multiplied into the copy the next GEMM reads -
    // fp16((x - mu) * gamma) - so that GEMM runs on the layer's own fp16 weights with cs[n] = sum_k gamma[k] W[n][k] (fold_ln's csg).
    // hl 0 / 3: out2 is that scaled copy; hl 1 / 2: out2 stays the stream's unscaled hi half and the scaled copy goes to out3 (row stride ld3)
    const float* gamma = nullptr;
    half_t* out3 = nullptr;
    int ld3 = 0;
};
// bytes of the `lo` buffer for M rows x N columns (whole 128 x 256 tiles)
inline size_t gemm_lo_bytes(int M, int N) { return (size_t)((M + 127) / 128) * (N / 256) * 65536; }

// Requirements: N % 128 == 0, K % 64 == 0, A readable for rows < M, 16-byte aligned rows.
// A must be allocated with its row count padded to a multiple of 256 (the ring kernel's DMA reads whole
// tiles; rows >= M are never stored).
hipError_t launch_gemm(int epi, const GemmArgs& a, hipStream_t s);
double gemm_flops(const GemmArgs& a);
// persistent ring kernel (hg_gemm_ring.hip) and the simple 128x128 kernel (hg_gemm.hip)
bool gemm_ring_ok(const GemmArgs& a);
hipError_t launch_gemm_ring(int epi, const GemmArgs& a, hipStream_t s);
bool gemm_ring2_ok(const GemmArgs& a);
// LayerNorm-folding epilogues exist only in the ring kernels: EPI_LN_* in gemm_ring (bias + column sums must fit
// behind the ring), EPI_RESID_LN_F32 in gemm_ring2
bool gemm_ln_ok(int epi, const GemmArgs& a);
hipError_t launch_gemm_ring2(int epi, const GemmArgs& a, hipStream_t s);
hipError_t launch_gemm_simple(int epi, const GemmArgs& a, hipStream_t s);
// c_fc -> QuickGELU -> c_proj of a block as ONE persistent launch (hg_mlp_pair.hip): fc = the EPI_LN_BIAS_QGELU_F16 GEMM, proj = the
// EPI_RESID_LN_F32 GEMM that reads fc.out; ready [mlp_pair_ready_words(M)] u32 zeroed on the stream before the launch; err: host-mapped
// word set when a hand-off wait times out; ch: 256-row panels of an XCD per chunk of the c_fc tile order; fc_slots: workgroups per XCD
// that run c_fc tiles (of n_cu / 8)
bool mlp_pair_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu);
bool mlp_pair_shapes_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu);      // ... without its bound of 2 048 rows
size_t mlp_pair_ready_words(int M);
hipError_t launch_mlp_pair(const GemmArgs& fc, const GemmArgs& proj, unsigned* ready, int* err, int ch, int fc_slots, int n_cu, hipStream_t s,
                           int grid_short = 0);      // grid_short (fault injection: hg_api.hip option mlp_pair_fault): workgroups NOT launched
// ... with c_proj on 256 x 256 tiles (hg_mlp_pair256.hip): the same arguments, ready words, error word and bits; no text-tower (gamma) form
bool mlp_pair256_ok(const GemmArgs& fc, const GemmArgs& proj, int n_cu, int min_m);
hipError_t launch_mlp_pair256(const GemmArgs& fc, const GemmArgs& proj, unsigned* ready, int* err, int ch, int ratio, int n_cu,
                              hipStream_t s, int grid_short = 0);      // ch: panels per chunk of the c_fc order; ratio: c_fc tile times per c_proj tile
// ... and c_proj's K loop in the two-phase form (hg_mlp_pair256p.hip): whatever mlp_pair256_ok takes, the same arguments and bits
hipError_t launch_mlp_pair256p(const GemmArgs& fc, const GemmArgs& proj, unsigned* ready, int* err, int ch, int ratio, int n_cu,
                               hipStream_t s, int grid_short = 0);
// two 4-wave workgroups per CU, 128x256 tiles, free-running (hg_gemm_duo.hip): residual GEMMs and fp16/fp32 outputs
bool gemm_duo_ok(int epi, const GemmArgs& a);
hipError_t launch_gemm_duo(int epi, const GemmArgs& a, hipStream_t s);

// ---- attention: softmax(Q K^T / sqrt(64) [+causal]) V, head_dim 64 --------------------------
// qkv fp16 [n_seq*L, 3*D] rows = tokens (q|k|v column blocks, head h = 64h..64h+63);
// out fp16 [n_seq*L, D].  1 <= L <= ATTN_LONG_MAX_L, either mask; above it hipErrorInvalidValue.
// L <= ATTN_MAX_L_RESIDENT: attention_kernel (hg_attn.hip, one wave per 32-query tile); longer: attention_long_kernel
// (hg_attn_long.hip, up to 16 waves walking the query tiles; 640 = the K and V rows that fill a CU's 160 KiB of LDS)
// ldo: row stride of out in halfs (0 = heads * 64)
// pack: L <= 32 (one wave per item) runs four items per workgroup (dispatch-bound otherwise; bit-identical)
static constexpr int ATTN_MAX_L_RESIDENT = 224;
static constexpr int ATTN_LONG_MAX_L = 640;
hipError_t launch_attention(const half_t* qkv, half_t* out, int n_seq, int L, int heads, bool causal,
                            hipStream_t s, int ldo = 0, bool pack = true);
// attention of ONE query row per sequence (row sel[seq], row 0 when sel is null; sel[seq] < L): K and V from
// qkv [n_seq*L, 3*heads*64], the queries from q0 [n_seq, heads*64] (dense), out [n_seq, heads*64] (dense)
hipError_t launch_attention_row0(const half_t* qkv, const half_t* q0, const int32_t* sel, half_t* out, int n_seq, int L,
                                 int heads, bool causal, hipStream_t s);
// the two forms for ATTN_MAX_L_RESIDENT < L <= ATTN_LONG_MAX_L (hg_attn_long.hip); launch_attention / launch_attention_row0 dispatch
hipError_t launch_attention_long(const half_t* qkv, half_t* out, int n_seq, int L, int heads, bool causal, hipStream_t s, int ldo);
hipError_t launch_attention_long_row0(const half_t* qkv, const half_t* q0, const int32_t* sel, half_t* out, int n_seq, int L,
                                      int heads, bool causal, hipStream_t s);

// ---- masked attention with head_dim 32 and separate query / key lengths (hg_detr_attn.hip: the DETR transformer) -------------
// out = softmax(q k^T / sqrt(32) + key_padding_mask) v per (sequence, head).  q [n_seq * Lq, ldq], k [n_seq * Lk, ldk],
// v [n_seq * Lk, ldv] fp16, each with its own pointer (16-byte aligned) and row stride in halfs (multiples of 8), head h = columns
// 32h .. 32h+31; mask uint8 [n_seq, Lk], 1 = padded key, nullable; out fp16 [n_seq * Lq, ldo] (ldo a multiple of 4).
// 1 <= Lq, Lk <= DETR_ATTN_MAX_L (42 x 42 = 1 764 tokens, the largest grid a stride-32 backbone makes of an 800 / 1333 resize in a
// batch of mixed orientations, rounded up to 32 keys); above it hipErrorInvalidValue and nothing launched.
// chunk: keys per LDS chunk - 0 = all keys at once while they fit (Lk <= DETR_ATTN_RESIDENT_L), DETR_ATTN_CHUNK_L beyond; otherwise a
// multiple of 32 up to DETR_ATTN_RESIDENT_L.  Every chunk size gives the same bits.
static constexpr int DETR_ATTN_MAX_L = 1792;
static constexpr int DETR_ATTN_RESIDENT_L = 1280;      // 2 x 64 B x 1 280 keys = a CU's 160 KiB
static constexpr int DETR_ATTN_CHUNK_L = 512;
static constexpr int DETR_ATTN_NW = 4;                 // waves per workgroup = 32-query tiles per slab (DetrAttnArgs::waves: 1 or 2 instead)
struct DetrAttnArgs {
    const half_t *q, *k, *v;
    int ldq, ldk, ldv;
    const uint8_t* mask;
    half_t* out;
    int ldo;
    int n_seq, Lq, Lk, heads;
    int chunk;
    int waves = 0;      // query tiles per slab = waves per workgroup: 0 = DETR_ATTN_NW, else 1, 2 or 4.  Same bits
};
int detr_attn_chunk_rows(int Lk, int chunk);      // keys per LDS chunk the launch uses
hipError_t launch_detr_attention(const DetrAttnArgs& a, hipStream_t s);

// ---- row kernels of the DETR encoder (hg_detr_rows.hip) ------------------------------------------------------------------------------
// entry: src / pos fp32 with element strides (batch, token) and contiguous channels -> x fp32 [B*S, D] (sequence-major per image),
// x16 = fp16(x), xp16 = fp16(x + pos), posb = pos batch-major [B*S, D]
hipError_t launch_detr_entry(const float* src, const float* pos, long long sb, long long ss, long long pb, long long ps, int B, int S, int D,
                             float* x, half_t* x16, half_t* xp16, float* posb, hipStream_t s);
// post-norm: x = LayerNorm(x; w, b) in place (fp32, eps 1e-5, biased variance), x16 = fp16(x), xp16 = fp16(x + posb) (xp16 nullable),
// copy = x (nullable: the trace; written element by element, 4-byte alignment is enough).  D a multiple of 4
hipError_t launch_detr_postnorm(float* x, const float* w, const float* b, const float* posb, half_t* x16, half_t* xp16, float* copy, int M,
                                int D, hipStream_t s);
// exit: out[b * ob + t * os + c] = x[(b * S + t) * D + c]
hipError_t launch_detr_exit(const float* x, float* out, long long ob, long long os, int B, int S, int D, hipStream_t s);

// ---- row kernels of the DETR decoder (hg_detr_rows.hip) ------------------------------------------------------------------------------
// entry: x fp32 [B*Q, D] (batch-major) = tgt (null: zeros, nothing is read), x16 = fp16(x), xp16 = fp16(x + query_pos), qposb =
// query_pos batch-major; tgt / query_pos element (b, q, ch) at b * stride_b + q * stride_q + ch (a batch stride of 0 broadcasts)
hipError_t launch_detr_dec_entry(const float* tgt, long long tb, long long tq, const float* qpos, long long qb, long long qq, int B, int Q,
                                 int D, float* x, half_t* x16, half_t* xp16, float* qposb, hipStream_t s);
// tail of a decoder layer: x = LayerNorm(((x + b2) + partial[0]) + ... + partial[n_slices - 1]; w3, b3) in place - b2 nullable (not
// added: the residual GEMM added it), partial [n_slices][M][D] fp32 in ascending slice order, n_slices >= 0 -, x16 = fp16(x), xp16 =
// fp16(x + qposb) (nullable), copy = x (nullable, 4-byte alignment), and with out: out[(row / Q) * ob + (row % Q) * oq + ch] =
// LayerNorm(x; wf, bf), which does not go back into the stream.  D a multiple of 4 up to 512
hipError_t launch_detr_dec_tail(float* x, const float* b2, const float* partial, int n_slices, const float* w3, const float* b3,
                                const float* qposb, half_t* x16, half_t* xp16, float* copy, const float* wf, const float* bf, float* out,
                                long long ob, long long oq, int Q, int M, int D, hipStream_t s);

// ---- the FFN of a short stream split over d_ff (hg_detr_ffn.hip): partial[slice][m][:] = fp16(relu(x16 W1[slice]^T + b1[slice])) W2[:, slice]^T
// x16 [M, D] fp16, W1 [F, D], W2 [D, F] fp16, b1 [F] fp32 (16-byte aligned); partial fp32 [F / DETR_FFN_SLICE][M][D]: exactly those
// bytes are written.  D = 128 or 256, F a multiple of DETR_FFN_SLICE up to 8192; otherwise hipErrorInvalidValue and nothing launched
static constexpr int DETR_FFN_ROWS = 32, DETR_FFN_SLICE = 128;
bool detr_ffn_ok(int M, int D, int F);
inline size_t detr_ffn_partial_bytes(int M, int D, int F) { return (size_t)(F / DETR_FFN_SLICE) * M * D * 4; }
hipError_t launch_detr_ffn(const half_t* x16, const half_t* W1, const float* b1, const half_t* W2, float* partial, int M, int D, int F,
                           hipStream_t s);

// ---- DETR's heads and PostProcess in one launch (hg_detr_heads.hip): class logits, the box MLP with its sigmoid, and - for the rows of
// the last level computed - softmax, the foreground maximum and the scaled xyxy boxes.  hs fp32 through element strides (level, image,
// query; channel stride 1), levels l0 .. l0 + L - 1 of it; wc [C1p, D] / bc [C1p] with C1p = C1 rounded up to 16, zero rows behind C1;
// w0, w1 [D, D]; w2 [16, D] / b2 [16] with zero rows behind 4 (fp16 matrices, fp32 biases, 16-byte aligned).  pred_logits [L, B, Q, C1]
// and pred_boxes [L, B, Q, 4] may be null; scores, labels [B, Q] and boxes [B, Q, 4] (16-byte aligned) may not.  sizes = (h, w) per image.
// vec4: hs and its strides allow 16-byte loads.  A shape outside detr_heads_ok: hipErrorInvalidValue and nothing launched.
static constexpr int DETR_HEADS_ROWS = 32, DETR_HEADS_MAX_C = 256, DETR_HEADS_MAX_L = 12, DETR_HEADS_MAX_B = 64, DETR_HEADS_MAX_Q = 1792;
struct DetrHeadsArgs {
    const float* hs;
    long long s_l, s_b, s_q;
    const half_t *wc, *w0, *w1, *w2;
    const float *bc, *b0, *b1, *b2;
    float *pred_logits, *pred_boxes, *scores;
    int32_t* labels;
    float* boxes;
    int D, C1, C1p, l0, L, B, Q, vec4;
    float sizes[2 * DETR_HEADS_MAX_B];
};
bool detr_heads_ok(int D, int C1, int L, int B, int Q);
hipError_t launch_detr_heads(const DetrHeadsArgs& a, hipStream_t s);

// ---- DETR's neck (hg_detr_neck.hip): src = fp16(x) fp16(W)^T + bias, the key-padding mask on the feature grid and the sine embedding.
// x fp32 [B, Cin, H W] through element strides x_sb (image) and x_sc (channel), token stride 1, no alignment beyond a float's; w fp16
// [D, Cin] and bias fp32 [D] (16-byte aligned); image_mask bytes [B, Hi, Wi], non-zero = padded; dim_t fp32 [D / 2].  src and pos fp32
// through element strides (image, token), channel stride 1; mask uint8 [B, H W]; pos and mask may be null.  nsplit slices of kslice =
// Cin / nsplit channels (a multiple of 64) each: with nsplit > 1 the slices go to partial, fp32 [nsplit][B H W][D] (16-byte aligned), and
// a second launch adds them in ascending order.  vec4: x and its strides allow 16-byte loads and H W is a multiple of 4; ovec4: src and
// its strides allow 16-byte stores.  A shape outside detr_neck_ok: hipErrorInvalidValue and nothing launched.
static constexpr int DETR_NECK_TOKENS = 32, DETR_NECK_MAX_CIN = 4096, DETR_NECK_MAX_B = 64, DETR_NECK_MAX_IMG = 8192;
struct DetrNeckArgs {
    const float* x;
    long long x_sb, x_sc;
    const half_t* w;
    const float *bias, *dim_t;
    const unsigned char* image_mask;
    float *src, *pos;
    long long src_sb, src_ss, pos_sb, pos_ss;
    unsigned char* mask;
    float* partial;
    float scale;
    int Cin, D, B, H, W, Hi, Wi, normalize, nsplit, kslice, vec4, ovec4;
};
bool detr_neck_ok(int Cin, int D, int B, int H, int W, int Hi, int Wi);
inline size_t detr_neck_partial_bytes(int nsplit, int B, int S, int D) { return nsplit > 1 ? (size_t)nsplit * B * S * D * 4 : 0; }
hipError_t launch_detr_neck(const DetrNeckArgs& a, hipStream_t s);

// ---- ResNet bottleneck convolutions (hg_resnet_conv.hip): out = epilogue(conv(x, w)) as one implicit GEMM over NHWC fp16 activations.
// x fp16 [B, H, W, Cin]; w fp16 in fragment order (launch_resnet_pack from torch's fp32 [Cout, Cin, R, R]); scale, bias fp32 [Cout];
// identity fp32 [B Ho Wo, Cout] (epi 3); out32 fp32 / out16 fp16 [B Ho Wo, Cout]; every pointer 16-byte aligned.  R in {1, 3}, stride in
// {1, 2}, pad (R - 1) / 2, Ho / Wo = resnet_out_size.  epi 1 relu(fmaf) -> out16; 2 fmaf -> out32; 3 relu(fmaf + identity) -> both.
// tile: output pixels of a work item, 0 = resnet_conv_tile's rule, else 32 or 128 (same bits either way).  A shape outside
// resnet_conv_ok: hipErrorInvalidValue and nothing launched.
static constexpr int RESNET_MAX_C = 2048, RESNET_MAX_C3 = 512, RESNET_MAX_SIDE = 1024, RESNET_MAX_B = 64, RESNET_MAX_BLOCKS = 64;
struct ResnetConvArgs {
    const half_t *x, *w;
    const float *scale, *bias, *identity;
    float* out32;
    half_t* out16;
    int B, H, W, Cin, Ho, Wo, Cout, R, stride, epi, tile;
};
inline int resnet_out_size(int H, int R, int stride) { return (H + 2 * ((R - 1) / 2) - R) / stride + 1; }
bool resnet_conv_ok(const ResnetConvArgs& a);
int resnet_conv_tile(long long M, int Cout);
hipError_t launch_resnet_conv(const ResnetConvArgs& a, hipStream_t s);
// w fp32 [Cout, Cin, R, R] -> the fp16 fragments; flag[0] = 1 where a weight is not finite or beyond fp16's range
hipError_t launch_resnet_pack(const float* w, half_t* out, int Cout, int Cin, int R, int* flag, hipStream_t s);
// x fp32 [B, C, H, W] through element strides (image, channel, row), column stride 1 -> fp32 and fp16 NHWC
hipError_t launch_resnet_entry(const float* x, long long sb, long long sc, long long sr, int B, int C, int H, int W, float* o32, half_t* o16,
                               hipStream_t s);
// x fp32 NHWC [B, S, C] -> out fp32 [B, C, S] through element strides (image, channel), token stride 1
hipError_t launch_resnet_exit(const float* x, int B, int C, int S, float* out, long long sb, long long sc, hipStream_t s);

// ---- global average pool + L2 normalisation behind the last block (hg_resnet_pool.hip): x fp32 NHWC [B, HW, C] -> pooled [B, C] = the
// mean over the HW positions (one fp32 accumulator per (image, channel), positions added in ascending order, one division by (float)HW)
// and features [B, C] = pooled / ||pooled||_2 (sum of squares, sqrtf, reciprocal, one multiply); either output nullable, not both.
// One workgroup of RESNET_POOL_THREADS threads per image, a thread's channels RESNET_POOL_THREADS apart.  C % 64 == 0, C <= RESNET_MAX_C,
// 1 <= HW <= RESNET_MAX_SIDE^2, B <= RESNET_MAX_B; outside resnet_pool_ok: hipErrorInvalidValue and nothing launched.
static constexpr int RESNET_POOL_THREADS = 256;
bool resnet_pool_ok(const float* x, int B, int HW, int C, const float* pooled, const float* features);
hipError_t launch_resnet_pool(const float* x, int B, int HW, int C, float* pooled, float* features, hipStream_t s);

// ---- ResNet stem (hg_resnet_stem.hip): maxpool3x3/2,pad1(relu(fmaf(conv7x7/2,pad3(x, w), scale, bias))) in one launch, 3 -> 64 channels.
// x fp32 [B, 3, Hi, Wi] through element strides sb, sc, sr (image, channel, row), column stride 1, 4-byte aligned; w fp16 in fragment
// order (launch_resnet_stem_pack from torch's fp32 [64, 3, 7, 7]); scale, bias fp32 [64]; out32 fp32 / out16 fp16 NHWC [B, Hp, Wp, 64],
// 16-byte aligned.  Hc / Wc = resnet_stem_conv_size, Hp / Wp = resnet_stem_pool_size of those, at most RESNET_MAX_SIDE.  One tile shape:
// RESNET_STEM_TILE_H x RESNET_STEM_TILE_W pooled pixels a work item.  Outside resnet_stem_ok: hipErrorInvalidValue and nothing launched.
static constexpr int RESNET_STEM_TILE_H = 4, RESNET_STEM_TILE_W = 8;
struct ResnetStemArgs {
    const float* x;
    long long sb, sc, sr;
    const half_t* w;
    const float *scale, *bias;
    float* out32;
    half_t* out16;
    int B, Hi, Wi, Hc, Wc, Hp, Wp;
};
inline int resnet_stem_conv_size(int Hi) { return (Hi - 1) / 2 + 1; }      // (Hi + 2 * 3 - 7) / 2 + 1
inline int resnet_stem_pool_size(int Hc) { return (Hc - 1) / 2 + 1; }      // (Hc + 2 * 1 - 3) / 2 + 1
bool resnet_stem_ok(const ResnetStemArgs& a);
hipError_t launch_resnet_stem(const ResnetStemArgs& a, hipStream_t s);
// w fp32 [64, 3, 7, 7] -> the fp16 fragments (24 KiB); flag[0] = 1 where a weight is not finite or beyond fp16's range
hipError_t launch_resnet_stem_pack(const float* w, half_t* out, int* flag, hipStream_t s);
static constexpr size_t RESNET_STEM_W_HALFS = 4 * 6 * 512;

// ---- fused in_proj + attention (hg_qkv_attn.hip): out = SDPA(LN-folded in_proj(x16)) with q, k, v kept in LDS ----------------
// x16 [n_seq * L, lda]: centred fp16 copy of the stream; wp / bcs: the LayerNorm-folded in_proj weight, bias' and column sums
// packed by launch_pack_qkv; mr [n_seq * L][2] = (row mean minus the copy's centre, rstd); out fp16 [n_seq * L, ldo].
struct QkvAttnArgs {
    const half_t* x16 = nullptr;
    int lda = 0;
    const half_t* wp = nullptr;
    const float* bcs = nullptr;
    const float* mr = nullptr;
    half_t* out = nullptr;
    int ldo = 0;                 // 0 = D
    int n_seq = 0, L = 0, D = 0, heads = 0;
    int K = 0;                   // row length of x16 / of W that is summed over (0 = D; D + 64 with the adapter's e columns behind x16)
    unsigned a_bytes = 0;        // bytes readable behind x16 (0: rows padded to a multiple of 256)
    int gsz = 0;                 // head pairs per XCD group (0 = all: the pairs of a sequence side by side)
    unsigned long long* dbg = nullptr;   // diagnostics: s_memtime totals per wave (HG_STAMPS build), normally null
};
// 192 < L <= 208, D = 64 * heads, heads even, D / 64 a multiple of 3 (ViT-B/16: L = 197, D = 768); K / 64 = 3 m or 3 m + 1
bool qkv_attn_ok(int n_seq, int L, int D, int heads, int lda, int K = 0);
// speed only: is the last round of (sequence, head pair) items filled well enough (n_cu <= 0: 256)
bool qkv_attn_pays(int n_seq, int heads, int n_cu);
// W [3D, K] fp16 (LayerNorm-folded), bias / cs [3D] -> Wp [3D * K] fp16 in fragment order, bcs [heads / 2][768] fp32 (null: not written)
hipError_t launch_pack_qkv(const half_t* W, const float* bias, const float* cs, half_t* Wp, float* bcs, int D, int heads,
                           hipStream_t s, int K = 0);
hipError_t launch_qkv_attn(const QkvAttnArgs& a, hipStream_t s);
// the causal short-sequence member (hg_qkv_attn_text.hip, the text tower): a work item is a pack of floor(160 / L) whole sequences x
// a head pair; K = D.  1 <= L <= 80, heads even, D = 64 * heads, D / 64 >= 6 and = 3 m or 3 m + 2 (D = 512, 768)
bool qkv_attn_text_ok(int n_seq, int L, int D, int heads, int lda);
int qkv_attn_text_items(int n_seq, int L, int heads);      // (pack, head pair) work items of a call
// speed only: is the one kernel expected to beat the two it replaces at this shape (n_cu <= 0: 256)
bool qkv_attn_text_pays(int n_seq, int L, int heads, int n_cu);
hipError_t launch_qkv_attn_text(const QkvAttnArgs& a, hipStream_t s);

// ---- CoOp-VAE as one kernel (hg_vae_fused.hip): Encoder -> reparameterise -> Generator with both hidden layers and z on chip --------
// (main_coop_vae.py:261-296,444-448).  wp = the weights packed by launch_pack_vae into the fragment stream the kernel walks:
// [E0 | E1 | G] passes (encoder halves for z columns [0,256) / [256,512), generator), each vae_fused_pass_bytes(hidden) long.
struct VaeFusedArgs {
    const float* x = nullptr;        // [R, 512] fp32: Encoder input (mode 2: the Generator's z)
    const half_t* x16 = nullptr;     // mode 2 only: z as fp16 [R, 512] instead of x (what the GEMM path's reparameterisation kernel writes)
    const float* eps = nullptr;      // [R, 512] fp32 (modes 0, 1)
    float* mean = nullptr;           // [R, 512] fp32 outputs; mean / logvar / z may be null
    float* logvar = nullptr;
    float* z = nullptr;
    float* bias = nullptr;           // Generator output (modes 0, 2)
    const half_t* wp = nullptr;
    const float* b0e = nullptr;      // Encoder.net.0.bias [eh]
    const float* bml = nullptr;      // mean.bias | log_var.bias [1024]
    const float* b0g = nullptr;      // Generator.net.0.bias [gh]
    const float* b2g = nullptr;      // Generator.net.2.bias [512]
    half_t* zpark = nullptr;         // scratch: vae_fused_park_bytes(R) (modes 0, 1)
    int R = 0, eh = 0, gh = 0;
    int mode = 0;                    // 0 Encoder + Generator, 1 Encoder only, 2 Generator only
    bool has_enc = true;             // wp starts with the two encoder passes (mode 2 skips them)
};
// dim == 512, hidden widths (0: that net is absent) multiples of 32 up to 4096 - what the kernel can walk.  What loads is narrower: hg_load_vae
// accepts hidden widths that are multiples of 128 only (the GEMM path's tiles), so 128, 256, ... 4096 are the widths that ever reach it.
bool vae_fused_ok(int dim, int eh, int gh);
size_t vae_fused_pass_bytes(int hidden);
int vae_fused_rows_per_item();                        // 128
inline size_t vae_fused_park_bytes(int R) { return (size_t)((R + 127) / 128) * 4 * 16 * 1024; }
hipError_t launch_pack_vae(const half_t* e_w0, const half_t* e_wml, int eh, const half_t* g_w0, const half_t* g_w2, int gh, half_t* wp,
                           hipStream_t s);
hipError_t launch_vae_fused(const VaeFusedArgs& a, hipStream_t s);

// ---- elementwise / row kernels ---------------------------------------------------------------
// LayerNorm over rows of fp32 x (eps 1e-5, biased variance; clipnet/model.py:153-159).
// Input row for output row r:  gather ? r*rows_per_seq + gather[r] : r*in_row_stride_rows.
hipError_t launch_layernorm_f16(const float* x, const float* w, const float* b, half_t* out, int M, int D,
                                const int32_t* gather, int rows_per_seq, int in_row_mul, hipStream_t s);
// pos / cls / L (ln_pre of the vision tower): row r is first replaced by (r % L == 0 ? cls : x[r]) + pos[r % L]
hipError_t launch_layernorm_f32(const float* x, const float* w, const float* b, float* out, int M, int D,
                                hipStream_t s, const float* pos = nullptr, const float* cls = nullptr, int L = 1);
// NCHW fp32 crops -> patch matrix fp16 [B*g*g, Kp] (token t = g*row+col, k = c*p*p+ky*p+kx), Kp = im2col_kp(p) = 3*p*p rounded up
// to 64 (the GEMMs' K step).  p % 8 == 0: 3*p*p is a multiple of 64 already (p = 16, 32), 8 pixels per thread, no pad columns.
// Any other p with R % p == 0 (p = 14: 588 -> 640): one thread per patch row, and columns 3*p*p .. Kp-1 are written as zeros on
// EVERY call (the matrix lives in a shared workspace; the weight's pad columns are zero, but 0 x NaN is NaN).
inline int im2col_kp(int p) { return (3 * p * p + 63) / 64 * 64; }
hipError_t launch_im2col(const float* x, half_t* out, int B, int R, int p, hipStream_t s);
// x[r][:] = table[ids[r/L*ld_ids + r%L]][:] + pos[r%L][:]   (text: token_embedding + positional).  This and the next two move rows in
// 16-byte chunks: D % 4 != 0 is refused (hipErrorInvalidValue), ids are clamped to the table
hipError_t launch_embed_tokens(const int32_t* ids, int ld_ids, const float* table, const float* pos, float* x,
                               int T, int L, int D, int vocab, hipStream_t s);
// x[r][:] = prompts[(r/L)*Lfull + r%L][:] + pos[r%L][:]
hipError_t launch_add_pos(const float* prompts, int Lfull, const float* pos, float* x, int R, int L, int D,
                          hipStream_t s);
hipError_t launch_gather_rows(const int32_t* ids, const float* table, float* out, int n, int D, int vocab,
                              hipStream_t s);
hipError_t launch_eot_argmax(const int32_t* ids, int T, int L, int32_t* eot, int32_t* max_eot, hipStream_t s);
// out[i] = min(max(in[i], 0), Leff - 1); *flag = 1 (host-mapped, sticky) and *flag_dev = 1 (device memory, per call) if any
// in[i] >= Leff.  in may equal out.
hipError_t launch_clamp_eot(const int32_t* in, int n, int Leff, int32_t* out, int32_t* flag, hipStream_t s, int32_t* flag_dev = nullptr);
// out[0..n) = NaN if *flag != 0 (flag: DEVICE memory, set earlier on the same stream)
hipError_t launch_poison_if_flag(float* out, size_t n, const int32_t* flag, hipStream_t s);
hipError_t launch_f32_to_f16(const float* in, half_t* out, size_t n, hipStream_t s);
hipError_t launch_f16_to_f32(const half_t* in, float* out, size_t n, hipStream_t s);
// out = 2^11 x fp16(in - fp16(in)): the lo operand of a weight held as hi + lo
hipError_t launch_f16_remainder(const float* in, half_t* out, size_t n, hipStream_t s);
// out[c][r] = in[r][c]  (fp32 or fp16 in -> fp16 out), used for `proj` / `text_projection` [in,out]
hipError_t launch_transpose_to_f16(const void* in, int in_dtype, half_t* out, int rows, int cols, hipStream_t s);
hipError_t launch_l2_normalize(const float* x, float* out, int R, int D, hipStream_t s);
hipError_t launch_assemble_prompts(const float* prefix, const float* suffix, const float* ctx, const float* bias,
                                   const int32_t* target, int R, int C, int L, int n_ctx, int D, float* prompts,
                                   hipStream_t s);
// z = exp(0.5 * logvar) * eps + mean  (main_coop_vae.py:445-447) from the mean / logvar planes [R, D]: z fp32 (optional)
// and z16 fp16 [R, ld16] (GEMM operand).  D % 4 == 0, 16-byte accesses.
hipError_t launch_reparam(const float* mean, const float* logvar, const float* eps, int R, int D, float* z, half_t* z16,
                          int ld16, hipStream_t s);
hipError_t launch_vae_loss(const float* recon, const float* x, const float* mean, const float* logvar, int R,
                           int D, float* loss, hipStream_t s);
// tokens [B*L, E] fp32 -> global [B,E] (token 0; may be null) and local [B,E,g,g] (tokens 1..; required), NCHW; E % 32 == 0
hipError_t launch_split_global_local(const float* tok, float* glob, float* local, int B, int L, int E,
                                     hipStream_t s);
hipError_t launch_copy_rows(const float* x, float* out, int B, int row_stride, int D, hipStream_t s,
                            const int32_t* gather = nullptr);   // row b*row_stride (+ gather[b], clamped); B * D within int (refused beyond, as below)
// the same from a stream held as centre + hi + lo (GemmArgs::hl): hi [*, D] row-major, lo in gemm_ring2's tile-fragment order
hipError_t launch_copy_rows_hilo(const half_t* hi, const half_t* lo, const float* muc, float* out, int B, int row_stride, int D,
                                 hipStream_t s);
// first N columns of a [R, ld] fp32 matrix -> dense [R, N]
hipError_t launch_copy_cols(const float* x, int ld, float* out, int R, int N, hipStream_t s);
// ---- LayerNorm folding support (DESIGN.md §4 "LayerNorm folded into the GEMMs")
// (N <= 0: nothing to do, success; K <= 0 refused)
// W16 [N,K], gamma/beta [K], bias [N]  ->  Wf16 = fp16(fl(W * gamma)) (two roundings: fp32, then fp16), cs[n] = sum_k float(Wf16[n][k]), bf[n] = bias[n] + sum_k W[n][k] * beta[k]
hipError_t launch_fold_ln(const half_t* w16, const float* gamma, const float* beta, const float* bias, half_t* wf16,
                          float* cs, float* bf, int N, int K, hipStream_t s, float* csg = nullptr);
// x fp32 [M,D] -> centred fp16 copy x16 = fp16(x - mean), mu[m] = mean, mr[m] = (0, rstd) (eps 1e-5, biased variance)
hipError_t launch_rowstats_cast(const float* x, half_t* x16, float* mr, float* mu, int M, int D, hipStream_t s,
                                float* muc = nullptr, const float* gamma = nullptr);   // muc (optional): centre of the copy as well (= mu)
// behind rowstats_cast: the copy and mr moved to the centre c[m] (hg_test_adapter: the state a preceding residual GEMM leaves)
hipError_t launch_recentre_cast(const float* x, const float* c, half_t* x16, int ld16, float* mr, const float* mu, float* muc, int M,
                                int D, hipStream_t s);
// x = LayerNorm(x; w, b) in place (fp32) followed by rowstats_cast of the result, in one pass (ln_pre of the vision tower)
hipError_t launch_layernorm_rowstats(float* x, const float* w, const float* b, half_t* x16, float* mr, float* mu, float* muc,
                                     int M, int D, hipStream_t s, const float* pos = nullptr, const float* cls = nullptr,
                                     int L = 1, int ld16 = 0);      // ld16: row stride of x16 in halfs (0 = D)
// stats [M][nt][2]: per column group of gw columns (sum, sum of squared deviations from the group mean)
// -> mr [M][2] = (mean - mu[m], rstd) over the nt * gw columns, eps 1e-5, then mu[m] = mean (the centre the next
// residual GEMM subtracts from its fp16 copy)
// muc (optional) receives the centre the CURRENT fp16 copy was written with (mu before this call)
// centred: the statistics are those of ALREADY CENTRED values (EPI_X16_SCALE_LN): mr = (mean, rstd), mu stays
// range_flag (optional, host-mapped): set to 1 when a row's reach from its centre mu[m], bounded through the statistics, exceeds fp16's 65 504
hipError_t launch_finalize_stats(const float* stats, float* mr, float* mu, int M, int nt, int gw, hipStream_t s,
                                 float* muc = nullptr, bool centred = false, int* range_flag = nullptr);
#define HG_PRE_HDR 24   // header words per box in the pre-processing table (layout: hg_preproc.hip)
// ---- crop pre-processing (hg_preproc.hip): head = per-box headers written by the host, tab receives the weight
// tables at word offsets tab_off[box]; tmp = uint8 scratch for the horizontal pass; out fp32 [n,3,n_px,n_px]; out_u8 (nullable) uint8
// [n,n_px,n_px,3] before normalisation
hipError_t launch_preprocess(const uint8_t* img, int H, int W, const int32_t* head, int32_t* tab,
                             const int32_t* tab_off, int n, int n_px, int max_rows, uint8_t* tmp, float* out,
                             uint8_t* out_u8, hipStream_t s, bool imagenet_norm = false);

// ---- crop pre-processing of a batch of images (hg_preproc_batch.hip; limits and layouts: hg_preproc_geom.h): boxes [n][4] and
// crop_image [n] are DEVICE arrays; head [n][24] and tab [n][2][n_px * 67] are workspace sized from n and n_px alone; status [n]
struct PreBatch {      // host-built, by value: the image table
    const uint8_t* img[64];
    int H[64], W[64];
    int B;
};
hipError_t launch_preprocess_batch(const PreBatch& pb, const int32_t* boxes, const int32_t* crop_image, int n, int n_px, int flags,
                                   uint32_t background, int32_t* head, int32_t* tab, float* out, uint8_t* out_u8, int32_t* status,
                                   hipStream_t s);

// ---- the detector's two views of a batch (hg_detector_views.hip; limits, sizes and tiling: hg_detector_views_geom.h): tab receives the
// images' weight tables, boxes [B][4] and crop_image [B] the arguments of the CLIP leg; u8 holds the resized image b at byte
// 256 * u8_256[b]; detr fp32 [B, 3, hmax, wmax]; mask uint8 [B, hmax, wmax]; max_bands: the most bands any image has (dv_bands)
struct DvBatch {      // host-built, by value: the image table
    const uint8_t* img[64];
    int32_t H[64], W[64], oh[64], ow[64];
    int32_t tab[64];          // word offset of the image's tables
    uint32_t u8_256[64];      // byte offset of its resized image / 256
    int32_t B, hmax, wmax;
};
hipError_t launch_detector_views(const DvBatch& dv, int max_bands, int32_t* tab, int32_t* boxes, int32_t* crop_image, uint8_t* u8,
                                 float* detr, uint8_t* mask, hipStream_t s);

// RoI-align (torchvision semantics, aligned=True, sampling_ratio=-1) of feat [C,H,W] for boxes [n,4] (device):
// out_pooled [n,C,P,P] and/or out_mean [n,C] (= .flatten(2).mean(-1)); either may be null
hipError_t launch_roi_align(const float* feat, int C, int H, int W, const float* boxes, int n, float spatial_scale,
                            int P, float* out_pooled, float* out_mean, hipStream_t s);

// ---- interaction head (hg_hoi_head.hip): batched pair RoI pooling, operand rows, logits / priors / scores ----------------------
static constexpr int HOI_MAX_IMAGES = 64;       // images per call (HoiBatch travels as a kernel argument)
static constexpr int HOI_MAX_SIDE = 32;         // H, W of the local map at most
static constexpr int HOI_MAX_C = 1024;
static constexpr int HOI_MAX_P = 32;          // bins per side: P * P stays an int far below 2^24, a set-up thread walks at most P * HOI_MAX_GRID samples
static constexpr int HOI_MAX_BRANCH = 6;
static constexpr int HOI_MAX_K_IMG = 4096;      // width of feat_image at most (HG_HOI_SRC_IMAGE)
static constexpr int HOI_MAX_GRID = 65536;      // samples per bin and axis beyond which a RoI is refused (its pooled row is NaN)
static constexpr int HOI_TAB = 72;              // words per RoI of the table hoi_setup_kernel writes (layout: hg_hoi_head.hip)
static constexpr size_t HOI_LDS_MAX = 160 * 1024;
struct HoiBatch {      // host-built, by value: boxes of image b are rows box_off[b] .. box_off[b + 1] - 1, its pairs pair_off[b] ..
    int B, N, Pt;      // images, boxes and pairs of the batch
    int box_off[HOI_MAX_IMAGES + 1], pair_off[HOI_MAX_IMAGES + 1];
};
struct HoiEpilogue {
    int n;
    const float* branch[HOI_MAX_BRANCH];      // [Pt, NC] each; a per-image branch: [B, NC], pair p reads the row of its image b(p)
    float scale[HOI_MAX_BRANCH];
    unsigned char per_image[HOI_MAX_BRANCH];  // 1: HG_HOI_SRC_IMAGE, computed once per image (hg_heads.hip)
    float* slab[HOI_MAX_BRANCH];              // nullable, per-image branches only: [Pt, NC] that receives the rows as the pairs read them
};
int hoi_pool_chunk(int H, int W);             // channels per LDS chunk: 64 while 64 x (H W | 1) floats fit HOI_LDS_MAX (24 x 24 does), else 32
hipError_t launch_hoi_setup(const HoiBatch& hb, const float* boxes, const int32_t* labels, float scale, int P, int H, int W,
                            int32_t* pair_h, int32_t* pair_o, int32_t* objects, float* union_boxes, float* tab, hipStream_t s);
hipError_t launch_hoi_pool(const HoiBatch& hb, const float* feat, int C, int H, int W, int P, const float* tab, float* pooled_single,
                           float* pooled_union, int n_cu, hipStream_t s);
// feats (nullable) fp32 [Pt, 3C] = human | object | union; ho16 [Pt, 2C], u16 [Pt, C], g16 (nullable; needs feat_global) [Pt, C]
hipError_t launch_hoi_feats(const HoiBatch& hb, const float* pooled_single, const float* pooled_union, const float* feat_global, int C,
                            float* feats, half_t* ho16, half_t* u16, half_t* g16, hipStream_t s);
// logits [Pt, NC], prior [2, Pt, NC], out_scores [Pt, NC]: each nullable
hipError_t launch_hoi_epilogue(const HoiBatch& hb, const HoiEpilogue& e, const float* scores, const int32_t* labels,
                               const uint8_t* obj2target, int n_obj, int NC, float score_pow, float* logits, float* prior,
                               float* out_scores, hipStream_t s);

// ---- region proposals and instance priors (hg_region_props.hip): NMS, selection, prior rows, priors_downproj ------------------------
static constexpr int PROPS_MAX_IMAGES = 64;     // images per call (PropsBatch travels as a kernel argument)
static constexpr int PROPS_MAX_Q = 512;         // detections per image at most: scores, labels, boxes and Q bit rows of Q bits stay in LDS
static constexpr int PROPS_WORDS = PROPS_MAX_Q / 32;
static constexpr int PROPS_MAX_CAP = 64;        // rows per image = 2 max_instances at most: one lane per output slot
static constexpr int PROPS_MAX_E = 1024;
static constexpr int PROPS_MAX_HID = 256;       // one thread per hidden column
static constexpr int PROPS_OUT = 64;            // the adapters' bottleneck
static constexpr int PROPS_MAX_CLASSES = 256;
static constexpr int PRIOR_ROWS = 16;           // rows per workgroup of prior_mlp_kernel
struct PropsBatch {      // host-built, by value: detections of image b are rows q_off[b] .. q_off[b + 1] - 1
    int B;
    int q_off[PROPS_MAX_IMAGES + 1];
    float img_h[PROPS_MAX_IMAGES], img_w[PROPS_MAX_IMAGES];
};
struct PropsSelect {
    float score_thr, nms_thr;
    int human_idx, min_inst, max_inst, cap;
    int n_classes;       // rows of the prior table the labels index (0: proposals only, labels unchecked)
};
struct PriorDev {        // fp32, linears as [in][out]: w0t [5 + E][hid], w1t [hid][hid], w2t [hid][64]; T [n_classes][hid]
    int hid;
    const float *w0t, *b0, *w1t, *b1, *w2t, *b2, *T;
};
// counts [B][4] = n, n_human, status, survivors; keep / out_scores / out_labels [B][cap], out_boxes [B][cap][4] (16-byte aligned, as
// boxes); survivors (nullable) [q_off[B]]: image b's NMS survivors in order from q_off[b] on
hipError_t launch_props_select(const PropsBatch& pb, const PropsSelect& ps, const float* scores, const int32_t* labels, const float* boxes,
                               int32_t* counts, int32_t* keep, float* out_boxes, float* out_scores, int32_t* out_labels,
                               int32_t* survivors, hipStream_t s);
hipError_t launch_prior_pack(const float* in, int N, int K, float* out, hipStream_t s);      // [N][K] -> [K][N]
hipError_t launch_prior_table(const float* emb, const float* w0t, int n_classes, int E, int hid, float* T, hipStream_t s);
// priors [B][cap][64], mask [B][cap] (1 = pad) from what launch_props_select wrote
hipError_t launch_prior_mlp(const PropsBatch& pb, const PriorDev& pw, int cap, const int32_t* counts, const float* sel_boxes,
                            const float* sel_scores, const int32_t* sel_labels, float* priors, uint8_t* mask, hipStream_t s);

// ---- detections and their association with the ground truth (hg_detections.hip) ---------------------------------------------------------
static constexpr int DET_MAX_IMAGES = 64;       // images per call (DetBatch travels as a kernel argument)
static constexpr int DET_MAX_NC = 1024;
static constexpr int DET_MAX_GT = 256;          // ground-truth pairs per image: one thread each, boxes, classes and keys in LDS
static constexpr int DET_ROWS = 64;             // pair rows per workgroup of det_count_kernel / det_write_kernel: one wave scans their counts
struct DetBatch {      // host-built, by value: pairs, boxes and ground-truth pairs of image b are rows x_off[b] .. x_off[b + 1] - 1
    int B, Pt;
    int pair_off[DET_MAX_IMAGES + 1], box_off[DET_MAX_IMAGES + 1], gt_off[DET_MAX_IMAGES + 1];
    int img_h[DET_MAX_IMAGES], img_w[DET_MAX_IMAGES];
};
struct DetEntries {    // one word per detection each, [cap]; each nullable for det_write_kernel
    int32_t *pair, *verb, *h, *o, *object;
    float* score;
    int32_t* interaction;
};
// cnt [Pt] and bsum [ceil(Pt / DET_ROWS)]: workspace.  det_off [B + 1]; status [B] nullable.  Nothing is written at or beyond slot cap.
hipError_t launch_det_compact(const DetBatch& db, const float* prior, const float* scores, const int32_t* pair_h, const int32_t* pair_o,
                              const int32_t* objects, const int32_t* conversion, int n_obj, int NC, int cap, int32_t* cnt, int32_t* bsum,
                              int32_t* det_off, const DetEntries& e, int32_t* status, hipStream_t s);
// needs e.h, e.o, e.score, e.interaction and det_gt; det_label, det_max_iou, gt_out [2][Gt][4] and status nullable
hipError_t launch_det_assoc(const DetBatch& db, const float* boxes, const float* gt_h, const float* gt_o, const int32_t* gt_hoi, int gt_format,
                            float min_iou, int cap, int Gt, const int32_t* det_off, const DetEntries& e, float* det_label, int32_t* det_gt,
                            float* det_max_iou, float* gt_out, int32_t* status, hipStream_t s);

// ---- backward of the frozen text tower (hg_text_grad.hip): the gradient with respect to the prompts, no weight gradients ----------------
// causal attention backward, head dim 64, 1 <= L <= TEXT_GRAD_MAX_L: qkv fp16 [n_seq * L, 3 * heads * 64] (q | k | v column blocks), dout
// fp16 [n_seq * L, heads * 64] -> dqkv fp16 [n_seq * L, 3 * heads * 64] (dq | dk | dv); exactly those rows are written
static constexpr int TEXT_GRAD_MAX_L = 80;
size_t text_attn_bwd_lds(int L);      // dynamic LDS bytes of a workgroup
hipError_t launch_text_attn_bwd(const half_t* qkv, const half_t* dout, half_t* dqkv, int n_seq, int L, int heads, hipStream_t s);
// g[row] += LayerNorm_backward(x[r], gamma, dy[r]) for r < M (x, dy dense [M, D] fp32; eps 1e-5, statistics recomputed from x);
// row = r, or r * rows_per_seq + sel[r] (clamped) with sel.  D % 4 == 0, D <= 1024
hipError_t launch_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* g, int M, int D, const int32_t* sel,
                                int rows_per_seq, hipStream_t s);
// du = fp16(df * quickgelu'(u)), n % 8 == 0, 16-byte aligned; du may be df
hipError_t launch_qgelu_bwd(const half_t* df, const half_t* u, half_t* du, size_t n, hipStream_t s);
// go16 [R, E] = fp16(s_r * go), sinv[r] = 1 / s_r with s_r = 2^-floor(log2(max_e |go[r][e]|)) (1 for a zero row)
hipError_t launch_grad_scale(const float* go, half_t* go16, float* sinv, int R, int E, hipStream_t s);
// out [R, L, D] = g [R, Leff, D] * sinv[r], zeros at positions >= Leff
hipError_t launch_grad_unscale(const float* g, const float* sinv, float* out, int R, int L, int Leff, int D, hipStream_t s);
// g [R, L, D] -> grad_bias [R, D] = sum_j g[r][1 + j], grad_ctx [n_ctx, D] = sum_r g[r][1 + j] through partial
// [ceil(R / PROMPTS_BWD_CHUNK)][n_ctx][D] (rows of a chunk ascending, then chunks ascending); either output nullable
static constexpr int PROMPTS_BWD_CHUNK = 64;
hipError_t launch_prompts_bwd(const float* g, int R, int L, int n_ctx, int D, float* partial, float* grad_ctx, float* grad_bias,
                              hipStream_t s);

// ---- adapter (variant C) --------------------------------------------------------------------
// tokens per image at most: the decoder keeps K and V of NKMAX = 224 keys on chip (hg_adapter.hip); a longer tower loads without adapters only
static constexpr int ADAPTER_MAX_L = 224;
// ... unless option adapter_long is on: up to 640 tokens on the decoder of hg_adapter_long.hip (query chunks of at most 224 tokens,
// K and V of a sequence that is its own memory streamed through the same LDS area in key chunks); not folded into the block's GEMMs
static constexpr int ADAPTER_LONG_MAX_L = 640;
struct AdapterDev {      // device pointers, all fp32 except the two MFMA operands
    const half_t* down_w;   // [d, D] fp16
    const float* down_b;    // [d]
    const half_t* up_w;     // [D, d] fp16
    const float* up_b;      // [D]
    const float* scale;     // [D]
    // decoder layers [0] = mhsa_layers.0 (prior memory), [1] = mhsa (self memory); fp32, weights
    // transposed to [in][out]:  0 WqT 1 WkT 2 WvT 3 bq 4 bk 5 bv 6 WoT 7 bo 8 {norm2.w,norm2.b,norm3.w,
    // norm3.b} 9 W1T [d][2d] 10 b1 11 {W2T [2d][d], b2}
    const float* dl[2][12];
    // fp16 [out][in] copies for the MFMA decoder: 0 Wq 1 Wk 2 Wv [64,64] (rows of in_proj_weight), 3 Wo [64,64],
    // 4 W1 [128,64], 5 W2 [64,128]; null -> the fp32 VALU kernel runs
    const half_t* w16[2][6];
};
// down32 [M,128] fp32 (cols 0..63 = relu(down_proj(x))) -> out16 [M,64] fp16 (decoder layer output);
// kv: scratch [B*Nmem, 2, 64] fp32 with Nmem = N (prior given) or L (prior == nullptr).
// chain32 (optional, adapter_num_layers > 1): write the layer's output as fp32 into this [M,128] buffer (may be down32
// itself) instead of out16, for the next decoder layer of the chain
// ld16: row stride of out16 in halfs (64 = dense; D + 64 when the rows are the right-hand columns of the K-concatenated
// out-proj operand [att | d])
// fold (MFMA path, last layer of a chain only): the layer writes e = [z_0 .. z_62, 1] (norm3 without its affine part) instead
// of d and replaces mr[row] = (mean_x - c, rstd_x) by the LayerNorm statistics of x + a, a = Q e (adapter_q_kernel); it reads
// w' = x16 Q from columns 64..127 of down32
struct AdapterFoldDev {
    const half_t* g16 = nullptr;   // [64][64] fp16 Q^T Q
    const float* qm = nullptr;     // [64] column sums of Q
    float* mr = nullptr;           // [M][2], updated in place; null = off
    float inv_D = 0.f;
    half_t* e2 = nullptr;          // a second home of e (row stride ld16): the out-proj operand buffer when it is not the in_proj one
};
// dn (MFMA path, first layer of a chain): down_proj runs inside the kernel - [relu(down) | x16 Q] = [x16 + muc] w^T + b with
// w [128, K] fp16 (AdapterW::Fold::down2), b / cs [128]; down32 is then only written (chain32: the fp32 hand-over to the next
// layer, x16 Q in its columns 64..127) or not touched at all
struct AdapterDownDev {
    const half_t* x16 = nullptr;   // [M, ldx] centred fp16 copy of the stream
    int ldx = 0, K = 0;
    const half_t* w = nullptr;
    const float* b = nullptr;
    const float* cs = nullptr;
    const float* muc = nullptr;    // [M] centre of the copy
};
hipError_t launch_adapter_decoder(const float* down32, const AdapterDev& ad, const float* priors,
                                  const uint8_t* mask, int B, int L, int N, float* kv, half_t* out16,
                                  hipStream_t s, float* chain32 = nullptr, int ld16 = 64, const AdapterFoldDev* fold = nullptr,
                                  const AdapterDownDev* dn = nullptr);
bool adapter_decoder_mfma_ok(const AdapterDev& ad, bool priors, int L, int N);
bool adapter_decoder_fused_down_ok(const AdapterDev& ad, bool priors, int L, int N);
// 224 < L <= 640 (hg_adapter_long.hip; launch_adapter_decoder goes there by itself): fp16 weights present and, with priors, N <= 32.
// kv16 = the same scratch as `kv`, read as fp16 K [B][Lp][64] and V^T [B][64][Lp], Lp = L rounded up to 32 (self memory only)
bool adapter_decoder_long_ok(const AdapterDev& ad, bool priors, int L, int N);
hipError_t launch_adapter_decoder_long(const float* down32, const AdapterDev& ad, const float* priors, const uint8_t* mask, int B, int L,
                                       int N, void* kv16, half_t* out16, hipStream_t s, float* chain32, int ld16);
// weight-load time: Q (scratch q32 [D][64]) and the operands that carry it: down2 [128, D], wk_out [D, D+64] = [w_out | Q],
// wq_cat [3D, D+64] = [wf_qkv | wf_qkv Q], qm [64], g16 [64][64]; norms = the last decoder layer's {norm2.w, norm2.b, norm3.w, norm3.b}
hipError_t launch_adapter_fold(const half_t* up_w, const float* up_b, const float* scale, const float* norms,
                               const half_t* down_w, const half_t* w_out, const half_t* wf_qkv, int D, float* q32,
                               half_t* down2, half_t* wk_out, half_t* wq_cat, float* qm, half_t* g16, hipStream_t s);

}  // namespace hg
