// What the host files of the C ABI share (hg_api.hip, hg_load.hip, hg_tower.hip, hg_heads.hip, hg_detector_views.hip, hg_detr.hip,
// hg_detr_dec.hip, hg_detr_ends.hip, hg_resnet.hip, hg_test_hooks.hip): the context and the weight structs, error reporting, the
// grow-only workspace, the weight helpers of the loaders, the profiler scope and the GEMM / attention wrappers.  Host code only.
//
// Device data layout:
//   residual stream x   fp32 [M, D]      M = n_seq * L rows (token-major, sequence-contiguous)
//   h / att / fc        fp16 [M, D|4D]   MFMA A operands (K contiguous)
//   qkv                 fp16 [M, 3D]     q|k|v column blocks, head h = columns 64h..64h+63
//   linear weights      fp16 [N, K]      exactly nn.Linear's [out, in] -> both GEMM operands K-contiguous
//   proj/text_projection fp16 [E, D]     transposed once at load ([D,E] in the state dict)
//   biases, LN affine, embeddings, positional: fp32
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/hoigen_amd.h"
#include "hg_kernels.h"

using namespace hg;

namespace hg_host {      // (the host files' own names: nothing as plain as fail / gemm / ensure leaves the library unqualified)
struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct BlockW {
    half_t *w_qkv, *w_out, *w_fc, *w_proj;
    float *b_qkv, *b_out, *b_fc, *b_proj, *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    // LayerNorm folded into the consuming GEMM: W' = fp16(W * gamma), cs[n] = sum_k W'[n][k],
    // b' = b + W beta;  LN(x) W^T + b = rstd * (x16 W'^T - mean * cs) + b'
    half_t *wf_qkv, *wf_fc;
    float *cs_qkv, *bf_qkv, *cs_fc, *bf_fc;
    // column sums sum_k gamma[k] W[n][k] for the form that keeps the LayerNorm weight in the activation copy and W unrounded (text tower)
    float *csg_qkv, *csg_fc;
    // wf_qkv / bf_qkv / cs_qkv once more in the order the fused in_proj + attention kernel streams them (hg_qkv_attn.hip:
    // MFMA fragments per head pair); null when the width does not qualify
    half_t* wp_qkv;
    float* bcs_qkv;
    // the same packing of the layer's OWN w_qkv with bf_qkv / csg_qkv: the operands of the fused kernel where the LayerNorm weight
    // rides in the activation copy (text tower, text_ln_fold = 1: hg_qkv_attn_text.hip); null elsewhere
    half_t* wpg_qkv;
    float* bcsg_qkv;
    // c_proj as hi + lo on image towers beyond the short adapters' 224 tokens whose weights arrive in fp32: 2^11 x fp16(W - w_proj),
    // used by calls that run instance adapters there (hg_load_vit; launch_mlp); null elsewhere
    half_t* w_proj_lo;
};

struct AdapterW {
    bool present = false;
    int d = 0;
    half_t* down_w = nullptr;  // [128 (padded), D]
    float* down_b = nullptr;   // [128]
    float* down_cs = nullptr;  // [128] row sums of the fp16 weight: down_proj on the CENTRED fp16 copy adds mu * cs back
    half_t* up_w = nullptr;    // [D, 64]
    float* up_b = nullptr;
    float* scale = nullptr;
    half_t* up_w_lo = nullptr; // towers beyond 224 tokens, fp32 weights: 2^11 x fp16(W_up - up_w), and
    float* scale_lo = nullptr; //   [D] 2^-11 x scale: the pass in front of up_proj that adds the remainder (run_adapter)
    // The adapter folded into the block's GEMMs altogether (hg_elem.hip adapter_q_kernel): a = Q e with e = the last decoder
    // layer's normalised output; [0] = prior path (last layer of the mhsa_layers chain), [1] = self path (mhsa)
    struct Fold {
        half_t* down2 = nullptr;    // [128, D]: down_proj rows | Q^T (the cross term of the statistics rides in the padded half)
        half_t* wk_out = nullptr;   // [D, D + 64] = [W_out | Q]
        half_t* wq_cat = nullptr;   // [3D, D + 64] = [W'_qkv | W'_qkv Q]
        half_t* wp_qcat = nullptr;  // wq_cat in the fused in_proj + attention kernel's fragment order (launch_pack_qkv, K = D + 64)
        half_t* g16 = nullptr;      // [64, 64] Q^T Q
        float* qm = nullptr;        // [64] column sums of Q
    } fold[2];
    float* dl[2][12] = {};     // see AdapterDev
    half_t* w16[2][6] = {};    // see AdapterDev
    struct Extra { float* dl[12] = {}; half_t* w16[6] = {}; };
    std::vector<Extra> extra;  // mhsa_layers.1 .. N-1 (adapter_num_layers > 1), prior path only
};

struct Vit {
    bool loaded = false;
    int D = 0, layers = 0, heads = 0, patch = 0, res = 0, grid = 0, L = 0, E = 0, Kp = 0;
    half_t* w_patch = nullptr;
    float *cls = nullptr, *pos = nullptr, *lnpre_w = nullptr, *lnpre_b = nullptr, *lnpost_w = nullptr,
          *lnpost_b = nullptr;
    half_t* w_projT = nullptr;
    half_t* w_projT_lo = nullptr;     // variant C of towers beyond the adapters' 224 tokens: 2^11 x the fp16 remainder of proj (hg_load_vit)
    float* proj_lo_scale = nullptr;   // [E] 2^-11, and [E] zeros behind it (the second pass's bias)
    float* lo_scale = nullptr;        // the same for the blocks' width: [D] 2^-11, [D] zeros (BlockW::w_proj_lo, AdapterW::up_w_lo)
    std::vector<BlockW> blocks;
    std::vector<AdapterW> adapters;
    std::vector<void*> owned, owned_adapters;
};

struct Text {
    bool loaded = false;
    int D = 0, layers = 0, heads = 0, ctx = 0, vocab = 0, E = 0;
    float *tok = nullptr, *pos = nullptr, *lnf_w = nullptr, *lnf_b = nullptr;
    half_t* w_projT = nullptr;
    std::vector<BlockW> blocks;
    std::vector<void*> owned;
    // the input gradient of the tower (hg_text_bwd.hip): the linears once more, transposed, so that dX = dY W runs on the GEMM kernels
    // as they are - built by ensure_text_grad on the first backward call, dropped with the weights by hg_load_text
    struct GradW { half_t *wT_qkv, *wT_out, *wT_fc, *wT_proj; };      // [D, 3D], [D, D], [D, 4D], [4D, D]
    std::vector<GradW> grad;
    half_t* g_proj = nullptr;      // text_projection as the state dict holds it: [D, E]
    float* g_zero = nullptr;       // [4D] zeros: the backward GEMMs' bias
    std::vector<void*> owned_grad;
};

struct Vae {
    bool enc = false, gen = false;
    int dim = 0, eh = 0, gh = 0;
    half_t *e_w0 = nullptr, *e_wml = nullptr, *g_w0 = nullptr, *g_w2 = nullptr;
    float *e_b0 = nullptr, *e_bml = nullptr, *g_b0 = nullptr, *g_b2 = nullptr;
    half_t* wp = nullptr;      // the same weights as the fragment stream of the one-kernel path (hg_vae_fused.hip): [E0 | E1 | G]
    // the same stacked mean | log_var operand with its rows interleaved in blocks of 128 (EPI_VAE_REPARAM_F32)
    std::vector<void*> owned;
};

struct Cache {
    bool loaded = false, has_labels = false;
    int S = 0, K = 0, C = 0, Sp = 0, Cp = 0;
    half_t *w16 = nullptr, *lt16 = nullptr;   // [Sp,K] ; labels^T [Cp,Sp]
    float *b = nullptr, *bias_c = nullptr, *scale = nullptr;   // [Sp] ; [Cp] bias @ labels ; [Cp] 1 / (lens * post_div)
    std::vector<void*> owned;
};

struct Mlp {
    bool loaded = false;
    int in = 0, hid = 0, out = 0;
    half_t *w0 = nullptr, *w2 = nullptr, *w4 = nullptr;
    float *b0 = nullptr, *b2 = nullptr, *b4 = nullptr;
    std::vector<void*> owned;
};

struct Priors {      // priors_downproj + object_embedding (hg_load_priors): fp32, linears as [in][out], and the folded table T
    bool loaded = false;
    int E = 0, hid = 0, n_classes = 0;
    float *w0t = nullptr, *b0 = nullptr, *w1t = nullptr, *b1 = nullptr, *w2t = nullptr, *b2 = nullptr, *T = nullptr;
    std::vector<void*> owned;
};
struct DetrLayerW {      // one post-norm encoder layer (detr/models/transformer.py:127-162): linears fp16 [out, in], the rest fp32
    half_t *w_in, *w_out, *w1, *w2;      // in_proj [3D, D] (q | k | v rows), out_proj [D, D], linear1 [F, D], linear2 [D, F]
    float *b_in, *b_out, *b1, *b2, *n1_w, *n1_b, *n2_w, *n2_b;
};
struct DetrEnc {         // hg_load_detr_encoder
    bool loaded = false;
    int D = 0, heads = 0, F = 0;
    std::vector<DetrLayerW> layers;
    std::vector<void*> owned;
};
struct DetrDecLayerW {   // one post-norm decoder layer (transformer.py:187-233): the encoder layer's tensors, multihead_attn's q rows and out_proj, norm3
    DetrLayerW sa;
    half_t *wq_c, *w_out_c;
    float *bq_c, *b_out_c, *n3_w, *n3_b;
};
struct DetrDec {         // hg_load_detr_decoder
    bool loaded = false;
    int D = 0, heads = 0, F = 0;
    std::vector<DetrDecLayerW> layers;
    half_t *wk_all = nullptr, *wv_all = nullptr;      // [n_layers * D, D]: the K / V rows of every layer's multihead_attn.in_proj_weight
    float *bk_all = nullptr, *bv_all = nullptr, *nf_w = nullptr, *nf_b = nullptr;
    std::vector<void*> owned;
};
struct DetrHeads {       // hg_load_detr_heads: class_embed (rows gathered, padded to C1p = a multiple of 16) and bbox_embed (layers.2 padded to 16 rows)
    bool loaded = false;
    int D = 0, C1 = 0, C1p = 0;
    half_t *wc = nullptr, *w0 = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *bc = nullptr, *b0 = nullptr, *b1 = nullptr, *b2 = nullptr;
    std::vector<void*> owned;
};
struct DetrNeck {        // hg_load_detr_neck: input_proj's weight as fp16 [D, Cin], its bias, and the sine embedding's dim_t table [D / 2]
    bool loaded = false;
    int D = 0, Cin = 0, normalize = 0;
    float scale = 0.f;
    half_t* w = nullptr;
    float *bias = nullptr, *dim_t = nullptr;
    std::vector<void*> owned;
};
struct ResnetConvW {     // one convolution with its norm: the weight as fp16 MFMA fragments (launch_resnet_pack), scale and bias fp32 [cout]
    half_t* w = nullptr;
    float *scale = nullptr, *bias = nullptr;
    int cin = 0, cout = 0, R = 0, stride = 0;
};
struct ResnetBlockW {
    ResnetConvW c1, c2, c3, cd;
    bool down = false;
};
struct ResnetStages {    // hg_load_resnet_stages
    bool loaded = false;
    std::vector<ResnetBlockW> blocks;
    std::vector<void*> owned;
};
struct ResnetStem {      // hg_load_resnet_stem: conv1 as hg_resnet_stem.hip's fp16 fragments (launch_resnet_stem_pack), bn1 as scale and bias
    bool loaded = false;
    ResnetConvW conv;
    std::vector<void*> owned;
};
}  // namespace hg_host
using namespace hg_host;

struct hg_ctx {
    int device = 0;
    std::string err;
    Vit vit;
    Text text;
    Vae vae[HG_MAX_SLOTS];
    Mlp mlp[HG_MAX_SLOTS];
    Cache cache[HG_MAX_CACHE_SLOTS];
    Priors prior[HG_MAX_PRIOR_SLOTS];
    DetrEnc detr;
    DetrDec detr_dec;
    DetrHeads detr_heads;
    DetrNeck detr_neck;
    ResnetStages resnet;
    ResnetStem resnet_stem;
    // workspace (grow-only)
    Buf x, h, qkv, att, fc, head16, tok32, small, i32, ad32, ad16, adkv, mr, mu, muc, stats, pre, pretab, cx, ca, ch, cf, cq;
    Buf hg;              // folded path with the LayerNorm weight in the activation copy (text tower): that copy, beside the stream's hi half in h
    Buf att2;            // variant C with the stream as centre + hi + lo: the out-proj operand [att | e] beside the in_proj one [x16 | e]
    Buf zpark;           // hg_vae_fused.hip: the encoder's first z half as fp16 fragments, per wave
    Buf xlo;             // low half of the residual stream while it is held as centre + hi + lo (GemmArgs::hl)
    Buf pair_ready;      // hg_mlp_pair.hip: ready counters [blocks][256-row panels], zeroed at the start of every tower pass
    Buf hoi_tab, hoi_pool, hoi_a16, hoi_br;      // hg_hoi_head: RoI table; pooled means; fp16 operand rows HO | U | G; branch logits
    Buf hoi_img16, hoi_img;                      // hg_hoi_head's image branches: the 256-row fp16 operand of feat_image; their [n, B, NC] logits
    Buf props;           // hg_region_priors: keep, boxes, scores, labels of the selected instances where the caller does not ask for them
    Buf det;             // hg_hoi_detections: row counts, workgroup sums, and the entry arrays the association reads where the caller does not ask for them
    Buf prebatch;        // hg_preprocess_batch: per-crop headers and weight tables, sized from n and n_px alone
    Buf detr_ws;         // hg_detr_encoder: the fp32 stream, the batch-major pos, and the fp16 operands x, x + pos, q | k, v, attention output, FFN hidden
    Buf detr_dec_ws;     // hg_detr_decoder: memory's fp16 copies and every layer's cross-attention K and V, the decoder stream and its fp16 operands, the split FFN's partial sums
    Buf detr_neck_ws;    // hg_detr_neck: the fp32 partial sums of a split over Cin
    Buf resnet_ws;       // hg_resnet_stages / hg_resnet_body: the fp32 stream in and out, its fp16 copies, the downsample's output, conv1's and conv2's outputs
    Buf tgrad;           // hg_text_backward_embeds: the fp32 gradient stream, its fp16 copy, and the fp16 / fp32 gradients of a block's activations
    Buf pgrad;           // hg_assemble_prompts_backward: the per-chunk partial sums of grad_ctx
    Buf resnet_stem_ws;  // hg_resnet_stem: the NHWC fp32 + fp16 pair the kernel writes, ahead of the NCHW copy the caller gets
    Buf dviews;          // hg_detector_views: the CLIP leg's boxes, the weight tables, and the resized images where the caller does not ask for them
    int max_chunk_img = 256;
    int text_rows_budget = 65536;      // rows (prompts x executed tokens) per pass of the text tower (text_chunk_prompts)
    int max_chunk_rows = 32768;
    // behaviour options: hg_set_option; the environment (HG_LAST_BLOCK_ROW0, HG_LN_FUSE, HG_ADAPTER_FUSE, HG_ADAPTER_FOLD,
    // HG_CHUNK_ROWS) only gives their values at hg_create - nothing on the call path reads the environment
    int opt_row0 = 1;            // last block of a tower without token outputs on the one row that leaves it
    int opt_ln_fuse = 1;         // LayerNorm folded into the GEMMs where the shapes allow
    int opt_adapter_fuse = 1;    // ... also behind the instance adapters (variant C)
    int opt_adapter_fold = 1;    // adapter folded into the block's own QKV / out-proj GEMMs (0: separate up_proj GEMM)
    int opt_stream_hilo = 1;     // residual stream as centre + hi + lo (fp16 copy + bf8 remainder) between the folded blocks (0: fp32)
    int opt_qkv_attn = 1;        // in_proj + attention as one kernel, q / k / v kept in LDS (vision tower, folded blocks; 0: two kernels)
    int opt_qkv_attn_min_seq = 32;   // ... from this many sequences per call on, and where its last round of items is filled well
                                     // enough (qkv_attn_pays; qkv_attn = 2: wherever the shapes allow)
    int opt_qkv_attn_gsz = 0;    // head pairs per XCD group of that kernel (0 = all)
    int opt_text_ln_fold = 1;    // text tower: 1 (default) LayerNorm folded into its GEMMs with the LayerNorm weight in the ACTIVATION copy (GemmArgs::gamma:
                                 // the GEMMs keep the layer's own fp16 weights - closer to the reference than the separate kernels, 4 % faster);
                                 // 2 the weight folded into fp16(W * gamma) as in the vision tower (10 % faster, 7.6e-4 instead of 6.2e-4); 0 separate kernels
    int opt_adapter_long = 0;    // instance adapters on towers of 225 .. 640 tokens (hg_adapter_long.hip): 0 refuses them as before (at most 224 tokens),
                                 // 1 accepts them - read at hg_load_vit, hg_update_adapters, the image entry points and hg_test_adapter
    int opt_qkv_attn_text = 0;   // text tower: in_proj + causal attention as one kernel for L <= 80 (hg_qkv_attn_text.hip; folded blocks): 0 two kernels,
                                 // 1 where it measured faster (qkv_attn_text_pays: profiles/qkv_attn_text.txt), 2 wherever the shapes allow
    int opt_qkv_attn_c = 1;      // ... also in the blocks that carry a folded adapter (variant C on the hi / lo stream: K = D + 64)
    int opt_vae_fused = 1;       // CoOp-VAE Encoder -> reparameterise -> Generator as ONE kernel (hg_vae_fused.hip) for the rows that fill
                                 // whole rounds of 128-row items over the CUs (the rest: the GEMM path); 2: every row; 0: GEMM path only
    int opt_mlp_pair = 1;        // c_fc -> QuickGELU -> c_proj of a LayerNorm-folded block as ONE persistent launch with per-row-panel ready
                                 // counters between its tiles (hg_mlp_pair.hip; both towers, variant A); bit-identical to the two launches
    int opt_mlp_pair_chunk = 32; // ... 256-row panels of an XCD per chunk
    int opt_mlp_pair_fc_slots = 32;  // ... workgroups per XCD that run c_fc tiles (the rest start with c_proj)
    int opt_mlp_pair256 = 1;     // ... with c_proj on 256 x 256 tiles (hg_mlp_pair256.hip) where mlp_pair256_ok holds; 0: hg_mlp_pair.hip's 128-row tiles.  Same bits
    int opt_mlp_pair256_min_m = 25000; // ... from this many rows on: 25 216 rows (128 crops) is the smallest measured call it wins, 18 912 (96) loses (profiles/mlp_pair256.txt)
    int opt_mlp_pair256_chunk = 6;     // ... 256-row panels of an XCD per chunk of ITS c_fc order (small, so that the slots that reach c_proj first find whole
                                       // panels; 6 measured best of 1 .. 32 on the headline step: profiles/mlp_pair256.txt)
    int opt_mlp_pair256_ratio = 4;     // ... c_fc tile times a 256 x 256 c_proj tile takes, what its dealing balances with: 166-176 k against 43-44 k ticks per
                                       // tile in the per-slot stamps (profiles/mlp_pair256.txt)
    int opt_mlp_pair256_ph2 = 1;       // ... c_proj's K loop there in two phases (hg_mlp_pair256p.hip) instead of four (hg_mlp_pair256.hip).  Same bits
                                       // (profiles/mlp_pair256_ph2.txt)
    int n_pair256_launches = 0;  // ... launches of that kernel so far (option "mlp_pair256_launches": read it; setting it restarts the count; the profiler
                                 // record is the pair launch's, so this is how a caller tells which kernel ran)
    int opt_detr_attn_chunk = 0;     // hg_detr_attn.hip: keys per LDS chunk (0: all keys at once while they fit, 512 beyond; else a multiple of 32 up to 1 280).  Same bits
    int opt_detr_attn_waves = 0;     // ... query tiles per slab = waves per workgroup: 0 = 4 (measured best or equal in every case: profiles/detr_encoder.txt), else 1, 2 or 4.  Same bits
    int opt_detr_ffn = 0;            // FFN of a DETR decoder layer: 0 the split-over-d_ff kernel (hg_detr_ffn.hip) up to opt_detr_ffn_max_m rows where the shape allows,
                                     // 1 the two GEMMs, 2 the split kernel or HG_ERR_INVALID
    int opt_detr_ffn_max_m = 1000;   // ... rows (B * Q) up to which 0 picks the split kernel: it wins by 25 - 31 us a layer from 100 to 950 rows; at 2 888 rows
                                     // by 7 us, which is the spread of repeated runs (profiles/detr_decoder.txt)
    int opt_detr_neck_split = 0;     // slices of Cin of hg_detr_neck's projection: 0 the rule of detr_neck_default_split (hg_detr_ends.hip), 1 no split, n that many
    int opt_mlp_pair_fault = 0;      // fault injection for the tests: that launch goes out one workgroup short, so that a hand-off wait meets its bound
    int n_cu = 256;
    // sticky device->host flag (host-mapped): a hand-off wait inside the MLP pair kernel gave up (a workgroup of its grid never became
    // resident); the call in flight returned garbage, the next tower call reports HG_ERR_HIP
    int32_t* pair_err = nullptr;
    // sticky device->host flag (host-mapped): inside a tower with folded LayerNorms a row reached further from its centre than the centred
    // fp16 copy / the hi half of the stream can hold (|x - row centre| > 65504, bounded through the row statistics: finalize_stats).
    // Reported as HG_ERR_INVALID by the next tower call.
    int32_t* range_flag = nullptr;
    // sticky device->host flag (host-mapped): set by clamp_eot when a caller-supplied text truncation was shorter than
    // max(EOT)+1 (a stale host memo); reported as HG_ERR_INVALID by the next text call
    int32_t* eot_flag = nullptr;
    int32_t* eot_flag_dev = nullptr;   // the same condition for the call in flight, in device memory (zeroed per call): poison_if_flag polls it
    // live per-kernel timing for bench.py (hg_profile_begin/end): hipEvent pairs around the launches of one kernel
    // kind (or of every GEMM and attention launch), on the stream the kernel is launched on
    int prof_kind = HG_PROF_OFF;
    std::vector<hipEvent_t> prof_ev;
    std::vector<hg_prof_rec> prof_rec;
    size_t prof_n = 0;
};

namespace hg_host {
// every workspace buffer of a context: what hg_destroy frees and hg_workspace_bytes adds up
#define HG_WORKSPACE_BUFS(c)                                                                                                          \
    {&(c)->x, &(c)->h, &(c)->qkv, &(c)->att, &(c)->fc, &(c)->head16, &(c)->tok32, &(c)->small, &(c)->i32, &(c)->ad32, &(c)->ad16,    \
     &(c)->adkv, &(c)->mr, &(c)->mu, &(c)->muc, &(c)->stats, &(c)->pre, &(c)->pretab, &(c)->cx, &(c)->ca, &(c)->ch, &(c)->cf,        \
     &(c)->cq, &(c)->xlo, &(c)->zpark, &(c)->att2, &(c)->hg, &(c)->pair_ready, &(c)->hoi_tab, &(c)->hoi_pool, &(c)->hoi_a16,    \
     &(c)->hoi_br, &(c)->hoi_img16, &(c)->hoi_img, &(c)->props, &(c)->det, &(c)->prebatch, &(c)->dviews, &(c)->detr_ws, &(c)->detr_dec_ws, &(c)->detr_neck_ws, &(c)->resnet_ws, \
     &(c)->resnet_stem_ws, &(c)->tgrad, &(c)->pgrad}

inline int fail(hg_ctx* c, int code, const char* fmt, ...) {
    char tmp[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tmp, sizeof tmp, fmt, ap);
    va_end(ap);
    if (c) c->err = tmp;
    return code;
}

#define HG_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(c, HG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                     \
    } while (0)

// Entry points run on the context's device and give the caller's current device back on return (torch tracks the
// current device per thread; a library that silently changes it redirects the caller's next allocation).
struct DevGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DevGuard(const hg_ctx* c) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device) err = hipSetDevice(c->device);
        else prev = -1;
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define HG_ON_DEVICE(c)                                                                                 \
    DevGuard dev_guard_(c);                                                                             \
    if (dev_guard_.err != hipSuccess)                                                                   \
        return fail(c, HG_ERR_HIP, "hipSetDevice(%d) failed: %s", (c)->device, hipGetErrorString(dev_guard_.err))
// tokens per image a tower with instance adapters may have (option adapter_long), and what a refusal adds while the option could help
inline int adapter_max_tokens(const hg_ctx* c) { return c->opt_adapter_long ? hg::ADAPTER_LONG_MAX_L : hg::ADAPTER_MAX_L; }
inline const char* adapter_long_hint(const hg_ctx* c, int L) {
    return !c->opt_adapter_long && L <= hg::ADAPTER_LONG_MAX_L ? "; set option adapter_long = 1 (up to 640 tokens)" : "";
}
// first failing status wins (OR-ing negative codes can turn OOM into another code)
inline void keep_first(int& rc, int r) {
    if (!rc) rc = r;
}

inline int ensure(hg_ctx* c, Buf& b, size_t bytes) {
    if (b.bytes >= bytes) return HG_OK;
    if (b.p) HG_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    bytes = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) return fail(c, HG_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    // growth only (never in steady state): zero the padding rows and order the memset against every stream, also
    // non-blocking ones that do not synchronise with the null stream
    HG_HIP(hipMemset(b.p, 0, bytes));
    HG_HIP(hipDeviceSynchronize());
    b.bytes = bytes;
    return HG_OK;
}

inline void free_all(std::vector<void*>& v) {
    for (void* p : v) (void)hipFree(p);
    v.clear();
}

inline size_t rup(size_t v, size_t m) { return (v + m - 1) / m * m; }

// ---- weights into device memory: what every loader shares (synchronous; load time only) ------------------------------------------------
inline int dev_alloc(hg_ctx* c, std::vector<void*>& owned, size_t bytes, void** out) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(c, HG_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    owned.push_back(p);
    *out = p;
    return HG_OK;
}

template <typename T>
inline int dev_alloc_n(hg_ctx* c, std::vector<void*>& owned, size_t n, T** out) {      // n elements
    void* p;
    int rc = dev_alloc(c, owned, n * sizeof(T), &p);
    if (!rc) *out = (T*)p;
    return rc;
}

// n elements of t from element `off` on, as fp16 / fp32, into dst: a copy where the dtype matches, the conversion kernel where it is the
// other one.  The message is `who` ("" or "hg_load_x: ") and the tensor's `name` as the caller formatted it.
inline int cvt_f16(hg_ctx* c, const hg_tensor& t, size_t off, size_t n, half_t* dst, const char* who, const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "%smissing tensor %s", who, name);
    if (t.dtype == HG_F16) HG_HIP(hipMemcpy(dst, (const half_t*)t.ptr + off, n * 2, hipMemcpyDeviceToDevice));
    else if (t.dtype == HG_F32) HG_HIP(launch_f32_to_f16((const float*)t.ptr + off, dst, n, 0));
    else return fail(c, HG_ERR_INVALID, "%sbad dtype for %s", who, name);
    return HG_OK;
}

inline int cvt_f32(hg_ctx* c, const hg_tensor& t, size_t off, size_t n, float* dst, const char* who, const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "%smissing tensor %s", who, name);
    if (t.dtype == HG_F32) HG_HIP(hipMemcpy(dst, (const float*)t.ptr + off, n * 4, hipMemcpyDeviceToDevice));
    else if (t.dtype == HG_F16) HG_HIP(launch_f16_to_f32((const half_t*)t.ptr + off, dst, n, 0));
    else return fail(c, HG_ERR_INVALID, "%sbad dtype for %s", who, name);
    return HG_OK;
}

// ... into memory of their own, which `owned` keeps
inline int as_f16(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, size_t n, half_t** out, const char* name, const char* who = "",
                  size_t off = 0) {
    int rc = dev_alloc_n(c, owned, n, out);
    return rc ? rc : cvt_f16(c, t, off, n, *out, who, name);
}

inline int as_f32(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, size_t n, float** out, const char* name, const char* who = "",
                  size_t off = 0) {
    int rc = dev_alloc_n(c, owned, n, out);
    return rc ? rc : cvt_f32(c, t, off, n, *out, who, name);
}

// hipEvent pair around one launch when its kind is being profiled
struct ProfScope {
    hg_ctx* c;
    hipStream_t s;
    bool on;
    ProfScope(hg_ctx* c_, hipStream_t s_, int kind, int M, int N, int K) : c(c_), s(s_), on(false) {
        if (c->prof_kind == HG_PROF_OFF || (c->prof_kind != HG_PROF_ALL && c->prof_kind != kind)) return;
        if (2 * c->prof_n + 1 >= c->prof_ev.size()) return;
        if (hipEventRecord(c->prof_ev[2 * c->prof_n], s) != hipSuccess) return;
        c->prof_rec[c->prof_n] = hg_prof_rec{kind, M, N, K, 0.f};
        on = true;
    }
    void finish() {
        if (on && hipEventRecord(c->prof_ev[2 * c->prof_n + 1], s) == hipSuccess) c->prof_n++;
        on = false;
    }
    ~ProfScope() { finish(); }
};

inline hipError_t gemm(hg_ctx* c, int epi, const GemmArgs& g, hipStream_t s) {
    ProfScope ps(c, s, epi, g.M, g.N, g.K);
    return launch_gemm(epi, g, s);
}

inline hipError_t attention(hg_ctx* c, const half_t* qkv, half_t* out, int n_seq, int L, int heads, bool causal, hipStream_t s,
                     int ldo = 0) {
    ProfScope ps(c, s, HG_PROF_ATTENTION, n_seq, L, heads);
    return launch_attention(qkv, out, n_seq, L, heads, causal, s, ldo);
}

// the nine fields every GEMM call sets; what a call sets beyond them it sets behind this
inline GemmArgs gemm_args(const half_t* A, int lda, const half_t* W, const float* bias, void* out, int ldc, int M, int N, int K) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.bias = bias; g.out = out; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    return g;
}

// hg_load.hip: the text tower's in_proj operands in the fused kernel's fragment order, packed on the first call that needs them
int ensure_text_packs(hg_ctx* c, std::vector<void*>& owned, std::vector<BlockW>& blocks, int D, bool gamma);
// hg_text_bwd.hip: the transposed weights of the text tower's input gradient, built on first use
int ensure_text_grad(hg_ctx* c);
// ... one block of that backward: g [M, D] fp32 (in place: the gradient of the block's output -> of its input) from the block's saved
// input x_in [M, D]; the block is recomputed into the tower workspace, the gradients live in c->tgrad (text_grad_ws)
int text_grad_ws(hg_ctx* c, int M, int R);
int text_block_backward(hg_ctx* c, int block, const float* x_in, float* g, int n_seq, int L, hipStream_t s);
}  // namespace hg_host
