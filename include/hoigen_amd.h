/*
 * hoigen_amd — C ABI of the MI355X (gfx950) hot path of HOIGen.
 *
 * The reference (soberguo/HOIGen) has no FFI: its boundary is Python duck-typing on nn.Module
 * attributes.  This header is the boundary a binding for that path would target;
 * `hoigen_amd/_lib.py` is the ctypes binding and `hoigen_amd/{clip,model,vae}.py` present the
 * reference's own Python signatures on top of it.  Every entry point names the reference
 * interface it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *  - All data pointers are DEVICE pointers to contiguous row-major buffers owned by the caller.
 *  - Calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *  - Return value: 0 on success, negative hg_status on failure; text via hg_last_error().
 *  - One context per device per process; a context is not re-entrant (the reference is
 *    single-threaded per process, one process per GPU: main_tip_finetune.py:1205-1208).
 *  - The library allocates device memory only in hg_create / hg_load_* / on workspace growth
 *    (monotonic); steady-state calls do not allocate or synchronise (hipGraph-capturable).
 *  - Arithmetic: fp16 MFMA operands, fp32 accumulation; residual stream, LayerNorm statistics and
 *    softmax in fp32.  Inference only (no autograd).
 */
#ifndef HOIGEN_AMD_H
#define HOIGEN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hg_ctx hg_ctx;

typedef enum {
    HG_OK = 0,
    HG_ERR_INVALID = -1,     /* bad argument / unsupported shape            */
    HG_ERR_HIP = -2,         /* a HIP runtime call failed                   */
    HG_ERR_NOT_LOADED = -3,  /* weights for this entry point not loaded yet */
    HG_ERR_OOM = -4
} hg_status;

typedef enum { HG_F32 = 0, HG_F16 = 1 } hg_dtype;

/* A weight tensor handed to hg_load_*: device pointer + element type.  ptr == NULL means absent. */
typedef struct {
    const void* ptr;
    int32_t dtype; /* hg_dtype */
} hg_tensor;

/* ResidualAttentionBlock parameters — clipnet/model.py:167-188; state-dict keys
 * `{prefix}.resblocks.{i}.{attn.in_proj_weight,...}`.  Linear weights are [out,in]. */
typedef struct {
    hg_tensor in_proj_weight;  /* [3D, D]  rows q|k|v */
    hg_tensor in_proj_bias;    /* [3D]                */
    hg_tensor out_proj_weight; /* [D, D]              */
    hg_tensor out_proj_bias;   /* [D]                 */
    hg_tensor ln_1_weight, ln_1_bias; /* [D] */
    hg_tensor c_fc_weight;     /* [4D, D] */
    hg_tensor c_fc_bias;       /* [4D]    */
    hg_tensor c_proj_weight;   /* [D, 4D] */
    hg_tensor c_proj_bias;     /* [D]     */
    hg_tensor ln_2_weight, ln_2_bias; /* [D] */
} hg_block_weights;

/* TransformerDecoderLayer(64, nhead=2, ffn=128) as used by the adapter —
 * CLIP_models_adapter_prior2.py:27-72 (forward_post; norm1 exists but is unused). */
typedef struct {
    hg_tensor attn_in_proj_weight;  /* [3d, d] */
    hg_tensor attn_in_proj_bias;    /* [3d]    */
    hg_tensor attn_out_proj_weight; /* [d, d]  */
    hg_tensor attn_out_proj_bias;   /* [d]     */
    hg_tensor linear1_weight, linear1_bias; /* [2d, d], [2d] */
    hg_tensor linear2_weight, linear2_bias; /* [d, 2d], [d]  */
    hg_tensor norm2_weight, norm2_bias;     /* [d] */
    hg_tensor norm3_weight, norm3_bias;     /* [d] */
} hg_decoder_layer_weights;

/* Adapter — CLIP_models_adapter_prior2.py:142-203; keys `...resblocks.{i}.adaptermlp.*`. */
typedef struct {
    int32_t present;                 /* 0: this block has no adapter (adapter_pos, :958-967) */
    int32_t bottleneck;              /* 64 */
    hg_tensor scale;                 /* [D]   */
    hg_tensor down_proj_weight, down_proj_bias; /* [d, D], [d] */
    hg_tensor up_proj_weight, up_proj_bias;     /* [D, d], [D] */
    hg_decoder_layer_weights prior_layer;       /* mhsa_layers.0 (memory = prior tokens) */
    hg_decoder_layer_weights self_layer;        /* mhsa          (memory = down itself)  */
    /* adapter_num_layers > 1 (CLIP_models_adapter_prior2.py:150,179,190-195): mhsa_layers.1 .. N-1, applied one after
     * the other on the prior path; NULL / 0 for the default single layer */
    int32_t n_extra_prior_layers;
    const hg_decoder_layer_weights* extra_prior_layers;
} hg_adapter_weights;

/* VisionTransformer — clipnet/model.py:202-236 (variant A) and
 * CLIP_models_adapter_prior2.py:471-506 (variant C). */
typedef struct {
    int32_t width, layers, heads, patch_size, input_resolution, output_dim;
    hg_tensor conv1_weight;          /* [D, 3, p, p]     */
    hg_tensor class_embedding;       /* [D]              */
    hg_tensor positional_embedding;  /* [g*g+1, D]       */
    hg_tensor ln_pre_weight, ln_pre_bias, ln_post_weight, ln_post_bias; /* [D] */
    hg_tensor proj;                  /* [D, E]  (x @ proj) */
    const hg_block_weights* blocks;      /* [layers] */
    const hg_adapter_weights* adapters;  /* NULL or [layers] */
} hg_vit_weights;

/* Text tower of CLIP — clipnet/model.py:282-292,339-352. */
typedef struct {
    int32_t width, layers, heads, context_length, vocab_size, output_dim;
    hg_tensor token_embedding;       /* [V, D]  */
    hg_tensor positional_embedding;  /* [L, D]  */
    hg_tensor ln_final_weight, ln_final_bias; /* [D] */
    hg_tensor text_projection;       /* [D, E]  (x @ text_projection) */
    const hg_block_weights* blocks;  /* [layers] */
} hg_text_weights;

/* CoOp-VAE — main_coop_vae.py:261-296.  Any of the two halves may be absent (ptr NULL). */
typedef struct {
    int32_t dim, enc_hidden, gen_hidden;       /* 512, 2048, 4096 */
    hg_tensor enc_w0, enc_b0;                  /* Encoder.net.0     [2048,512],[2048] */
    hg_tensor enc_mean_w, enc_mean_b;          /* Encoder.mean      [512,2048],[512]  */
    hg_tensor enc_logvar_w, enc_logvar_b;      /* Encoder.log_var   [512,2048],[512]  */
    hg_tensor gen_w0, gen_b0;                  /* Generator.net.0   [4096,512],[4096] */
    hg_tensor gen_w2, gen_b2;                  /* Generator.net.2   [512,4096],[512]  */
} hg_vae_weights;

/* mlp_net(512,512,512) — finetune_ship.py:302-314 / main_tip_finetune.py:313-324. */
typedef struct {
    int32_t in_dim, hidden_dim, out_dim;
    hg_tensor w0, b0, w2, b2, w4, b4;
} hg_mlp_weights;

#define HG_MAX_SLOTS 16 /* independent VAE / mlp_net weight sets per context: three branches (hoi, human, object) x Encoder, Generator, VAE + spares */

/* ---- lifecycle ------------------------------------------------------------------------- */
hg_ctx* hg_create(int device);                 /* NULL on failure (no HIP device)               */
void hg_destroy(hg_ctx*);
const char* hg_last_error(hg_ctx*);            /* valid until the next call on the context      */
const char* hg_version(void);

/* ---- weights (replace nn.Module.load_state_dict / build_model: clipnet/model.py:395-432,
 *      CLIP_models_adapter_prior2.py:934-984).  Weights are copied/converted; the caller may free
 *      its tensors afterwards.  Loading again replaces the previous set. -------------------------- */
/* hg_load_vit limits: width a multiple of 128 with heads = width / 64, width <= 1024; output_dim a multiple of 128; any patch
 * size p that divides input_resolution (p = 16, 32: 8 pixels per thread; any other p, e.g. 14: one patch row per thread, the patch
 * GEMM's K = 3 p p padded with zeros to a multiple of 64, 588 -> 640); tokens per image L = (input_resolution / p)^2 + 1 <= 640
 * (ViT-B/16: 197, ViT-L/14: 257, ViT-L/14@336px: 577; L <= 224 and 225 .. 640 run different attention kernels).  Instance adapters
 * need L <= 224, or L <= 640 with option "adapter_long" = 1 (set before the load): otherwise adapter weights for a tower with more
 * tokens are refused here and by hg_update_adapters (HG_ERR_INVALID, the message says so); such a tower runs variants A and
 * C-without-adapters (hg_encode_image_prior with priors == NULL). */
int hg_load_vit(hg_ctx*, const hg_vit_weights*);
int hg_load_text(hg_ctx*, const hg_text_weights*);
int hg_load_vae(hg_ctx*, int slot, const hg_vae_weights*);
int hg_load_mlp(hg_ctx*, int slot, const hg_mlp_weights*);
/* Refresh only the adapter tensors of an already-loaded ViT (they are the trainable part:
 * main_tip_finetune.py:955-962). */
int hg_update_adapters(hg_ctx*, const hg_adapter_weights* adapters, int layers);

/* ---- image tower --------------------------------------------------------------------------- */
/* CLIP.encode_image / VisionTransformer.forward, variant A (clipnet/model.py:219-236,336-337):
 * x [B,3,R,R] fp32 NCHW -> out [B,E] fp32.  Any B: a call runs in passes of 256 crops (L <= 224 tokens per image) or of
 * 256 * 224 / L crops (longer towers: 99 crops of 577 tokens), which bounds the workspaces; results do not depend on where a pass
 * ends.  Limits of L and p: hg_load_vit. */
int hg_encode_image(hg_ctx*, const float* x_nchw, int B, float* out, void* stream);
/* Variant C VisionTransformer.forward(x, prior) (CLIP_models_adapter_prior2.py:489-506).
 * priors [B,N,64] fp32 and mask [B,N] uint8 (1 = padded key) or both NULL / N == 0 for prior=None.
 * out_global [B,E]; out_local [B,E,g,g] (NCHW).  Blocks without a loaded adapter behave as A.  Towers of more than 224 tokens
 * per image loaded with an fp32 proj apply it as hi + lo fp16 (two GEMM passes) in this entry point. */
int hg_encode_image_prior(hg_ctx*, const float* x_nchw, const float* priors, const uint8_t* mask,
                          int B, int N, float* out_global, float* out_local_nchw, void* stream);
/* Test hook: as hg_encode_image, additionally copies the CLS row of the residual stream after
 * ln_pre and after every block into trace [(layers+1), B, D] fp32. */
int hg_encode_image_trace(hg_ctx*, const float* x_nchw, int B, float* out, float* trace, void* stream);

/* ---- text tower ---------------------------------------------------------------------------- */
/* CLIP.encode_text (clipnet/model.py:339-352): ids [T,L] int32 (L <= context_length), zero padded,
 * EOT = largest id per row -> out [T,E] fp32.  `trunc` != 0 runs the causal tower only on the first
 * max(EOT)+1 positions (identical selected outputs; SURVEY.md §5 "Long-context"). */
int hg_encode_text_ids(hg_ctx*, const int32_t* ids, int T, int L, float* out, int trunc, void* stream);
/* TextEncoder.forward(prompts, tokenized_prompts) (main_coop_vae.py:54-63): prompts [R,L,D] fp32
 * already embedded, eot_idx [R] int32 = tokenized_prompts.argmax(-1) -> out [R,E] fp32. */
int hg_encode_text_embeds(hg_ctx*, const float* prompts, const int32_t* eot_idx, int R, int L,
                          float* out, int trunc, void* stream);
/* The input gradient of TextEncoder.forward: what the CoOp-VAE training loop back-propagates through the frozen tower
 * (main_coop_vae.py:452-468 with CLIP frozen at :316-318).  No weight gradient of the tower is computed.
 *
 * hg_encode_text_embeds_save is hg_encode_text_embeds - the same plan, launches and bits in `out` - and additionally copies into the
 * caller's `saved`, fp32 [layers * R * Leff + R][D], the stream as it enters every block ([layers][R * Leff][D]) and the last block's
 * output on the EOT rows ([R][D]); Leff = trunc where 0 < trunc < L, else L.  The state lives in the caller's memory because every other
 * entry point reuses the context's workspace between forward and backward.  One pass of the text tower at most (a budget of 65 536 rows:
 * 256 prompts of 77 tokens are one pass); a longer call is refused with HG_ERR_INVALID.
 *
 * hg_text_backward_embeds: grad_out [R,E] fp32 -> grad_prompts [R,L,D] fp32 from that `saved`, the same eot_idx, L and trunc.  Each
 * block is recomputed from its saved input and walked backwards; Leff <= 80.  Gradients that are MFMA operands are
 * fp16, so the backward runs on grad_out scaled per prompt by the power of two that brings its largest element into [1, 2) and is
 * unscaled at its end; nothing saturates (an overflow shows as Inf / NaN in that prompt's gradient).  Rows behind a prompt's EOT and
 * positions >= Leff are exactly 0.  The transposed copies of the linears the backward GEMMs read (76 MB for ViT-B/16's text tower) are
 * built on the first call - synchronously, on the null stream, so not inside a stream capture - and dropped by hg_load_text.  Workspace
 * of the context beyond the forward's: 26 bytes x rows x D (263 MB for 256 prompts of 77 tokens at D = 512). */
int hg_encode_text_embeds_save(hg_ctx*, const float* prompts, const int32_t* eot_idx, int R, int L, float* out, int trunc,
                               float* saved, void* stream);
int hg_text_backward_embeds(hg_ctx*, const float* saved, const int32_t* eot_idx, const float* grad_out, int R, int L, int trunc,
                            float* grad_prompts, void* stream);
/* token_embedding(ids) (clipnet/model.py:340): ids [n] int32 -> out [n,D] fp32 (exact gather). */
int hg_token_embedding(hg_ctx*, const int32_t* ids, int n, float* out, void* stream);

/* ---- CoOp-VAE ------------------------------------------------------------------------------ */
/* Encoder -> reparameterise(eps given) -> Generator (main_coop_vae.py:444-448).
 * x, eps [R,dim] fp32 -> mean, logvar, z, bias [R,dim] fp32 (any output may be NULL). */
int hg_vae_forward(hg_ctx*, int slot, const float* x, const float* eps, int R, float* mean,
                   float* logvar, float* z, float* bias, void* stream);
/* Generator.forward (main_coop_vae.py:293-296): z [R,dim] -> bias [R,dim]. */
int hg_generator(hg_ctx*, int slot, const float* z, int R, float* bias, void* stream);
/* mlp_net.forward (finetune_ship.py:312-314). */
int hg_mlp_net(hg_ctx*, int slot, const float* x, int R, float* out, void* stream);
/* PromptLearner_*.forward (main_coop_vae.py:119-128): prefix [C,1,D], suffix [C,L-1-n_ctx,D],
 * ctx [n_ctx,D], bias [R,D], target [R] int32 -> prompts [R,L,D]; all fp32. */
int hg_assemble_prompts(hg_ctx*, const float* prefix, const float* suffix, const float* ctx,
                        const float* bias, const int32_t* target, int R, int C, int L, int n_ctx,
                        int D, float* prompts, void* stream);
/* Backward of PromptLearner_*.forward (main_coop_vae.py:119-128: prompts = [prefix | ctx + bias | suffix]): grad_prompts [R,L,D] ->
 * grad_bias [R,D] = sum_j g[r][1 + j] and grad_ctx [n_ctx,D] = sum_r g[r][1 + j]; either may be NULL.  grad_ctx is summed in two stages
 * in a fixed order (64 prompts of a chunk in ascending order, then the chunks): no atomics, the same bits on every run. */
int hg_assemble_prompts_backward(hg_ctx*, const float* grad_prompts, int R, int L, int n_ctx, int D, float* grad_ctx,
                                 float* grad_bias, void* stream);
/* x / x.norm(dim=-1, keepdim=True) (main_coop_vae.py:438,466); in == out allowed. */
int hg_l2_normalize(hg_ctx*, const float* x, int R, int D, float* out, void* stream);
/* RoI-align over the variant-C local feature map (SURVEY.md 8f-4;
 * upt_tip_cache_model_free_finetune_distill3.py:1026-1037): torchvision.ops.roi_align(feat[None], [boxes],
 * output_size=(P,P), spatial_scale, sampling_ratio=-1, aligned=True) -> out_pooled [n,C,P,P] (nullable) and its
 * .flatten(2).mean(-1) -> out_mean [n,C] (nullable).  feat: fp32 [C,H,W] (one image of hg_encode_image_prior's
 * out_local), boxes: fp32 [n,4] (x1,y1,x2,y2) in image pixels; all device pointers. */
int hg_roi_align(hg_ctx*, const float* feat, int C, int H, int W, const float* boxes, int n, float spatial_scale,
                 int P, float* out_pooled, float* out_mean, void* stream);

/* Cache-model (Tip-adapter) logits on the embeddings (SURVEY.md 8f-3;
 * upt_tip_cache_model_free_finetune_distill3.py:1158-1170):
 *   phi = f @ weight.T + bias ; logits = (phi @ labels) / sample_lens / post_div          -> [R, C]
 * weight [S,K] (cached, L2-normalised embeddings; K % 64 == 0), bias [S] (nullable = 0), labels [S,C] multi-hot
 * (values exactly representable in fp16), sample_lens [C], post_div (2 for the HO branch, else 1).
 * With labels.ptr == NULL the slot is a plain linear map (logits_text = f @ weight.T + bias -> [R, S]). */
#define HG_MAX_CACHE_SLOTS 8
typedef struct {
    hg_tensor weight, bias, labels, sample_lens;
    int32_t S, K, C;
    float post_div;
} hg_cache_weights;
int hg_load_cache(hg_ctx*, int slot, const hg_cache_weights* w);
int hg_cache_logits(hg_ctx*, int slot, const float* feats, int R, float* out, void* stream);

/* The interaction head for a batch of images in one call: UPT.compute_roi_embeddings in eval mode with individual_norm = True,
 * logits_type = 'HO+U+T', the DINO branch as a per-image source (below), no use_weight_pred, generated features not appended
 * (upt_tip_cache_model_free_finetune_distill3.py:959-1268), compute_prior_scores (:806-833) and the score of postprocessing
 * (:1408-1427).  Image b has the boxes box_off[b] .. box_off[b + 1] - 1, HUMANS FIRST (the caller applies the permutation of
 * :988-996), n_human[b] of them humans.  Its pairs are all (x, y) with x < n_human[b], y != x, row-major (:1007-1012):
 * n_human (n - 1) of them, none when n_human == 0 or n <= 1 (:998).  Pt = all pairs of the batch, N = box_off[B].
 *   pair_h / pair_o / objects  int32 [Pt]: x, y (local to the image) and labels[y]                                      (:1245-1247)
 *   union_boxes                [Pt, 4]: min / max of the two boxes' corners                                             (:1019-1023)
 *   pooled_single [N, C], pooled_union [Pt, C]: torchvision.ops.roi_align(.., (P, P), spatial_scale, aligned=True)
 *       .flatten(2).mean(-1) of every box and union box (:1027-1037), as ONE contraction per RoI and channel against the separable
 *       weights of its samples - not hg_roi_align's operation order: equal within both rounding bounds, not bit for bit
 *   feats                      [Pt, 3C] = human | object | union rows, each x / x.norm() (:1044-1050) as hg_l2_normalize computes it
 *   branch_logits              [n_branch, Pt, num_classes]: branch i = hg_cache_logits(branch[i].slot) on the rows of its source:
 *       human, object, union [Pt, C], human|object [Pt, 2C] (:1166) or feat_global[b] / its norm repeated over the image's pairs
 *       (:960, :1132-1138)                                                                                              (:1156-1170)
 *   logits                     [Pt, num_classes] = branch_0 * scale_0 + branch_1 * scale_1 + .., left to right          (:1195-1196)
 *   prior                      [2, Pt, num_classes]: scores[x] ^ score_pow and scores[y] ^ score_pow on the columns where
 *       obj2target[labels[y]] is set (uint8 [n_obj_classes, num_classes], device), 0 elsewhere                          (:806-833)
 *   scores                     [Pt, num_classes] = sigmoid(logits) * prior[0] * prior[1]                                (:1417-1423)
 * A zero-area box pools to 0 and its normalised row is NaN, as in the reference; so are the rows of every pair that contains it.
 * feat_local fp32 [B, C, H, W] (hg_encode_image_prior's out_local), feat_global fp32 [B, C] (nullable without a global branch),
 * boxes [N, 4] (x1, y1, x2, y2, image pixels), scores [N], labels int32 [N]: device.  box_off [B + 1], n_human [B]: HOST.
 * The DINO branch (:1111-1115, :1184-1207) is a branch of source HG_HOI_SRC_IMAGE, through hg_hoi_head_image (below): branch i = hg_cache_logits(branch[i].slot) on the B
 * rows of feat_image [B, K_img] TAKEN AS THEY ARE (the caller normalises: hg_resnet_features' `features`), converted to fp16 once and
 * computed ONCE PER IMAGE - for all B images whenever Pt > 0 - on a zero-padded 256-row operand of its own whose padding rows are
 * rewritten on every call; pair p reads row b(p).  The sum stays scale_0 * branch_0 + scale_1 * branch_1 + .. in list order, so
 * [H, O, U, text, global, image] is :1205-1207 term for term.  image_logits (nullable) receives [n image branches, B, num_classes] in
 * list order; in branch_logits an image branch's [Pt, num_classes] slab holds the broadcast rows.  HG_ERR_INVALID for an image source
 * without feat_image, K_img <= 0, K_img % 64 != 0 or K_img > 4096, a slot whose K != K_img or whose width is not num_classes.
 * Limits: B <= 64, H, W <= 32, C <= 1024, P <= 32, n_branch <= 6; with branches C % 64 == 0, every slot loaded (hg_load_cache) with K = C
 * (2C for human|object) and output width num_classes.  n_branch == 0 pools only (any C; logits may be NULL, prior may be asked for, scores_out may not: HG_ERR_INVALID).  Every output but
 * logits may be NULL.  Asynchronous on `stream`. */
#define HG_HOI_MAX_BRANCH 6
#define HG_HOI_SRC_HUMAN 0
#define HG_HOI_SRC_OBJECT 1
#define HG_HOI_SRC_UNION 2
#define HG_HOI_SRC_HUMAN_OBJECT 3
#define HG_HOI_SRC_GLOBAL 4
#define HG_HOI_SRC_IMAGE 5 /* a row per IMAGE from feat_image, computed once per image and added to every pair of it (the DINO branch) */
typedef struct {
    int32_t source, slot;
    float scale;
} hg_hoi_branch;
typedef struct {
    const float *feat_local, *feat_global, *boxes, *scores;
    const int32_t* labels;
    const int32_t *box_off, *n_human;
    int32_t B, C, H, W, P;
    float spatial_scale;
    int32_t n_branch;
    hg_hoi_branch branch[HG_HOI_MAX_BRANCH];
    const uint8_t* obj2target;
    int32_t n_obj_classes, num_classes;
    float score_pow;
    int32_t *pair_h, *pair_o, *objects;
    float *union_boxes, *pooled_single, *pooled_union, *feats, *branch_logits, *logits, *prior, *scores_out;
} hg_hoi_head_args;
int hg_hoi_head(hg_ctx*, const hg_hoi_head_args* args, void* stream);
/* hg_hoi_head_image: hg_hoi_head with the rows of the HG_HOI_SRC_IMAGE branches.  hg_hoi_head_args keeps its layout, so the three
 * values travel in a struct of their own; `image` NULL is hg_hoi_head itself (which is this call with NULL: the same launches as before the source existed - the
 * epilogue kernel's by-value argument struct grew by the per-branch flags - and an image branch in its list is refused for want of
 * feat_image). */
typedef struct {
    const float* feat_image;               /* fp32 [B, K_img], device */
    int32_t K_img;
    float* image_logits;                   /* nullable: [n image branches, B, num_classes] */
} hg_hoi_image_args;
int hg_hoi_head_image(hg_ctx*, const hg_hoi_head_args* args, const hg_hoi_image_args* image, void* stream);

/* Region proposals and instance priors for a batch of images in one call: what UPT.forward does between DETR's PostProcess and the
 * encoders (upt_tip_cache_model_free_finetune_distill3.py:1543-1660).
 *
 * hg_load_priors: priors_downproj = MLP(E + 5, hidden, 64, 3) (:40-52, :520; state-dict keys layers.{0,1,2}.{weight,bias}) and
 * object_embedding [n_obj_classes, E] (:1464) for prior_type 'cbe', prior_method 0 (:468-469).  The label-dependent part of the first
 * layer is folded into a table here: T[c][n] = sum_k object_embedding[c][k] * w0[n][5 + k] (fp32, k ascending, one accumulator, multiply
 * and add rounded separately).  Calling it again on a loaded slot is the update path (priors_downproj is trainable during adapter
 * fine-tuning); the next hg_region_priors sees the new weights.  Synchronous.
 * Limits: E <= 1024, hidden <= 256, out == 64, n_obj_classes <= 256. */
#define HG_MAX_PRIOR_SLOTS 4
typedef struct {
    int32_t E, hidden, out, n_obj_classes;
    hg_tensor w0, b0; /* [hidden, E + 5], [hidden] */
    hg_tensor w1, b1; /* [hidden, hidden], [hidden] */
    hg_tensor w2, b2; /* [out, hidden], [out] */
    hg_tensor object_embedding; /* [n_obj_classes, E] */
} hg_prior_weights;
int hg_load_priors(hg_ctx*, int slot, const hg_prior_weights* w);
/* hg_region_priors: prepare_region_proposals (:1361-1406), get_prior (:1445-1495) and priors_downproj (:1492) of B images.
 * Input: what DETR's PostProcess returns (detr/models/detr.py:258-290), concatenated: scores [Qt], labels int32 [Qt], boxes [Qt, 4]
 * (x1, y1, x2, y2 in pixels; 16-byte aligned), image b = rows q_off[b] .. q_off[b + 1] - 1.
 *   class-aware NMS   torchvision.ops.boxes._batched_nms_coordinate_trick (the path batched_nms takes below 4 000 boxes), restated in
 *       fp32, one rounding per operation: off = (float)label * (max coordinate of the image + 1.0f), every coordinate + off, a STABLE
 *       order by descending score (ties to the lower input index - the reference's argsort leaves them open), greedy suppression where
 *       inter / ((area_i + area_j) - inter) > nms_thresh, inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0),
 *       area = (x2 - x1) * (y2 - y1) on the offset boxes.  0 / 0 is not > nms_thresh: the box stays.                         (:1367)
 *   selection         over the survivors in order: h = humans (label == human_idx) with score >= box_score_thresh; h < min_instances
 *       takes the first min_instances humans of ALL survivors (or as many as there are), h > max_instances the first max_instances,
 *       otherwise those h; the other labels likewise; output = humans, then the others, each by descending score         (:1371-1398)
 *   priors            row = (score, x1 / w, y1 / h, x2 / w, y2 / h, object_embedding[label]) with (h, w) = image_sizes[b], a division;
 *       three linears, ReLU behind the first two; rows n_b .. cap - 1 hold the MLP of a zero row, as the reference's padded tensor
 *       does; mask = 1 there                                                                                              (:1445-1495)
 * Output, cap = 2 * max_instances slots per image:
 *   counts      int32 [B, 4] = n, n_human, status, number of NMS survivors
 *   keep        int32 [B, cap]   indices into the image's input list (-1 behind n)
 *   out_boxes [B, cap, 4] (16-byte aligned), out_scores [B, cap], out_labels int32 [B, cap]   (0, 0, -1 behind n)
 *   survivors   int32 [Qt], nullable: image b's NMS survivors in order, from q_off[b] on (counts[b][3] of them; the rest is not written)
 *   priors      [B, cap, 64], mask uint8 [B, cap]        (prior_slot >= 0)
 *   table_out   [n_obj_classes, hidden], nullable: the slot's table T
 * keep, out_boxes, out_scores and out_labels may be NULL together (the library's workspace holds them).  prior_slot = -1: proposals only.
 * status: bit 0 = the image has a non-finite score or coordinate, bit 1 = a label outside [0, n_obj_classes) (prior_slot >= 0 only);
 * such an image gets n = 0 and pad rows; the other images of the batch are not affected.
 * q_off [B + 1] and image_sizes [B, 2] = (h, w) as floats: HOST.  Limits: B <= 64, q_off[b + 1] - q_off[b] <= 512,
 * 0 <= min_instances <= max_instances, 1 <= max_instances <= 32.  No host synchronisation, no allocation in steady state. */
typedef struct {
    const float* scores;
    const int32_t* labels;
    const float* boxes;
    const int32_t* q_off;
    const float* image_sizes;
    int32_t B;
    float box_score_thresh, nms_thresh;
    int32_t human_idx, min_instances, max_instances, prior_slot;
    int32_t *counts, *keep;
    float *out_boxes, *out_scores;
    int32_t *out_labels, *survivors;
    float* priors;
    uint8_t* mask;
    float* table_out;
} hg_region_priors_args;
int hg_region_priors(hg_ctx*, const hg_region_priors_args* args, void* stream);

/* hg_hoi_detections: what follows hg_hoi_head, for the B images of that call - the detections of UPT.postprocessing
 * (upt_tip_cache_model_free_finetune_distill3.py:1408-1427) compacted on the device, and, with ground truth, test_hico's per-image body
 * (utils_tip_cache_and_union_finetune.py:376-409): conversion[objects, verbs] (:385-388), recover_boxes (upt...:1269-1274,
 * detr/util/box_ops.py:9-13), the `for hoi_idx in unique_hoi` loop (:394-407) with BoxPairAssociation(min_iou)
 * (pocket/pocket/utils/association.py:17-116) for all classes of an image at once.
 * Input: hg_hoi_head's prior [2, Pt, NC], scores_out [Pt, NC], pair_h / pair_o / objects [Pt] and the batch's boxes [N, 4]: device.
 * pair_off [B + 1], box_off [B + 1]: HOST.  conversion int32 [n_obj_classes, NC], device, nullable: object_n_verb_to_interaction with -1
 * where the reference has None; NULL = the interaction is the verb (num_classes 600).
 *   detections   every (p, c) with prior[0][p][c] * prior[1][p][c] != 0 - ONE fp32 multiply, a NaN counts, as torch.nonzero has it - in
 *       row-major order (:1418).  Image b's entries are the slots det_off[b] .. det_off[b + 1] - 1:
 *       det_pair = p - pair_off[b], det_verb = c, det_h / det_o = pair_h[p] / pair_o[p], det_object = objects[p],
 *       det_score = the word scores[p][c], det_interaction = conversion[objects[p]][c] or c.  Nothing is written at or beyond slot cap;
 *       det_off always holds the true counts.
 *   ground truth (gt_off != NULL): gt_boxes_h, gt_boxes_o [Gt, 4], gt_hoi int32 [Gt]: device; gt_off [B + 1], gt_sizes int32 [B, 2] =
 *       (h, w): HOST.  gt_format 0 = x1, y1, x2, y2 in pixels, taken as they are; 1 = normalised cx, cy, w, h recovered as
 *       ((cx - 0.5f w) (float)w_img, (cy - 0.5f h) (float)h_img, (cx + 0.5f w) (float)w_img, (cy + 0.5f h) (float)h_img), one rounding per
 *       operation.  gt_boxes_out [2, Gt, 4] = the recovered boxes, human then object.
 *   association  for detection d and every ground-truth pair g of its image with gt_hoi[g] == det_interaction[d] (>= 0):
 *       iou = min(iou_h, iou_o), each torchvision's box_iou in fp32, one rounding per operation: area = (x2 - x1) * (y2 - y1),
 *       inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0), iou = inter / ((area_g + area_d) - inter); minimum, maximum and the
 *       clamp hand a NaN on as torch's do.  det_max_iou / det_gt = iou.max(0): the first index of the maximum, relative to the image; a NaN
 *       makes the maximum NaN (written as 0x7FC00000) from its first index on.  No ground truth of the class (or interaction -1, or a
 *       pair index outside the image's boxes): det_gt = -1, det_max_iou = 0.  d is a candidate of det_gt[d] alone, and only if
 *       det_max_iou > min_iou (strict; NaN is not greater).  Per ground-truth pair the candidate with the highest score gets det_label 1
 *       (a NaN score ranks above every number, -0 == +0, ties go to the lowest detection index, as argmax has it), every other
 *       detection 0.
 *   status       int32 [B]: bit 0 = an entry whose conversion is negative or whose object lies outside the table (its interaction is -1 and
 *       its label 0), bit 1 = a non-finite recovered ground-truth box, bit 2 = the image's entries end behind slot cap.
 * The results do not depend on the batch around an image or on the order in which workgroups run: slots come from a prefix sum, the winner
 * of a ground-truth pair from the maximum of distinct keys.  Every output but det_off [B + 1] may be NULL; det_label, det_gt, det_max_iou and
 * gt_boxes_out need gt_off and stay untouched without it.  Limits (HG_ERR_INVALID otherwise): B <= 64, 1 <= num_classes <= 1024, at most
 * 256 ground-truth pairs an image, at most 2^24 pairs, pairs x num_classes < 2^31, cap >= 0.  No host synchronisation, no allocation in
 * steady state, asynchronous on `stream`. */
typedef struct {
    const float *prior, *scores;
    const int32_t *pair_h, *pair_o, *objects;
    const float* boxes;
    const int32_t *pair_off, *box_off; /* HOST */
    int32_t B, num_classes;
    const int32_t* conversion;
    int32_t n_obj_classes;
    const float *gt_boxes_h, *gt_boxes_o;
    const int32_t* gt_hoi;
    const int32_t *gt_off, *gt_sizes; /* HOST */
    int32_t gt_format;
    float min_iou;
    int32_t cap;
    int32_t *det_off, *det_pair, *det_verb, *det_h, *det_o, *det_object;
    float* det_score;
    int32_t* det_interaction;
    float* det_label;
    int32_t* det_gt;
    float *det_max_iou, *gt_boxes_out;
    int32_t* status;
} hg_hoi_detections_args;
int hg_hoi_detections(hg_ctx*, const hg_hoi_detections_args* args, void* stream);

/* Crop pre-processing in front of encode_image: for every box of one image
 *   image.crop(box)                       pre_images/crop_images.py:204-219 (PIL: zeros outside the image)
 *   [expand2square(crop, background)]     utils_tip_cache_and_union_finetune.py:201-212  (pad_square != 0)
 *   Resize(n_px, BICUBIC), CenterCrop(n_px), ToTensor, Normalize      clipnet/clip.py:75-82
 * with Pillow's 8-bit resampling arithmetic (bit-exact uint8).  img: uint8 [H,W,3] RGB on the device;
 * boxes_host: int32 [n][4] = (x0, y0, x1, y1) in HOST memory (PIL convention, may leave the image);
 * background: 0x00BBGGRR; out: fp32 [n,3,n_px,n_px] (device); out_u8: optional uint8 [n,n_px,n_px,3] (device),
 * the resized crops before normalisation.
 * `pad_square` is a set of flags: HG_PRE_PAD_SQUARE (expand2square first), HG_PRE_STRETCH (the detector's CLIP view,
 * IResize([n_px, n_px]): both sides are resized to n_px, no centre crop; detr/datasets/transforms_clip.py:139-171,
 * :279-288), HG_PRE_IMAGENET_NORM (Normalize with the ImageNet constants of utils_tip_cache_and_union_finetune.py:86-89
 * instead of CLIP's). */
#define HG_PRE_PAD_SQUARE 1
#define HG_PRE_STRETCH 2
#define HG_PRE_IMAGENET_NORM 4
int hg_preprocess_crops(hg_ctx*, const uint8_t* img, int H, int W, const int32_t* boxes_host, int n, int n_px,
                        int pad_square, uint32_t background, float* out, uint8_t* out_u8, void* stream);
/* Crop pre-processing for the crops of a batch of images in one call: crop i of image crop_image[i] receives exactly the bytes and
 * fp32 bits hg_preprocess_crops gives for that box on that image with the same flags - image.crop / expand2square / _transform(n_px)
 * (pre_images/crop_images.py:204-219, utils_tip_cache_and_union_finetune.py:201-212, clipnet/clip.py:75-82) or, with HG_PRE_STRETCH |
 * HG_PRE_IMAGENET_NORM and the whole-image box, the detector's CLIP view of every image of a batch
 * (utils_tip_cache_and_union_finetune.py:105-114).  The boxes are in DEVICE memory and the host never reads them: no host
 * synchronisation, no device-to-host copy, no allocation in steady state; the workspace is n * (24 + 2 * n_px * 67) words, sized
 * from n and n_px alone.  Asynchronous on `stream`.
 * Limits (HG_ERR_INVALID with a message): 1 <= B <= 64, 0 <= n <= 4096, 1 <= n_px <= 518.  Checked per crop on the device, reported in
 * status[i] (0: done) while every other crop of the call is unaffected:
 *   bit 0  empty box (x1 <= x0 or y1 <= y0)
 *   bit 1  more than 65 taps on either axis (a downscale above 16), or a box coordinate outside +-2^20
 *   bit 2  crop_image[i] outside [0, B)
 * A crop with a non-zero status has NaN in all its fp32 planes and 0 in its uint8 output. */
typedef struct {
    const uint8_t* const* images;      /* HOST [B]: device pointers, uint8 [H_b, W_b, 3] RGB */
    const int32_t *heights, *widths;   /* HOST [B] */
    int32_t B;
    const int32_t* boxes;              /* DEVICE int32 [n][4] = (x0, y0, x1, y1), PIL convention, may leave the image */
    const int32_t* crop_image;         /* DEVICE int32 [n]: the image of crop i */
    int32_t n, n_px, flags;            /* flags: HG_PRE_PAD_SQUARE | HG_PRE_STRETCH | HG_PRE_IMAGENET_NORM, per call */
    uint32_t background;               /* 0x00BBGGRR */
    float* out;                        /* DEVICE fp32 [n, 3, n_px, n_px] */
    uint8_t* out_u8;                   /* DEVICE, nullable: uint8 [n, n_px, n_px, 3] */
    int32_t* status;                   /* DEVICE int32 [n] */
} hg_preprocess_batch_args;
int hg_preprocess_batch(hg_ctx*, const hg_preprocess_batch_args* args, void* stream);
/* The detector's two views of a batch from raw images: what DataFactory.__getitem__, its collate and UPT.forward make of every image on
 * the host (utils_tip_cache_and_union_finetune.py:109-114, :193-196; upt...:1593, :1613), in one call on the device:
 *   RandomResize([size], max_size)      detr/datasets/transforms_clip.py:139-170: a Pillow BICUBIC resize of the whole image
 *   IResize([clip_px, clip_px])         of THAT RESIZED image (transforms_clip.py:279-288)
 *   ToTensor + Normalize (ImageNet)     utils_tip_cache_and_union_finetune.py:86-89, on both
 *   nested_tensor_from_tensor_list      detr/util/misc.py:307-329: zero padding to the batch maxima, mask 1 in the padding
 *
 * hg_detector_view_shapes is pure host code: no context, no device.  It restates get_size_with_aspect_ratio (transforms_clip.py:142-161)
 * in doubles for B images of heights[b] x widths[b]; max_size = 0 means None.  With mn = (double)min(w, h), mx = (double)max(w, h): if
 * mx / mn * size > max_size then size = (int)nearbyint((double)max_size * mn / mx) - Python's round, half to even: a 5 x 132 image at
 * size 40, max_size 66 gets 2, not 3.  If the short side equals size the output is (h, w); else if w < h, ow = size and
 * oh = (int)((double)((long long)size * h) / (double)w); otherwise the mirror.  out_sizes [B][2] = (oh, ow) (nullable); *hmax, *wmax the
 * maxima; u8_off [B + 1] (nullable): the byte offset of every resized image in one buffer, each a multiple of 256, and the total.
 * Returns HG_OK, or HG_ERR_INVALID at the first image it refuses, with that image's index in *hmax (-1: B < 1, size outside 1 .. 2048
 * or max_size outside 0 .. 2048) and the reason in *wmax: 1 an output side of 0 (Pillow raises there), 2 an output side above 2048,
 * 3 more than 65 taps on an axis (a downscale above 16), 4 a height or width below 1.
 *
 * hg_detector_views writes, for image b with (oh, ow) and u8_off as above,
 *   resized_u8 + u8_off[b]  uint8 [oh, ow, 3]: Pillow's 8-bit ImagingResample of the whole image to (ow, oh), bit for bit: horizontal
 *                           pass first, uint8 rounding after each pass, 22-bit weights (precompute_coeffs) evaluated on the device in IEEE
 *                           double with one rounding per operation
 *   detr[b, c, y, x]        ((float)u / 255.0f - mean_c) / std_c of that byte inside (oh, ow), 0 outside
 *   mask[b, y, x]           0 inside (oh, ow), 1 outside
 *   clip[b]                 what hg_preprocess_batch gives for the whole-image box of the resized image with HG_PRE_STRETCH |
 *                           HG_PRE_IMAGENET_NORM at n_px = clip_px (its kernels run inside this call)
 * Every byte of detr and mask is written: nothing outside detr, mask, clip and resized_u8 [0, u8_off[B]) is touched.  hmax, wmax: the
 * padded extent; 0, 0 means the maxima of this call's images, anything else must be at least those and at most 2048 (a call that writes
 * a slice of a larger batch).  No host synchronisation, no device-to-host copy, no allocation in steady state (grow-only
 * workspace: tables of (ow * (2 + taps_h) + oh * (2 + taps_v)) words an image, and the resized images where resized_u8 is NULL).
 * Asynchronous on `stream`.  Everything is validated on the host before anything is launched: HG_ERR_INVALID, with the image named in
 * hg_last_error, for what hg_detector_view_shapes refuses, B outside 1 .. 64, clip_px outside 0 .. 518, a null image, or a resized
 * image that clip_px is a downscale above 16 of. */
int hg_detector_view_shapes(const int32_t* heights, const int32_t* widths, int B, int size, int max_size, int32_t* out_sizes,
                            int32_t* hmax, int32_t* wmax, int64_t* u8_off);
typedef struct {
    const uint8_t* const* images;      /* HOST [B]: device pointers, uint8 [H_b, W_b, 3] RGB */
    const int32_t *heights, *widths;   /* HOST [B] */
    int32_t B;                         /* <= 64 */
    int32_t size, max_size;            /* RandomResize([size], max_size); max_size 0: None */
    int32_t clip_px;                   /* 0: no CLIP view, else <= 518 */
    int32_t hmax, wmax;                /* 0, 0: this call's maxima */
    uint8_t* resized_u8;               /* DEVICE, nullable (then in the workspace): image b at u8_off[b] as uint8 [oh_b, ow_b, 3] */
    float* detr;                       /* DEVICE fp32 [B, 3, hmax, wmax] */
    uint8_t* mask;                     /* DEVICE uint8 [B, hmax, wmax], 1 = padding */
    float* clip;                       /* DEVICE fp32 [B, 3, clip_px, clip_px]; unused with clip_px 0 */
} hg_detector_views_args;
int hg_detector_views(hg_ctx*, const hg_detector_views_args* args, void* stream);

/* ---- DETR transformer encoder (detr/models/transformer.py:62-83 TransformerEncoder over :127-162 TransformerEncoderLayer.forward_post;
 * called from the detector at upt_tip_cache_model_free_finetune_distill3.py:1594-1605 through detr.py's transformer(...)) ---------------
 * Six post-norm layers in the detector: q = k = src + pos, v = src, nn.MultiheadAttention with key_padding_mask (head dim 32), residual,
 * norm1, linear1 -> ReLU -> linear2, residual, norm2.  Dropout is the identity (inference).
 *
 * hg_load_detr_encoder: per-layer device pointers with a dtype flag (state-dict keys layers.N.self_attn.in_proj_weight / in_proj_bias,
 * self_attn.out_proj.weight / bias, linear1, linear2, norm1, norm2); the fp16 copies of the matrices are made here.  Accepted:
 * 1 .. 12 layers, d_model = 32 * heads and a multiple of 128, d_ff a multiple of 128.  normalize_before != 0 (the pre-norm layer,
 * transformer.py:164-176) and any activation but ReLU (activation != 0) are refused with a message: HG_ERR_INVALID. */
typedef struct {
    hg_tensor in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight, linear2_bias,
        norm1_weight, norm1_bias, norm2_weight, norm2_bias;
} hg_detr_layer_weights;
typedef struct {
    int32_t d_model, heads, d_ff, n_layers;
    int32_t normalize_before;              /* must be 0 */
    int32_t activation;                    /* 0 = relu; anything else is refused */
    const hg_detr_layer_weights* layers;   /* HOST array [n_layers] */
} hg_detr_encoder_weights;
int hg_load_detr_encoder(hg_ctx*, const hg_detr_encoder_weights*);
/* hg_detr_encoder (transformer.py:70-83 with mask = None and norm = None): src, pos (nullable: no positional embedding), out are DEVICE
 * fp32 with element strides (batch, token, channel) - the reference's [S, B, C] layout is (C, B * C, 1), a batch-first [B, S, C] one
 * (S * C, C, 1); the channel stride must be 1.  mask DEVICE uint8 [B, S], 1 = padded token (src_key_padding_mask), nullable.  Padded
 * tokens are still queries and their rows are computed; an image without a visible token gets NaN rows, as nn.MultiheadAttention
 * gives, and no other image is touched by them.  trace (nullable) DEVICE fp32 [n_layers, B * S, d_model]: the stream after every
 * layer, batch-major.  src, pos, out and trace need no alignment beyond a float's.  Asynchronous on `stream`, no host wait; the workspace is grow-only: a steady-state call neither allocates nor
 * synchronises.  HG_ERR_NOT_LOADED before a load; HG_ERR_INVALID with a message and nothing launched for B < 1, S < 1, S > 1792
 * (hoigen_amd/csrc/hg_kernels.h: DETR_ATTN_MAX_L), B * S > 2^20, a channel stride other than 1 or a null src / out. */
typedef struct {
    const float* src;
    const float* pos;
    const uint8_t* mask;
    float* out;
    float* trace;
    int32_t B, S;
    int64_t src_stride[3], pos_stride[3], out_stride[3];      /* elements: batch, token, channel */
} hg_detr_encoder_args;
int hg_detr_encoder(hg_ctx*, const hg_detr_encoder_args* args, void* stream);

/* ---- DETR transformer decoder (detr/models/transformer.py:86-124 TransformerDecoder over :212-233 TransformerDecoderLayer.forward_post;
 * the second half of the detector's transformer(...) call, transformer.py:56-58) ----------------------------------------------------------
 * Per layer: q = k = tgt + query_pos, v = tgt, self-attention, residual, norm1; cross-attention with q = tgt + query_pos, k = memory +
 * pos, v = memory under memory_key_padding_mask, residual, norm2; linear1 -> ReLU -> linear2, residual, norm3.  The decoder's final
 * norm is applied to what leaves (every layer with return_intermediate, else the last), never to the stream.
 *
 * hg_load_detr_decoder: a slot of its own (a context may hold an encoder, a decoder or both).  A layer is the encoder layer's twelve
 * tensors, multihead_attn's four and norm3; refused (HG_ERR_INVALID with a message) as by hg_load_detr_encoder, and where the final
 * norm is missing.  The K rows of every layer's multihead_attn.in_proj_weight are kept as ONE fp16 [n_layers * d_model, d_model] matrix
 * and the V rows likewise: memory is the same for every layer, so a call computes all cross-attention keys and values in two GEMMs. */
typedef struct {
    hg_tensor in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, linear1_weight, linear1_bias, linear2_weight, linear2_bias,
        norm1_weight, norm1_bias, norm2_weight, norm2_bias;       /* self_attn.*, linear1, linear2, norm1, norm2 */
    hg_tensor cross_in_proj_weight, cross_in_proj_bias, cross_out_proj_weight, cross_out_proj_bias;      /* multihead_attn.* */
    hg_tensor norm3_weight, norm3_bias;
} hg_detr_dec_layer_weights;
typedef struct {
    int32_t d_model, heads, d_ff, n_layers;
    int32_t normalize_before;              /* must be 0 */
    int32_t activation;                    /* 0 = relu; anything else is refused */
    hg_tensor norm_weight, norm_bias;      /* the decoder's final norm: required */
    const hg_detr_dec_layer_weights* layers;   /* HOST array [n_layers] */
} hg_detr_decoder_weights;
int hg_load_detr_decoder(hg_ctx*, const hg_detr_decoder_weights*);
/* hg_detr_decoder: DEVICE fp32 tensors with element strides.  tgt [B, Q, C] (batch, query, channel), nullable = zeros (what the detector
 * passes; nothing is read then); query_pos likewise, required, a batch stride of 0 broadcasts a [Q, C] embedding; memory and pos
 * (nullable) [B, S, C] (batch, token, channel) as in hg_detr_encoder_args; memory_mask uint8 [B, S], 1 = padded token, nullable;
 * out (layer, batch, query, channel): layers 0 .. n_layers - 1 with return_intermediate, else the last layer at layer index 0 and
 * nothing else.  trace (nullable) fp32 [n_layers, B * Q, d_model]: the stream after every layer (after norm3), batch-major.  An image
 * whose memory is all padding gets NaN in its own queries, as nn.MultiheadAttention gives, and no other image is touched.
 * Asynchronous on `stream`, no host wait; the workspace is grow-only.  HG_ERR_NOT_LOADED before a load; HG_ERR_INVALID with a message
 * and nothing launched for B, S or Q below 1, S or Q above 1792, B * max(S, Q) > 2^20, a channel stride other than 1, a null memory,
 * query_pos or out, and for option detr_ffn = 2 on a shape the split kernel does not cover. */
typedef struct {
    const float* tgt;
    const float* query_pos;
    const float* memory;
    const float* pos;
    const uint8_t* memory_mask;
    float* out;
    float* trace;
    int32_t B, S, Q, return_intermediate;
    int64_t tgt_stride[3], query_pos_stride[3];            /* elements: batch, query, channel */
    int64_t memory_stride[3], pos_stride[3];               /* elements: batch, token, channel */
    int64_t out_stride[4];                                 /* elements: layer, batch, query, channel */
} hg_detr_decoder_args;
int hg_detr_decoder(hg_ctx*, const hg_detr_decoder_args* args, void* stream);

/* ---- DETR heads and PostProcess (upt_tip_cache_model_free_finetune_distill3.py:1598-1605: class_embed(hs), bbox_embed(hs).sigmoid(),
 * the V-COCO row selection and the postprocessor; detr/models/detr.py:37-38 the two heads, :293-305 MLP, :269-282 PostProcess.forward,
 * detr/util/box_ops.py:9-13 box_cxcywh_to_xyxy) in ONE launch (hoigen_amd/csrc/hg_detr_heads.hip) -------------------------------------
 *
 * hg_load_detr_heads (detr.py:37-38; state-dict keys weight / bias of class_embed and layers.{0,1,2}.weight / bias of bbox_embed, an
 * MLP(d_model, d_model, 4, 3)): a slot of its own beside the encoder's and the decoder's.  class_rows (HOST, nullable) is the V-COCO
 * path, outputs_class[..., reserve_indices] at upt...:1600-1602: those rows of class_weight and class_bias are gathered here, so the
 * number of logits C1 becomes n_class_rows (else n_logits); the LAST of them is the no-object column.  The fp16 copies of the matrices
 * are made here.  Synchronous.  HG_ERR_INVALID with a message for d_model outside {128, 256}, C1 outside 2 .. 256, a class_rows index
 * outside [0, n_logits) (the slot keeps what it held), and for a missing tensor or a dtype other than fp32 / fp16 (the slot is then empty). */
typedef struct {
    hg_tensor class_weight, class_bias;    /* [n_logits, d_model], [n_logits] */
    hg_tensor l0_w, l0_b, l1_w, l1_b;      /* [d_model, d_model], [d_model] each */
    hg_tensor l2_w, l2_b;                  /* [4, d_model], [4] */
    int32_t d_model, n_logits;
    const int32_t* class_rows;             /* HOST [n_class_rows], nullable */
    int32_t n_class_rows;
} hg_detr_heads_weights;
int hg_load_detr_heads(hg_ctx*, const hg_detr_heads_weights*);
/* hg_detr_heads (upt...:1598-1605): hs DEVICE fp32 [L, B, Q, d_model] through element strides hs_stride = (level, image, query), channel
 * stride 1 (no alignment beyond a float's).  Per row: logits = fp16(hs) Wc^T + bc, pred_box = sigmoid(MLP(fp16(hs))) with fp16 hidden
 * layers, fp32 accumulation.  PostProcess on level L - 1 (detr.py:274-282): softmax over all C1 logits, score and label = the maximum
 * over the first C1 - 1 (ties to the lower index), boxes = box_cxcywh_to_xyxy(pred_box) * (w, h, w, h) of the row's image, each
 * operation rounded on its own in fp32.  target_sizes: HOST float [B, 2] = (h, w), as hg_region_priors takes its image_sizes; it
 * travels in the launch's arguments.
 *   pred_logits [L, B, Q, C1], pred_boxes [L, B, Q, 4]   fp32, nullable; when BOTH are null only level L - 1 is computed
 *   scores [B, Q], labels int32 [B, Q], boxes [B, Q, 4] (16-byte aligned)     required
 * Asynchronous on `stream`; no host wait, no allocation, no workspace.  HG_ERR_NOT_LOADED before a load; HG_ERR_INVALID with a message
 * and nothing launched for L outside 1 .. 12, B outside 1 .. 64, Q outside 1 .. 1792, a null hs, target_sizes, scores, labels or boxes,
 * or boxes off a 16-byte boundary. */
typedef struct {
    const float* hs;
    int64_t hs_stride[3];                  /* elements: level, image, query */
    int32_t L, B, Q;
    const float* target_sizes;
    float* pred_logits;
    float* pred_boxes;
    float* scores;
    int32_t* labels;
    float* boxes;
} hg_detr_heads_args;
int hg_detr_heads(hg_ctx*, const hg_detr_heads_args* args, void* stream);

/* ---- DETR neck: what stands between the ResNet body and the transformer (upt_tip_cache_model_free_finetune_distill3.py:1594-1597:
 * the padding mask on the feature grid, detr/models/backbone.py:78; PositionEmbeddingSine.forward, detr/models/position_encoding.py:28-48;
 * input_proj, detr/models/detr.py:40 and :65; the flatten(2).permute(2, 0, 1) of detr/models/transformer.py:50-51) in one call
 * (hoigen_amd/csrc/hg_detr_neck.hip) ----------------------------------------------------------------------------------------------------
 *
 * hg_load_detr_neck (detr.py:40, position_encoding.py:17-26): a slot of its own beside the encoder's, the decoder's and the heads'.
 * weight is input_proj.weight, [d_model, cin] or the conv's [d_model, cin, 1, 1] (the same bytes), bias [d_model].  The fp16 copy of the
 * weight and the table dim_t[i] = fp32(temperature ** (2 * (i / 2) / num_pos_feats)) (position_encoding.py:37-38, computed on the
 * host in double) are made here.  Synchronous.  HG_ERR_INVALID with a message for d_model outside {128, 256}, cin no multiple of 64 or
 * above 4096, num_pos_feats != d_model / 2, a temperature <= 0 (the slot keeps what it held), a missing tensor or a dtype other than
 * fp32 / fp16. */
typedef struct {
    hg_tensor weight, bias;
    int32_t cin, d_model, num_pos_feats;
    float temperature;
    int32_t normalize;                     /* position_encoding.py:21 */
    float scale;                           /* position_encoding.py:26: 2 pi where the module was given none */
} hg_detr_neck_weights;
int hg_load_detr_neck(hg_ctx*, const hg_detr_neck_weights*);
/* hg_detr_neck (upt...:1594-1597).  x: the body's map, DEVICE fp32 [B, cin, H, W] through element strides x_stride = (image, channel,
 * token); the token stride must be 1, nothing else is assumed - no alignment beyond a float's - and x is read where it lies, never
 * copied.  image_mask: the NestedTensor's mask, DEVICE bytes [B, Hi, Wi] contiguous (uint8 or bool), non-zero = padded.
 *   src [B, H W, d_model]   fp32 through src_stride = (image, token) in elements, channel stride 1 (the [S, B, C] view works too):
 *                           fp16(x[b, :, s]) . fp16(W)^T + bias, fp32 accumulation (detr.py:65 with transformer.py:50)
 *   pos [B, H W, d_model]   fp32 likewise through pos_stride, nullable: PositionEmbeddingSine on the downsampled mask, every operation
 *                           of the argument rounded once in fp32 in the reference's order, then sinf / cosf (transformer.py:51)
 *   mask [B, H W]           uint8 contiguous, 1 = padded, nullable: F.interpolate(m[None].float(), size=(H, W)).to(bool)[0] bit for bit -
 *                           source row min((int)floorf(y * ((float)Hi / (float)H)), Hi - 1), columns likewise (backbone.py:78)
 * A null pos or mask is not computed; image_mask, Hi and Wi are read only where one of them is wanted.  Asynchronous on `stream`; no
 * host wait; the workspace (the partial sums of a split, option "detr_neck_split") is grow-only.  For a given shape and option value the
 * result is a fixed function of the inputs.  HG_ERR_NOT_LOADED before a load; HG_ERR_INVALID with a message and nothing launched for B
 * outside 1 .. 64, H W outside 1 .. 1792, Hi or Wi outside 1 .. 8192, a token stride of x other than 1, a null x or src, pos or mask
 * without image_mask, and a detr_neck_split the loaded cin does not admit. */
typedef struct {
    const float* x;
    int64_t x_stride[3];                   /* elements: image, channel, token (= 1) */
    const uint8_t* image_mask;
    int32_t Hi, Wi;
    int32_t B, H, W;
    float* src;
    int64_t src_stride[2];                 /* elements: image, token */
    float* pos;
    int64_t pos_stride[2];
    uint8_t* mask;
} hg_detr_neck_args;
int hg_detr_neck(hg_ctx*, const hg_detr_neck_args* args, void* stream);

/* ---- ResNet stages: the bottleneck blocks layer1 .. layer4 of the detector's body (detr/models/backbone.py:83-93 builds torchvision's
 * ResNet-50 with the FrozenBatchNorm2d of :19-55; inference.py:950 and main_tip_finetune.py:1057 choose it; the same network runs as
 * the DINO backbone at upt_tip_cache_model_free_finetune_distill3.py:1617) on one implicit-GEMM convolution
 * (hoigen_amd/csrc/hg_resnet_conv.hip).  The stem - conv1 7 x 7, bn1, ReLU, max-pool - stays with the caller of hg_resnet_stages;
 * hg_resnet_stem computes it and hg_resnet_body runs both (below). -----------------------------------------------------------------------
 *
 * A block is conv1 -> bn1 -> ReLU -> conv2 -> bn2 -> ReLU -> conv3 -> bn3, + identity, -> ReLU; identity = the block's input, or
 * down_bn(down_conv(input)) where has_downsample.  Convolutions read fp16 operands (the weight rounded once, the activation rounded once)
 * and accumulate in fp32 in a fixed order: taps (r, s) ascending, then input channels ascending.  A norm is not folded into the
 * weights: scale = weight / sqrt(running_var + eps) and bias = bias - running_mean * scale are made on the host in double, rounded to
 * fp32, and applied as fmaf(acc, scale, bias) (backbone.py:45-55).  Between blocks the stream is fp32, with an fp16 copy as the next
 * convolution's operand; the identity is always read as fp32.  Inside a block conv1's and conv2's outputs exist as fp16 only.
 *
 * hg_load_resnet_stages: a slot of its own beside the DETR slots.  Every pointer is DEVICE fp32, contiguous; weight is torch's
 * [cout, cin, kh, kw].  Strides are read from the convolutions, so the stride may sit on conv2 (torchvision, v1.5) or on conv1 (the
 * original placement).  Synchronous.  HG_ERR_INVALID with a message, nothing launched for: n_blocks outside 1 .. 64;
 * cin or cout no multiple of 64 or above 2048; a 3 x 3 with more than 512 input channels; a kernel other than 1 x 1 or 3 x 3; padding
 * other than (k - 1) / 2; a stride outside {1, 2} or different per axis; dilation other than 1 (the reference's --dilation is store_true and off by
 * default, detr/main.py:37; backbone.py:90); groups other than 1; a convolution with a bias; channel counts that do not chain (conv2.cin !=
 * conv1.cout ..., a block's cin != its predecessor's cout); a missing downsample where the block changes the channel count or the
 * size; a downsample whose stride is not the product of the block's strides; a null pointer.  HG_ERR_INVALID after the weights were
 * read for a weight that is not finite or rounds beyond fp16's range.  After any failure the slot keeps what it held. */
typedef struct {
    const float* weight;                   /* [cout, cin, kh, kw] */
    int32_t cout, cin, kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups, has_bias;
} hg_resnet_conv;
typedef struct {
    const float* weight;
    const float* bias;
    const float* running_mean;
    const float* running_var;              /* [channels] each */
    double eps;                            /* FrozenBatchNorm2d: 1e-5 (backbone.py:50); nn.BatchNorm2d in eval(): its own */
} hg_resnet_norm;
typedef struct {
    hg_resnet_conv conv1, conv2, conv3, down_conv;
    hg_resnet_norm bn1, bn2, bn3, down_bn;
    int32_t has_downsample;
    int32_t ends_level;                    /* 1: the last block of layer1 / 2 / 3 / 4 (informational) */
} hg_resnet_block;
typedef struct {
    const hg_resnet_block* blocks;
    int32_t n_blocks;
} hg_resnet_weights;
int hg_load_resnet_stages(hg_ctx*, const hg_resnet_weights*);
/* hg_resnet_out_shape: pure host, no context, reads the descriptors' integers only.  (C, H, W) behind blocks first .. last for an
 * H x W input of block `first`: per convolution (H + 2 pad - k) / stride + 1 in integer division.  HG_ERR_INVALID for a range outside
 * the blocks or H, W < 1. */
int hg_resnet_out_shape(const hg_resnet_weights*, int first_block, int last_block, int H, int W, int32_t* C, int32_t* Ho, int32_t* Wo);
/* hg_resnet_stages: blocks first_block .. last_block (inclusive) of the loaded stages.
 *   x      DEVICE fp32 [B, cin of first_block, H, W] through element strides x_stride = (image, channel, row); the column stride is 1.
 *          The stem's map for first_block = 0; layer3's map to run layer4 alone.  Read once, never copied as fp32 NCHW.
 *   out    fp32 [B, C, Ho, Wo] through out_stride = (image, channel) in elements, token stride 1: what hg_detr_neck reads.
 *   trace  nullable: HOST array of last_block - first_block + 1 DEVICE pointers (each nullable), block i's output as contiguous fp32
 *          [B, C_i, H_i, W_i] - for the tests.
 * Asynchronous on `stream`; no host wait.  The workspace is grow-only and owned by the context: with E = the largest B H W C of a
 * block's input or output in the range, T1 / T2 = the largest conv1 / conv2 output, it is 2 x 4 E (the fp32 stream, in and out) +
 * 2 x 2 E (its fp16 copy) + 4 E (the downsample's output) + 2 T1 + 2 T2 bytes.  The result is a fixed function of the inputs and an
 * image's result does not depend on the rest of the batch.  HG_ERR_NOT_LOADED before a load; HG_ERR_INVALID with a message and nothing
 * launched for B outside 1 .. 64, H or W outside 1 .. 1024, a block range outside the loaded blocks, a null x or out. */
typedef struct {
    const float* x;
    int64_t x_stride[3];                   /* elements: image, channel, row */
    int32_t B, H, W;
    int32_t first_block, last_block;
    float* out;
    int64_t out_stride[2];                 /* elements: image, channel */
    float* const* trace;
} hg_resnet_args;
int hg_resnet_stages(hg_ctx*, const hg_resnet_args* args, void* stream);

/* ---- ResNet stem: conv1 7 x 7 / 2 pad 3 (3 -> 64), bn1, ReLU and the 3 x 3 / 2 pad 1 max-pool in front of the stages, as ONE launch
 * (hoigen_amd/csrc/hg_resnet_stem.hip; backbone.py:83-93 under the FrozenBatchNorm2d of :19-55). -----------------------------------
 *
 * out = maxpool(relu(fmaf(conv(x, w), scale, bias))).  Arithmetic: every image value and every weight is rounded once to fp16 (RNE);
 * the 147 products of a conv pixel are accumulated in fp32 from zero on the matrix unit in one fixed order, k = (c 7 + r) 8 + s ascending
 * (c input channel, r tap row, s tap column; s = 7 and (c 7 + r) >= 21 are zero padding of K to 192 on both operands) - no split over K, no
 * atomics, so a conv pixel is a fixed function of its own window; scale and bias are made on the host in double exactly as for the
 * stages and applied as one fmaf; relu(v) = v < 0 ? 0 : v; the max is over the conv pixels of the 3 x 3 window that lie inside the
 * conv map (a position outside it takes no part) and keeps a NaN as torch's max_pool2d does; padding of the image is real zeros that
 * form no address.  The non-finite outputs are exactly those whose windows hold a non-finite input.  Sizes: Hc = (Hi - 1) / 2 + 1,
 * Hp = (Hc - 1) / 2 + 1 in integer division, the same for W.
 *
 * hg_load_resnet_stem: a slot of its own beside the stages.  Pointers as for hg_load_resnet_stages.  Synchronous.  HG_ERR_INVALID with
 * a message, nothing launched and the slot keeping what it held for: a convolution other than 7 x 7, stride (2, 2), padding (3, 3),
 * dilation 1, groups 1, no bias, 3 -> 64 channels; a pool other than kernel 3, stride 2, padding 1, dilation 1, ceil_mode 0; an eps
 * outside [0, 1]; a null pointer; and, after the weights were read, a weight that is not finite or rounds beyond fp16's range. */
typedef struct {
    hg_resnet_conv conv1;
    hg_resnet_norm bn1;
    int32_t pool_kernel, pool_stride, pool_padding, pool_dilation, pool_ceil_mode;
} hg_resnet_stem_weights;
int hg_load_resnet_stem(hg_ctx*, const hg_resnet_stem_weights*);
/* hg_resnet_stem_out_shape: pure host, no context.  The pooled size of an Hi x Wi image.  HG_ERR_INVALID for Hi or Wi < 1. */
int hg_resnet_stem_out_shape(int Hi, int Wi, int32_t* Hp, int32_t* Wp);
/* hg_resnet_stem: the stem's map of a batch of images.
 *   x      DEVICE fp32 [B, 3, Hi, Wi] through element strides x_stride = (image, channel, row); the column stride is 1.  Any Wi, any
 *          row stride, any 4-byte aligned base: read where it lies with 64-bit offsets, and nothing beyond its last element is read.
 *   out    fp32 [B, 64, Hp, Wp] through out_stride = (image, channel) in elements, token stride 1: what hg_resnet_stages takes as x.
 * Asynchronous on `stream`; no host wait.  Workspace (grow-only, the context's): 6 B Hp Wp 64 bytes, the NHWC fp32 + fp16 pair the
 * kernel writes.  HG_ERR_NOT_LOADED before a load; HG_ERR_INVALID with a message and nothing launched for B outside 1 .. 64, Hi or Wi
 * outside 1 .. 4096 (a pooled map of at most 1024 a side), a null or misaligned x, a null out. */
typedef struct {
    const float* x;
    int64_t x_stride[3];                   /* elements: image, channel, row */
    int32_t B, Hi, Wi;
    float* out;
    int64_t out_stride[2];                 /* elements: image, channel */
} hg_resnet_stem_args;
int hg_resnet_stem(hg_ctx*, const hg_resnet_stem_args* args, void* stream);
/* hg_resnet_body: the stem and blocks 0 .. last_block of the loaded stages from the images, as hg_resnet_stem followed by
 * hg_resnet_stages would compute them, bit for bit - but the stem kernel writes straight into the stages' workspace pair: there is no
 * NCHW stem map and no layout pass between the two.  x as hg_resnet_stem's; out, trace as hg_resnet_stages' (trace: last_block + 1
 * pointers).  Workspace: hg_resnet_stages' rule with the stem's B Hp Wp 64 as block 0's input.  HG_ERR_NOT_LOADED if either slot is
 * empty; HG_ERR_INVALID if the stem's cout is not block 0's cin, and for what either call refuses. */
typedef struct {
    const float* x;
    int64_t x_stride[3];
    int32_t B, Hi, Wi;
    int32_t last_block;
    float* out;
    int64_t out_stride[2];
    float* const* trace;
} hg_resnet_body_args;
int hg_resnet_body(hg_ctx*, const hg_resnet_body_args* args, void* stream);
/* hg_resnet_features: the network as the reference's DINO backbone runs it (torchvision's resnet50 with fc = Identity on the 224 x 224
 * view, upt_tip_cache_model_free_finetune_distill3.py:1617-1618): the stem, EVERY loaded block, then one launch that pools and
 * normalises the last block's fp32 NHWC stream where it lies in the workspace (hoigen_amd/csrc/hg_resnet_pool.hip) - no NCHW map is
 * written unless map_out asks for it.  x as hg_resnet_body's.  Outputs, each nullable, at least one required:
 *   pooled    fp32 [B, C] contiguous: avgpool + flatten.  Per (image, channel) one fp32 accumulator, the Ho Wo positions added in
 *             ascending order, then one IEEE division by (float)(Ho Wo).
 *   features  fp32 [B, C] contiguous: pooled / pooled.norm(dim=-1, keepdim=True) - the sum of squares in a fixed order, sqrtf, one
 *             reciprocal, one multiply per element.  An all-zero row is NaN, as the reference's 0 / 0 is.
 *   map_out   fp32 [B, C, Ho, Wo] through map_stride = (image, channel) in elements, token stride 1: hg_resnet_body's out, bit for bit.
 * A non-finite image makes its own rows non-finite and no other image's.  Workspace: hg_resnet_body's.  Asynchronous on `stream`.
 * HG_ERR_NOT_LOADED if either slot is empty; HG_ERR_INVALID with a message and nothing launched for what hg_resnet_body refuses and
 * for a call without an output. */
typedef struct {
    const float* x;
    int64_t x_stride[3];                   /* elements: image, channel, row */
    int32_t B, Hi, Wi;
    float* pooled;
    float* features;
    float* map_out;
    int64_t map_stride[2];                 /* elements: image, channel */
} hg_resnet_features_args;
int hg_resnet_features(hg_ctx*, const hg_resnet_features_args* args, void* stream);
/* vae_loss forward value (main_coop_vae.py:300-303) -> loss[1] fp32. */
int hg_vae_loss(hg_ctx*, const float* recon, const float* x, const float* mean, const float* logvar,
                int R, int D, float* loss, void* stream);

/* ---- behaviour options (no reference counterpart) ------------------------------------------
 * Per context; the environment only supplies the initial values at hg_create (variable in brackets).  Keys:
 *   "last_block_row0" [HG_LAST_BLOCK_ROW0] 1: towers without token outputs run their LAST block on the one row per sequence
 *                      that reaches the output (class / EOT token); 0: on every row, like the reference
 *   "ln_fuse"         [HG_LN_FUSE]         1: LayerNorm folded into the GEMMs (both towers, calls of at least 512 rows; the text tower's
 *                      form: "text_ln_fold"); 0: separate LayerNorm kernels everywhere
 *   "adapter_fuse"    [HG_ADAPTER_FUSE]    1: ... also around the instance adapters of variant C
 *   "adapter_fold"    [HG_ADAPTER_FOLD]    1: adapter update folded into the block's own GEMMs; 0: separate up_proj GEMM
 *   "adapter_long"    [HG_ADAPTER_LONG]    0 (default): instance adapters need a tower of at most 224 tokens per image; 1: up to 640
 *                      (ViT-L/14@336px: 577) on the decoder of hoigen_amd/csrc/hg_adapter_long.hip: a sequence in query chunks of at
 *                      most 224 tokens, its K / V streamed in key chunks when it is its own memory; at most 32 prior tokens on MFMA
 *                      (more: the fp32 one-lane-per-token kernels, adapter_num_layers = 1 only); never folded into the block's GEMMs.
 *                      Read by hg_load_vit, hg_update_adapters, hg_encode_image_prior and hg_test_adapter: back at 0, a tower loaded
 *                      under 1 is refused again at its next call.  Towers of at most 224 tokens run exactly as with 0.  Calls with
 *                      adapters on a longer tower whose weights arrive in fp32 run c_proj and the adapters' up_proj as hi + lo fp16
 *                      (a second GEMM pass each; hg_test_adapter launches the one-pass up_proj).
 *   "stream_hilo"     [HG_STREAM_HILO]     1: between the LayerNorm-folded blocks of variant A, of the text tower (and of variant C when every
 *                      block's adapter is folded into its GEMMs) the residual stream is held as
 *                      centre + hi + lo (the centred fp16 copy the GEMMs read + its remainder as bf8: read-only option
 *                      "stream_lo_bits" = 8); 0: as fp32 throughout
 *   "qkv_attn"        [HG_QKV_ATTN]        1: in the LayerNorm-folded blocks of the vision tower in_proj and attention run as ONE kernel
 *                      (hoigen_amd/csrc/hg_qkv_attn.hip: q, k, v stay in LDS; 192 < tokens <= 208, i.e. ViT-B/16); 0: two kernels with the
 *                      qkv matrix in HBM between them; 2: the one kernel wherever the shapes allow (1 also asks that the last round
 *                      of its (sequence, head pair) items is well filled: speed only).  Bit-identical results either way.
 *   "qkv_attn_text"   [HG_QKV_ATTN_TEXT]   the same for the text tower (hoigen_amd/csrc/hg_qkv_attn_text.hip: causal, tokens <= 80, a work item is a
 *                      pack of floor(160 / tokens) whole prompts x a head pair; width 512 or 768; either folded text_ln_fold form; not the
 *                      last block's EOT-row path).  0 (default): two kernels; 1: the one kernel where it measured faster: at least one
 *                      round of (pack, head pair) items on the CUs and a last round that leaves at most a fifth of the launch idle
 *                      (qkv_attn_text_pays; profiles/qkv_attn_text.txt: 600 prompts x 77 tokens yes, -3 %; 600 x 13 no); 2: wherever the shapes allow.  Bit-identical results.
 *   "qkv_attn_min_seq" [HG_QKV_ATTN_MIN_SEQ] ... from this many sequences per call on (default 32)
 *   "qkv_attn_gsz"    [HG_QKV_ATTN_GSZ]    head pairs per XCD group of that kernel (0 = all six side by side; speed only)
 *   "text_ln_fold"    [HG_TEXT_LN_FOLD]    how the text tower's LayerNorms reach its GEMMs.  1 (default): folded, with the LayerNorm weight
 *                      multiplied into the fp16 ACTIVATION copy the residual GEMM hands on, so that in_proj / c_fc run on the layer's own
 *                      fp16 weights as the reference does (600 prompts x 77 tokens: 5.35 -> 5.15 ms; against the reference's outputs 6.2e-4,
 *                      worst prompt 7.5e-4); 0: separate LayerNorm kernels (6.5e-4, worst prompt 7.9e-4); 2: the weight folded into
 *                      fp16(W * gamma) as in the vision tower - the fastest (4.8 ms) and, through that second rounding of the weights, the
 *                      least close (7.6e-4, worst prompt 9.6e-4 of the 1e-3 tolerance).  Calls of fewer than 512 rows (prompts x executed
 *                      tokens) take the separate kernels whatever the setting (as the vision tower does below 512 rows): a prompt's bits
 *                      depend on which of the two paths its call takes, never on its neighbours in the call.
 *   "qkv_attn_c"      [HG_QKV_ATTN_C]      1 (default): also in the blocks whose instance adapter is folded into in_proj (variant C on the
 *                      hi / lo stream: the same kernel summing over D + 64 columns); 0: those blocks keep the two kernels.  Bit-identical.
 *   "vae_fused"       [HG_VAE_FUSED]       1: hg_vae_forward / hg_generator run Encoder -> reparameterise -> Generator as ONE kernel
 *                      (hoigen_amd/csrc/hg_vae_fused.hip: both hidden layers and z stay on chip; dim 512, hidden widths multiples of 128
 *                      up to 4096) for the leading rows that fill whole rounds of its 128-row work items over the CUs, the GEMM path for
 *                      the rest (and for calls too small to fill 70 % of one round); 2: the one kernel for every row; 0: GEMM path only.
 *                      Same fp16 operand roundings on both paths; results differ by fp32 summation order.
 *   "mlp_pair"        [HG_MLP_PAIR]        1 (default): in the LayerNorm-folded blocks of both towers (variant A; every form of the residual stream and
 *                      of the LayerNorm weight) c_fc -> QuickGELU -> c_proj run as ONE persistent launch (hoigen_amd/csrc/hg_mlp_pair.hip: the c_fc
 *                      tiles publish per-256-row-panel ready counters, the c_proj tiles of a panel - on the same XCD by its hardware id -
 *                      wait for them; results do not depend on workgroup placement; a wait that times out makes the NEXT call return
 *                      HG_ERR_HIP; devices with 8 x 32 CUs, otherwise the two launches run; the launch's workgroups wait for each other: the library
 *                      orders such launches across the streams of one process; PROCESSES that share a GPU and both run it can hold each other up
 *                      until that bound - set 0 there); 0: two launches.  Bit-identical results in both.
 *   "mlp_pair_chunk"  [HG_MLP_PAIR_CHUNK]  1 .. 64: 256-row panels of an XCD per chunk of that launch's c_fc tile order (default 32: the XCD's whole list
 *                      column group by column group, as in the stand-alone kernel; speed only)
 *   "mlp_pair_fc_slots" [HG_MLP_PAIR_FC_SLOTS] 1 .. 64: workgroups per XCD (of 32) that run c_fc tiles in that launch (default 32); the others start with
 *                      their c_proj tiles, i.e. sleep until the first row panels are complete (speed only)
 *   "mlp_pair256"     [HG_MLP_PAIR256]     1 (default): where that launch runs on the fp32 or the hi / lo stream without the LayerNorm weight in the
 *                      activation copy (the vision tower), its c_proj tiles are 256 x 256 instead of 128 x 256 (hoigen_amd/csrc/hg_mlp_pair256.hip:
 *                      a third less global -> LDS traffic per flop, the work slots of an XCD share its tiles by work); the text tower's form and
 *                      0: 128 x 256.  Bit-identical results in both; the same ready words, error word and profiler record.
 *   "mlp_pair256_min_m" [HG_MLP_PAIR256_MIN_M] >= 256: rows from which on "mlp_pair256" applies (default 25000: measured faster from 128 crops =
 *                      25 216 rows on, slower at 96 crops and below, where a slot owns too few of the big tiles)
 *   "mlp_pair256_chunk" [HG_MLP_PAIR256_CHUNK] 1 .. 64: 256-row panels of an XCD per chunk of that kernel's c_fc tile order (default 6; speed only)
 *   "mlp_pair256_ratio" [HG_MLP_PAIR256_RATIO] 1 .. 8: c_fc tile times its dealing counts for a c_proj tile (default 4: measured 3.8 - 4.1; speed only)
 *   "mlp_pair256_ph2" [HG_MLP_PAIR256_PH2] 1 (default): wherever "mlp_pair256" applies, c_proj runs the two-phase K loop c_fc already runs (half the
 *                      barriers, no decisions inside the loop: hoigen_amd/csrc/hg_mlp_pair256p.hip); 0: the four-phase loop
 *                      (hg_mlp_pair256.hip).  Bit-identical results in both; the same launch count and profiler record.
 *   "mlp_pair256_launches" [HG_MLP_PAIR256_LAUNCHES] a counter, not a switch: hg_get_option reads how many launches of that kernel the context has
 *                      made (its profiler record is the pair launch's); setting it (>= 0) restarts the count from that value
 *   "mlp_pair_fault"  [HG_MLP_PAIR_FAULT]  test hook, default 0.  1: that launch goes out one workgroup short - a work slot nobody takes -, so that the
 *                      hand-off waits that depend on it meet their bound (~0.6 s), the results of the call are wrong and the NEXT call returns
 *                      HG_ERR_HIP (tests/test_gpu_scale.py exercises "an error, never a hang" with it, and the recovery once it is 0 again)
 *   "detr_attn_chunk" [HG_DETR_ATTN_CHUNK] keys per LDS chunk of the DETR attention kernel (hoigen_amd/csrc/hg_detr_attn.hip): 0 (default) all keys
 *                      of a (sequence, head) at once while they fit the 160 KiB (Lk <= 1 280), 512 beyond; otherwise a multiple of 32 up to
 *                      1 280 (a value that is no multiple of 32 makes the calls that use it return HG_ERR_INVALID).  Every value gives the same bits.
 *   "detr_attn_waves" [HG_DETR_ATTN_WAVES] query tiles per work item (= waves per workgroup) of that kernel: 0 (default) = 4, a 128-query slab; 1 or 2:
 *                      smaller slabs, a wider grid (one image of 950 tokens: 240 or 120 workgroups instead of 64) that stages K and V more often -
 *                      measured equal for one image and slower for a batch (profiles/detr_encoder.txt); 3 makes the calls that use it return
 *                      HG_ERR_INVALID.  Every value gives the same bits.
 *   "detr_ffn"        [HG_DETR_FFN]        the FFN of a DETR decoder layer: 0 (default) the split-over-d_ff kernel (hoigen_amd/csrc/hg_detr_ffn.hip) where the
 *                      shape allows (d_model 128 or 256) and the call has at most detr_ffn_max_m rows, the two GEMMs elsewhere; 1 always the two
 *                      GEMMs; 2 always the split kernel (a shape it does not cover: HG_ERR_INVALID).  hg_detr_encoder never uses it.
 *   "detr_ffn_max_m"  [HG_DETR_FFN_MAX_M]  rows (B * Q) up to which detr_ffn = 0 picks the split kernel (default 1000: measured faster by 25 - 31 us a layer
 *                      from 100 to 950 rows, by no more than the spread of repeated runs at 2 888: profiles/detr_decoder.txt)
 *   "detr_neck_split" [HG_DETR_NECK_SPLIT] slices of cin over which hg_detr_neck's projection is split (hoigen_amd/csrc/hg_detr_neck.hip): 0 (default) a rule
 *                      by the number of 32-token tiles (profiles/detr_neck.txt); 1 no split, one launch; n = 2 .. 64:
 *                      n slices, whose fp32 partial sums a second launch adds in ascending order.  cin must be n multiples of 64, else the
 *                      calls that use it return HG_ERR_INVALID.  For one shape and value the result is a fixed function of the inputs.
 *   "chunk_rows"      [HG_CHUNK_ROWS]      rows per VAE / mlp_net / cache-logits chunk (>= 256; default 32768; the last chunk of a
 *                      call absorbs a tail of up to an eighth of it)
 * Unknown keys and out-of-range values return HG_ERR_INVALID. */
int hg_set_option(hg_ctx*, const char* key, int value);
int hg_get_option(hg_ctx*, const char* key, int* value);

/* ---- introspection for bench.py (no reference counterpart) --------------------------------- */
int hg_workspace_bytes(hg_ctx*, uint64_t* bytes);
/* Live per-kernel timing: from hg_profile_begin until hg_profile_end every launch of kernel kind `kind` (or, with
 * HG_PROF_ALL, every GEMM and attention launch of the towers and the VAE) is bracketed by a hipEvent pair on the
 * stream it is launched on (an event record costs a few microseconds on the stream: profile a few steps, not all).
 * GEMM kinds are the epilogue classes: 0 bias->f16, 1 bias+QuickGELU->f16, 2 bias+ReLU->f16, 3 bias+residual f32,
 * 4 bias->f32, 5 patch embedding, 6 bias+ReLU->f32, 7 scale+residual, 8 LayerNorm-folded bias->f16 [QKV],
 * 9 LayerNorm-folded bias+QuickGELU->f16 [c_fc], 10 residual + fp16 copy + row statistics [out_proj, c_proj],
 * 11 adapter down_proj on the centred copy, 12 adapter up_proj (scaled residual + fp16 copy + statistics).  hg_profile_end synchronises and returns one record per
 * timed launch, in launch order. */
#define HG_PROF_OFF (-1)
#define HG_PROF_ALL (-2)
#define HG_PROF_ATTENTION 100 /* M = sequences, N = tokens per sequence, K = heads */
#define HG_PROF_QKV_ATTN 101  /* fused in_proj + attention: M = sequences, N = tokens per sequence, K = heads */
#define HG_PROF_VAE_FUSED 102 /* CoOp-VAE as one kernel: M = rows, N = passes per item (3 Encoder + Generator, 2 Encoder, 1 Generator), K = hidden width of the first pass */
#define HG_PROF_DETR_FFN 104  /* the DETR decoder's split FFN kernel: M = rows, N = d_ff, K = d_model */
#define HG_PROF_DETR_ROWS 105 /* row kernels of hg_detr_decoder (entries, post-norms, tails): M = rows, N = d_model, K = slices summed */
#define HG_PROF_DETR_NECK 106 /* hg_detr_neck's launch(es): M = rows (B * H * W), N = slices of cin, K = cin */
#define HG_PROF_RESNET_CONV 107 /* one convolution launch of hg_resnet_stages / hg_test_resnet_conv: M = output pixels (B * Ho * Wo), N = cout, K = k * k * cin */
#define HG_PROF_RESNET_STEM 108 /* the stem launch of hg_resnet_stem / hg_resnet_body / hg_test_resnet_stem: M = pooled pixels (B * Hp * Wp), N = 64, K = 147 */
#define HG_PROF_RESNET_POOL 109 /* the pool + normalise launch of hg_resnet_features / hg_test_resnet_pool: M = images, N = channels, K = positions (Ho * Wo) */
#define HG_PROF_TEXT_ATTN_BWD 110 /* attention backward of hg_text_backward_embeds: M = prompts, N = tokens per prompt, K = heads */
#define HG_PROF_TEXT_GRAD_ROWS 111 /* its row and elementwise launches (LayerNorm backward, qgelu', fp16 casts, scale, copies): M = rows, N = width, K = 0 */
#define HG_PROF_MLP_PAIR 103/* c_fc -> QuickGELU -> c_proj as one launch: M = rows, N = hidden width (4 D), K = D */
typedef struct {
    int32_t kind; /* GEMM epilogue class or HG_PROF_ATTENTION */
    int32_t M, N, K;
    float ms;
} hg_prof_rec;
int hg_profile_begin(hg_ctx*, int kind, int max_launches);
int hg_profile_end(hg_ctx*, hg_prof_rec* recs, int max_recs, int32_t* n_recs);
/* Test hook for the GEMM kernels: out[M,N] fp32 = epilogue(fp16(a[M,K]) x fp16(w[N,K])^T) (for the residual
 * epilogue `out` is read-modify-written).  epi: 0 bias->f16, 1 bias+QuickGELU->f16, 2 bias+ReLU->f16,
 * 3 bias+residual(f32), 4 bias->f32, 6 bias+ReLU->f32.  kernel: 0 auto, 1 simple 128x128, 2 persistent ring family,
 * 3 two-workgroups-per-CU (duo) kernel; a shape the chosen kernel does not take is an error. */
int hg_test_gemm(hg_ctx*, const float* a, const float* w, const float* bias, float* out, int M, int N, int K,
                 int epi, int kernel, void* stream);
/* Test hook: ONE GEMM launch with the arguments hg_test_gemm / hg_test_gemm_ln cannot set.  All pointers are device fp32; a and w
 * are rounded to fp16 inside, fp16 outputs (epi 0, 1, 2) come back as fp32.  Only columns < N of a row of `out` are written.
 *   a [M, lda] (lda >= K), w [N, K], bias [N] or NULL, out [rows, ldc] (ldc >= N); lda and ldc multiples of 8
 *   epi 0 .. 4, 6 as hg_test_gemm; with out_hi (epi 4 / 6): columns n >= n_split go to out_hi[m * ldc + n - n_split] (n_split % 16 == 0),
 *          and ldc only has to hold the wider half
 *   epi 5  patch embedding: row m = (b, t) of a, t < G, goes to out row b * L + 1 + t (+ pos[1 + t] when pos [L, N] is given);
 *          out has (M / G) * L rows, the rows b * L are not written
 *   epi 7  out += (acc + bias) * scale[n]
 *   epi 11 out = relu(acc + mu[m] * cs[n] + bias[n]); with n_split > 0 the columns >= n_split stay linear (simple kernel only)
 *   epi 10 (kernel 4 only) x [M, ldc] in `out` += acc + bias through gemm_ring2 + finalize_stats: mu [M] the copy's centre, out2 [M, ld2]
 *          and out3 [M, ld3] (0 = ldc; whole rows come back, the columns behind N as 203.25), mr_out [M][2], mu_out [M] as hg_test_gemm_ln.
 *          gamma [N] or NULL: the copy times gamma.  chain = 0: one launch on the fp32 stream (hl 0; out2 = the copy, scaled if gamma).
 *          chain = 2 .. 16: launches planned with the stream as centre + hi + lo between them (hl 1, 2 .., 3), of which the first `stop`
 *          are made: after a launch with hl 1 / 2 `out` is not written, out2 is the stream's unscaled hi half and out3 (gamma
 *          given) the scaled copy; after the last (hl 3) `out` is the fp32 stream and out2 the copy, scaled if gamma
 *   kernel 0 dispatcher, 1 simple 128x128, 2 ring family as the dispatcher enters it, 3 duo, 4 ring2 (128x256) directly
 * HG_ERR_INVALID, and nothing launched, where the chosen kernel's own eligibility test (gemm_ring_ok, gemm_ring2_ok, gemm_duo_ok, the
 * simple kernel's N % 128 and K % 64) refuses the call. */
typedef struct {
    const float* a;
    const float* w;
    const float* bias;
    float* out;
    float* out_hi;
    const float* pos;
    const float* scale;
    const float* mu;
    const float* cs;
    const float* gamma;
    float* out2;
    float* out3;
    float* mr_out;
    float* mu_out;
    int32_t M, N, K, lda, ldc, epi, kernel, G, L, n_split, ld2, ld3, chain, stop;
} hg_test_gemm_ex_args;
int hg_test_gemm_ex(hg_ctx*, const hg_test_gemm_ex_args* args, void* stream);
/* Test hook for the LayerNorm-folded / statistics-emitting epilogues the vision tower actually runs:
 *   epi 8 / 9  (ring):  out = fp16( rstd[m] * (acc - mean[m] * cs[n]) + bias[n] ) [9: QuickGELU first], mr = [M][2] (mean, rstd)
 *   epi 10     (ring2 / duo): x[M,N] (in `out`, read-modify-written) += acc + bias; out2 = fp16(x' - mu[m]);
 *              per-row partial statistics -> finalize_stats -> mr_out [M][2] = (mean - mu[m], rstd), mu_out [M] = mean
 *   epi 12     (duo, K >= 64): as 10 with the update scaled per column: x += (acc + bias) * scale[n]
 * All pointers are device fp32; a / w are rounded to fp16 inside; out2 comes back as fp32.  kernel: 0 dispatcher, 2 ring
 * family, 3 duo.  Unused pointers may be NULL. */
int hg_test_gemm_ln(hg_ctx*, const float* a, const float* w, const float* bias, float* out, int M, int N, int K, int epi,
                    int kernel, const float* cs, const float* mr, const float* mu, const float* scale, float* out2,
                    float* mr_out, float* mu_out, void* stream);
/* Test hook for the residual stream held as centre + hi + lo: `steps` (2..16) residual updates
 * x += a W^T + bias in a row through gemm_ring2 + finalize_stats, the stream between them as centre + hi + lo (hilo = 1: the
 * first update reads fp32 x, the last writes fp32 x) or as fp32 throughout (hilo = 0).  x [M,N] and mu [M] (centre of the
 * first copy in, last mean out) are read-modify-written; out2 = the last centred copy (fp32), mr_out [M][2]; both may be NULL. */
int hg_test_gemm_hilo(hg_ctx*, const float* a, const float* w, const float* bias, float* x, int M, int N, int K, int steps,
                      int hilo, float* mu, float* out2, float* mr_out, void* stream);
/* Test hook for the attention kernels (clipnet/model.py:171,181-183: the SDPA inside nn.MultiheadAttention, head_dim
 * 64): qkv [n_seq*L, 3*heads*64] fp32 on the device (rounded to fp16 inside).  q0 == NULL: full attention, out
 * [n_seq*L, heads*64].  q0 != NULL: [n_seq, heads*64] queries of ONE row per sequence (row sel[seq], device int32, or
 * row 0 when sel is NULL - the row index only matters for the causal mask), out [n_seq, heads*64].
 * 1 <= L <= 640 in both forms, either mask (L <= 224: hg_attn.hip; 225 .. 640: hg_attn_long.hip; 640 is what a compute unit's
 * 160 KiB of LDS holds of K and V); L > 640: HG_ERR_INVALID.  Under hg_profile_begin(HG_PROF_ATTENTION) the full form's kernel
 * launch is recorded. */
int hg_test_attention(hg_ctx*, const float* qkv, const float* q0, const int32_t* sel, int n_seq, int L, int heads,
                      int causal, float* out, void* stream);
/* Test hook for the DETR attention kernel alone (hoigen_amd/csrc/hg_detr_attn.hip; the SDPA with key_padding_mask inside
 * nn.MultiheadAttention at detr/models/transformer.py:155-156, head dim 32): q [n_seq*Lq, heads*32], k and v [n_seq*Lk, heads*32] fp32 on
 * the device holding fp16 values (rounded to fp16 inside), mask uint8 [n_seq, Lk] (1 = padded key, nullable), out fp32
 * [n_seq*Lq + 8, ldo] with ldo >= heads*32 a multiple of 8 (0 = heads*32): the kernel's whole output buffer with 8 canary rows behind
 * it - whatever the kernel does not write (columns >= heads*32, the canary rows) comes back as 203.25.  chunk: keys per LDS chunk (-1: the
 * context's option detr_attn_chunk).  layout 0: q | k in one [*, 2*heads*32] buffer and v in its own, as the encoder runs it (needs
 * Lq == Lk); 1: q, k, v in three buffers; 2: one [*, 3*heads*32] buffer (needs Lq == Lk).  HG_ERR_INVALID with nothing written for
 * Lq or Lk outside 1 .. 1792, a chunk that is no multiple of 32 or above 1 280, or a layout that needs Lq == Lk.  Under
 * hg_profile_begin(HG_PROF_ATTENTION) the kernel launch is recorded. */
int hg_test_detr_attention(hg_ctx*, const float* q, const float* k, const float* v, const uint8_t* mask, int n_seq, int Lq, int Lk,
                           int heads, int chunk, int layout, int ldo, float* out, void* stream);
/* Test hook for the FFN of a DETR decoder layer with its tail (hoigen_amd/csrc/hg_detr_ffn.hip and detr_dec_tail_kernel;
 * transformer.py:231-233): y = LayerNorm(x + linear2(relu(linear1(x)))) for x [M, D] fp32 on the device, w1 [F, D], b1 [F], w2 [D, F],
 * b2 [D], norm_w / norm_b [D] fp32 (matrices and fp16(x) rounded inside, as the decoder holds them).  Option detr_ffn picks the path as
 * in hg_detr_decoder (0: the default rule; 1: the two GEMMs; 2: the split kernel, HG_ERR_INVALID where it does not cover the shape).
 * y [M, D] fp32: exactly M rows are written.  partials (nullable) fp32 [F / 128, M, D]: the split kernel's partial sums before the
 * reduce (only where that kernel ran; HG_ERR_INVALID when asked for on the GEMM path).  1 <= M <= 2^20, D a multiple of 128 up to
 * 512, F a multiple of 128.  Under hg_profile_begin the split kernel (HG_PROF_DETR_FFN) or the two GEMMs, and the tail
 * (HG_PROF_DETR_ROWS), are recorded. */
int hg_test_detr_ffn(hg_ctx*, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* norm_w,
                     const float* norm_b, int M, int D, int F, float* y, float* partials, void* stream);

/* Test hook for the fused in_proj + attention kernel (hoigen_amd/csrc/hg_qkv_attn.hip; the reference ops it replaces:
 * clipnet/model.py:171,181-183).  a [n_seq*L, D] fp32 (rounded to fp16 inside: the centred copy of the stream), w [3D, D] the
 * LayerNorm-folded in_proj weight, bias / cs [3D], mr [n_seq*L, 2] = (mean - centre, rstd), D = 64 * heads; out [n_seq*L, D]
 * fp32 = the attention output.  fused bit 0 set: the one kernel (192 < L <= 208, heads even, D / 64 a multiple of 3);
 * clear: the folded GEMM followed by hg_test_attention's kernel - the two must agree bit for bit.  fused bit 1 set: a is
 * [n_seq*L, D + 64] and w [3D, D + 64], the summed length of a block whose adapter is folded into in_proj (variant C).
 * fused bit 2 set: the causal mask (not with bit 1).  With bit 0: the text tower's kernel (hg_qkv_attn_text.hip: L <= 80, heads even,
 * D / 64 >= 6 and 3 m or 3 m + 2); without: the folded GEMM (over zero rows up to 512 where the call has fewer) followed by the causal
 * attention launch run_blocks picks at that L.  Values above 5 are HG_ERR_INVALID. */
int hg_test_qkv_attn(hg_ctx*, const float* a, const float* w, const float* bias, const float* cs, const float* mr, int n_seq,
                     int L, int heads, int fused, float* out, void* stream);
/* Test hook: hg_test_qkv_attn with the arguments a tower call sets and that hook cannot (it is this one with lda = ldo = 0, pad_fill = 0,
 * qkv_out = NULL).  All pointers are device fp32.
 *   a [M, K]       dense, M = n_seq * L, K = D (+ 64 with fused bit 1); laid out inside as fp16 rows of stride lda
 *   w [3D, K], bias [3D] or NULL, cs [3D], mr [M, 2], n_seq, L, heads, fused: as hg_test_qkv_attn
 *   lda            0 = K; >= K, a multiple of 8.  A tower call has lda = D + 64 with K = D in a block whose adapter is not folded
 *   ldo            0 = D; >= D, a multiple of 8.  out [M, ldo]: WHOLE rows come back; the fp16 output buffer is filled with the pattern
 *                  0x5A5A first, so every column >= D of a row (and whatever else a kernel leaves unwritten) comes back as 203.25
 *   pad_fill       what rows M .. Mp - 1 (Mp = M rounded up to 256; 512 at least under the causal mask) and columns K .. lda - 1 of the
 *                  operand buffer hold: 0 zeros, 1 fp16 NaN.  The pad rows of mr are zero either way.  The kernels are told
 *                  a_bytes = Mp * lda * 2 readable bytes, as a tower call computes it
 *   qkv_out        NULL, or [M, 3D]: the fp16 q | k | v the folded GEMM wrote.  With fused bit 0 clear only
 * HG_ERR_INVALID, with nothing written, for lda / ldo / pad_fill out of range, qkv_out with fused bit 0 set, and whatever the
 * launchers' own eligibility tests (qkv_attn_ok, qkv_attn_text_ok, gemm_ln_ok) refuse. */
typedef struct {
    const float* a;
    const float* w;
    const float* bias;
    const float* cs;
    const float* mr;
    float* out;
    float* qkv_out;
    int32_t n_seq, L, heads, fused, lda, ldo, pad_fill;
} hg_test_qkv_attn_ex_args;
int hg_test_qkv_attn_ex(hg_ctx*, const hg_test_qkv_attn_ex_args* args, void* stream);

/* Test hooks for the whole residual stream of a tower (every row, not only the rows that reach an output): as
 * hg_encode_image / hg_encode_text_ids (same options, `out` bit for bit the same), additionally copying the stream into
 * trace [(layers+1), rows, D] fp32 on the device, rows = B * tokens (image) or T * Leff (text; Leff = trunc when
 * 0 < trunc < L, else L).  Entry 0 is the stream entering block 0 (after ln_pre / after token + positional embedding),
 * entry i the stream after block i-1 as block i reads it (centre + hi + lo summed when it is held so).  With option
 * last_block_row0 = 1 the last entry holds the B / T rows that block ran on densely, in its first rows.  HG_ERR_INVALID
 * for a vision context with adapters loaded and for calls longer than one pass (256 crops; 256 * 224 / L for L > 224) / one text pass. */
int hg_test_image_stream(hg_ctx*, const float* x_nchw, int B, float* out, float* trace, void* stream);
int hg_test_text_stream(hg_ctx*, const int32_t* ids, int T, int L, int trunc, float* out, float* trace, void* stream);

/* Test hook for the instance adapter in front of block `block` of a vision tower loaded with adapters (variant C;
 * CLIP_models_adapter_prior2.py:183-203, :456): ONE call of the routine the tower runs there, on the caller's stream x [n_seq*L, D]
 * fp32 (device; D must be the tower's width), 1 <= L <= 224 (640 with option adapter_long = 1: modes 0 and 1) whatever the tower's own length; priors [n_seq, N, 64] fp32 and mask
 * [n_seq, N] bytes (non-zero = pad) or NULL (memory = the sequence itself; mask alone may be NULL).  The workspace is prepared as a
 * tower call leaves it in front of the block.  In modes 1 and 2 that is the centred fp16 copy of x, its centre muc, mu = the row mean
 * and mr = (mean - muc, rstd): with centre == NULL as ln_pre leaves them in front of block 0 (muc = the mean, mr[.][0] = 0), with
 * centre [n_seq*L] as a preceding block's last residual GEMM does (the copy is fp16(x - centre[m]), muc = centre, mr[.][0] = mean -
 * centre: the row's previous mean in a tower).
 *   mode 0  separate path: fp32 -> fp16 copy, down_proj GEMM, decoder, up_proj with the scaled residual epilogue.  out [M, D] = y.
 *   mode 1  LayerNorm folding on, adapter not folded: out = y, copy_out [M, D] = the re-emitted fp16 copy (as fp32), mr_out [M, 2] and
 *           muc_out [M] of y.  Needs M = n_seq * L >= 512.
 *   mode 2  adapter folded into the block's GEMMs: out [M, 64] = e (fp16 values as fp32; the update is Q e), mr_out = the statistics of
 *           x + Q e, muc_out, q_out [D, 64] (may be NULL) = Q as the block's GEMMs hold it (fp16 values).  down_proj runs inside the
 *           decoder from L = 161 on.  Any number of rows: a tower folds the adapter from 512 rows on, but nothing this mode launches
 *           depends on the row count (one workgroup per sequence; down_proj on the simple GEMM or inside the decoder).  The second
 *           operand buffer of the hi / lo stream (a second store of e) is not written.
 * path (host, may be NULL): path[0] = 1 MFMA decoder / 2 the MFMA decoder of 225 .. 640 tokens / 0 the fp32 one-lane-per-token kernels
 * (N > 32), path[1] = 1 when down_proj ran inside the decoder.  HG_ERR_INVALID for what run_adapter has no path for or a tower refuses
 * at load: L > 224 (option adapter_long = 1: L > 640, and mode 2 at L > 224), D other than the tower's, a
 * width that is no multiple of 256 in modes 1 and 2, N > 32 in mode 2 or with adapter_num_layers > 1, fewer than 512 rows in mode 1,
 * a centre in mode 0. */
int hg_test_adapter(hg_ctx*, int block, int mode, const float* x, const float* centre, int n_seq, int L, int D, const float* priors,
                    const uint8_t* mask, int N, float* out, float* copy_out, float* mr_out, float* muc_out, float* q_out,
                    int32_t* path, void* stream);

/* Test hook for the row / elementwise kernels (hoigen_amd/csrc/hg_elem.hip): ONE launch_* call with the caller's device pointers, in
 * the kernels' own types (fp32, fp16, int32, bytes - nothing is converted on the way), on the caller's stream.  No workspace of the
 * context is used, no option read, no tower touched.  HG_ERR_INVALID, with the HIP error in hg_last_error, where the launcher refuses
 * the call (nothing was launched then); HG_ERR_HIP for any other HIP error.  Unused pointers are NULL, unused ints 0.
 *   op                     p[0 ..]                                                          i[0 ..]                        n
 *   0  layernorm_f16       x, w, b, out (fp16), gather (int32)                              M, D, rows_per_seq, in_row_mul
 *   1  layernorm_f32       x, w, b, out, pos, cls                                           M, D, L
 *   2  layernorm_rowstats  x (in place), w, b, x16 (fp16), mr, mu, muc, pos, cls            M, D, L, ld16
 *   3  rowstats_cast       x, x16 (fp16), mr, mu, muc, gamma                                M, D
 *   4  finalize_stats      stats, mr, mu, muc, range_flag (int32)                           M, nt, gw, centred
 *   5  fold_ln             w16 (fp16), gamma, beta, bias, wf16 (fp16), cs, bf, csg          N, K
 *   6  copy_rows           x, out, gather (int32)                                           B, row_stride, D
 *   7  copy_rows_hilo      hi (fp16), lo (bytes), muc, out                                  B, row_stride, D
 *   8  copy_cols           x, out                                                           ld, R, N
 *   9  im2col              x, out (fp16)                                                    B, R, p
 *   10 embed_tokens        ids (int32), table, pos, x                                       ld_ids, T, L, D, vocab
 *   11 add_pos             prompts, pos, x                                                  Lfull, R, L, D
 *   12 gather_rows         ids (int32), table, out                                          n, D, vocab
 *   13 eot_argmax          ids (int32), eot (int32), max_eot (int32)                        T, L
 *   14 clamp_eot           in (int32), out (int32), flag (int32), flag_dev (int32)          n, Leff
 *   15 poison_if_flag      out, flag (int32)                                                                               elements
 *   16 f32_to_f16          in, out (fp16)                                                                                  elements
 *   17 f16_to_f32          in (fp16), out                                                                                  elements
 *   18 f16_remainder       in, out (fp16)                                                                                  elements
 *   19 transpose_to_f16    in (fp32 or fp16), out (fp16)                                    in_dtype (0 fp32, 1 fp16), rows, cols
 *   20 l2_normalize        x, out                                                           R, D
 *   21 assemble_prompts    prefix, suffix, ctx, bias, target (int32), prompts               R, C, L, n_ctx, D
 *   22 vae_loss            recon, x, mean, logvar, loss                                     R, D
 *   23 split_global_local  tok, glob, local                                                 B, L, E
 * (pointers fp32 where no type is given; the launchers' own argument names, hoigen_amd/csrc/hg_kernels.h) */
typedef struct {
    void* p[9];
    uint64_t n;
    int32_t i[6];
} hg_test_elem_args;
int hg_test_elem(hg_ctx*, int op, const hg_test_elem_args* args, void* stream);

/* Test hook for the backward of the text tower (hoigen_amd/csrc/hg_text_grad.hip, hg_text_bwd.hip; main_coop_vae.py:452-468): ONE
 * launcher with the caller's device buffers in the kernels' own types, or (op 6) one whole block backward on the loaded text tower.
 *   op                     p[0 ..]                                                          i[0 ..]                       n
 *   0  text_attn_bwd       qkv (fp16), dout (fp16), dqkv (fp16)                             n_seq, L, heads
 *   1  layernorm_bwd       x, gamma, dy, g (in place), sel (int32, nullable)                M, D, rows_per_seq
 *   2  qgelu_bwd           df (fp16), u (fp16), du (fp16)                                                                 elements
 *   3  grad_scale          go, go16 (fp16), sinv                                            R, E
 *   4  grad_unscale        g, sinv, out                                                     R, L, Leff, D
 *   5  prompts_bwd         g, partial, grad_ctx, grad_bias                                  R, L, n_ctx, D
 *   6  block backward      x_in [n_seq * L, D], g [n_seq * L, D] (in place)                 block, n_seq, L
 * (pointers fp32 where no type is given) */
int hg_test_text_grad(hg_ctx*, int op, const hg_test_elem_args* args, void* stream);

/* Test hook for the row kernels of the DETR encoder and decoder (hoigen_amd/csrc/hg_detr_rows.hip): ONE launch_detr_* call with the
 * caller's device pointers, in the kernels' own types (fp32, fp16 - nothing is converted on the way), on the caller's stream.  No
 * workspace of the context is used, no option read, no loaded model touched.  HG_ERR_INVALID, with the HIP error in hg_last_error, where
 * the launcher refuses the call (nothing was launched then); HG_ERR_HIP for any other HIP error.  Unused pointers are NULL, unused
 * strides and ints 0.  The vector kernels (1, 4) ask 16-byte alignment of every pointer but copy and out (a float's).
 *   op            p[0 ..]                                                                      s[0 ..] (elements)   i[0 ..]
 *   0  entry      src, pos, x, x16 (fp16), xp16 (fp16), posb                                   sb, ss, pb, ps       B, S, D
 *   1  postnorm   x (in place), w, b, posb, x16 (fp16), xp16 (fp16), copy                                           M, D
 *   2  exit       x, out                                                                       ob, os               B, S, D
 *   3  dec_entry  tgt, qpos, x, x16 (fp16), xp16 (fp16), qposb                                 tb, tq, qb, qq       B, Q, D
 *   4  dec_tail   x (in place), b2, partial, w3, b3, qposb, x16 (fp16), xp16 (fp16), copy,     ob, oq               n_slices, Q, M, D
 *                 wf, bf, out
 * (pointers fp32 where no type is given; the launchers' own argument names, hoigen_amd/csrc/hg_kernels.h) */
typedef struct {
    void* p[12];
    int64_t s[4];
    int32_t i[4];
} hg_test_detr_rows_args;
int hg_test_detr_rows(hg_ctx*, int op, const hg_test_detr_rows_args* args, void* stream);

/* Test hook for the bottleneck convolution (hoigen_amd/csrc/hg_resnet_conv.hip): ONE launch from fp32 device tensors, the loader's
 * packing included.  x [B, H, W, cin] NHWC and w [cout, cin, k, k] (torch's order) are rounded to fp16 inside; x's fp16 copy is an
 * allocation of exactly its size, so its first pixel is the first byte and its last pixel the last bytes of an allocation.  scale,
 * bias [cout]; identity [B Ho Wo, cout] fp32 NHWC (epi 3).  epi 1: relu(fmaf(acc, scale, bias)) -> out16; 2: fmaf -> out32; 3:
 * relu(fmaf + identity) -> out32 and out16.  out32 / out16 [B Ho Wo, cout] fp32 (the fp16 output comes back as fp32).  k in {1, 3},
 * stride in {1, 2}; tile 0 (the rule), 32 or 128 output pixels a work item.  Synchronous.  HG_ERR_INVALID where the launcher refuses. */
typedef struct {
    const float* x;
    const float* w;
    const float* scale;
    const float* bias;
    const float* identity;
    float* out32;
    float* out16;
    int32_t B, H, W, cin, cout, k, stride, epi, tile;
} hg_test_resnet_conv_args;
int hg_test_resnet_conv(hg_ctx*, const hg_test_resnet_conv_args* args, void* stream);

/* Test hook for the stem (hoigen_amd/csrc/hg_resnet_stem.hip): ONE launch from fp32 device tensors, the loader's packing included.
 * x [B, 3, Hi, Wi] contiguous NCHW, read where the caller put it (any 4-byte aligned address; the caller makes the allocation exactly
 * its size); w [64, 3, 7, 7]; scale, bias [64].  out32 / out16 [B Hp Wp, 64] fp32 NHWC (the fp16 output comes back as fp32).  There is
 * one tile shape, so no selector.  Synchronous.  HG_ERR_INVALID where the launcher refuses. */
typedef struct {
    const float* x;
    const float* w;
    const float* scale;
    const float* bias;
    float* out32;
    float* out16;
    int32_t B, Hi, Wi;
} hg_test_resnet_stem_args;
int hg_test_resnet_stem(hg_ctx*, const hg_test_resnet_stem_args* args, void* stream);

/* Test hook for the pool + normalise kernel (hoigen_amd/csrc/hg_resnet_pool.hip): ONE launch on the caller's fp32 NHWC map x_nhwc
 * [B, HW, C], read where it lies.  pooled, features fp32 [B, C], either nullable, not both.  C a multiple of 64 up to 2048, HW from 1
 * to 1024^2, B from 1 to 64.  Synchronous.  HG_ERR_INVALID where the launcher refuses, and nothing launched. */
int hg_test_resnet_pool(hg_ctx*, const float* x_nhwc, int B, int HW, int C, float* pooled, float* features, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOIGEN_AMD_H */
