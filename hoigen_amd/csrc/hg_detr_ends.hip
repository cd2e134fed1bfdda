// What stands in front of and behind the DETR transformer, host side: the loaders and entry points of the neck (hg_load_detr_neck,
// hg_detr_neck: upt_tip_cache_model_free_finetune_distill3.py:1594-1597) and of the heads (hg_load_detr_heads, hg_detr_heads: :1598-1605).
// Host code only; the kernels are hg_detr_neck.hip and hg_detr_heads.hip.
#include "hg_host.h"

namespace {

// hg_load_detr_heads: `rows` rows of t [n_in, D] (all of them in order where rows is null) as fp16 [n_pad, D] (mat) or one value a row as
// fp32 [n_pad] (!mat), zero behind the rows taken.  tmp holds the converted copy of the whole tensor until the load ends.
int heads_rows(hg_ctx* c, std::vector<void*>& owned, std::vector<void*>& tmp, const hg_tensor& t, bool mat, int n_in, int D, const int32_t* rows,
               int n_rows, int n_pad, void** out, const char* name) {
    const size_t row = mat ? (size_t)D * 2 : 4, n = (size_t)n_in * (mat ? D : 1);
    half_t* full16 = nullptr;
    float* full32 = nullptr;
    int rc = mat ? as_f16(c, tmp, t, n, &full16, name, "hg_load_detr_heads: ") : as_f32(c, tmp, t, n, &full32, name, "hg_load_detr_heads: ");
    if (rc) return rc;
    const void* full = mat ? (const void*)full16 : full32;
    HG_HIP(hipDeviceSynchronize());
    void* dst;
    rc = dev_alloc(c, owned, n_pad * row, &dst);
    if (rc) return rc;
    HG_HIP(hipMemset(dst, 0, n_pad * row));
    if (!rows) HG_HIP(hipMemcpy(dst, full, n_rows * row, hipMemcpyDeviceToDevice));
    else
        for (int i = 0; i < n_rows; ++i) HG_HIP(hipMemcpy((char*)dst + i * row, (const char*)full + rows[i] * row, row, hipMemcpyDeviceToDevice));
    *out = dst;
    return HG_OK;
}

}  // namespace

extern "C" {

// detr/models/detr.py:37-38 (class_embed, bbox_embed = MLP(hidden_dim, hidden_dim, 4, 3)); class_rows: the reserve_indices of
// upt_tip_cache_model_free_finetune_distill3.py:1600-1602
int hg_load_detr_heads(hg_ctx* c, const hg_detr_heads_weights* w) {
    if (!c) return HG_ERR_INVALID;
    if (!w) return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: weights are required");
    const int D = w->d_model, NL = w->n_logits;
    if (D != 128 && D != 256) return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: d_model must be 128 or 256 (got %d)", D);
    if (NL < 1 || NL > (1 << 16)) return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: n_logits = %d, 1 .. 65536", NL);
    if (w->class_rows ? w->n_class_rows < 0 : w->n_class_rows != 0)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: n_class_rows = %d without class_rows, or negative", w->n_class_rows);
    const int C1 = w->class_rows ? w->n_class_rows : NL;
    if (C1 < 2 || C1 > DETR_HEADS_MAX_C)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: %d logits (classes + 1), 2 .. %d", C1, DETR_HEADS_MAX_C);
    for (int i = 0; w->class_rows && i < C1; ++i)
        if (w->class_rows[i] < 0 || w->class_rows[i] >= NL)
            return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: class_rows[%d] = %d is outside [0, %d)", i, w->class_rows[i], NL);
    HG_ON_DEVICE(c);
    DetrHeads& h = c->detr_heads;
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    free_all(h.owned);
    h = DetrHeads{};
    h.D = D; h.C1 = C1; h.C1p = (int)rup(C1, 16);
    std::vector<void*> tmp;
    int rc = 0;
    keep_first(rc, heads_rows(c, h.owned, tmp, w->class_weight, true, NL, D, w->class_rows, C1, h.C1p, (void**)&h.wc, "class_embed.weight"));
    keep_first(rc, heads_rows(c, h.owned, tmp, w->class_bias, false, NL, D, w->class_rows, C1, h.C1p, (void**)&h.bc, "class_embed.bias"));
    keep_first(rc, heads_rows(c, h.owned, tmp, w->l0_w, true, D, D, nullptr, D, D, (void**)&h.w0, "bbox_embed.layers.0.weight"));
    keep_first(rc, heads_rows(c, h.owned, tmp, w->l0_b, false, D, D, nullptr, D, D, (void**)&h.b0, "bbox_embed.layers.0.bias"));
    keep_first(rc, heads_rows(c, h.owned, tmp, w->l1_w, true, D, D, nullptr, D, D, (void**)&h.w1, "bbox_embed.layers.1.weight"));
    keep_first(rc, heads_rows(c, h.owned, tmp, w->l1_b, false, D, D, nullptr, D, D, (void**)&h.b1, "bbox_embed.layers.1.bias"));
    keep_first(rc, heads_rows(c, h.owned, tmp, w->l2_w, true, 4, D, nullptr, 4, 16, (void**)&h.w2, "bbox_embed.layers.2.weight"));
    keep_first(rc, heads_rows(c, h.owned, tmp, w->l2_b, false, 4, D, nullptr, 4, 16, (void**)&h.b2, "bbox_embed.layers.2.bias"));
    (void)hipDeviceSynchronize();
    free_all(tmp);
    if (rc) {
        free_all(h.owned);
        h = DetrHeads{};
        return rc;
    }
    h.loaded = true;
    return HG_OK;
}

// upt_tip_cache_model_free_finetune_distill3.py:1598-1605 with detr/models/detr.py:274-282 behind the last line
int hg_detr_heads(hg_ctx* c, const hg_detr_heads_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    const DetrHeads& h = c->detr_heads;
    if (!h.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_detr_heads: no heads loaded (hg_load_detr_heads)");
    if (!a || !a->hs || !a->target_sizes || !a->scores || !a->labels || !a->boxes)
        return fail(c, HG_ERR_INVALID, "hg_detr_heads: hs, target_sizes, scores, labels and boxes are required");
    if (a->L < 1 || a->L > DETR_HEADS_MAX_L) return fail(c, HG_ERR_INVALID, "hg_detr_heads: L = %d levels, 1 .. %d", a->L, DETR_HEADS_MAX_L);
    if (a->B < 1 || a->B > DETR_HEADS_MAX_B) return fail(c, HG_ERR_INVALID, "hg_detr_heads: B = %d images, 1 .. %d", a->B, DETR_HEADS_MAX_B);
    if (a->Q < 1 || a->Q > DETR_HEADS_MAX_Q) return fail(c, HG_ERR_INVALID, "hg_detr_heads: Q = %d queries, 1 .. %d", a->Q, DETR_HEADS_MAX_Q);
    if ((uintptr_t)a->boxes & 15) return fail(c, HG_ERR_INVALID, "hg_detr_heads: boxes must be 16-byte aligned");
    HG_ON_DEVICE(c);
    DetrHeadsArgs k{};
    const bool all = a->pred_logits || a->pred_boxes;
    k.hs = a->hs; k.s_l = a->hs_stride[0]; k.s_b = a->hs_stride[1]; k.s_q = a->hs_stride[2];
    k.wc = h.wc; k.bc = h.bc; k.w0 = h.w0; k.b0 = h.b0; k.w1 = h.w1; k.b1 = h.b1; k.w2 = h.w2; k.b2 = h.b2;
    k.pred_logits = a->pred_logits; k.pred_boxes = a->pred_boxes; k.scores = a->scores; k.labels = a->labels; k.boxes = a->boxes;
    k.D = h.D; k.C1 = h.C1; k.C1p = h.C1p; k.l0 = all ? 0 : a->L - 1; k.L = all ? a->L : 1; k.B = a->B; k.Q = a->Q;
    k.vec4 = !((uintptr_t)a->hs & 15) && !(k.s_l & 3) && !(k.s_b & 3) && !(k.s_q & 3);
    memcpy(k.sizes, a->target_sizes, sizeof(float) * 2 * a->B);
    hipError_t he = launch_detr_heads(k, (hipStream_t)stream);
    if (he != hipSuccess) return fail(c, HG_ERR_HIP, "hg_detr_heads: launch failed: %s", hipGetErrorString(he));
    return HG_OK;
}

// detr/models/detr.py:40 (input_proj = nn.Conv2d(backbone.num_channels, hidden_dim, kernel_size=1)) and
// detr/models/position_encoding.py:17-26, :37-38 (PositionEmbeddingSine's attributes and its dim_t)
int hg_load_detr_neck(hg_ctx* c, const hg_detr_neck_weights* w) {
    if (!c) return HG_ERR_INVALID;
    if (!w) return fail(c, HG_ERR_INVALID, "hg_load_detr_neck: weights are required");
    const int D = w->d_model, Cin = w->cin;
    if (D != 128 && D != 256) return fail(c, HG_ERR_INVALID, "hg_load_detr_neck: d_model must be 128 or 256 (got %d)", D);
    if (Cin < 64 || Cin % 64 || Cin > DETR_NECK_MAX_CIN)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_neck: cin must be a multiple of 64 up to %d (got %d)", DETR_NECK_MAX_CIN, Cin);
    if (w->num_pos_feats != D / 2)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_neck: num_pos_feats = %d, and pos has d_model = %d channels: it must be d_model / 2", w->num_pos_feats, D);
    if (!(w->temperature > 0.f)) return fail(c, HG_ERR_INVALID, "hg_load_detr_neck: temperature must be positive");
    if (!w->weight.ptr || !w->bias.ptr) return fail(c, HG_ERR_INVALID, "hg_load_detr_neck: missing tensor %s", w->weight.ptr ? "bias" : "weight");
    for (const hg_tensor* t : {&w->weight, &w->bias})
        if (t->dtype != HG_F16 && t->dtype != HG_F32) return fail(c, HG_ERR_INVALID, "hg_load_detr_neck: bad dtype for %s", t == &w->bias ? "bias" : "weight");
    HG_ON_DEVICE(c);
    DetrNeck& n = c->detr_neck;
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    free_all(n.owned);
    n = DetrNeck{};
    n.D = D; n.Cin = Cin; n.normalize = w->normalize != 0; n.scale = w->scale;
    int rc = 0;
    keep_first(rc, as_f16(c, n.owned, w->weight, (size_t)D * Cin, &n.w, "weight", "hg_load_detr_neck: "));
    keep_first(rc, as_f32(c, n.owned, w->bias, D, &n.bias, "bias", "hg_load_detr_neck: "));
    keep_first(rc, dev_alloc_n(c, n.owned, D / 2, &n.dim_t));
    if (rc) {
        free_all(n.owned);
        n = DetrNeck{};
        return rc;
    }
    // dim_t[i] = fp32(temperature ** (2 * (i // 2) / num_pos_feats))      (position_encoding.py:37-38)
    std::vector<float> dim_t(D / 2);
    for (int i = 0; i < D / 2; ++i) dim_t[i] = (float)pow((double)w->temperature, 2.0 * (i / 2) / (double)(D / 2));
    HG_HIP(hipMemcpy(n.dim_t, dim_t.data(), dim_t.size() * 4, hipMemcpyHostToDevice));
    HG_HIP(hipDeviceSynchronize());
    n.loaded = true;
    return HG_OK;
}

// Slices of Cin where option detr_neck_split = 0.  A work item is a tile of 32 tokens and a slice, and it walks its slice block by block,
// so a launch of few tiles is as long as one walk of all of Cin: measured at Cin 2048 (profiles/detr_neck.txt), one slice takes 65 - 69 us
// from 30 to 182 tiles and 86 us at 264; 8 slices take 31 us at 30 tiles and 41 - 47 us at 120 and 182 (4 slices: 43 - 45 us, within
// the spread), 2 slices 73 us at 264 - the launch that adds the partial sums included; gaps of 13 to 33 us against spreads of 1 to 6.
// So: double the slices while there are fewer than 512 work items, up to 8.
static int detr_neck_default_split(int Cin, int B, int S) {
    const int tiles = B * ((S + DETR_NECK_TOKENS - 1) / DETR_NECK_TOKENS);
    int n = 1;
    while (n < 8 && tiles * n < 512 && Cin % (128 * n) == 0) n *= 2;
    return n;
}

// upt_tip_cache_model_free_finetune_distill3.py:1594-1597: backbone.py:78 (the mask), position_encoding.py:28-48, input_proj (detr.py:65),
// and transformer.py:50-51 (the flatten / permute that the batch-first outputs make unnecessary)
int hg_detr_neck(hg_ctx* c, const hg_detr_neck_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    const DetrNeck& n = c->detr_neck;
    if (!n.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_detr_neck: no neck loaded (hg_load_detr_neck)");
    if (!a || !a->x || !a->src) return fail(c, HG_ERR_INVALID, "hg_detr_neck: x and src are required");
    if ((a->pos || a->mask) && !a->image_mask) return fail(c, HG_ERR_INVALID, "hg_detr_neck: pos and mask need image_mask");
    if (a->B < 1 || a->B > DETR_NECK_MAX_B) return fail(c, HG_ERR_INVALID, "hg_detr_neck: B = %d images, 1 .. %d", a->B, DETR_NECK_MAX_B);
    if (a->H < 1 || a->W < 1 || (long long)a->H * a->W > DETR_ATTN_MAX_L)
        return fail(c, HG_ERR_INVALID, "hg_detr_neck: H x W = %d x %d tokens, 1 .. %d", a->H, a->W, DETR_ATTN_MAX_L);
    if (a->image_mask && (a->Hi < 1 || a->Wi < 1 || a->Hi > DETR_NECK_MAX_IMG || a->Wi > DETR_NECK_MAX_IMG))
        return fail(c, HG_ERR_INVALID, "hg_detr_neck: image_mask is Hi x Wi = %d x %d, 1 .. %d each", a->Hi, a->Wi, DETR_NECK_MAX_IMG);
    if (a->x_stride[2] != 1) return fail(c, HG_ERR_INVALID, "hg_detr_neck: the token stride of x must be 1 (got %lld)", (long long)a->x_stride[2]);
    const int S = a->H * a->W, opt = c->opt_detr_neck_split;
    const int nsplit = opt ? opt : detr_neck_default_split(n.Cin, a->B, S);
    if (n.Cin % (64 * nsplit))
        return fail(c, HG_ERR_INVALID, "hg_detr_neck: option detr_neck_split = %d, and cin = %d is not that many slices of a multiple of 64", nsplit, n.Cin);
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    DetrNeckArgs k{};
    if (nsplit > 1) {
        int rc = ensure(c, c->detr_neck_ws, detr_neck_partial_bytes(nsplit, a->B, S, n.D));
        if (rc) return rc;
        k.partial = (float*)c->detr_neck_ws.p;
    }
    k.x = a->x; k.x_sb = a->x_stride[0]; k.x_sc = a->x_stride[1];
    k.w = n.w; k.bias = n.bias; k.dim_t = n.dim_t; k.image_mask = a->image_mask;
    k.src = a->src; k.src_sb = a->src_stride[0]; k.src_ss = a->src_stride[1];
    k.pos = a->pos; k.pos_sb = a->pos ? a->pos_stride[0] : 0; k.pos_ss = a->pos ? a->pos_stride[1] : 0;
    k.mask = a->mask; k.scale = n.scale; k.normalize = n.normalize;
    k.Cin = n.Cin; k.D = n.D; k.B = a->B; k.H = a->H; k.W = a->W; k.Hi = a->image_mask ? a->Hi : 1; k.Wi = a->image_mask ? a->Wi : 1;
    k.nsplit = nsplit; k.kslice = n.Cin / nsplit;
    k.vec4 = !((uintptr_t)a->x & 15) && !(k.x_sb & 3) && !(k.x_sc & 3) && !(S & 3);
    k.ovec4 = !((uintptr_t)a->src & 15) && !(k.src_sb & 3) && !(k.src_ss & 3);
    ProfScope ps(c, s, HG_PROF_DETR_NECK, a->B * S, nsplit, n.Cin);
    hipError_t he = launch_detr_neck(k, s);
    ps.finish();
    if (he != hipSuccess) return fail(c, HG_ERR_HIP, "hg_detr_neck: launch failed: %s", hipGetErrorString(he));
    return HG_OK;
}

}  // extern "C"
