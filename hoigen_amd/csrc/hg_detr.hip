// DETR transformer encoder on the HIP path (detr/models/transformer.py:62-83 over the post-norm layer :149-162): the weight loader and
// the layer runner.  Host code only; the kernels are hg_detr_attn.hip (attention), hg_detr_rows.hip (entry, post-norm, exit) and the
// project's GEMMs.
#include "hg_host.h"

namespace {

int detr_alloc(hg_ctx* c, std::vector<void*>& owned, size_t bytes, void** out) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(c, HG_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    owned.push_back(p);
    *out = p;
    return HG_OK;
}

int detr_f16(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, size_t n, half_t** out, int layer, const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: missing tensor layers.%d.%s", layer, name);
    void* p;
    int rc = detr_alloc(c, owned, n * 2, &p);
    if (rc) return rc;
    if (t.dtype == HG_F16) HG_HIP(hipMemcpy(p, t.ptr, n * 2, hipMemcpyDeviceToDevice));
    else if (t.dtype == HG_F32) HG_HIP(launch_f32_to_f16((const float*)t.ptr, (half_t*)p, n, 0));
    else return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: bad dtype for layers.%d.%s", layer, name);
    *out = (half_t*)p;
    return HG_OK;
}

int detr_f32(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, size_t n, float** out, int layer, const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: missing tensor layers.%d.%s", layer, name);
    void* p;
    int rc = detr_alloc(c, owned, n * 4, &p);
    if (rc) return rc;
    if (t.dtype == HG_F32) HG_HIP(hipMemcpy(p, t.ptr, n * 4, hipMemcpyDeviceToDevice));
    else if (t.dtype == HG_F16) HG_HIP(launch_f16_to_f32((const half_t*)t.ptr, (float*)p, n, 0));
    else return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: bad dtype for layers.%d.%s", layer, name);
    *out = (float*)p;
    return HG_OK;
}

// hg_load_detr_heads: `rows` rows of t [n_in, D] (all of them in order where rows is null) as fp16 [n_pad, D] (mat) or one value a row as
// fp32 [n_pad] (!mat), zero behind the rows taken.  tmp holds the converted copy of the whole tensor until the load ends.
int heads_rows(hg_ctx* c, std::vector<void*>& owned, std::vector<void*>& tmp, const hg_tensor& t, bool mat, int n_in, int D, const int32_t* rows,
               int n_rows, int n_pad, void** out, const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: missing tensor %s", name);
    if (t.dtype != HG_F16 && t.dtype != HG_F32) return fail(c, HG_ERR_INVALID, "hg_load_detr_heads: bad dtype for %s", name);
    const size_t row = mat ? (size_t)D * 2 : 4, n = (size_t)n_in * (mat ? D : 1);
    void *full, *dst;
    int rc = detr_alloc(c, tmp, n * (mat ? 2 : 4), &full);
    if (rc) return rc;
    if (mat) {
        if (t.dtype == HG_F16) HG_HIP(hipMemcpy(full, t.ptr, n * 2, hipMemcpyDeviceToDevice));
        else HG_HIP(launch_f32_to_f16((const float*)t.ptr, (half_t*)full, n, 0));
    } else {
        if (t.dtype == HG_F32) HG_HIP(hipMemcpy(full, t.ptr, n * 4, hipMemcpyDeviceToDevice));
        else HG_HIP(launch_f16_to_f32((const half_t*)t.ptr, (float*)full, n, 0));
    }
    HG_HIP(hipDeviceSynchronize());
    rc = detr_alloc(c, owned, n_pad * row, &dst);
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

// detr/models/transformer.py:127-144 (the layer's parameters) for every layer of :62-68
int hg_load_detr_encoder(hg_ctx* c, const hg_detr_encoder_weights* w) {
    if (!c) return HG_ERR_INVALID;
    if (!w || !w->layers) return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: weights are required");
    if (w->normalize_before)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: normalize_before (the pre-norm layer) is not implemented: the detector is post-norm");
    if (w->activation != 0) return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: only the ReLU activation is implemented (activation = 0)");
    const int D = w->d_model, H = w->heads, F = w->d_ff, NL = w->n_layers;
    if (NL < 1 || NL > 12) return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: 1 .. 12 layers (got %d)", NL);
    if (H < 1 || D != 32 * H || D % 128) return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: d_model must be 32 * heads and a multiple of 128 (got d_model %d, heads %d)", D, H);
    if (F < 128 || F % 128) return fail(c, HG_ERR_INVALID, "hg_load_detr_encoder: d_ff must be a multiple of 128 (got %d)", F);
    HG_ON_DEVICE(c);
    DetrEnc& e = c->detr;
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    free_all(e.owned);
    e = DetrEnc{};
    e.D = D; e.heads = H; e.F = F;
    e.layers.resize(NL);
    int rc = 0;
    for (int l = 0; l < NL; ++l) {
        const hg_detr_layer_weights& s = w->layers[l];
        DetrLayerW& d = e.layers[l];
        keep_first(rc, detr_f16(c, e.owned, s.in_proj_weight, (size_t)3 * D * D, &d.w_in, l, "self_attn.in_proj_weight"));
        keep_first(rc, detr_f32(c, e.owned, s.in_proj_bias, (size_t)3 * D, &d.b_in, l, "self_attn.in_proj_bias"));
        keep_first(rc, detr_f16(c, e.owned, s.out_proj_weight, (size_t)D * D, &d.w_out, l, "self_attn.out_proj.weight"));
        keep_first(rc, detr_f32(c, e.owned, s.out_proj_bias, D, &d.b_out, l, "self_attn.out_proj.bias"));
        keep_first(rc, detr_f16(c, e.owned, s.linear1_weight, (size_t)F * D, &d.w1, l, "linear1.weight"));
        keep_first(rc, detr_f32(c, e.owned, s.linear1_bias, F, &d.b1, l, "linear1.bias"));
        keep_first(rc, detr_f16(c, e.owned, s.linear2_weight, (size_t)D * F, &d.w2, l, "linear2.weight"));
        keep_first(rc, detr_f32(c, e.owned, s.linear2_bias, D, &d.b2, l, "linear2.bias"));
        keep_first(rc, detr_f32(c, e.owned, s.norm1_weight, D, &d.n1_w, l, "norm1.weight"));
        keep_first(rc, detr_f32(c, e.owned, s.norm1_bias, D, &d.n1_b, l, "norm1.bias"));
        keep_first(rc, detr_f32(c, e.owned, s.norm2_weight, D, &d.n2_w, l, "norm2.weight"));
        keep_first(rc, detr_f32(c, e.owned, s.norm2_bias, D, &d.n2_b, l, "norm2.bias"));
        if (rc) break;
    }
    if (rc) {
        free_all(e.owned);
        e = DetrEnc{};
        return rc;
    }
    HG_HIP(hipDeviceSynchronize());
    e.loaded = true;
    return HG_OK;
}

// detr/models/transformer.py:70-83 (mask = None, norm = None): every layer is :149-162
int hg_detr_encoder(hg_ctx* c, const hg_detr_encoder_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    DetrEnc& e = c->detr;
    if (!e.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_detr_encoder: no encoder loaded (hg_load_detr_encoder)");
    if (!a || !a->src || !a->out) return fail(c, HG_ERR_INVALID, "hg_detr_encoder: src and out are required");
    const int B = a->B, S = a->S;
    if (B < 1 || S < 1) return fail(c, HG_ERR_INVALID, "hg_detr_encoder: B and S must be at least 1 (got B %d, S %d)", B, S);
    if (S > DETR_ATTN_MAX_L) return fail(c, HG_ERR_INVALID, "hg_detr_encoder: S = %d tokens, at most %d", S, DETR_ATTN_MAX_L);
    if ((long long)B * S > (1LL << 20)) return fail(c, HG_ERR_INVALID, "hg_detr_encoder: B * S = %lld rows, at most 2^20", (long long)B * S);
    if (a->src_stride[2] != 1 || a->out_stride[2] != 1 || (a->pos && a->pos_stride[2] != 1))
        return fail(c, HG_ERR_INVALID, "hg_detr_encoder: the channel stride of src, pos and out must be 1");
    const int chunk = c->opt_detr_attn_chunk;
    if (chunk % 32) return fail(c, HG_ERR_INVALID, "hg_detr_encoder: option detr_attn_chunk = %d is no multiple of 32", chunk);
    if (c->opt_detr_attn_waves == 3) return fail(c, HG_ERR_INVALID, "hg_detr_encoder: option detr_attn_waves must be 0, 1, 2 or 4");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const int D = e.D, F = e.F, M = B * S, NL = (int)e.layers.size();
    // workspace: A operands of the GEMMs with their row count padded to 256 (hg_kernels.h)
    const size_t Mp = rup(M, 256);
    const size_t o_x = 0, o_pos = o_x + Mp * D * 4, o_x16 = o_pos + Mp * D * 4, o_xp16 = o_x16 + Mp * D * 2, o_qk = o_xp16 + Mp * D * 2,
                 o_v = o_qk + Mp * 2 * D * 2, o_att = o_v + Mp * D * 2, o_ff = o_att + Mp * D * 2, total = o_ff + Mp * F * 2;
    int rc = ensure(c, c->detr_ws, total);
    if (rc) return rc;
    char* ws = (char*)c->detr_ws.p;
    float* x = (float*)(ws + o_x);
    float* posb = (float*)(ws + o_pos);
    half_t *x16 = (half_t*)(ws + o_x16), *xp16 = (half_t*)(ws + o_xp16), *qk = (half_t*)(ws + o_qk), *v = (half_t*)(ws + o_v),
           *att = (half_t*)(ws + o_att), *ff = (half_t*)(ws + o_ff);
    HG_HIP(launch_detr_entry(a->src, a->pos, a->src_stride[0], a->src_stride[1], a->pos ? a->pos_stride[0] : 0, a->pos ? a->pos_stride[1] : 0,
                             B, S, D, x, x16, xp16, posb, s));
    for (int l = 0; l < NL; ++l) {
        const DetrLayerW& w = e.layers[l];
        // q | k = fp16(x + pos) W[0:2D]^T + b, v = fp16(x) W[2D:3D]^T + b            (transformer.py:154-156: in_proj of self_attn)
        HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(xp16, D, w.w_in, w.b_in, qk, 2 * D, M, 2 * D, D), s));
        HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(x16, D, w.w_in + (size_t)2 * D * D, w.b_in + 2 * D, v, D, M, D, D), s));
        {
            DetrAttnArgs da{};
            da.q = qk; da.k = qk + D; da.v = v; da.ldq = da.ldk = 2 * D; da.ldv = D;
            da.mask = a->mask; da.out = att; da.ldo = D; da.n_seq = B; da.Lq = da.Lk = S; da.heads = e.heads; da.chunk = chunk;
            da.waves = c->opt_detr_attn_waves;
            ProfScope ps(c, s, HG_PROF_ATTENTION, B, S, e.heads);
            hipError_t he = launch_detr_attention(da, s);
            ps.finish();
            if (he != hipSuccess) return fail(c, HG_ERR_HIP, "hg_detr_encoder: attention launch failed: %s", hipGetErrorString(he));
        }
        // src = norm1(src + out_proj(attention))                                      (transformer.py:157-158)
        HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(att, D, w.w_out, w.b_out, x, D, M, D, D), s));
        HG_HIP(launch_detr_postnorm(x, w.n1_w, w.n1_b, nullptr, x16, nullptr, nullptr, M, D, s));
        // src = norm2(src + linear2(relu(linear1(src))))                              (transformer.py:159-161)
        HG_HIP(gemm(c, EPI_BIAS_RELU_F16, gemm_args(x16, D, w.w1, w.b1, ff, F, M, F, D), s));
        HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(ff, F, w.w2, w.b2, x, D, M, D, F), s));
        HG_HIP(launch_detr_postnorm(x, w.n2_w, w.n2_b, posb, x16, l + 1 < NL ? xp16 : nullptr,
                                    a->trace ? a->trace + (size_t)l * M * D : nullptr, M, D, s));
    }
    HG_HIP(launch_detr_exit(x, a->out, a->out_stride[0], a->out_stride[1], B, S, D, s));
    return HG_OK;
}

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
    keep_first(rc, detr_f16(c, n.owned, w->weight, (size_t)D * Cin, &n.w, 0, "input_proj.weight"));
    keep_first(rc, detr_f32(c, n.owned, w->bias, D, &n.bias, 0, "input_proj.bias"));
    void* tab = nullptr;
    keep_first(rc, detr_alloc(c, n.owned, (size_t)(D / 2) * 4, &tab));
    if (rc) {
        free_all(n.owned);
        n = DetrNeck{};
        return rc;
    }
    // dim_t[i] = fp32(temperature ** (2 * (i // 2) / num_pos_feats))      (position_encoding.py:37-38)
    std::vector<float> dim_t(D / 2);
    for (int i = 0; i < D / 2; ++i) dim_t[i] = (float)pow((double)w->temperature, 2.0 * (i / 2) / (double)(D / 2));
    HG_HIP(hipMemcpy(tab, dim_t.data(), dim_t.size() * 4, hipMemcpyHostToDevice));
    HG_HIP(hipDeviceSynchronize());
    n.dim_t = (float*)tab;
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
