// DETR transformer encoder on the HIP path (detr/models/transformer.py:62-83 over the post-norm layer :149-162): the weight loader and
// the layer runner.  Host code only; the kernels are hg_detr_attn.hip (attention), hg_detr_rows.hip (entry, post-norm, exit) and the
// project's GEMMs.  What it shares with the decoder is in hg_detr_host.h.
#include "hg_detr_host.h"

extern "C" {

// detr/models/transformer.py:127-144 (the layer's parameters) for every layer of :62-68
int hg_load_detr_encoder(hg_ctx* c, const hg_detr_encoder_weights* w) {
    if (!c) return HG_ERR_INVALID;
    int rc = detr_check_dims(c, "hg_load_detr_encoder", w);
    if (rc) return rc;
    HG_ON_DEVICE(c);
    DetrEnc& e = c->detr;
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    free_all(e.owned);
    e = DetrEnc{};
    e.D = w->d_model; e.heads = w->heads; e.F = w->d_ff;
    e.layers.resize(w->n_layers);
    for (int l = 0; l < w->n_layers && !rc; ++l) {
        DetrLayerLoader ld{c, e.owned, "hg_load_detr_encoder: ", l, 0};
        ld.common(w->layers[l], e.D, e.F, e.layers[l]);
        rc = ld.rc;
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
    int rc = detr_check_attn_options(c, "hg_detr_encoder");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const int D = e.D, F = e.F, M = B * S, NL = (int)e.layers.size();
    // workspace: A operands of the GEMMs with their row count padded to 256 (hg_kernels.h)
    const size_t Mp = rup(M, 256);
    const size_t o_x = 0, o_pos = o_x + Mp * D * 4, o_x16 = o_pos + Mp * D * 4, o_xp16 = o_x16 + Mp * D * 2, o_qk = o_xp16 + Mp * D * 2,
                 o_v = o_qk + Mp * 2 * D * 2, o_att = o_v + Mp * D * 2, o_ff = o_att + Mp * D * 2, total = o_ff + Mp * F * 2;
    rc = ensure(c, c->detr_ws, total);
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
        // src = norm1(src + out_proj(attention(q = k = src + pos, v = src)))             (transformer.py:154-158)
        if ((rc = detr_self_attention(c, "hg_detr_encoder: attention", w, x16, xp16, qk, v, att, x, a->mask, B, S, e.heads, s))) return rc;
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

}  // extern "C"
