// DETR transformer decoder on the HIP path (detr/models/transformer.py:86-124 over the post-norm layer :212-233): the weight loader and
// the layer runner.  Host code only; the kernels are hg_detr_attn.hip (both attentions), hg_detr_ffn.hip (the FFN split over d_ff),
// hg_detr_rows.hip (entries, post-norms, the layer tail) and the project's GEMMs.  What it shares with the encoder is in hg_detr_host.h.
#include "hg_detr_host.h"

namespace {

// a row kernel of the decoder under the profiler
struct RowScope : ProfScope {
    RowScope(hg_ctx* c, hipStream_t s, int M, int D, int slices) : ProfScope(c, s, HG_PROF_DETR_ROWS, M, D, slices) {}
};

}  // namespace

extern "C" {

// detr/models/transformer.py:187-204 (the layer's parameters) for every layer of :88-93, and the decoder's norm
int hg_load_detr_decoder(hg_ctx* c, const hg_detr_decoder_weights* w) {
    if (!c) return HG_ERR_INVALID;
    int rc = detr_check_dims(c, "hg_load_detr_decoder", w);
    if (rc) return rc;
    const int D = w->d_model, F = w->d_ff, NL = w->n_layers;
    if (D > 512) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: d_model at most 512 (got %d)", D);
    if (!w->norm_weight.ptr || !w->norm_bias.ptr)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: the decoder's final norm (norm.weight, norm.bias) is required");
    HG_ON_DEVICE(c);
    DetrDec& e = c->detr_dec;
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    free_all(e.owned);
    e = DetrDec{};
    e.D = D; e.heads = w->heads; e.F = F;
    e.layers.resize(NL);
    const size_t DD = (size_t)D * D;
    const char* who = "hg_load_detr_decoder: ";
    keep_first(rc, dev_alloc_n(c, e.owned, NL * DD, &e.wk_all));
    keep_first(rc, dev_alloc_n(c, e.owned, NL * DD, &e.wv_all));
    keep_first(rc, dev_alloc_n(c, e.owned, (size_t)NL * D, &e.bk_all));
    keep_first(rc, dev_alloc_n(c, e.owned, (size_t)NL * D, &e.bv_all));
    DetrLayerLoader norm{c, e.owned, who, -1, rc};
    norm.f32(w->norm_weight, D, &e.nf_w, "norm.weight");
    norm.f32(w->norm_bias, D, &e.nf_b, "norm.bias");
    rc = norm.rc;
    for (int l = 0; l < NL && !rc; ++l) {
        const hg_detr_dec_layer_weights& s = w->layers[l];
        DetrDecLayerW& d = e.layers[l];
        DetrLayerLoader ld{c, e.owned, who, l, 0};
        ld.common(s, D, F, d.sa);
        // multihead_attn.in_proj: the q rows stay with the layer, the k and v rows join the stacked matrices
        ld.f16(s.cross_in_proj_weight, DD, &d.wq_c, "multihead_attn.in_proj_weight");
        ld.f32(s.cross_in_proj_bias, D, &d.bq_c, "multihead_attn.in_proj_bias");
        if (!ld.rc) {
            const std::string in_w = ld.name("multihead_attn.in_proj_weight"), in_b = ld.name("multihead_attn.in_proj_bias");
            keep_first(ld.rc, cvt_f16(c, s.cross_in_proj_weight, DD, DD, e.wk_all + l * DD, who, in_w.c_str()));
            keep_first(ld.rc, cvt_f16(c, s.cross_in_proj_weight, 2 * DD, DD, e.wv_all + l * DD, who, in_w.c_str()));
            keep_first(ld.rc, cvt_f32(c, s.cross_in_proj_bias, D, D, e.bk_all + (size_t)l * D, who, in_b.c_str()));
            keep_first(ld.rc, cvt_f32(c, s.cross_in_proj_bias, (size_t)2 * D, D, e.bv_all + (size_t)l * D, who, in_b.c_str()));
        }
        ld.f16(s.cross_out_proj_weight, DD, &d.w_out_c, "multihead_attn.out_proj.weight");
        ld.f32(s.cross_out_proj_bias, D, &d.b_out_c, "multihead_attn.out_proj.bias");
        ld.f32(s.norm3_weight, D, &d.n3_w, "norm3.weight");
        ld.f32(s.norm3_bias, D, &d.n3_b, "norm3.bias");
        rc = ld.rc;
    }
    if (rc) {
        free_all(e.owned);
        e = DetrDec{};
        return rc;
    }
    HG_HIP(hipDeviceSynchronize());
    e.loaded = true;
    return HG_OK;
}

// detr/models/transformer.py:95-124 (tgt_mask = memory_mask = tgt_key_padding_mask = None): every layer is :212-233
int hg_detr_decoder(hg_ctx* c, const hg_detr_decoder_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    DetrDec& e = c->detr_dec;
    if (!e.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_detr_decoder: no decoder loaded (hg_load_detr_decoder)");
    if (!a || !a->memory || !a->query_pos || !a->out) return fail(c, HG_ERR_INVALID, "hg_detr_decoder: memory, query_pos and out are required");
    const int B = a->B, S = a->S, Q = a->Q;
    if (B < 1 || S < 1 || Q < 1) return fail(c, HG_ERR_INVALID, "hg_detr_decoder: B, S and Q must be at least 1 (got B %d, S %d, Q %d)", B, S, Q);
    if (S > DETR_ATTN_MAX_L || Q > DETR_ATTN_MAX_L)
        return fail(c, HG_ERR_INVALID, "hg_detr_decoder: S = %d tokens and Q = %d queries, at most %d each", S, Q, DETR_ATTN_MAX_L);
    if ((long long)B * std::max(S, Q) > (1LL << 20))
        return fail(c, HG_ERR_INVALID, "hg_detr_decoder: B * max(S, Q) = %lld rows, at most 2^20", (long long)B * std::max(S, Q));
    if (a->memory_stride[2] != 1 || a->query_pos_stride[2] != 1 || a->out_stride[3] != 1 || (a->pos && a->pos_stride[2] != 1) ||
        (a->tgt && a->tgt_stride[2] != 1))
        return fail(c, HG_ERR_INVALID, "hg_detr_decoder: the channel stride of tgt, query_pos, memory, pos and out must be 1");
    int rc = detr_check_attn_options(c, "hg_detr_decoder");
    if (rc) return rc;
    const int D = e.D, F = e.F, Ms = B * S, Mq = B * Q, NL = (int)e.layers.size(), ND = NL * D;
    const bool ffn_fits = detr_ffn_ok(Mq, D, F);
    if (c->opt_detr_ffn == 2 && !ffn_fits)
        return fail(c, HG_ERR_INVALID, "hg_detr_decoder: option detr_ffn = 2, and the split FFN kernel does not cover d_model %d, d_ff %d", D, F);
    const bool split = c->opt_detr_ffn == 2 || (c->opt_detr_ffn == 0 && ffn_fits && Mq <= c->opt_detr_ffn_max_m);
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    // workspace: A operands of the GEMMs with their row count padded to 256 (hg_kernels.h)
    const size_t Sp = rup(Ms, 256), Qp = rup(Mq, 256);
    const size_t o_mx = 0, o_mpos = o_mx + Sp * D * 4, o_m16 = o_mpos + Sp * D * 4, o_mp16 = o_m16 + Sp * D * 2, o_kall = o_mp16 + Sp * D * 2,
                 o_vall = o_kall + Sp * ND * 2, o_x = o_vall + Sp * ND * 2, o_qpos = o_x + Qp * D * 4, o_x16 = o_qpos + Qp * D * 4,
                 o_xp16 = o_x16 + Qp * D * 2, o_qk = o_xp16 + Qp * D * 2, o_v = o_qk + Qp * 2 * D * 2, o_q = o_v + Qp * D * 2,
                 o_att = o_q + Qp * D * 2, o_ff = o_att + Qp * D * 2,
                 total = o_ff + (split ? rup(detr_ffn_partial_bytes(Mq, D, F), 256) : Qp * F * 2);
    rc = ensure(c, c->detr_dec_ws, total);
    if (rc) return rc;
    char* ws = (char*)c->detr_dec_ws.p;
    float *mx = (float*)(ws + o_mx), *mpos = (float*)(ws + o_mpos), *x = (float*)(ws + o_x), *qposb = (float*)(ws + o_qpos);
    half_t *m16 = (half_t*)(ws + o_m16), *mp16 = (half_t*)(ws + o_mp16), *kall = (half_t*)(ws + o_kall), *vall = (half_t*)(ws + o_vall),
           *x16 = (half_t*)(ws + o_x16), *xp16 = (half_t*)(ws + o_xp16), *qk = (half_t*)(ws + o_qk), *v = (half_t*)(ws + o_v),
           *q = (half_t*)(ws + o_q), *att = (half_t*)(ws + o_att), *ff = (half_t*)(ws + o_ff);
    float* part = (float*)(ws + o_ff);
    {
        RowScope ps(c, s, Ms, D, 0);
        HG_HIP(launch_detr_entry(a->memory, a->pos, a->memory_stride[0], a->memory_stride[1], a->pos ? a->pos_stride[0] : 0,
                                 a->pos ? a->pos_stride[1] : 0, B, S, D, mx, m16, mp16, mpos, s));
    }
    // k = fp16(memory + pos) Wk^T + b and v = fp16(memory) Wv^T + b of EVERY layer (transformer.py:225-227: memory is the same for all)
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(mp16, D, e.wk_all, e.bk_all, kall, ND, Ms, ND, D), s));
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(m16, D, e.wv_all, e.bv_all, vall, ND, Ms, ND, D), s));
    {
        RowScope ps(c, s, Mq, D, 0);
        HG_HIP(launch_detr_dec_entry(a->tgt, a->tgt ? a->tgt_stride[0] : 0, a->tgt ? a->tgt_stride[1] : 0, a->query_pos, a->query_pos_stride[0],
                                     a->query_pos_stride[1], B, Q, D, x, x16, xp16, qposb, s));
    }
    for (int l = 0; l < NL; ++l) {
        const DetrDecLayerW& w = e.layers[l];
        // self-attention: tgt = norm1(tgt + out_proj(attention(q = k = tgt + query_pos, v = tgt)))                                   (:219-223)
        if ((rc = detr_self_attention(c, "hg_detr_decoder: self-attention", w.sa, x16, xp16, qk, v, att, x, nullptr, B, Q, e.heads, s))) return rc;
        {
            RowScope ps(c, s, Mq, D, 0);
            HG_HIP(launch_detr_postnorm(x, w.sa.n1_w, w.sa.n1_b, qposb, x16, xp16, nullptr, Mq, D, s));
        }
        // cross-attention: q = fp16(tgt + query_pos) Wq^T + b against this layer's columns of the stacked K and V; norm2             (:224-229)
        HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(xp16, D, w.wq_c, w.bq_c, q, D, Mq, D, D), s));
        hipError_t he = detr_attention(c, q, D, kall + (size_t)l * D, ND, vall + (size_t)l * D, ND, a->memory_mask, att, B, Q, S, e.heads, s);
        if (he != hipSuccess) return fail(c, HG_ERR_HIP, "hg_detr_decoder: cross-attention launch failed: %s", hipGetErrorString(he));
        HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(att, D, w.w_out_c, w.b_out_c, x, D, Mq, D, D), s));
        {
            RowScope ps(c, s, Mq, D, 0);
            HG_HIP(launch_detr_postnorm(x, w.sa.n2_w, w.sa.n2_b, nullptr, x16, nullptr, nullptr, Mq, D, s));
        }
        // tgt = norm3(tgt + linear2(relu(linear1(tgt))))                                                                             (:230-232)
        if (split) {
            ProfScope ps(c, s, HG_PROF_DETR_FFN, Mq, F, D);
            HG_HIP(launch_detr_ffn(x16, w.sa.w1, w.sa.b1, w.sa.w2, part, Mq, D, F, s));
        } else {
            HG_HIP(gemm(c, EPI_BIAS_RELU_F16, gemm_args(x16, D, w.sa.w1, w.sa.b1, ff, F, Mq, F, D), s));
            HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(ff, F, w.sa.w2, w.sa.b2, x, D, Mq, D, F), s));
        }
        const bool leaves = a->return_intermediate || l == NL - 1;
        float* dst = leaves ? a->out + (a->return_intermediate ? (long long)l * a->out_stride[0] : 0) : nullptr;
        {
            RowScope ps(c, s, Mq, D, split ? F / DETR_FFN_SLICE : 0);
            HG_HIP(launch_detr_dec_tail(x, split ? w.sa.b2 : nullptr, split ? part : nullptr, split ? F / DETR_FFN_SLICE : 0, w.n3_w, w.n3_b, qposb,
                                        x16, l + 1 < NL ? xp16 : nullptr, a->trace ? a->trace + (size_t)l * Mq * D : nullptr, e.nf_w, e.nf_b,
                                        dst, a->out_stride[1], a->out_stride[2], Q, Mq, D, s));
        }
    }
    return HG_OK;
}

}  // extern "C"
