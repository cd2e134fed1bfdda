// DETR transformer decoder on the HIP path (detr/models/transformer.py:86-124 over the post-norm layer :212-233): the weight loader and
// the layer runner.  Host code only; the kernels are hg_detr_attn.hip (both attentions), hg_detr_ffn.hip (the FFN split over d_ff),
// hg_detr_rows.hip (entries, post-norms, the layer tail) and the project's GEMMs.
#include "hg_host.h"

namespace {

// n elements of t from element `off` on, as fp16 / fp32, into dst (device memory of the decoder slot)
int dec_cvt16(hg_ctx* c, const hg_tensor& t, size_t off, size_t n, half_t* dst, int layer, const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: missing tensor layers.%d.%s", layer, name);
    if (t.dtype == HG_F16) HG_HIP(hipMemcpy(dst, (const half_t*)t.ptr + off, n * 2, hipMemcpyDeviceToDevice));
    else if (t.dtype == HG_F32) HG_HIP(launch_f32_to_f16((const float*)t.ptr + off, dst, n, 0));
    else return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: bad dtype for layers.%d.%s", layer, name);
    return HG_OK;
}

int dec_cvt32(hg_ctx* c, const hg_tensor& t, size_t off, size_t n, float* dst, int layer, const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: missing tensor layers.%d.%s", layer, name);
    if (t.dtype == HG_F32) HG_HIP(hipMemcpy(dst, (const float*)t.ptr + off, n * 4, hipMemcpyDeviceToDevice));
    else if (t.dtype == HG_F16) HG_HIP(launch_f16_to_f32((const half_t*)t.ptr + off, dst, n, 0));
    else return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: bad dtype for layers.%d.%s", layer, name);
    return HG_OK;
}

template <typename T>
int dec_alloc(hg_ctx* c, std::vector<void*>& owned, size_t n, T** out) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, n * sizeof(T) ? n * sizeof(T) : 16);
    if (e != hipSuccess) return fail(c, HG_ERR_OOM, "hipMalloc(%zu) failed: %s", n * sizeof(T), hipGetErrorString(e));
    owned.push_back(p);
    *out = (T*)p;
    return HG_OK;
}

int dec_f16(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, size_t off, size_t n, half_t** out, int layer, const char* name) {
    int rc = dec_alloc(c, owned, n, out);
    return rc ? rc : dec_cvt16(c, t, off, n, *out, layer, name);
}

int dec_f32(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, size_t off, size_t n, float** out, int layer, const char* name) {
    int rc = dec_alloc(c, owned, n, out);
    return rc ? rc : dec_cvt32(c, t, off, n, *out, layer, name);
}

// a row kernel of the decoder under the profiler
struct RowScope : ProfScope {
    RowScope(hg_ctx* c, hipStream_t s, int M, int D, int slices) : ProfScope(c, s, HG_PROF_DETR_ROWS, M, D, slices) {}
};

}  // namespace

extern "C" {

// detr/models/transformer.py:187-204 (the layer's parameters) for every layer of :88-93, and the decoder's norm
int hg_load_detr_decoder(hg_ctx* c, const hg_detr_decoder_weights* w) {
    if (!c) return HG_ERR_INVALID;
    if (!w || !w->layers) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: weights are required");
    if (w->normalize_before)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: normalize_before (the pre-norm layer) is not implemented: the detector is post-norm");
    if (w->activation != 0) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: only the ReLU activation is implemented (activation = 0)");
    const int D = w->d_model, H = w->heads, F = w->d_ff, NL = w->n_layers;
    if (NL < 1 || NL > 12) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: 1 .. 12 layers (got %d)", NL);
    if (H < 1 || D != 32 * H || D % 128) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: d_model must be 32 * heads and a multiple of 128 (got d_model %d, heads %d)", D, H);
    if (D > 512) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: d_model at most 512 (got %d)", D);
    if (F < 128 || F % 128) return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: d_ff must be a multiple of 128 (got %d)", F);
    if (!w->norm_weight.ptr || !w->norm_bias.ptr)
        return fail(c, HG_ERR_INVALID, "hg_load_detr_decoder: the decoder's final norm (norm.weight, norm.bias) is required");
    HG_ON_DEVICE(c);
    DetrDec& e = c->detr_dec;
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    free_all(e.owned);
    e = DetrDec{};
    e.D = D; e.heads = H; e.F = F;
    e.layers.resize(NL);
    const size_t DD = (size_t)D * D;
    int rc = 0;
    keep_first(rc, dec_alloc(c, e.owned, NL * DD, &e.wk_all));
    keep_first(rc, dec_alloc(c, e.owned, NL * DD, &e.wv_all));
    keep_first(rc, dec_alloc(c, e.owned, (size_t)NL * D, &e.bk_all));
    keep_first(rc, dec_alloc(c, e.owned, (size_t)NL * D, &e.bv_all));
    keep_first(rc, dec_f32(c, e.owned, w->norm_weight, 0, D, &e.nf_w, -1, "norm.weight"));
    keep_first(rc, dec_f32(c, e.owned, w->norm_bias, 0, D, &e.nf_b, -1, "norm.bias"));
    for (int l = 0; l < NL && !rc; ++l) {
        const hg_detr_dec_layer_weights& s = w->layers[l];
        DetrDecLayerW& d = e.layers[l];
        keep_first(rc, dec_f16(c, e.owned, s.in_proj_weight, 0, 3 * DD, &d.sa.w_in, l, "self_attn.in_proj_weight"));
        keep_first(rc, dec_f32(c, e.owned, s.in_proj_bias, 0, (size_t)3 * D, &d.sa.b_in, l, "self_attn.in_proj_bias"));
        keep_first(rc, dec_f16(c, e.owned, s.out_proj_weight, 0, DD, &d.sa.w_out, l, "self_attn.out_proj.weight"));
        keep_first(rc, dec_f32(c, e.owned, s.out_proj_bias, 0, D, &d.sa.b_out, l, "self_attn.out_proj.bias"));
        keep_first(rc, dec_f16(c, e.owned, s.linear1_weight, 0, (size_t)F * D, &d.sa.w1, l, "linear1.weight"));
        keep_first(rc, dec_f32(c, e.owned, s.linear1_bias, 0, F, &d.sa.b1, l, "linear1.bias"));
        keep_first(rc, dec_f16(c, e.owned, s.linear2_weight, 0, (size_t)D * F, &d.sa.w2, l, "linear2.weight"));
        keep_first(rc, dec_f32(c, e.owned, s.linear2_bias, 0, D, &d.sa.b2, l, "linear2.bias"));
        keep_first(rc, dec_f32(c, e.owned, s.norm1_weight, 0, D, &d.sa.n1_w, l, "norm1.weight"));
        keep_first(rc, dec_f32(c, e.owned, s.norm1_bias, 0, D, &d.sa.n1_b, l, "norm1.bias"));
        keep_first(rc, dec_f32(c, e.owned, s.norm2_weight, 0, D, &d.sa.n2_w, l, "norm2.weight"));
        keep_first(rc, dec_f32(c, e.owned, s.norm2_bias, 0, D, &d.sa.n2_b, l, "norm2.bias"));
        // multihead_attn.in_proj: the q rows stay with the layer, the k and v rows join the stacked matrices
        keep_first(rc, dec_f16(c, e.owned, s.cross_in_proj_weight, 0, DD, &d.wq_c, l, "multihead_attn.in_proj_weight"));
        keep_first(rc, dec_f32(c, e.owned, s.cross_in_proj_bias, 0, D, &d.bq_c, l, "multihead_attn.in_proj_bias"));
        if (!rc) {
            keep_first(rc, dec_cvt16(c, s.cross_in_proj_weight, DD, DD, e.wk_all + l * DD, l, "multihead_attn.in_proj_weight"));
            keep_first(rc, dec_cvt16(c, s.cross_in_proj_weight, 2 * DD, DD, e.wv_all + l * DD, l, "multihead_attn.in_proj_weight"));
            keep_first(rc, dec_cvt32(c, s.cross_in_proj_bias, D, D, e.bk_all + (size_t)l * D, l, "multihead_attn.in_proj_bias"));
            keep_first(rc, dec_cvt32(c, s.cross_in_proj_bias, (size_t)2 * D, D, e.bv_all + (size_t)l * D, l, "multihead_attn.in_proj_bias"));
        }
        keep_first(rc, dec_f16(c, e.owned, s.cross_out_proj_weight, 0, DD, &d.w_out_c, l, "multihead_attn.out_proj.weight"));
        keep_first(rc, dec_f32(c, e.owned, s.cross_out_proj_bias, 0, D, &d.b_out_c, l, "multihead_attn.out_proj.bias"));
        keep_first(rc, dec_f32(c, e.owned, s.norm3_weight, 0, D, &d.n3_w, l, "norm3.weight"));
        keep_first(rc, dec_f32(c, e.owned, s.norm3_bias, 0, D, &d.n3_b, l, "norm3.bias"));
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
    const int chunk = c->opt_detr_attn_chunk;
    if (chunk % 32) return fail(c, HG_ERR_INVALID, "hg_detr_decoder: option detr_attn_chunk = %d is no multiple of 32", chunk);
    if (c->opt_detr_attn_waves == 3) return fail(c, HG_ERR_INVALID, "hg_detr_decoder: option detr_attn_waves must be 0, 1, 2 or 4");
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
    int rc = ensure(c, c->detr_dec_ws, total);
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
    auto attend = [&](const half_t* aq, int ldq, const half_t* ak, int ldk, const half_t* av, int ldv, const uint8_t* mask, int Lk) {
        DetrAttnArgs da{};
        da.q = aq; da.k = ak; da.v = av; da.ldq = ldq; da.ldk = ldk; da.ldv = ldv;
        da.mask = mask; da.out = att; da.ldo = D; da.n_seq = B; da.Lq = Q; da.Lk = Lk; da.heads = e.heads; da.chunk = chunk;
        da.waves = c->opt_detr_attn_waves;
        ProfScope ps(c, s, HG_PROF_ATTENTION, B, Lk, e.heads);
        return launch_detr_attention(da, s);
    };
    for (int l = 0; l < NL; ++l) {
        const DetrDecLayerW& w = e.layers[l];
        // self-attention: q | k = fp16(tgt + query_pos) W[0:2D]^T + b, v = fp16(tgt) W[2D:3D]^T + b; tgt = norm1(tgt + out_proj(.))   (:219-223)
        HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(xp16, D, w.sa.w_in, w.sa.b_in, qk, 2 * D, Mq, 2 * D, D), s));
        HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(x16, D, w.sa.w_in + (size_t)2 * D * D, w.sa.b_in + 2 * D, v, D, Mq, D, D), s));
        hipError_t he = attend(qk, 2 * D, qk + D, 2 * D, v, D, nullptr, Q);
        if (he != hipSuccess) return fail(c, HG_ERR_HIP, "hg_detr_decoder: self-attention launch failed: %s", hipGetErrorString(he));
        HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(att, D, w.sa.w_out, w.sa.b_out, x, D, Mq, D, D), s));
        {
            RowScope ps(c, s, Mq, D, 0);
            HG_HIP(launch_detr_postnorm(x, w.sa.n1_w, w.sa.n1_b, qposb, x16, xp16, nullptr, Mq, D, s));
        }
        // cross-attention: q = fp16(tgt + query_pos) Wq^T + b against this layer's columns of the stacked K and V; norm2             (:224-229)
        HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(xp16, D, w.wq_c, w.bq_c, q, D, Mq, D, D), s));
        he = attend(q, D, kall + (size_t)l * D, ND, vall + (size_t)l * D, ND, a->memory_mask, S);
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
