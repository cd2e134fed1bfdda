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

}  // extern "C"
