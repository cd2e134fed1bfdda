// What the host files of the DETR transformer share (hg_detr.hip: the encoder; hg_detr_dec.hip: the decoder): the loaders' dimension
// checks and the twelve tensors a layer of either holds, the runners' option checks, the attention launch and the self-attention step.
// Host code only.
#pragma once
#include "hg_host.h"

namespace hg_host {

// hg_load_detr_encoder / hg_load_detr_decoder (`who`): what both refuse of the descriptor's integers
template <class W>
inline int detr_check_dims(hg_ctx* c, const char* who, const W* w) {
    if (!w || !w->layers) return fail(c, HG_ERR_INVALID, "%s: weights are required", who);
    if (w->normalize_before)
        return fail(c, HG_ERR_INVALID, "%s: normalize_before (the pre-norm layer) is not implemented: the detector is post-norm", who);
    if (w->activation != 0) return fail(c, HG_ERR_INVALID, "%s: only the ReLU activation is implemented (activation = 0)", who);
    const int D = w->d_model, H = w->heads, F = w->d_ff, NL = w->n_layers;
    if (NL < 1 || NL > 12) return fail(c, HG_ERR_INVALID, "%s: 1 .. 12 layers (got %d)", who, NL);
    if (H < 1 || D != 32 * H || D % 128) return fail(c, HG_ERR_INVALID, "%s: d_model must be 32 * heads and a multiple of 128 (got d_model %d, heads %d)", who, D, H);
    if (F < 128 || F % 128) return fail(c, HG_ERR_INVALID, "%s: d_ff must be a multiple of 128 (got %d)", who, F);
    return HG_OK;
}

// The tensors of layer l into a loader's slot: a message names them `who` ("hg_load_x: ") "layers.<l>.<key>" (the decoder's final norm
// goes as layer -1).  rc keeps the first failure; later tensors are still tried, as the loaders always did.
struct DetrLayerLoader {
    hg_ctx* c;
    std::vector<void*>& owned;
    const char* who;
    int l, rc;
    std::string name(const char* key) const { return "layers." + std::to_string(l) + "." + key; }
    void f16(const hg_tensor& t, size_t n, half_t** out, const char* key) { keep_first(rc, as_f16(c, owned, t, n, out, name(key).c_str(), who)); }
    void f32(const hg_tensor& t, size_t n, float** out, const char* key) { keep_first(rc, as_f32(c, owned, t, n, out, name(key).c_str(), who)); }
    // the tensors an encoder layer and a decoder layer both hold (S: hg_detr_layer_weights or hg_detr_dec_layer_weights)
    template <class S>
    void common(const S& s, int D, int F, DetrLayerW& d) {
        f16(s.in_proj_weight, (size_t)3 * D * D, &d.w_in, "self_attn.in_proj_weight");
        f32(s.in_proj_bias, (size_t)3 * D, &d.b_in, "self_attn.in_proj_bias");
        f16(s.out_proj_weight, (size_t)D * D, &d.w_out, "self_attn.out_proj.weight");
        f32(s.out_proj_bias, D, &d.b_out, "self_attn.out_proj.bias");
        f16(s.linear1_weight, (size_t)F * D, &d.w1, "linear1.weight");
        f32(s.linear1_bias, F, &d.b1, "linear1.bias");
        f16(s.linear2_weight, (size_t)D * F, &d.w2, "linear2.weight");
        f32(s.linear2_bias, D, &d.b2, "linear2.bias");
        f32(s.norm1_weight, D, &d.n1_w, "norm1.weight");
        f32(s.norm1_bias, D, &d.n1_b, "norm1.bias");
        f32(s.norm2_weight, D, &d.n2_w, "norm2.weight");
        f32(s.norm2_bias, D, &d.n2_b, "norm2.bias");
    }
};

// hg_detr_encoder / hg_detr_decoder (`who`): the options of the attention kernel that a call reads
inline int detr_check_attn_options(hg_ctx* c, const char* who) {
    if (c->opt_detr_attn_chunk % 32)
        return fail(c, HG_ERR_INVALID, "%s: option detr_attn_chunk = %d is no multiple of 32", who, c->opt_detr_attn_chunk);
    if (c->opt_detr_attn_waves == 3) return fail(c, HG_ERR_INVALID, "%s: option detr_attn_waves must be 0, 1, 2 or 4", who);
    return HG_OK;
}

// one launch of hg_detr_attn.hip under the profiler: Lq queries against Lk keys for each of n_seq sequences, out [n_seq * Lq, 32 * heads]
inline hipError_t detr_attention(hg_ctx* c, const half_t* q, int ldq, const half_t* k, int ldk, const half_t* v, int ldv, const uint8_t* mask,
                                 half_t* out, int n_seq, int Lq, int Lk, int heads, hipStream_t s) {
    DetrAttnArgs da{};
    da.q = q; da.k = k; da.v = v; da.ldq = ldq; da.ldk = ldk; da.ldv = ldv;
    da.mask = mask; da.out = out; da.ldo = 32 * heads; da.n_seq = n_seq; da.Lq = Lq; da.Lk = Lk; da.heads = heads;
    da.chunk = c->opt_detr_attn_chunk; da.waves = c->opt_detr_attn_waves;
    ProfScope ps(c, s, HG_PROF_ATTENTION, n_seq, Lk, heads);
    return launch_detr_attention(da, s);
}

// The self-attention step of a post-norm layer on the M = n_seq * L rows of the stream x (transformer.py:154-157, :219-222):
// q | k = xp16 W[0:2D]^T + b, v = x16 W[2D:3D]^T + b, the attention under `mask`, x += out_proj(.).  `what` opens the message of a
// failed attention launch ("hg_detr_x: attention").
inline int detr_self_attention(hg_ctx* c, const char* what, const DetrLayerW& w, const half_t* x16, const half_t* xp16, half_t* qk, half_t* v,
                               half_t* att, float* x, const uint8_t* mask, int n_seq, int L, int heads, hipStream_t s) {
    const int D = 32 * heads, M = n_seq * L;
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(xp16, D, w.w_in, w.b_in, qk, 2 * D, M, 2 * D, D), s));
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(x16, D, w.w_in + (size_t)2 * D * D, w.b_in + 2 * D, v, D, M, D, D), s));
    hipError_t he = detr_attention(c, qk, 2 * D, qk + D, 2 * D, v, D, mask, att, n_seq, L, L, heads, s);
    if (he != hipSuccess) return fail(c, HG_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(he));
    HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(att, D, w.w_out, w.b_out, x, D, M, D, D), s));
    return HG_OK;
}

}  // namespace hg_host
