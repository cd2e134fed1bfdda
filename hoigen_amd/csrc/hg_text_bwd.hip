// The input gradient of the frozen text tower: grad_prompts [R, L, D] from grad_out [R, E] for TextEncoder.forward
// (main_coop_vae.py:54-63), the one heavy thing the CoOp-VAE training loop back-propagates through (main_coop_vae.py:452-468; CLIP is
// frozen there, :316-318, so no weight gradient of the tower is computed).  Host code only; the kernels are hg_text_grad.hip and the
// GEMMs of the forward (dX = dY W on the weights held once more, transposed).  DESIGN.md section 23.
//
// Activation checkpointing: hg_encode_text_embeds_save kept the stream as it entered every block; each block is recomputed from it with
// the plain launch sequence (launch_row0_block spells the same one out for a dense stream) and then walked backwards.  The residual
// gradient g stays fp32; a gradient is fp16 where it is an MFMA operand, which is why the whole backward runs on grad_out scaled per
// prompt by an exact power of two (the backward is linear in grad_out, and prompts never meet) and is unscaled at its end.
#include "hg_host.h"

namespace hg_host {

// the allocations and the transposes; on any error the caller frees what was allocated
static int build_text_grad(hg_ctx* c, std::vector<Text::GradW>& gw) {
    Text& t = c->text;
    const int D = t.D;
    for (size_t i = 0; i < t.blocks.size(); ++i) {
        const BlockW& w = t.blocks[i];
        int rc = 0;
        keep_first(rc, dev_alloc_n(c, t.owned_grad, (size_t)3 * D * D, &gw[i].wT_qkv));
        keep_first(rc, dev_alloc_n(c, t.owned_grad, (size_t)D * D, &gw[i].wT_out));
        keep_first(rc, dev_alloc_n(c, t.owned_grad, (size_t)4 * D * D, &gw[i].wT_fc));
        keep_first(rc, dev_alloc_n(c, t.owned_grad, (size_t)4 * D * D, &gw[i].wT_proj));
        if (rc) return rc;
        HG_HIP(launch_transpose_to_f16(w.w_qkv, HG_F16, gw[i].wT_qkv, 3 * D, D, 0));
        HG_HIP(launch_transpose_to_f16(w.w_out, HG_F16, gw[i].wT_out, D, D, 0));
        HG_HIP(launch_transpose_to_f16(w.w_fc, HG_F16, gw[i].wT_fc, 4 * D, D, 0));
        HG_HIP(launch_transpose_to_f16(w.w_proj, HG_F16, gw[i].wT_proj, D, 4 * D, 0));
    }
    int rc = 0;
    keep_first(rc, dev_alloc_n(c, t.owned_grad, (size_t)D * t.E, &t.g_proj));
    keep_first(rc, dev_alloc_n(c, t.owned_grad, (size_t)4 * D, &t.g_zero));
    if (rc) return rc;
    HG_HIP(launch_transpose_to_f16(t.w_projT, HG_F16, t.g_proj, t.E, D, 0));
    HG_HIP(hipMemset(t.g_zero, 0, (size_t)4 * D * 4));
    HG_HIP(hipDeviceSynchronize());
    return HG_OK;
}

// Load-time work done at the first backward call, like a loader: synchronous, on the null stream, ending in a device synchronisation -
// not on the caller's stream.  A first backward call inside a stream capture therefore fails; make one differentiable call before capturing.
int ensure_text_grad(hg_ctx* c) {
    Text& t = c->text;
    if (!t.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_text has not been called");
    if (!t.grad.empty()) return HG_OK;
    std::vector<Text::GradW> gw(t.blocks.size());
    if (int rc = build_text_grad(c, gw)) {      // whatever the failing step: nothing stays allocated, the next call starts over
        free_all(t.owned_grad);
        t.g_proj = nullptr; t.g_zero = nullptr;
        return rc;
    }
    t.grad = std::move(gw);
    return HG_OK;
}

// c->tgrad, carved: g16 fp16 [Mp, D] | da fp16 [Mp, D] | dfc fp16 [Mp, 4D] | dqkv fp16 [Mp, 3D] | dh fp32 [Mp, D] | g fp32 [Mp, D] |
// go16 fp16 [Rp, E] | dhf fp32 [Rp, D] | sinv fp32 [Rp]; Mp, Rp = rows rounded up to 256 (the GEMMs read whole tiles of their A operand)
struct TextGradWs {
    half_t *g16, *da, *dfc, *dqkv, *go16;
    float *dh, *g, *dhf, *sinv;
};
static TextGradWs text_grad_carve(const hg_ctx* c, int M, int R) {
    const size_t Mp = rup(M, 256), Rp = rup(R > 0 ? R : 1, 256), D = c->text.D, E = c->text.E;
    TextGradWs w;
    char* p = (char*)c->tgrad.p;
    w.g16 = (half_t*)p; p += Mp * D * 2;
    w.da = (half_t*)p; p += Mp * D * 2;
    w.dfc = (half_t*)p; p += Mp * 4 * D * 2;
    w.dqkv = (half_t*)p; p += Mp * 3 * D * 2;
    w.dh = (float*)p; p += Mp * D * 4;
    w.g = (float*)p; p += Mp * D * 4;
    w.go16 = (half_t*)p; p += Rp * E * 2;
    w.dhf = (float*)p; p += Rp * D * 4;
    w.sinv = (float*)p;
    return w;
}
int text_grad_ws(hg_ctx* c, int M, int R) {
    const size_t Mp = rup(M, 256), Rp = rup(R > 0 ? R : 1, 256), D = c->text.D, E = c->text.E;
    int rc = 0;
    keep_first(rc, ensure(c, c->tgrad, Mp * D * (2 + 2 + 8 + 6 + 4 + 4) + Rp * (E * 2 + D * 4 + 4)));
    // the recomputed block lives where the forward's does
    keep_first(rc, ensure(c, c->x, Mp * D * 4));
    keep_first(rc, ensure(c, c->h, Mp * D * 2));
    keep_first(rc, ensure(c, c->qkv, Mp * 3 * D * 2));
    keep_first(rc, ensure(c, c->att, Mp * D * 2));
    keep_first(rc, ensure(c, c->fc, Mp * 4 * D * 2));
    return rc;
}

// a row / elementwise launch under the profiler's HG_PROF_TEXT_GRAD_ROWS
#define HG_ROWS(call)                                           \
    do {                                                        \
        ProfScope ps_(c, s, HG_PROF_TEXT_GRAD_ROWS, M, D, 0);   \
        HG_HIP(call);                                           \
    } while (0)

int text_block_backward(hg_ctx* c, int block, const float* x_in, float* g, int n_seq, int L, hipStream_t s) {
    const Text& t = c->text;
    const BlockW& w = t.blocks[block];
    const Text::GradW& gw = t.grad[block];
    const int D = t.D, M = n_seq * L;
    const TextGradWs ws = text_grad_carve(c, M, 0);
    float* x = (float*)c->x.p;
    half_t *h = (half_t*)c->h.p, *qkv = (half_t*)c->qkv.p, *att = (half_t*)c->att.p, *u = (half_t*)c->fc.p;
    const float* zero = t.g_zero;
    // ---- the block again, from its saved input: qkv, x_mid (in x) and the pre-activation u of the MLP
    HG_ROWS(launch_layernorm_f16(x_in, w.ln1_w, w.ln1_b, h, M, D, nullptr, 0, 1, s));
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(h, D, w.w_qkv, w.b_qkv, qkv, 3 * D, M, 3 * D, D), s));
    HG_HIP(attention(c, qkv, att, n_seq, L, t.heads, true, s));
    HG_ROWS(hipMemcpyAsync(x, x_in, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(att, D, w.w_out, w.b_out, x, D, M, D, D), s));
    HG_ROWS(launch_layernorm_f16(x, w.ln2_w, w.ln2_b, h, M, D, nullptr, 0, 1, s));
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(h, D, w.w_fc, w.b_fc, u, 4 * D, M, 4 * D, D), s));
    // ---- MLP: df = fp16(g) W_proj, du = df qgelu'(u), dh2 = du W_fc, g += LN2_backward(x_mid, dh2)
    HG_ROWS(launch_f32_to_f16(g, ws.g16, (size_t)M * D, s));
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(ws.g16, D, gw.wT_proj, zero, ws.dfc, 4 * D, M, 4 * D, D), s));
    HG_ROWS(launch_qgelu_bwd(ws.dfc, u, ws.dfc, (size_t)M * 4 * D, s));
    HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(ws.dfc, 4 * D, gw.wT_fc, zero, ws.dh, D, M, D, 4 * D), s));
    HG_ROWS(launch_layernorm_bwd(x, w.ln2_w, ws.dh, g, M, D, nullptr, 0, s));
    // ---- attention: da = fp16(g) W_out, dqkv = attention_backward(qkv, da), dh1 = dqkv W_qkv, g += LN1_backward(x_in, dh1)
    HG_ROWS(launch_f32_to_f16(g, ws.g16, (size_t)M * D, s));
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(ws.g16, D, gw.wT_out, zero, ws.da, D, M, D, D), s));
    {
        ProfScope ps(c, s, HG_PROF_TEXT_ATTN_BWD, n_seq, L, t.heads);
        HG_HIP(launch_text_attn_bwd(qkv, ws.da, ws.dqkv, n_seq, L, t.heads, s));
    }
    HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(ws.dqkv, 3 * D, gw.wT_qkv, zero, ws.dh, D, M, D, 3 * D), s));
    HG_ROWS(launch_layernorm_bwd(x_in, w.ln1_w, ws.dh, g, M, D, nullptr, 0, s));
    return HG_OK;
}

}  // namespace hg_host

extern "C" {

int hg_text_backward_embeds(hg_ctx* c, const float* saved, const int32_t* eot_idx, const float* grad_out, int R, int L, int trunc,
                            float* grad_prompts, void* stream) {
    if (!c) return HG_ERR_INVALID;
    Text& t = c->text;
    if (!t.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_text has not been called");
    if (R == 0) return HG_OK;
    if (R < 0 || !saved || !eot_idx || !grad_out || !grad_prompts || L < 1 || L > t.ctx)
        return fail(c, HG_ERR_INVALID, "bad arguments to text_backward_embeds");
    const int Leff = (trunc > 0 && trunc < L) ? trunc : L;
    if (Leff > TEXT_GRAD_MAX_L) return fail(c, HG_ERR_INVALID, "hg_text_backward_embeds: at most %d tokens per prompt (got %d)", TEXT_GRAD_MAX_L, Leff);
    if ((long long)R * Leff > c->text_rows_budget)
        return fail(c, HG_ERR_INVALID, "hg_text_backward_embeds: %d prompts of %d tokens are more than one pass of the text tower (a row budget of "
                                       "%d rows)", R, Leff, c->text_rows_budget);
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    if (int rc = ensure_text_grad(c)) return rc;
    const int D = t.D, E = t.E, M = R * Leff, layers = (int)t.blocks.size();
    if (int rc = text_grad_ws(c, M, R)) return rc;
    const TextGradWs ws = text_grad_carve(c, M, R);
    const size_t entry = (size_t)M * D;
    // ---- tail: d h_f = fp16(s grad_out) text_projection^T, then ln_final backward on the saved EOT rows, scattered into a zero stream
    HG_ROWS(launch_grad_scale(grad_out, ws.go16, ws.sinv, R, E, s));
    HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(ws.go16, E, t.g_proj, t.g_zero, ws.dhf, D, R, D, E), s));
    HG_ROWS(hipMemsetAsync(ws.g, 0, entry * 4, s));
    HG_ROWS(launch_layernorm_bwd(saved + layers * entry, t.lnf_w, ws.dhf, ws.g, R, D, eot_idx, Leff, s));
    for (int i = layers - 1; i >= 0; --i)
        if (int rc = text_block_backward(c, i, saved + i * entry, ws.g, R, Leff, s)) return rc;
    // ---- the positional embedding is added to the prompts: its backward is the identity.  Unscale; positions >= Leff are zeros
    HG_ROWS(launch_grad_unscale(ws.g, ws.sinv, grad_prompts, R, L, Leff, D, s));
    return HG_OK;
}

}  // extern "C"
