// Weights into the device layout (hg_host.h): the conversion helpers, the loaders of both towers, the adapters, the VAE / mlp_net /
// cache slots.  Synchronous; load time only.
#include "hg_host.h"

namespace {

// ---- weight conversion helpers beyond hg_host.h's dev_alloc / as_f16 / as_f32 (synchronous; load time only) -------------------------------
// [rows, cols] -> fp16 [cols, rows]
int as_f16_T(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, int rows, int cols, half_t** out,
             const char* name) {
    if (!t.ptr) return fail(c, HG_ERR_INVALID, "missing tensor %s", name);
    void* p;
    int rc = dev_alloc(c, owned, (size_t)rows * cols * 2, &p);
    if (rc) return rc;
    HG_HIP(launch_transpose_to_f16(t.ptr, t.dtype, (half_t*)p, rows, cols, 0));
    *out = (half_t*)p;
    return HG_OK;
}

// fp32 [rows, cols] -> fp32 [cols, rows] via host (tiny adapter matrices)
int as_f32_T(hg_ctx* c, std::vector<void*>& owned, const hg_tensor& t, int rows, int cols, float** out,
             const char* name) {
    float* tmp;
    std::vector<void*> scratch;
    int rc = as_f32(c, scratch, t, (size_t)rows * cols, &tmp, name);
    if (rc) { free_all(scratch); return rc; }
    std::vector<float> h((size_t)rows * cols), ht((size_t)rows * cols);
    hipError_t e = hipMemcpy(h.data(), tmp, h.size() * 4, hipMemcpyDeviceToHost);
    free_all(scratch);
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hipMemcpy D2H failed for %s", name);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < cols; ++k) ht[(size_t)k * rows + r] = h[(size_t)r * cols + k];
    void* p;
    rc = dev_alloc(c, owned, ht.size() * 4, &p);
    if (rc) return rc;
    HG_HIP(hipMemcpy(p, ht.data(), ht.size() * 4, hipMemcpyHostToDevice));
    *out = (float*)p;
    return HG_OK;
}

int upload_f32(hg_ctx* c, std::vector<void*>& owned, const std::vector<float>& v, float** out) {
    void* p;
    int rc = dev_alloc(c, owned, v.size() * 4, &p);
    if (rc) return rc;
    HG_HIP(hipMemcpy(p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    *out = (float*)p;
    return HG_OK;
}

int to_host_f32(hg_ctx* c, const hg_tensor& t, size_t n, std::vector<float>& out, const char* name) {
    std::vector<void*> sc;
    float* d = nullptr;
    int rc = as_f32(c, sc, t, n, &d, name);
    if (rc) { free_all(sc); return rc; }
    out.resize(n);
    hipError_t e = hipMemcpy(out.data(), d, n * 4, hipMemcpyDeviceToHost);
    free_all(sc);
    return e == hipSuccess ? HG_OK : fail(c, HG_ERR_HIP, "hipMemcpy D2H failed for %s", name);
}

int load_blocks(hg_ctx* c, std::vector<void*>& owned, const hg_block_weights* src, int layers, int D,
                std::vector<BlockW>& dst, bool fold_ln) {
    if (!src) return fail(c, HG_ERR_INVALID, "blocks == NULL");
    dst.assign(layers, BlockW{});
    for (int i = 0; i < layers; ++i) {
        const hg_block_weights& s = src[i];
        BlockW& b = dst[i];
        int rc = 0;
        keep_first(rc, as_f16(c, owned, s.in_proj_weight, (size_t)3 * D * D, &b.w_qkv, "attn.in_proj_weight"));
        keep_first(rc, as_f32(c, owned, s.in_proj_bias, (size_t)3 * D, &b.b_qkv, "attn.in_proj_bias"));
        keep_first(rc, as_f16(c, owned, s.out_proj_weight, (size_t)D * D, &b.w_out, "attn.out_proj.weight"));
        keep_first(rc, as_f32(c, owned, s.out_proj_bias, D, &b.b_out, "attn.out_proj.bias"));
        keep_first(rc, as_f32(c, owned, s.ln_1_weight, D, &b.ln1_w, "ln_1.weight"));
        keep_first(rc, as_f32(c, owned, s.ln_1_bias, D, &b.ln1_b, "ln_1.bias"));
        keep_first(rc, as_f16(c, owned, s.c_fc_weight, (size_t)4 * D * D, &b.w_fc, "mlp.c_fc.weight"));
        keep_first(rc, as_f32(c, owned, s.c_fc_bias, (size_t)4 * D, &b.b_fc, "mlp.c_fc.bias"));
        keep_first(rc, as_f16(c, owned, s.c_proj_weight, (size_t)4 * D * D, &b.w_proj, "mlp.c_proj.weight"));
        keep_first(rc, as_f32(c, owned, s.c_proj_bias, D, &b.b_proj, "mlp.c_proj.bias"));
        keep_first(rc, as_f32(c, owned, s.ln_2_weight, D, &b.ln2_w, "ln_2.weight"));
        keep_first(rc, as_f32(c, owned, s.ln_2_bias, D, &b.ln2_b, "ln_2.bias"));
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
        if (!fold_ln) continue;
        keep_first(rc, dev_alloc(c, owned, (size_t)3 * D * D * 2, (void**)&b.wf_qkv));
        keep_first(rc, dev_alloc(c, owned, (size_t)3 * D * 4, (void**)&b.cs_qkv));
        keep_first(rc, dev_alloc(c, owned, (size_t)3 * D * 4, (void**)&b.csg_qkv));
        keep_first(rc, dev_alloc(c, owned, (size_t)4 * D * 4, (void**)&b.csg_fc));
        keep_first(rc, dev_alloc(c, owned, (size_t)3 * D * 4, (void**)&b.bf_qkv));
        keep_first(rc, dev_alloc(c, owned, (size_t)4 * D * D * 2, (void**)&b.wf_fc));
        keep_first(rc, dev_alloc(c, owned, (size_t)4 * D * 4, (void**)&b.cs_fc));
        keep_first(rc, dev_alloc(c, owned, (size_t)4 * D * 4, (void**)&b.bf_fc));
        if (rc) return rc < 0 ? rc : HG_ERR_OOM;
        HG_HIP(launch_fold_ln(b.w_qkv, b.ln1_w, b.ln1_b, b.b_qkv, b.wf_qkv, b.cs_qkv, b.bf_qkv, 3 * D, D, 0, b.csg_qkv));
        HG_HIP(launch_fold_ln(b.w_fc, b.ln2_w, b.ln2_b, b.b_fc, b.wf_fc, b.cs_fc, b.bf_fc, 4 * D, D, 0, b.csg_fc));
        if (qkv_attn_ok(1, 197, D, D / 64, D)) {      // (heads = width / 64 in every CLIP tower; L is checked per call)
            keep_first(rc, dev_alloc(c, owned, (size_t)3 * D * D * 2, (void**)&b.wp_qkv));
            keep_first(rc, dev_alloc(c, owned, (size_t)(D / 128) * 768 * 4, (void**)&b.bcs_qkv));
            if (rc) return rc < 0 ? rc : HG_ERR_OOM;
            HG_HIP(launch_pack_qkv(b.wf_qkv, b.bf_qkv, b.cs_qkv, b.wp_qkv, b.bcs_qkv, D, D / 64, 0));
        }

    }
    return HG_OK;
}

int load_decoder_layer(hg_ctx* c, std::vector<void*>& owned, const hg_decoder_layer_weights& s, int d,
                       float* dl[12], half_t* w16[6]) {
    {      // fp16 [out][in] operands of the MFMA decoder: the state dict's own layout
        half_t* inw16 = nullptr;
        int r16 = as_f16(c, owned, s.attn_in_proj_weight, (size_t)3 * d * d, &inw16, "adapter in_proj_weight");
        if (!r16) { w16[0] = inw16; w16[1] = inw16 + (size_t)d * d; w16[2] = inw16 + (size_t)2 * d * d; }
        if (!r16) r16 = as_f16(c, owned, s.attn_out_proj_weight, (size_t)d * d, &w16[3], "adapter out_proj.weight");
        if (!r16) r16 = as_f16(c, owned, s.linear1_weight, (size_t)2 * d * d, &w16[4], "adapter linear1.weight");
        if (!r16) r16 = as_f16(c, owned, s.linear2_weight, (size_t)2 * d * d, &w16[5], "adapter linear2.weight");
        if (r16) return r16;
    }
    // 0 WqT [d,d] (in->out), 1 bq, 2 WkT, 3 bk, 4 WvT, 5 bv : split of in_proj;  6 WoT, 7 bo ... see below
    std::vector<void*> scratch;
    float* inw;
    float* inb;
    int rc = as_f32(c, scratch, s.attn_in_proj_weight, (size_t)3 * d * d, &inw, "adapter in_proj_weight");
    if (!rc) rc = as_f32(c, scratch, s.attn_in_proj_bias, (size_t)3 * d, &inb, "adapter in_proj_bias");
    if (rc) { free_all(scratch); return rc; }
    for (int part = 0; part < 3 && !rc; ++part) {
        hg_tensor wt{inw + (size_t)part * d * d, HG_F32};
        hg_tensor bt{inb + (size_t)part * d, HG_F32};
        rc = as_f32_T(c, owned, wt, d, d, &dl[part], "adapter q/k/v weight");
        if (!rc) rc = as_f32(c, owned, bt, d, &dl[3 + part], "adapter q/k/v bias");
    }
    free_all(scratch);
    if (rc) return rc;
    keep_first(rc, as_f32_T(c, owned, s.attn_out_proj_weight, d, d, &dl[6], "adapter out_proj.weight"));
    keep_first(rc, as_f32(c, owned, s.attn_out_proj_bias, d, &dl[7], "adapter out_proj.bias"));
    // norm2 | norm3 packed: [w2, b2, w3, b3] (4*d)
    {
        float* p;
        int r2 = dev_alloc(c, owned, (size_t)4 * d * 4, (void**)&p);
        if (r2) return r2;
        const hg_tensor* ts[4] = {&s.norm2_weight, &s.norm2_bias, &s.norm3_weight, &s.norm3_bias};
        for (int k = 0; k < 4; ++k) {
            float* t;
            std::vector<void*> sc;
            int r3 = as_f32(c, sc, *ts[k], d, &t, "adapter norm");
            if (r3) { free_all(sc); return r3; }
            hipError_t e = hipMemcpy(p + (size_t)k * d, t, (size_t)d * 4, hipMemcpyDeviceToDevice);
            free_all(sc);
            if (e != hipSuccess) return fail(c, HG_ERR_HIP, "memcpy norm failed");
        }
        dl[8] = p;
    }
    keep_first(rc, as_f32_T(c, owned, s.linear1_weight, 2 * d, d, &dl[9], "adapter linear1.weight"));   // [d, 2d]
    keep_first(rc, as_f32(c, owned, s.linear1_bias, (size_t)2 * d, &dl[10], "adapter linear1.bias"));
    // linear2: weight^T [2d, d] followed by bias [d]
    {
        float* w2t;
        std::vector<void*> sc;
        int r2 = as_f32_T(c, sc, s.linear2_weight, d, 2 * d, &w2t, "adapter linear2.weight");
        float* b2 = nullptr;
        if (!r2) r2 = as_f32(c, sc, s.linear2_bias, d, &b2, "adapter linear2.bias");
        float* p = nullptr;
        if (!r2) r2 = dev_alloc(c, owned, ((size_t)2 * d * d + d) * 4, (void**)&p);
        if (!r2) {
            hipError_t e = hipMemcpy(p, w2t, (size_t)2 * d * d * 4, hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy(p + (size_t)2 * d * d, b2, (size_t)d * 4, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) r2 = fail(c, HG_ERR_HIP, "memcpy linear2 failed");
        }
        free_all(sc);
        if (r2) return r2;
        dl[11] = p;
    }
    return rc ? (rc < 0 ? rc : HG_ERR_INVALID) : HG_OK;
}

int load_adapters(hg_ctx* c, const hg_adapter_weights* src, int layers) {
    Vit& v = c->vit;
    free_all(v.owned_adapters);
    v.adapters.assign(v.layers, AdapterW{});
    if (!src) return HG_OK;
    if (layers != v.layers) return fail(c, HG_ERR_INVALID, "adapter layer count %d != %d", layers, v.layers);
    const int D = v.D;
    for (int i = 0; i < layers; ++i) {
        const hg_adapter_weights& s = src[i];
        if (!s.present) continue;
        if (s.bottleneck != 64) return fail(c, HG_ERR_INVALID, "adapter bottleneck must be 64 (got %d)", s.bottleneck);
        AdapterW& a = v.adapters[i];
        const int d = 64;
        a.d = d;
        std::vector<void*>& own = v.owned_adapters;
        // down_proj padded to 128 output rows (the GEMM tile is 128 wide); rows 64.. are zero
        void* p;
        int rc = dev_alloc(c, own, (size_t)128 * D * 2, &p);
        if (rc) return rc;
        HG_HIP(hipMemset(p, 0, (size_t)128 * D * 2));
        a.down_w = (half_t*)p;
        if (!s.down_proj_weight.ptr) return fail(c, HG_ERR_INVALID, "missing adapter down_proj.weight");
        if (s.down_proj_weight.dtype == HG_F16)
            HG_HIP(hipMemcpy(p, s.down_proj_weight.ptr, (size_t)d * D * 2, hipMemcpyDeviceToDevice));
        else HG_HIP(launch_f32_to_f16((const float*)s.down_proj_weight.ptr, a.down_w, (size_t)d * D, 0));
        rc = dev_alloc(c, own, 128 * 4, &p);
        if (rc) return rc;
        HG_HIP(hipMemset(p, 0, 128 * 4));
        a.down_b = (float*)p;
        {
            float* t;
            std::vector<void*> sc;
            rc = as_f32(c, sc, s.down_proj_bias, d, &t, "adapter down_proj.bias");
            if (!rc && hipMemcpy(p, t, d * 4, hipMemcpyDeviceToDevice) != hipSuccess) rc = HG_ERR_HIP;
            free_all(sc);
            if (rc) return rc;
        }
        {      // cs[n] = sum_k float(W16[n][k]) through the LayerNorm-folding helper with gamma = 1, beta = 0
            std::vector<float> ones(D, 1.0f), zeros(D, 0.0f);
            std::vector<void*> sc;
            float *g1 = nullptr, *b0 = nullptr, *bf = nullptr;
            half_t* wf = nullptr;
            int r2 = upload_f32(c, sc, ones, &g1);
            if (!r2) r2 = upload_f32(c, sc, zeros, &b0);
            if (!r2) r2 = dev_alloc(c, sc, (size_t)128 * D * 2, (void**)&wf);
            if (!r2) r2 = dev_alloc(c, sc, 128 * 4, (void**)&bf);
            if (!r2) r2 = dev_alloc(c, own, 128 * 4, (void**)&a.down_cs);
            if (!r2) {
                hipError_t e = launch_fold_ln(a.down_w, g1, b0, a.down_b, wf, a.down_cs, bf, 128, D, 0);
                if (e == hipSuccess) e = hipDeviceSynchronize();
                if (e != hipSuccess) r2 = fail(c, HG_ERR_HIP, "down_proj row sums failed: %s", hipGetErrorString(e));
            }
            free_all(sc);
            if (r2) return r2;
        }
        keep_first(rc, as_f16(c, own, s.up_proj_weight, (size_t)D * d, &a.up_w, "adapter up_proj.weight"));
        keep_first(rc, as_f32(c, own, s.up_proj_bias, D, &a.up_b, "adapter up_proj.bias"));
        keep_first(rc, as_f32(c, own, s.scale, D, &a.scale, "adapter scale"));
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
        if (v.lo_scale && s.up_proj_weight.dtype == HG_F32) {      // up_proj as hi + lo (hg_load_vit)
            std::vector<float> sc_lo;
            rc = to_host_f32(c, s.scale, D, sc_lo, "adapter scale");
            for (float& f : sc_lo) f *= 1.0f / 2048.0f;
            if (!rc) rc = upload_f32(c, own, sc_lo, &a.scale_lo);
            if (!rc) rc = dev_alloc(c, own, (size_t)D * d * 2, (void**)&a.up_w_lo);
            if (!rc && launch_f16_remainder((const float*)s.up_proj_weight.ptr, a.up_w_lo, (size_t)D * d, 0) != hipSuccess)
                rc = fail(c, HG_ERR_HIP, "splitting adapter up_proj.weight into hi + lo failed");
            if (rc) return rc;
        }
        rc = load_decoder_layer(c, own, s.prior_layer, d, a.dl[0], a.w16[0]);
        if (rc) return rc;
        rc = load_decoder_layer(c, own, s.self_layer, d, a.dl[1], a.w16[1]);
        if (rc) return rc;
        if (s.n_extra_prior_layers < 0 || (s.n_extra_prior_layers > 0 && !s.extra_prior_layers))
            return fail(c, HG_ERR_INVALID, "adapter %d: bad extra_prior_layers", i);
        a.extra.resize(s.n_extra_prior_layers);
        for (int z = 0; z < s.n_extra_prior_layers; ++z) {
            rc = load_decoder_layer(c, own, s.extra_prior_layers[z], d, a.extra[z].dl, a.extra[z].w16);
            if (rc) return rc;
        }
        // (the adapter is folded into the block's GEMMs on towers of at most 224 tokens only: a longer one packs no folded operands)
        if (v.L <= ADAPTER_MAX_L && (int)v.blocks.size() > i && v.blocks[i].w_out && v.blocks[i].wf_qkv) {
            std::vector<void*> sc;
            float* q32 = nullptr;
            keep_first(rc, dev_alloc(c, sc, (size_t)D * d * 4, (void**)&q32));
            for (int k = 0; k < 2 && !rc; ++k) {
                AdapterW::Fold& f = a.fold[k];
                keep_first(rc, dev_alloc(c, own, (size_t)128 * D * 2, (void**)&f.down2));
                keep_first(rc, dev_alloc(c, own, (size_t)D * (D + d) * 2, (void**)&f.wk_out));
                keep_first(rc, dev_alloc(c, own, (size_t)3 * D * (D + d) * 2, (void**)&f.wq_cat));
                keep_first(rc, dev_alloc(c, own, (size_t)d * d * 2, (void**)&f.g16));
                keep_first(rc, dev_alloc(c, own, (size_t)d * 4, (void**)&f.qm));
                if (rc) break;
                const float* norms = k == 0 ? (a.extra.empty() ? a.dl[0][8] : a.extra.back().dl[8]) : a.dl[1][8];
                hipError_t e = launch_adapter_fold(a.up_w, a.up_b, a.scale, norms, a.down_w, v.blocks[i].w_out, v.blocks[i].wf_qkv, D,
                                                   q32, f.down2, f.wk_out, f.wq_cat, f.qm, f.g16, 0);
                if (e == hipSuccess && d == 64 && qkv_attn_ok(1, 197, D, D / 64, D + 64, D + 64)) {
                    keep_first(rc, dev_alloc(c, own, (size_t)3 * D * (D + d) * 2, (void**)&f.wp_qcat));
                    if (rc) break;
                    e = launch_pack_qkv(f.wq_cat, nullptr, nullptr, f.wp_qcat, nullptr, D, D / 64, 0, D + 64);
                }
                if (e == hipSuccess) e = hipDeviceSynchronize();
                if (e != hipSuccess) rc = fail(c, HG_ERR_HIP, "adapter fold failed: %s", hipGetErrorString(e));
            }
            free_all(sc);
            if (rc) return rc;
        }
        a.present = true;
    }
    HG_HIP(hipDeviceSynchronize());
    return HG_OK;
}

}  // namespace

// Option qkv_attn_text: the in_proj operands of the text tower's blocks in the fused kernel's fragment order (hg_qkv_attn_text.hip),
// packed on the first text call that runs with the option on and only in the form that call's text_ln_fold needs (gamma: the layer's
// own w_qkv with csg_qkv; else wf_qkv with cs_qkv) - 3 D^2 x 2 bytes per block and form (18.9 MB for the 12 blocks of D = 512); with
// the option at 0 nothing is allocated.
int hg_host::ensure_text_packs(hg_ctx* c, std::vector<void*>& owned, std::vector<BlockW>& blocks, int D, bool gamma) {
    if (!qkv_attn_text_ok(1, 77, D, D / 64, D)) return HG_OK;
    bool packed = false;
    for (BlockW& b : blocks) {
        half_t*& wp = gamma ? b.wpg_qkv : b.wp_qkv;
        float*& bcs = gamma ? b.bcsg_qkv : b.bcs_qkv;
        if (wp) continue;
        if (!b.wf_qkv) return HG_OK;      // (loaded without the folded operands: the option does not apply)
        int rc = 0;
        half_t* wp_new = nullptr;
        keep_first(rc, dev_alloc(c, owned, (size_t)3 * D * D * 2, (void**)&wp_new));
        keep_first(rc, dev_alloc(c, owned, (size_t)(D / 128) * 768 * 4, (void**)&bcs));
        if (rc) return rc < 0 ? rc : HG_ERR_OOM;
        HG_HIP(launch_pack_qkv(gamma ? b.w_qkv : b.wf_qkv, b.bf_qkv, gamma ? b.csg_qkv : b.cs_qkv, wp_new, bcs, D, D / 64, 0));
        wp = wp_new;
        packed = true;
    }
    if (packed) HG_HIP(hipStreamSynchronize(0));      // (packed on the null stream, as at load time; the call's stream may be any)
    return HG_OK;
}

extern "C" {

int hg_load_vit(hg_ctx* c, const hg_vit_weights* w) {
    if (!c || !w) return HG_ERR_INVALID;
    HG_ON_DEVICE(c);
    Vit& v = c->vit;
    free_all(v.owned);
    free_all(v.owned_adapters);
    v = Vit{};
    const int D = w->width, p = w->patch_size;
    if (D <= 0 || D % 128 || w->heads * 64 != D)
        return fail(c, HG_ERR_INVALID, "vision width must be a multiple of 128 with heads = width/64 (got %d, %d)", D,
                    w->heads);
    if (p <= 0 || w->input_resolution <= 0 || w->input_resolution % p)
        return fail(c, HG_ERR_INVALID, "unsupported patch size %d / resolution %d (the resolution must be a multiple of the patch size)", p,
                    w->input_resolution);
    if (w->output_dim <= 0 || w->output_dim % 128)
        return fail(c, HG_ERR_INVALID, "output_dim must be a multiple of 128 (got %d)", w->output_dim);
    v.D = D; v.layers = w->layers; v.heads = w->heads; v.patch = p; v.res = w->input_resolution;
    // Kp: the patch GEMM's K = 3 p p rounded up to its 64-column step (p = 14: 588 -> 640; p % 8 == 0 needs no padding).  The weight's
    // pad columns are zero, the patch matrix's are written as zeros on every call (launch_im2col)
    v.grid = v.res / p; v.L = v.grid * v.grid + 1; v.E = w->output_dim; v.Kp = im2col_kp(p);
    if (v.L > ATTN_LONG_MAX_L)
        return fail(c, HG_ERR_INVALID, "at most %d tokens per image supported (got %d)", ATTN_LONG_MAX_L, v.L);
    if (v.L > adapter_max_tokens(c))
        for (int i = 0; w->adapters && i < w->layers; ++i)
            if (w->adapters[i].present)
                return fail(c, HG_ERR_INVALID, "instance adapters support at most %d tokens per image: this tower has %d (patch %d, resolution "
                                               "%d); load it without adapter weights (use_adapter=False)%s", adapter_max_tokens(c), v.L, p, v.res,
                            adapter_long_hint(c, v.L));
    int rc = 0;
    const int K0 = 3 * p * p;
    if (v.Kp == K0) {
        keep_first(rc, as_f16(c, v.owned, w->conv1_weight, (size_t)D * v.Kp, &v.w_patch, "visual.conv1.weight"));
    } else {
        std::vector<void*> sc;
        half_t* dense = nullptr;
        void* padded = nullptr;
        int r2 = as_f16(c, sc, w->conv1_weight, (size_t)D * K0, &dense, "visual.conv1.weight");
        if (!r2) r2 = dev_alloc(c, v.owned, (size_t)D * v.Kp * 2, &padded);
        if (!r2) {
            hipError_t e = hipMemset(padded, 0, (size_t)D * v.Kp * 2);
            if (e == hipSuccess) e = hipDeviceSynchronize();      // (the conversion ran on the null stream)
            if (e == hipSuccess)
                e = hipMemcpy2D(padded, (size_t)v.Kp * 2, dense, (size_t)K0 * 2, (size_t)K0 * 2, D, hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) r2 = fail(c, HG_ERR_HIP, "padding visual.conv1.weight failed: %s", hipGetErrorString(e));
        }
        free_all(sc);
        v.w_patch = (half_t*)padded;
        keep_first(rc, r2);
    }
    keep_first(rc, as_f32(c, v.owned, w->class_embedding, D, &v.cls, "visual.class_embedding"));
    keep_first(rc, as_f32(c, v.owned, w->positional_embedding, (size_t)v.L * D, &v.pos, "visual.positional_embedding"));
    keep_first(rc, as_f32(c, v.owned, w->ln_pre_weight, D, &v.lnpre_w, "visual.ln_pre.weight"));
    keep_first(rc, as_f32(c, v.owned, w->ln_pre_bias, D, &v.lnpre_b, "visual.ln_pre.bias"));
    keep_first(rc, as_f32(c, v.owned, w->ln_post_weight, D, &v.lnpost_w, "visual.ln_post.weight"));
    keep_first(rc, as_f32(c, v.owned, w->ln_post_bias, D, &v.lnpost_b, "visual.ln_post.bias"));
    keep_first(rc, as_f16_T(c, v.owned, w->proj, D, v.E, &v.w_projT, "visual.proj"));
    // Variant C of the reference keeps proj in fp32 (CLIP_models_adapter_prior2.py:980 converts nothing); its local map is summed over
    // hundreds of tokens by its users (RoI pooling), which weighs the fp16 rounding of a proj column as often: measured on the 576
    // tokens of ViT-L/14@336px, proj's rounding alone moves the map's sum by 9e-4.  Towers that only this head serves in variant C
    // (more tokens than the adapters take) therefore get proj as hi + lo: a second GEMM pass over 2^11 x fp16(W - hi), scaled back in
    // its epilogue (the remainder itself would sit in fp16's subnormals).  Towers of up to 224 tokens keep their one pass and their bits.
    if (!rc && v.L > ADAPTER_MAX_L && w->proj.dtype == HG_F32) {
        std::vector<void*> sc;
        float* p32 = nullptr;
        int r2 = as_f32(c, sc, w->proj, (size_t)D * v.E, &p32, "visual.proj");
        std::vector<float> host((size_t)D * v.E);
        if (!r2 && hipMemcpy(host.data(), p32, host.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) r2 = HG_ERR_HIP;
        free_all(sc);
        if (!r2) {
            std::vector<half_t> lo((size_t)v.E * D);
            for (int d = 0; d < D; ++d)
                for (int e = 0; e < v.E; ++e) {
                    const float x = host[(size_t)d * v.E + e];
                    lo[(size_t)e * D + d] = (half_t)((x - (float)(half_t)x) * 2048.0f);
                }
            std::vector<float> sb((size_t)2 * v.E, 0.f);
            for (int e = 0; e < v.E; ++e) sb[e] = 1.0f / 2048.0f;
            void *plo = nullptr, *psb = nullptr;
            r2 = dev_alloc(c, v.owned, lo.size() * 2, &plo);
            if (!r2) r2 = dev_alloc(c, v.owned, sb.size() * 4, &psb);
            if (!r2 && (hipMemcpy(plo, lo.data(), lo.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(psb, sb.data(), sb.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
                r2 = HG_ERR_HIP;
            if (!r2) { v.w_projT_lo = (half_t*)plo; v.proj_lo_scale = (float*)psb; }
        }
        if (r2) return fail(c, r2 < 0 ? r2 : HG_ERR_INVALID, "splitting visual.proj into hi + lo failed");
    }
    if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
    rc = load_blocks(c, v.owned, w->blocks, v.layers, D, v.blocks, true);
    if (rc) return rc;
    // The same remedy as proj's above where instance adapters run on such a tower (option adapter_long): the two GEMMs that write
    // the residual stream from an operand with a mean far from zero - c_proj (QuickGELU's output) and the adapter's up_proj (a
    // LayerNorm output with its bias) - get their weight as hi + lo.  The rounding of a weight column times the operand's mean is
    // common to all tokens: of the 1.9e-3 by which fp16 weights move the sum of the local map of ViT-L/14@336px with adapters (fp32
    // oracle, the sequence as memory), c_proj's rounding alone is 1.1e-3 and up_proj's 5e-4; in_proj, c_fc and out_proj together
    // 3.5e-4.  Calls without adapters do not run the extra pass and keep their bits.
    if (v.L > ADAPTER_MAX_L) {
        std::vector<float> sb((size_t)2 * D, 0.f);
        for (int d = 0; d < D; ++d) sb[d] = 1.0f / 2048.0f;
        rc = upload_f32(c, v.owned, sb, &v.lo_scale);
        for (int i = 0; i < v.layers && !rc; ++i) {
            const hg_tensor& t = w->blocks[i].c_proj_weight;
            if (t.dtype != HG_F32) continue;
            rc = dev_alloc(c, v.owned, (size_t)4 * D * D * 2, (void**)&v.blocks[i].w_proj_lo);
            if (!rc && launch_f16_remainder((const float*)t.ptr, v.blocks[i].w_proj_lo, (size_t)4 * D * D, 0) != hipSuccess)
                rc = fail(c, HG_ERR_HIP, "splitting mlp.c_proj.weight into hi + lo failed");
        }
        if (rc) return rc < 0 ? rc : HG_ERR_OOM;
    }
    rc = load_adapters(c, w->adapters, v.layers);
    if (rc) return rc;
    HG_HIP(hipDeviceSynchronize());
    v.loaded = true;
    return HG_OK;
}

int hg_update_adapters(hg_ctx* c, const hg_adapter_weights* adapters, int layers) {
    if (!c) return HG_ERR_INVALID;
    if (!c->vit.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_vit first");
    if (c->vit.L > adapter_max_tokens(c))
        for (int i = 0; adapters && i < layers; ++i)
            if (adapters[i].present)
                return fail(c, HG_ERR_INVALID, "instance adapters support at most %d tokens per image: this tower has %d%s", adapter_max_tokens(c),
                            c->vit.L, adapter_long_hint(c, c->vit.L));
    HG_ON_DEVICE(c);
    HG_HIP(hipDeviceSynchronize());
    return load_adapters(c, adapters, layers);
}

int hg_load_text(hg_ctx* c, const hg_text_weights* w) {
    if (!c || !w) return HG_ERR_INVALID;
    HG_ON_DEVICE(c);
    Text& t = c->text;
    free_all(t.owned);
    free_all(t.owned_grad);
    t = Text{};
    const int D = w->width;
    if (D <= 0 || D % 128 || w->heads * 64 != D)
        return fail(c, HG_ERR_INVALID, "text width must be a multiple of 128 with heads = width/64 (got %d, %d)", D,
                    w->heads);
    if (w->context_length > 224) return fail(c, HG_ERR_INVALID, "context_length > 224 unsupported");
    if (w->output_dim <= 0 || w->output_dim % 128) return fail(c, HG_ERR_INVALID, "output_dim %% 128 != 0");
    t.D = D; t.layers = w->layers; t.heads = w->heads; t.ctx = w->context_length; t.vocab = w->vocab_size;
    t.E = w->output_dim;
    int rc = 0;
    keep_first(rc, as_f32(c, t.owned, w->token_embedding, (size_t)t.vocab * D, &t.tok, "token_embedding.weight"));
    keep_first(rc, as_f32(c, t.owned, w->positional_embedding, (size_t)t.ctx * D, &t.pos, "positional_embedding"));
    keep_first(rc, as_f32(c, t.owned, w->ln_final_weight, D, &t.lnf_w, "ln_final.weight"));
    keep_first(rc, as_f32(c, t.owned, w->ln_final_bias, D, &t.lnf_b, "ln_final.bias"));
    keep_first(rc, as_f16_T(c, t.owned, w->text_projection, D, t.E, &t.w_projT, "text_projection"));
    if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
    rc = load_blocks(c, t.owned, w->blocks, t.layers, D, t.blocks, true);      // (folded operands too: option text_ln_fold)
    if (rc) return rc;
    HG_HIP(hipDeviceSynchronize());
    t.loaded = true;
    return HG_OK;
}

int hg_load_vae(hg_ctx* c, int slot, const hg_vae_weights* w) {
    if (!c || !w || slot < 0 || slot >= HG_MAX_SLOTS) return HG_ERR_INVALID;
    HG_ON_DEVICE(c);
    Vae& v = c->vae[slot];
    free_all(v.owned);
    v = Vae{};
    v.dim = w->dim; v.eh = w->enc_hidden; v.gh = w->gen_hidden;
    if (v.dim <= 0 || v.dim % 128) return fail(c, HG_ERR_INVALID, "vae dim must be a multiple of 128");
    int rc = 0;
    if (w->enc_w0.ptr) {
        if (v.eh <= 0 || v.eh % 128) return fail(c, HG_ERR_INVALID, "enc_hidden must be a multiple of 128");
        keep_first(rc, as_f16(c, v.owned, w->enc_w0, (size_t)v.eh * v.dim, &v.e_w0, "Encoder.net.0.weight"));
        keep_first(rc, as_f32(c, v.owned, w->enc_b0, v.eh, &v.e_b0, "Encoder.net.0.bias"));
        // mean | log_var stacked into one [2*dim, eh] GEMM operand
        void* p;
        keep_first(rc, dev_alloc(c, v.owned, (size_t)2 * v.dim * v.eh * 2, &p));
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
        v.e_wml = (half_t*)p;
        std::vector<void*> sc;
        half_t *m, *l;
        keep_first(rc, as_f16(c, sc, w->enc_mean_w, (size_t)v.dim * v.eh, &m, "Encoder.mean.weight"));
        keep_first(rc, as_f16(c, sc, w->enc_logvar_w, (size_t)v.dim * v.eh, &l, "Encoder.log_var.weight"));
        if (!rc) {
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(v.e_wml, m, (size_t)v.dim * v.eh * 2, hipMemcpyDeviceToDevice);
            (void)hipMemcpy(v.e_wml + (size_t)v.dim * v.eh, l, (size_t)v.dim * v.eh * 2, hipMemcpyDeviceToDevice);
        }
        free_all(sc);
        keep_first(rc, dev_alloc(c, v.owned, (size_t)2 * v.dim * 4, &p));
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
        v.e_bml = (float*)p;
        float *bm, *bl;
        keep_first(rc, as_f32(c, sc, w->enc_mean_b, v.dim, &bm, "Encoder.mean.bias"));
        keep_first(rc, as_f32(c, sc, w->enc_logvar_b, v.dim, &bl, "Encoder.log_var.bias"));
        if (!rc) {
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(v.e_bml, bm, (size_t)v.dim * 4, hipMemcpyDeviceToDevice);
            (void)hipMemcpy(v.e_bml + v.dim, bl, (size_t)v.dim * 4, hipMemcpyDeviceToDevice);
        }
        free_all(sc);
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
        v.enc = true;
    }
    if (w->gen_w0.ptr) {
        if (v.gh <= 0 || v.gh % 128) return fail(c, HG_ERR_INVALID, "gen_hidden must be a multiple of 128");
        keep_first(rc, as_f16(c, v.owned, w->gen_w0, (size_t)v.gh * v.dim, &v.g_w0, "Generator.net.0.weight"));
        keep_first(rc, as_f32(c, v.owned, w->gen_b0, v.gh, &v.g_b0, "Generator.net.0.bias"));
        keep_first(rc, as_f16(c, v.owned, w->gen_w2, (size_t)v.dim * v.gh, &v.g_w2, "Generator.net.2.weight"));
        keep_first(rc, as_f32(c, v.owned, w->gen_b2, v.dim, &v.g_b2, "Generator.net.2.bias"));
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
        v.gen = true;
    }
    // the one-kernel path's operand: the same fp16 weights as a linear stream of MFMA fragments in order of use
    if (vae_fused_ok(v.dim, v.enc ? v.eh : 0, v.gen ? v.gh : 0)) {
        const size_t bytes = (v.enc ? 2 * vae_fused_pass_bytes(v.eh) : 0) + (v.gen ? vae_fused_pass_bytes(v.gh) : 0);
        void* p;
        rc = dev_alloc(c, v.owned, bytes, &p);
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
        v.wp = (half_t*)p;
        HG_HIP(launch_pack_vae(v.enc ? v.e_w0 : nullptr, v.e_wml, v.eh, v.gen ? v.g_w0 : nullptr, v.g_w2, v.gh, v.wp, nullptr));
    }
    HG_HIP(hipDeviceSynchronize());
    return HG_OK;
}

int hg_load_mlp(hg_ctx* c, int slot, const hg_mlp_weights* w) {
    if (!c || !w || slot < 0 || slot >= HG_MAX_SLOTS) return HG_ERR_INVALID;
    HG_ON_DEVICE(c);
    Mlp& m = c->mlp[slot];
    free_all(m.owned);
    m = Mlp{};
    m.in = w->in_dim; m.hid = w->hidden_dim; m.out = w->out_dim;
    if (m.in % 64 || m.hid % 128 || m.out % 128 || m.in <= 0) return fail(c, HG_ERR_INVALID, "mlp_net dims must be multiples of 128");
    int rc = 0;
    keep_first(rc, as_f16(c, m.owned, w->w0, (size_t)m.hid * m.in, &m.w0, "mlp.net.0.weight"));
    keep_first(rc, as_f32(c, m.owned, w->b0, m.hid, &m.b0, "mlp.net.0.bias"));
    keep_first(rc, as_f16(c, m.owned, w->w2, (size_t)m.hid * m.hid, &m.w2, "mlp.net.2.weight"));
    keep_first(rc, as_f32(c, m.owned, w->b2, m.hid, &m.b2, "mlp.net.2.bias"));
    keep_first(rc, as_f16(c, m.owned, w->w4, (size_t)m.out * m.hid, &m.w4, "mlp.net.4.weight"));
    keep_first(rc, as_f32(c, m.owned, w->b4, m.out, &m.b4, "mlp.net.4.bias"));
    if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
    HG_HIP(hipDeviceSynchronize());
    m.loaded = true;
    return HG_OK;
}

int hg_load_cache(hg_ctx* c, int slot, const hg_cache_weights* w) {
    if (!c || !w || slot < 0 || slot >= HG_MAX_CACHE_SLOTS) return HG_ERR_INVALID;
    HG_ON_DEVICE(c);
    Cache& m = c->cache[slot];
    free_all(m.owned);
    m = Cache{};
    m.S = w->S; m.K = w->K; m.C = w->C; m.has_labels = w->labels.ptr != nullptr;
    if (m.S <= 0 || m.K <= 0 || m.K % 64 || (m.has_labels && m.C <= 0))
        return fail(c, HG_ERR_INVALID, "cache model: S > 0, K %% 64 == 0 (got S=%d K=%d C=%d)", m.S, m.K, m.C);
    m.Sp = (int)rup(m.S, 128);
    m.Cp = m.has_labels ? (int)rup(m.C, 128) : 0;
    // weight rows padded with zeros to a multiple of 128 (the GEMM's N granularity)
    int rc = dev_alloc(c, m.owned, (size_t)m.Sp * m.K * 2, (void**)&m.w16);
    if (rc) return rc;
    HG_HIP(hipMemset(m.w16, 0, (size_t)m.Sp * m.K * 2));
    if (!w->weight.ptr) return fail(c, HG_ERR_INVALID, "missing tensor cache weight");
    if (w->weight.dtype == HG_F16) HG_HIP(hipMemcpy(m.w16, w->weight.ptr, (size_t)m.S * m.K * 2, hipMemcpyDeviceToDevice));
    else HG_HIP(launch_f32_to_f16((const float*)w->weight.ptr, m.w16, (size_t)m.S * m.K, 0));
    std::vector<float> bias(m.Sp, 0.f);
    if (w->bias.ptr) {
        std::vector<float> b;
        rc = to_host_f32(c, w->bias, m.S, b, "cache bias");
        if (rc) return rc;
        for (int i = 0; i < m.S; ++i) bias[i] = b[i];
    }
    if (!m.has_labels) {
        rc = upload_f32(c, m.owned, bias, &m.b);
        if (rc) return rc;
    } else {
        // (f W^T + b) L / lens / post_div = ((f W^T) L + b L) * scale: the bias term is a per-class constant
        // (kept in fp32; phi = f W^T alone goes through fp16 for the second MFMA GEMM)
        std::vector<float> lab, lens;
        rc = to_host_f32(c, w->labels, (size_t)m.S * m.C, lab, "cache labels");
        if (!rc) rc = to_host_f32(c, w->sample_lens, m.C, lens, "cache sample_lens");
        if (rc) return rc;
        std::vector<float> lt((size_t)m.Cp * m.Sp, 0.f), bc(m.Cp, 0.f), sc(m.Cp, 0.f);
        for (int cc = 0; cc < m.C; ++cc) {
            double acc = 0.0;
            for (int i = 0; i < m.S; ++i) {
                const float v = lab[(size_t)i * m.C + cc];
                lt[(size_t)cc * m.Sp + i] = v;
                acc += (double)bias[i] * v;
            }
            bc[cc] = (float)acc;
            sc[cc] = 1.0f / (lens[cc] * (w->post_div != 0.f ? w->post_div : 1.f));
        }
        float* lt32 = nullptr;
        std::vector<void*> scratch;
        rc = upload_f32(c, scratch, lt, &lt32);
        if (!rc) rc = dev_alloc(c, m.owned, lt.size() * 2, (void**)&m.lt16);
        if (!rc) { hipError_t e = launch_f32_to_f16(lt32, m.lt16, lt.size(), 0); if (e != hipSuccess) rc = HG_ERR_HIP; }
        if (!rc) { hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) rc = HG_ERR_HIP; }
        free_all(scratch);
        if (!rc) rc = upload_f32(c, m.owned, bc, &m.bias_c);
        if (!rc) rc = upload_f32(c, m.owned, sc, &m.scale);
        if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
    }
    HG_HIP(hipDeviceSynchronize());
    m.loaded = true;
    return HG_OK;
}

// priors_downproj + object_embedding (hg_region_props.hip).  A second call on a loaded slot is the update path: everything is rebuilt,
// the table T included.
int hg_load_priors(hg_ctx* c, int slot, const hg_prior_weights* w) {
    if (!c) return HG_ERR_INVALID;
    if (!w || slot < 0 || slot >= HG_MAX_PRIOR_SLOTS) return fail(c, HG_ERR_INVALID, "hg_load_priors: slot %d (0 .. %d) / no weights", slot, HG_MAX_PRIOR_SLOTS - 1);
    if (w->E <= 0 || w->E > PROPS_MAX_E || w->hidden <= 0 || w->hidden > PROPS_MAX_HID || w->out != PROPS_OUT || w->n_obj_classes <= 0 ||
        w->n_obj_classes > PROPS_MAX_CLASSES)
        return fail(c, HG_ERR_INVALID, "hg_load_priors: E = %d, hidden = %d, out = %d, %d classes (E <= %d, hidden <= %d, out == %d, classes <= %d)",
                    w->E, w->hidden, w->out, w->n_obj_classes, PROPS_MAX_E, PROPS_MAX_HID, PROPS_OUT, PROPS_MAX_CLASSES);
    HG_ON_DEVICE(c);
    HG_HIP(hipDeviceSynchronize());      // (an update: no call in flight still reads the slot)
    Priors& m = c->prior[slot];
    free_all(m.owned);
    m = Priors{};
    m.E = w->E; m.hid = w->hidden; m.n_classes = w->n_obj_classes;
    const int K0 = m.E + 5, hid = m.hid;
    std::vector<void*> scratch;
    float *w0 = nullptr, *w1 = nullptr, *w2 = nullptr, *emb = nullptr;
    int rc = 0;
    keep_first(rc, as_f32(c, scratch, w->w0, (size_t)hid * K0, &w0, "priors_downproj.layers.0.weight"));
    keep_first(rc, as_f32(c, scratch, w->w1, (size_t)hid * hid, &w1, "priors_downproj.layers.1.weight"));
    keep_first(rc, as_f32(c, scratch, w->w2, (size_t)PROPS_OUT * hid, &w2, "priors_downproj.layers.2.weight"));
    keep_first(rc, as_f32(c, scratch, w->object_embedding, (size_t)m.n_classes * m.E, &emb, "object_embedding"));
    keep_first(rc, as_f32(c, m.owned, w->b0, hid, &m.b0, "priors_downproj.layers.0.bias"));
    keep_first(rc, as_f32(c, m.owned, w->b1, hid, &m.b1, "priors_downproj.layers.1.bias"));
    keep_first(rc, as_f32(c, m.owned, w->b2, PROPS_OUT, &m.b2, "priors_downproj.layers.2.bias"));
    keep_first(rc, dev_alloc(c, m.owned, (size_t)K0 * hid * 4, (void**)&m.w0t));
    keep_first(rc, dev_alloc(c, m.owned, (size_t)hid * hid * 4, (void**)&m.w1t));
    keep_first(rc, dev_alloc(c, m.owned, (size_t)hid * PROPS_OUT * 4, (void**)&m.w2t));
    keep_first(rc, dev_alloc(c, m.owned, (size_t)m.n_classes * hid * 4, (void**)&m.T));
    hipError_t e = hipSuccess;
    if (!rc) e = launch_prior_pack(w0, hid, K0, m.w0t, 0);
    if (!rc && e == hipSuccess) e = launch_prior_pack(w1, hid, hid, m.w1t, 0);
    if (!rc && e == hipSuccess) e = launch_prior_pack(w2, PROPS_OUT, hid, m.w2t, 0);
    if (!rc && e == hipSuccess) e = launch_prior_table(emb, m.w0t, m.n_classes, m.E, hid, m.T, 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    free_all(scratch);
    if (rc) return rc < 0 ? rc : HG_ERR_INVALID;
    if (e != hipSuccess) return fail(c, HG_ERR_HIP, "hg_load_priors: %s", hipGetErrorString(e));
    m.loaded = true;
    return HG_OK;
}

}  // extern "C"
