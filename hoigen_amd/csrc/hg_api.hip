// C ABI of hoigen_amd (include/hoigen_amd.h): the context, its options, profiler and workspace report, and the small entry points.
// The weights: hg_load.hip; the towers: hg_tower.hip; VAE / mlp_net / cache logits: hg_heads.hip; test hooks: hg_test_hooks.hip.
// Host code only; kernels live in hg_gemm*.hip / hg_attn*.hip / hg_elem.hip / hg_adapter.hip / ...
#include <limits.h>

#include "hg_host.h"
#include "hg_preproc_geom.h"

namespace {

// Every behaviour option, once: its key (hg_set_option / hg_get_option), the environment variable that gives its value at hg_create,
// where it lives and what it accepts: a switch (any value != 0 sets 1), or lo .. hi with `want`, the range as the refusal words it
// (say_got: the refusal also names the value it got)
struct Option { const char *key, *env; int hg_ctx::*member; bool is_switch; int lo = 0, hi = 1; const char* want = nullptr; bool say_got = true; };
const Option OPTIONS[] = {
    {"chunk_rows", "HG_CHUNK_ROWS", &hg_ctx::max_chunk_rows, false, 256, INT_MAX, ">= 256", false},      // rows per VAE / mlp_net / cache-logits chunk
    {"last_block_row0", "HG_LAST_BLOCK_ROW0", &hg_ctx::opt_row0, true},
    {"ln_fuse", "HG_LN_FUSE", &hg_ctx::opt_ln_fuse, true},
    {"adapter_fuse", "HG_ADAPTER_FUSE", &hg_ctx::opt_adapter_fuse, true},
    {"adapter_fold", "HG_ADAPTER_FOLD", &hg_ctx::opt_adapter_fold, true},
    {"stream_hilo", "HG_STREAM_HILO", &hg_ctx::opt_stream_hilo, true},
    {"adapter_long", "HG_ADAPTER_LONG", &hg_ctx::opt_adapter_long, true},
    {"qkv_attn", "HG_QKV_ATTN", &hg_ctx::opt_qkv_attn, false, 0, 2, "0, 1 or 2"},
    {"qkv_attn_text", "HG_QKV_ATTN_TEXT", &hg_ctx::opt_qkv_attn_text, false, 0, 2, "0, 1 or 2"},
    {"qkv_attn_min_seq", "HG_QKV_ATTN_MIN_SEQ", &hg_ctx::opt_qkv_attn_min_seq, false, 1, INT_MAX, ">= 1"},
    {"qkv_attn_gsz", "HG_QKV_ATTN_GSZ", &hg_ctx::opt_qkv_attn_gsz, false, 0, 6, "0 .. 6"},
    {"qkv_attn_c", "HG_QKV_ATTN_C", &hg_ctx::opt_qkv_attn_c, false, 0, 1, "0 or 1"},
    {"text_ln_fold", "HG_TEXT_LN_FOLD", &hg_ctx::opt_text_ln_fold, false, 0, 2, "0, 1 or 2"},
    {"vae_fused", "HG_VAE_FUSED", &hg_ctx::opt_vae_fused, false, 0, 2, "0, 1 or 2"},
    {"mlp_pair", "HG_MLP_PAIR", &hg_ctx::opt_mlp_pair, false, 0, 1, "0 or 1"},
    {"mlp_pair_chunk", "HG_MLP_PAIR_CHUNK", &hg_ctx::opt_mlp_pair_chunk, false, 1, 64, "1 .. 64"},
    {"mlp_pair_fc_slots", "HG_MLP_PAIR_FC_SLOTS", &hg_ctx::opt_mlp_pair_fc_slots, false, 1, 64, "1 .. 64"},
    {"mlp_pair256", "HG_MLP_PAIR256", &hg_ctx::opt_mlp_pair256, false, 0, 1, "0 or 1"},
    {"mlp_pair256_min_m", "HG_MLP_PAIR256_MIN_M", &hg_ctx::opt_mlp_pair256_min_m, false, 256, INT_MAX, ">= 256"},
    {"mlp_pair256_chunk", "HG_MLP_PAIR256_CHUNK", &hg_ctx::opt_mlp_pair256_chunk, false, 1, 64, "1 .. 64"},
    {"mlp_pair256_ratio", "HG_MLP_PAIR256_RATIO", &hg_ctx::opt_mlp_pair256_ratio, false, 1, 8, "1 .. 8"},
    {"mlp_pair256_ph2", "HG_MLP_PAIR256_PH2", &hg_ctx::opt_mlp_pair256_ph2, false, 0, 1, "0 or 1"},
    {"mlp_pair256_launches", "HG_MLP_PAIR256_LAUNCHES", &hg_ctx::n_pair256_launches, false, 0, INT_MAX, ">= 0"},      // (a counter: see the header)
    {"detr_attn_chunk", "HG_DETR_ATTN_CHUNK", &hg_ctx::opt_detr_attn_chunk, false, 0, 1280, "0 .. 1280 (a multiple of 32)"},
    {"detr_attn_waves", "HG_DETR_ATTN_WAVES", &hg_ctx::opt_detr_attn_waves, false, 0, 4, "0, 1, 2 or 4"},
    {"detr_ffn", "HG_DETR_FFN", &hg_ctx::opt_detr_ffn, false, 0, 2, "0, 1 or 2"},
    {"detr_ffn_max_m", "HG_DETR_FFN_MAX_M", &hg_ctx::opt_detr_ffn_max_m, false, 0, 1 << 20, "0 .. 2^20"},
    {"detr_neck_split", "HG_DETR_NECK_SPLIT", &hg_ctx::opt_detr_neck_split, false, 0, 64, "0 .. 64"},
    {"mlp_pair_fault", "HG_MLP_PAIR_FAULT", &hg_ctx::opt_mlp_pair_fault, false, 0, 1, "0 or 1"},
};
const Option* find_option(const char* key) {
    for (const Option& o : OPTIONS)
        if (!strcmp(o.key, key)) return &o;
    return nullptr;
}

}  // namespace

extern "C" {

const char* hg_version(void) { return "hoigen_amd 0.1 (gfx950)"; }

hg_ctx* hg_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return nullptr;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess) return nullptr;      // creates the primary context if needed
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    hg_ctx* c = new hg_ctx();
    c->device = device;
    {
        DevGuard g(c);
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) c->n_cu = ncu;
        if (hipHostMalloc((void**)&c->eot_flag, 64, hipHostMallocMapped) == hipSuccess && c->eot_flag) *c->eot_flag = 0;
        else c->eot_flag = nullptr;
        if (hipMalloc((void**)&c->eot_flag_dev, 64) != hipSuccess) c->eot_flag_dev = nullptr;
        else (void)hipMemset(c->eot_flag_dev, 0, 64);
        if (hipHostMalloc((void**)&c->pair_err, 64, hipHostMallocMapped) == hipSuccess && c->pair_err) *c->pair_err = 0;
        else c->pair_err = nullptr;
        if (hipHostMalloc((void**)&c->range_flag, 64, hipHostMallocMapped) == hipSuccess && c->range_flag) *c->range_flag = 0;
        else c->range_flag = nullptr;
    }
    for (const Option& o : OPTIONS)
        if (const char* e = getenv(o.env)) (void)hg_set_option(c, o.key, atoi(e));      // (out-of-range values are ignored)
    c->err.clear();
    return c;
}
int hg_set_option(hg_ctx* c, const char* key, int value) {
    if (!c || !key) return HG_ERR_INVALID;
    const Option* o = find_option(key);
    if (!o) return fail(c, HG_ERR_INVALID, "unknown option '%s'", key);
    if (!o->is_switch && (value < o->lo || value > o->hi)) return fail(c, HG_ERR_INVALID, o->say_got ? "%s must be %s (got %d)" : "%s must be %s", key, o->want, value);
    c->*(o->member) = o->is_switch ? value != 0 : value;
    return HG_OK;
}

int hg_get_option(hg_ctx* c, const char* key, int* value) {
    if (!c || !key || !value) return HG_ERR_INVALID;
    const Option* o = find_option(key);
    if (o) *value = c->*(o->member);
    else if (!strcmp(key, "stream_lo_bits")) *value = 8;      // read-only: the low half of the stream is bf8
    else return fail(c, HG_ERR_INVALID, "unknown option '%s'", key);
    return HG_OK;
}
void hg_destroy(hg_ctx* c) {
    if (!c) return;
    DevGuard dev_guard_(c);
    (void)hipDeviceSynchronize();
    free_all(c->vit.owned);
    free_all(c->vit.owned_adapters);
    free_all(c->text.owned);
    free_all(c->text.owned_grad);
    for (auto& v : c->vae) free_all(v.owned);
    for (auto& m : c->mlp) free_all(m.owned);
    for (auto& m : c->cache) free_all(m.owned);
    for (auto& m : c->prior) free_all(m.owned);
    free_all(c->detr.owned);
    free_all(c->detr_dec.owned);
    free_all(c->detr_heads.owned);
    free_all(c->detr_neck.owned);
    free_all(c->resnet.owned);
    free_all(c->resnet_stem.owned);
    Buf* bufs[] = HG_WORKSPACE_BUFS(c);
    for (Buf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->eot_flag) (void)hipHostFree(c->eot_flag);
    if (c->eot_flag_dev) (void)hipFree(c->eot_flag_dev);
    if (c->pair_err) (void)hipHostFree(c->pair_err);
    if (c->range_flag) (void)hipHostFree(c->range_flag);
    delete c;
}

const char* hg_last_error(hg_ctx* c) { return c ? c->err.c_str() : "null context"; }

int hg_preprocess_crops(hg_ctx* c, const uint8_t* img, int H, int W, const int32_t* boxes_host, int n, int n_px,
                        int pad_square, uint32_t background, float* out, uint8_t* out_u8, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (n == 0) return HG_OK;
    if (!img || !boxes_host || !out || n < 0 || H <= 0 || W <= 0 || n_px <= 0 || n_px > 4096)
        return fail(c, HG_ERR_INVALID, "hg_preprocess_crops: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    // host part: geometry of every crop (sizes, padding, resize target, centre-crop offsets, tap counts, the
    // source rows the vertical pass needs); the weight tables themselves are filled on the device
    std::vector<int32_t> head((size_t)n * (HG_PRE_HDR + 1), 0);      // headers, then the n table offsets
    int32_t* off = head.data() + (size_t)n * HG_PRE_HDR;
    size_t words = 0, tmp = 0;
    int max_rows = 0;
    for (int b = 0; b < n; ++b) {
        const int32_t* bx = boxes_host + 4 * (size_t)b;
        const int cw = bx[2] - bx[0], ch = bx[3] - bx[1];
        if (cw <= 0 || ch <= 0) return fail(c, HG_ERR_INVALID, "hg_preprocess_crops: empty box %d", b);
        int sw = cw, sh = ch, px = 0, py = 0;
        if ((pad_square & HG_PRE_PAD_SQUARE) && cw != ch) {                       // expand2square: centred, floor((side - short) / 2)
            if (cw > ch) py = (cw - ch) / 2; else px = (ch - cw) / 2;
            sw = sh = cw > ch ? cw : ch;
        }
        // torchvision Resize: short side -> n_px, long side -> int(n_px * long / short); CenterCrop offsets
        // int(round(d / 2.0)) with Python's round-half-to-even
        int nw, nh;
        if (pad_square & HG_PRE_STRETCH) { nw = nh = n_px; }        // IResize([n_px, n_px]): both sides, no centre crop
        else if (sw <= sh) { nw = n_px; nh = (int)((double)((long long)n_px * sh) / (double)sw); }
        else { nw = (int)((double)((long long)n_px * sw) / (double)sh); nh = n_px; }
        const int left = (int)nearbyint((double)(nw - n_px) / 2.0), top = (int)nearbyint((double)(nh - n_px) / 2.0);
        auto taps = [](int in, int outn) {
            const double sc = (double)in / (double)outn, fs = sc < 1.0 ? 1.0 : sc;
            return (int)ceil(2.0 * fs) * 2 + 1;
        };
        auto first_tap = [](int in, int outn, int idx) {
            const double sc = (double)in / (double)outn, fs = sc < 1.0 ? 1.0 : sc;
            const int v = (int)(((double)idx + 0.5) * sc - 2.0 * fs + 0.5);
            return v < 0 ? 0 : v;
        };
        auto end_tap = [](int in, int outn, int idx) {
            const double sc = (double)in / (double)outn, fs = sc < 1.0 ? 1.0 : sc;
            const int v = (int)(((double)idx + 0.5) * sc + 2.0 * fs + 0.5);
            return v > in ? in : v;
        };
        const int ks_h = taps(sw, nw), ks_v = taps(sh, nh);
        const int row_lo = first_tap(sh, nh, top), n_rows = end_tap(sh, nh, top + n_px - 1) - row_lo;
        if (tmp + (size_t)n_rows * n_px * 3 >= ((size_t)1 << 31))
            return fail(c, HG_ERR_INVALID, "hg_preprocess_crops: scratch of one call >= 2 GiB; split the boxes");
        int32_t* h = head.data() + (size_t)b * HG_PRE_HDR;
        h[0] = bx[0]; h[1] = bx[1]; h[2] = cw; h[3] = ch; h[4] = px; h[5] = py; h[6] = sw; h[7] = sh;
        h[8] = ks_h; h[9] = ks_v; h[10] = row_lo; h[11] = n_rows; h[12] = (int32_t)tmp; h[13] = (int32_t)background;
        h[14] = nw; h[15] = nh; h[16] = left; h[17] = top;
        off[b] = (int32_t)words;
        words += (size_t)n_px * (4 + ks_h + ks_v);
        tmp += ((size_t)n_rows * n_px * 3 + 15) / 16 * 16;
        if (n_rows > max_rows) max_rows = n_rows;
        if (words >= ((size_t)1 << 30)) return fail(c, HG_ERR_INVALID, "hg_preprocess_crops: too many boxes in one call");
    }
    int rc = ensure(c, c->pre, tmp ? tmp : 16);
    if (!rc) rc = ensure(c, c->pretab, (head.size() + words) * 4);
    if (rc) return rc;
    int32_t* head_d = (int32_t*)c->pretab.p;                          // [n][HG_PRE_HDR] | off[n] | tables
    int32_t* tab_off = head_d + (size_t)n * HG_PRE_HDR;
    int32_t* tab = tab_off + n;
    HG_HIP(hipMemcpyAsync(head_d, head.data(), head.size() * 4, hipMemcpyHostToDevice, s));
    HG_HIP(hipStreamSynchronize(s));      // `head` is a stack-lifetime host buffer
    HG_HIP(launch_preprocess(img, H, W, head_d, tab, tab_off, n, n_px, max_rows, (uint8_t*)c->pre.p, out, out_u8, s,
                             (pad_square & HG_PRE_IMAGENET_NORM) != 0));
    return HG_OK;
}

int hg_preprocess_batch(hg_ctx* c, const hg_preprocess_batch_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!a) return fail(c, HG_ERR_INVALID, "hg_preprocess_batch: null arguments");
    if (a->n == 0) return HG_OK;
    if (a->B < 1 || a->B > PREB_MAX_IMAGES) return fail(c, HG_ERR_INVALID, "hg_preprocess_batch: B must be 1 .. %d (got %d)", PREB_MAX_IMAGES, a->B);
    if (a->n < 0 || a->n > PREB_MAX_N) return fail(c, HG_ERR_INVALID, "hg_preprocess_batch: n must be 0 .. %d (got %d)", PREB_MAX_N, a->n);
    if (a->n_px < 1 || a->n_px > PREB_MAX_NPX) return fail(c, HG_ERR_INVALID, "hg_preprocess_batch: n_px must be 1 .. %d (got %d)", PREB_MAX_NPX, a->n_px);
    if (!a->images || !a->heights || !a->widths || !a->boxes || !a->crop_image || !a->out || !a->status)
        return fail(c, HG_ERR_INVALID, "hg_preprocess_batch: null pointer among images, heights, widths, boxes, crop_image, out, status");
    PreBatch pb = {};
    pb.B = a->B;
    for (int b = 0; b < a->B; ++b) {
        if (!a->images[b] || a->heights[b] <= 0 || a->widths[b] <= 0)
            return fail(c, HG_ERR_INVALID, "hg_preprocess_batch: image %d is null or has a side <= 0", b);
        pb.img[b] = a->images[b]; pb.H[b] = a->heights[b]; pb.W[b] = a->widths[b];
    }
    HG_ON_DEVICE(c);
    // headers [n][24] | tables [n][2][n_px * 67]: from n, n_px and the tap limit alone (the boxes never reach the host)
    const size_t head_words = (size_t)a->n * PREB_HDR;
    int rc = ensure(c, c->prebatch, (head_words + (size_t)a->n * 2 * preb_axis_words(a->n_px)) * 4);
    if (rc) return rc;
    int32_t* head = (int32_t*)c->prebatch.p;
    HG_HIP(launch_preprocess_batch(pb, a->boxes, a->crop_image, a->n, a->n_px, a->flags, a->background, head, head + head_words, a->out,
                                   a->out_u8, a->status, (hipStream_t)stream));
    return HG_OK;
}

int hg_profile_begin(hg_ctx* c, int kind, int max_launches) {
    if (!c || max_launches < 0) return HG_ERR_INVALID;
    HG_ON_DEVICE(c);
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    c->prof_ev.clear();
    c->prof_rec.clear();
    c->prof_n = 0;
    c->prof_kind = kind;
    if (kind == HG_PROF_OFF) return HG_OK;
    c->prof_ev.resize((size_t)2 * max_launches);
    c->prof_rec.resize((size_t)max_launches);
    for (auto& e : c->prof_ev) HG_HIP(hipEventCreate(&e));
    return HG_OK;
}

int hg_profile_end(hg_ctx* c, hg_prof_rec* recs, int max_recs, int32_t* n_recs) {
    if (!c || !n_recs || (max_recs > 0 && !recs)) return HG_ERR_INVALID;
    HG_ON_DEVICE(c);
    int n = 0;
    for (size_t i = 0; i < c->prof_n && n < max_recs; ++i, ++n) {
        HG_HIP(hipEventSynchronize(c->prof_ev[2 * i + 1]));
        float ms = 0.f;
        HG_HIP(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        recs[n] = c->prof_rec[i];
        recs[n].ms = ms;
    }
    *n_recs = n;
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    c->prof_ev.clear();
    c->prof_rec.clear();
    c->prof_kind = HG_PROF_OFF;
    c->prof_n = 0;
    return HG_OK;
}

int hg_workspace_bytes(hg_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return HG_ERR_INVALID;
    Buf* bufs[] = HG_WORKSPACE_BUFS(c);
    uint64_t t = 0;
    for (Buf* b : bufs) t += b->bytes;
    *bytes = t;
    return HG_OK;
}

int hg_roi_align(hg_ctx* c, const float* feat, int C, int H, int W, const float* boxes, int n, float spatial_scale,
                 int P, float* out_pooled, float* out_mean, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (n == 0) return HG_OK;
    if (!feat || !boxes || n < 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0 || (!out_pooled && !out_mean))
        return fail(c, HG_ERR_INVALID, "hg_roi_align: bad arguments");
    HG_ON_DEVICE(c);
    HG_HIP(launch_roi_align(feat, C, H, W, boxes, n, spatial_scale, P, out_pooled, out_mean, (hipStream_t)stream));
    return HG_OK;
}

int hg_assemble_prompts(hg_ctx* c, const float* prefix, const float* suffix, const float* ctx, const float* bias,
                        const int32_t* target, int R, int C, int L, int n_ctx, int D, float* prompts, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!prefix || !suffix || !ctx || !bias || !target || !prompts || R < 0 || C <= 0)
        return fail(c, HG_ERR_INVALID, "bad arguments to assemble_prompts");
    HG_ON_DEVICE(c);
    HG_HIP(launch_assemble_prompts(prefix, suffix, ctx, bias, target, R, C, L, n_ctx, D, prompts, (hipStream_t)stream));
    return HG_OK;
}

int hg_assemble_prompts_backward(hg_ctx* c, const float* grad_prompts, int R, int L, int n_ctx, int D, float* grad_ctx, float* grad_bias,
                                 void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (R == 0) return HG_OK;
    if (!grad_prompts || (!grad_ctx && !grad_bias) || R < 0 || n_ctx < 1 || n_ctx >= L || D < 1)
        return fail(c, HG_ERR_INVALID, "bad arguments to assemble_prompts_backward");
    HG_ON_DEVICE(c);
    const size_t n_part = ((size_t)R + PROMPTS_BWD_CHUNK - 1) / PROMPTS_BWD_CHUNK;
    if (int rc = ensure(c, c->pgrad, n_part * n_ctx * D * 4)) return rc;
    HG_HIP(launch_prompts_bwd(grad_prompts, R, L, n_ctx, D, (float*)c->pgrad.p, grad_ctx, grad_bias, (hipStream_t)stream));
    return HG_OK;
}

int hg_l2_normalize(hg_ctx* c, const float* x, int R, int D, float* out, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!x || !out || R < 0 || D <= 0) return fail(c, HG_ERR_INVALID, "bad arguments to l2_normalize");
    HG_ON_DEVICE(c);
    HG_HIP(launch_l2_normalize(x, out, R, D, (hipStream_t)stream));
    return HG_OK;
}

int hg_vae_loss(hg_ctx* c, const float* recon, const float* x, const float* mean, const float* logvar, int R,
                int D, float* loss, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!recon || !x || !mean || !logvar || !loss || R <= 0) return fail(c, HG_ERR_INVALID, "bad arguments to vae_loss");
    HG_ON_DEVICE(c);
    HG_HIP(launch_vae_loss(recon, x, mean, logvar, R, D, loss, (hipStream_t)stream));
    return HG_OK;
}

}  // extern "C"
