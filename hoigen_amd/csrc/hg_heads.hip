// The row-parallel heads: CoOp-VAE (Encoder -> reparameterise -> Generator), mlp_net and the cache-model logits, in chunks of rows.
#include "hg_host.h"

namespace {

// Rows of the next chunk of a row-parallel call with `left` rows to go: max_chunk_rows, except that the LAST chunk absorbs a
// tail of up to an eighth of it (100 000 rows = 32 768 + 32 768 + 34 464 instead of + 32 768 + 1 696: the four dependent GEMMs of a
// 1 696-row chunk fill 14-56 tiles each and cost 0.12 ms for 1.7 % of the rows; workspace +5 %)
inline int chunk_rows(const hg_ctx* c, int left) {
    const int m = c->max_chunk_rows;
    return left <= m + m / 8 ? left : m;
}

// Rows (from row 0) that go to the one-kernel path: its work items are 128 rows and take 0.3-0.4 ms each, so it only pays for whole
// rounds of items over the CUs (100 000 rows = 782 items = 3 rounds of 256 + 14: the 14 would cost a fourth round); the rest - and calls
// too small to fill most of one round - take the GEMM path, whose 256 x 256 tiles quantise a hundred times finer.
inline int fused_item_rows(const hg_ctx* c, int opt, int R) {
    if (opt == 0 || R <= 0) return 0;
    if (opt == 2) return R;
    const int per = vae_fused_rows_per_item();
    const long items = ((long)R + per - 1) / per, ncu = c->n_cu;
    const long full = items / ncu * ncu, rem = items - full;
    const long take = full + (rem * 100 >= ncu * 70 ? rem : 0);
    const long rows = take * per;
    return (int)(rows < R ? rows : R);
}

// One chunk of Rc rows of a cache slot from its fp16 operand f16 [rup(Rc, 256), lda] -> out [Rc, Nout]: what hg_cache_logits issues per
// chunk behind its conversion, and what hg_hoi_head issues per branch on the rows hoi_feats_kernel wrote (lda = 2 K for the human and
// the object half of the human | object buffer).
int cache_logits_rows(hg_ctx* c, Cache& m, const half_t* f16, int lda, int Rc, float* out, hipStream_t s) {
    const size_t Rp = rup(Rc, 256);
    const int Np = m.has_labels ? m.Cp : m.Sp, Nout = m.has_labels ? m.C : m.S;
    int rc = ensure(c, c->att, Rp * m.Sp * 2);
    if (!rc) rc = ensure(c, c->x, Rp * Np * 4);
    if (rc) return rc;
    half_t* phi = (half_t*)c->att.p;
    float* tmp = (float*)c->x.p;
    if (!m.has_labels) {
        HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(f16, lda, m.w16, m.b, tmp, m.Sp, Rc, m.Sp, m.K), s));
    } else {
        HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(f16, lda, m.w16, nullptr, phi, m.Sp, Rc, m.Sp, m.K), s));
        HG_HIP(hipMemsetAsync(tmp, 0, (size_t)Rc * m.Cp * 4, s));
        GemmArgs g = gemm_args(phi, m.Sp, m.lt16, m.bias_c, tmp, m.Cp, Rc, m.Cp, m.Sp);
        g.pos = m.scale;
        HG_HIP(gemm(c, EPI_SCALE_RESID_F32, g, s));          // 0 + (phi L + b L) * scale
    }
    HG_HIP(launch_copy_cols(tmp, Np, out, Rc, Nout, s));
    return HG_OK;
}

}  // namespace

extern "C" {

// ---- cache-model logits -----------------------------------------------------------------
int hg_cache_logits(hg_ctx* c, int slot, const float* feats, int R, float* out, void* stream) {
    if (!c || slot < 0 || slot >= HG_MAX_CACHE_SLOTS) return HG_ERR_INVALID;
    Cache& m = c->cache[slot];
    if (!m.loaded) return fail(c, HG_ERR_NOT_LOADED, "cache slot %d not loaded", slot);
    if (R == 0) return HG_OK;
    if (R < 0 || !feats || !out) return fail(c, HG_ERR_INVALID, "bad arguments to cache_logits");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    for (int r0 = 0, Rc = 0; r0 < R; r0 += Rc) {
        Rc = chunk_rows(c, R - r0);
        int rc = ensure(c, c->h, rup(Rc, 256) * m.K * 2);
        if (rc) return rc;
        half_t* f16 = (half_t*)c->h.p;
        HG_HIP(launch_f32_to_f16(feats + (size_t)r0 * m.K, f16, (size_t)Rc * m.K, s));
        rc = cache_logits_rows(c, m, f16, m.K, Rc, out + (size_t)r0 * (m.has_labels ? m.C : m.S), s);
        if (rc) return rc;
    }
    return HG_OK;
}

// ---- interaction head (hg_hoi_head.hip) --------------------------------------------------------------------------------------------
int hg_hoi_head(hg_ctx* c, const hg_hoi_head_args* a, void* stream) { return hg_hoi_head_image(c, a, nullptr, stream); }

// ... with the rows of its per-image branches (HG_HOI_SRC_IMAGE); im == nullptr: none
int hg_hoi_head_image(hg_ctx* c, const hg_hoi_head_args* a, const hg_hoi_image_args* im, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!a) return fail(c, HG_ERR_INVALID, "hg_hoi_head: no arguments");
    const float* feat_image = im ? im->feat_image : nullptr;
    const int K_img = im ? im->K_img : 0;
    float* image_logits = im ? im->image_logits : nullptr;
    if (a->B < 0 || a->B > HOI_MAX_IMAGES) return fail(c, HG_ERR_INVALID, "hg_hoi_head: %d images (at most %d a call)", a->B, HOI_MAX_IMAGES);
    if (a->B == 0) return HG_OK;
    if (!a->box_off || !a->n_human) return fail(c, HG_ERR_INVALID, "hg_hoi_head: box_off / n_human missing");
    if (a->H <= 0 || a->W <= 0 || a->H > HOI_MAX_SIDE || a->W > HOI_MAX_SIDE || a->C <= 0 || a->C > HOI_MAX_C || a->P <= 0 ||
        a->P > HOI_MAX_P)
        return fail(c, HG_ERR_INVALID, "hg_hoi_head: map %d x %d x %d, P = %d (H, W <= %d, C <= %d, P <= %d)", a->C, a->H, a->W, a->P, HOI_MAX_SIDE,
                    HOI_MAX_C, HOI_MAX_P);
    if (a->n_branch < 0 || a->n_branch > HG_HOI_MAX_BRANCH)
        return fail(c, HG_ERR_INVALID, "hg_hoi_head: %d branches (at most %d)", a->n_branch, HG_HOI_MAX_BRANCH);
    HoiBatch hb{};
    hb.B = a->B;
    long pairs = 0;
    for (int b = 0; b < a->B; ++b) {
        const long n = (long)a->box_off[b + 1] - a->box_off[b], nh = a->n_human[b];
        if (a->box_off[0] != 0 || n < 0) return fail(c, HG_ERR_INVALID, "hg_hoi_head: box_off must start at 0 and not decrease (image %d)", b);
        if (nh < 0 || nh > n) return fail(c, HG_ERR_INVALID, "hg_hoi_head: image %d has %ld humans among %ld boxes", b, nh, n);
        hb.box_off[b] = a->box_off[b];
        hb.pair_off[b] = (int)pairs;
        pairs += n > 1 ? nh * (n - 1) : 0;
        if (pairs > (1 << 24)) return fail(c, HG_ERR_INVALID, "hg_hoi_head: more than 2^24 pairs");
    }
    hb.box_off[a->B] = hb.N = a->box_off[a->B];
    hb.pair_off[a->B] = hb.Pt = (int)pairs;
    if (hb.N == 0) return HG_OK;
    const int C = a->C, NC = a->num_classes, nb = a->n_branch, Pt = hb.Pt;
    if (!a->feat_local || !a->boxes) return fail(c, HG_ERR_INVALID, "hg_hoi_head: feat_local / boxes missing");
    bool global = false;
    int n_img = 0;
    if (nb > 0) {
        if (C % 64) return fail(c, HG_ERR_INVALID, "hg_hoi_head: C = %d is not a multiple of 64 (the branch GEMMs' K)", C);
        if (NC <= 0 || !a->logits) return fail(c, HG_ERR_INVALID, "hg_hoi_head: num_classes / logits missing");
        for (int i = 0; i < nb; ++i) {
            const hg_hoi_branch& br = a->branch[i];
            if (br.source < HG_HOI_SRC_HUMAN || br.source > HG_HOI_SRC_IMAGE)
                return fail(c, HG_ERR_INVALID, "hg_hoi_head: branch %d has source %d", i, br.source);
            const bool image = br.source == HG_HOI_SRC_IMAGE;
            if (image && !feat_image) return fail(c, HG_ERR_INVALID, "hg_hoi_head: an image branch without feat_image");
            if (image && (K_img <= 0 || K_img % 64 || K_img > HOI_MAX_K_IMG))
                return fail(c, HG_ERR_INVALID, "hg_hoi_head: K_img = %d (a multiple of 64 from 64 to %d)", K_img, HOI_MAX_K_IMG);
            if (br.slot < 0 || br.slot >= HG_MAX_CACHE_SLOTS || !c->cache[br.slot].loaded)
                return fail(c, HG_ERR_INVALID, "hg_hoi_head: branch %d: cache slot %d not loaded", i, br.slot);
            const Cache& m = c->cache[br.slot];
            const int K = image ? K_img : br.source == HG_HOI_SRC_HUMAN_OBJECT ? 2 * C : C, Nout = m.has_labels ? m.C : m.S;
            if (m.K != K || Nout != NC)
                return fail(c, HG_ERR_INVALID, "hg_hoi_head: branch %d: slot %d maps %d -> %d, the branch needs %d -> %d", i, br.slot, m.K, Nout, K, NC);
            if (br.source == HG_HOI_SRC_GLOBAL) global = true;
            n_img += image;
        }
        if (global && !a->feat_global) return fail(c, HG_ERR_INVALID, "hg_hoi_head: a global branch without feat_global");
    }
    const bool want_prior = a->prior || a->scores_out;
    if (nb == 0 && a->scores_out) return fail(c, HG_ERR_INVALID, "hg_hoi_head: scores need logits, and there is no branch");
    if (want_prior && (!a->scores || !a->labels || !a->obj2target || a->n_obj_classes <= 0 || NC <= 0))
        return fail(c, HG_ERR_INVALID, "hg_hoi_head: prior / scores need scores, labels, obj2target and num_classes");
    if (a->objects && !a->labels) return fail(c, HG_ERR_INVALID, "hg_hoi_head: objects need labels");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t Rp = rup(std::max(Pt, 1), 256);
    int rc = ensure(c, c->hoi_tab, (size_t)(hb.N + Pt) * HOI_TAB * 4);
    if (!rc && !(a->pooled_single && (a->pooled_union || !Pt))) rc = ensure(c, c->hoi_pool, (size_t)(hb.N + Pt) * C * 4);
    if (!rc && nb > 0 && Pt > 0) rc = ensure(c, c->hoi_a16, Rp * C * 2 * (global ? 4 : 3));
    if (!rc && nb > 0 && Pt > 0 && !a->branch_logits) rc = ensure(c, c->hoi_br, (size_t)nb * Pt * NC * 4);
    if (!rc && n_img > 0 && Pt > 0) rc = ensure(c, c->hoi_img16, (size_t)256 * K_img * 2);
    if (!rc && n_img > 0 && Pt > 0 && !image_logits) rc = ensure(c, c->hoi_img, (size_t)n_img * a->B * NC * 4);
    if (rc) return rc;
    float* tab = (float*)c->hoi_tab.p;
    float* ps = a->pooled_single ? a->pooled_single : (float*)c->hoi_pool.p;
    float* pu = a->pooled_union ? a->pooled_union : (float*)c->hoi_pool.p + (size_t)hb.N * C;
    HG_HIP(launch_hoi_setup(hb, a->boxes, a->labels, a->spatial_scale, a->P, a->H, a->W, a->pair_h, a->pair_o, a->objects, a->union_boxes, tab, s));
    HG_HIP(launch_hoi_pool(hb, a->feat_local, C, a->H, a->W, a->P, tab, ps, pu, c->n_cu, s));
    if (Pt == 0) return HG_OK;
    half_t* ho16 = nb > 0 ? (half_t*)c->hoi_a16.p : nullptr;
    half_t* u16 = nb > 0 ? ho16 + Rp * 2 * C : nullptr;
    half_t* g16 = global ? u16 + Rp * C : nullptr;
    if (nb > 0 || a->feats) HG_HIP(launch_hoi_feats(hb, ps, pu, a->feat_global, C, a->feats, ho16, u16, g16, s));
    HoiEpilogue e{};
    e.n = nb;
    float* br_out = a->branch_logits ? a->branch_logits : (float*)c->hoi_br.p;
    // The image branches' operand: the B rows of feat_image as fp16 in a 256-row buffer of their own (HOI_MAX_IMAGES <= 256: one tile
    // of rows), the rows behind them zeroed on every call - the GEMMs read whole 256-row tiles of A.  One row per IMAGE, not per pair.
    half_t* img16 = n_img > 0 ? (half_t*)c->hoi_img16.p : nullptr;
    float* img_out = n_img > 0 ? (image_logits ? image_logits : (float*)c->hoi_img.p) : nullptr;
    if (n_img > 0) {
        HG_HIP(launch_f32_to_f16(feat_image, img16, (size_t)a->B * K_img, s));
        HG_HIP(hipMemsetAsync(img16 + (size_t)a->B * K_img, 0, (size_t)(256 - a->B) * K_img * 2, s));
    }
    for (int i = 0, i_img = 0; i < nb; ++i) {
        const hg_hoi_branch& br = a->branch[i];
        Cache& m = c->cache[br.slot];
        if (br.source == HG_HOI_SRC_IMAGE) {
            float* rows = img_out + (size_t)i_img++ * a->B * NC;
            rc = cache_logits_rows(c, m, img16, K_img, a->B, rows, s);
            if (rc) return rc;
            e.branch[i] = rows;
            e.scale[i] = br.scale;
            e.per_image[i] = 1;
            e.slab[i] = a->branch_logits ? br_out + (size_t)i * Pt * NC : nullptr;
            continue;
        }
        const half_t* A = br.source == HG_HOI_SRC_UNION ? u16 : br.source == HG_HOI_SRC_GLOBAL ? g16 : ho16 + (br.source == HG_HOI_SRC_OBJECT ? C : 0);
        const int lda = br.source == HG_HOI_SRC_UNION || br.source == HG_HOI_SRC_GLOBAL ? C : 2 * C;
        float* out = br_out + (size_t)i * Pt * NC;
        // Chunks are cut at multiples of 256 rows (option chunk_rows takes any value from 256 on): the GEMMs read whole 256-row tiles of
        // A, and with every r0 a multiple of 256 the last chunk's tiles end at row rup(Pt, 256) = Rp, the rows each operand of hoi_a16 has.
        for (int r0 = 0, Rc = 0; r0 < Pt; r0 += Rc) {
            Rc = chunk_rows(c, Pt - r0);
            if (r0 + Rc < Pt) Rc -= Rc % 256;
            rc = cache_logits_rows(c, m, A + (size_t)r0 * lda, lda, Rc, out + (size_t)r0 * NC, s);
            if (rc) return rc;
        }
        e.branch[i] = out;
        e.scale[i] = br.scale;
    }
    if (nb > 0 || want_prior)
        HG_HIP(launch_hoi_epilogue(hb, e, a->scores, a->labels, a->obj2target, a->n_obj_classes, NC, a->score_pow, nb > 0 ? a->logits : nullptr,
                                   a->prior, a->scores_out, s));
    return HG_OK;
}

// ---- region proposals and instance priors (hg_region_props.hip) ----------------------------------------------------------------------
int hg_region_priors(hg_ctx* c, const hg_region_priors_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!a) return fail(c, HG_ERR_INVALID, "hg_region_priors: no arguments");
    if (a->B < 0 || a->B > PROPS_MAX_IMAGES) return fail(c, HG_ERR_INVALID, "hg_region_priors: %d images (at most %d a call)", a->B, PROPS_MAX_IMAGES);
    if (a->max_instances < 1 || 2 * a->max_instances > PROPS_MAX_CAP || a->min_instances < 0 || a->min_instances > a->max_instances)
        return fail(c, HG_ERR_INVALID, "hg_region_priors: min_instances = %d, max_instances = %d (0 <= min <= max, 1 <= max, 2 max <= %d rows an image)",
                    a->min_instances, a->max_instances, PROPS_MAX_CAP);
    if (a->prior_slot < -1 || a->prior_slot >= HG_MAX_PRIOR_SLOTS)
        return fail(c, HG_ERR_INVALID, "hg_region_priors: prior slot %d (-1 .. %d)", a->prior_slot, HG_MAX_PRIOR_SLOTS - 1);
    const bool want_priors = a->prior_slot >= 0;
    if (want_priors && !c->prior[a->prior_slot].loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_region_priors: prior slot %d not loaded", a->prior_slot);
    if (a->B == 0) return HG_OK;
    if (!a->q_off || !a->counts) return fail(c, HG_ERR_INVALID, "hg_region_priors: q_off / counts missing");
    if (want_priors && (!a->image_sizes || !a->priors || !a->mask)) return fail(c, HG_ERR_INVALID, "hg_region_priors: priors need image_sizes, priors and mask");
    if (a->table_out && !want_priors) return fail(c, HG_ERR_INVALID, "hg_region_priors: table_out without a prior slot");
    PropsBatch pb{};
    pb.B = a->B;
    if (a->q_off[0] != 0) return fail(c, HG_ERR_INVALID, "hg_region_priors: q_off must start at 0");
    for (int b = 0; b < a->B; ++b) {
        const long q = (long)a->q_off[b + 1] - a->q_off[b];
        if (q < 0 || q > PROPS_MAX_Q) return fail(c, HG_ERR_INVALID, "hg_region_priors: image %d has %ld detections (0 .. %d)", b, q, PROPS_MAX_Q);
        pb.q_off[b] = a->q_off[b];
        pb.img_h[b] = a->image_sizes ? a->image_sizes[2 * b] : 1.f;
        pb.img_w[b] = a->image_sizes ? a->image_sizes[2 * b + 1] : 1.f;
    }
    pb.q_off[a->B] = a->q_off[a->B];
    if (pb.q_off[a->B] > 0 && (!a->scores || !a->labels || !a->boxes)) return fail(c, HG_ERR_INVALID, "hg_region_priors: scores / labels / boxes missing");
    const int n_out = (a->keep != nullptr) + (a->out_boxes != nullptr) + (a->out_scores != nullptr) + (a->out_labels != nullptr);
    if (n_out != 0 && n_out != 4) return fail(c, HG_ERR_INVALID, "hg_region_priors: keep, out_boxes, out_scores and out_labels come together or not at all");
    if (((uintptr_t)a->boxes | (uintptr_t)a->out_boxes) & 15) return fail(c, HG_ERR_INVALID, "hg_region_priors: boxes / out_boxes must be 16-byte aligned");
    const int cap = 2 * a->max_instances;
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    int32_t *keep = a->keep, *out_labels = a->out_labels;
    float *out_boxes = a->out_boxes, *out_scores = a->out_scores;
    if (!n_out) {
        const size_t slots = (size_t)a->B * cap;
        int rc = ensure(c, c->props, slots * 7 * 4);
        if (rc) return rc;
        out_boxes = (float*)c->props.p;
        out_scores = out_boxes + 4 * slots;
        keep = (int32_t*)(out_scores + slots);
        out_labels = keep + slots;
    }
    PropsSelect ps{};
    ps.score_thr = a->box_score_thresh; ps.nms_thr = a->nms_thresh;
    ps.human_idx = a->human_idx; ps.min_inst = a->min_instances; ps.max_inst = a->max_instances; ps.cap = cap;
    ps.n_classes = want_priors ? c->prior[a->prior_slot].n_classes : 0;
    HG_HIP(launch_props_select(pb, ps, a->scores, a->labels, a->boxes, a->counts, keep, out_boxes, out_scores, out_labels, a->survivors, s));
    if (!want_priors) return HG_OK;
    const Priors& m = c->prior[a->prior_slot];
    PriorDev pw{m.hid, m.w0t, m.b0, m.w1t, m.b1, m.w2t, m.b2, m.T};
    HG_HIP(launch_prior_mlp(pb, pw, cap, a->counts, out_boxes, out_scores, out_labels, a->priors, a->mask, s));
    if (a->table_out) HG_HIP(hipMemcpyAsync(a->table_out, m.T, (size_t)m.n_classes * m.hid * 4, hipMemcpyDeviceToDevice, s));
    return HG_OK;
}

// ---- detections and ground-truth matching (hg_detections.hip) -------------------------------------------------------------------------
int hg_hoi_detections(hg_ctx* c, const hg_hoi_detections_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!a) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: no arguments");
    if (a->B < 0 || a->B > DET_MAX_IMAGES) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: %d images (at most %d a call)", a->B, DET_MAX_IMAGES);
    if (a->num_classes <= 0 || a->num_classes > DET_MAX_NC)
        return fail(c, HG_ERR_INVALID, "hg_hoi_detections: num_classes = %d (1 .. %d)", a->num_classes, DET_MAX_NC);
    if (a->cap < 0) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: cap = %d", a->cap);
    if (!a->det_off) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: det_off missing");
    if (!a->pair_off || !a->box_off) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: pair_off / box_off missing");
    const bool assoc = a->gt_off != nullptr;
    if (assoc && !a->gt_sizes && a->gt_format == 1) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: gt_format 1 needs gt_sizes");
    if (assoc && a->gt_format != 0 && a->gt_format != 1) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: gt_format = %d (0 or 1)", a->gt_format);
    if (a->conversion && a->n_obj_classes <= 0) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: conversion without n_obj_classes");
    DetBatch db{};
    db.B = a->B;
    if (a->pair_off[0] != 0 || a->box_off[0] != 0 || (assoc && a->gt_off[0] != 0))
        return fail(c, HG_ERR_INVALID, "hg_hoi_detections: pair_off, box_off and gt_off must start at 0");
    for (int b = 0; b < a->B; ++b) {
        const long np = (long)a->pair_off[b + 1] - a->pair_off[b], nb = (long)a->box_off[b + 1] - a->box_off[b];
        const long ng = assoc ? (long)a->gt_off[b + 1] - a->gt_off[b] : 0;
        if (np < 0 || nb < 0) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: pair_off / box_off decrease at image %d", b);
        if (ng < 0 || ng > DET_MAX_GT) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: image %d has %ld ground-truth pairs (0 .. %d)", b, ng, DET_MAX_GT);
        if (a->pair_off[b + 1] > (1 << 24)) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: more than 2^24 pairs");
        db.pair_off[b + 1] = a->pair_off[b + 1];
        db.box_off[b + 1] = a->box_off[b + 1];
        db.gt_off[b + 1] = assoc ? a->gt_off[b + 1] : 0;
        db.img_h[b] = a->gt_sizes ? a->gt_sizes[2 * b] : 1;
        db.img_w[b] = a->gt_sizes ? a->gt_sizes[2 * b + 1] : 1;
    }
    const int B = a->B, Pt = db.Pt = db.pair_off[B], NC = a->num_classes, Gt = db.gt_off[B], cap = a->cap;
    if ((long)Pt * NC > 0x7FFFFFFFl) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: %d pairs x %d classes do not fit a 32-bit count", Pt, NC);
    if (Pt > 0 && (!a->prior || !a->pair_h || !a->pair_o || !a->objects))
        return fail(c, HG_ERR_INVALID, "hg_hoi_detections: prior / pair_h / pair_o / objects missing");
    if (Pt > 0 && cap > 0 && a->det_score && !a->scores) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: det_score needs scores");
    if (assoc && Pt > 0 && cap > 0 && (!a->scores || !a->boxes)) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: the association needs scores and boxes");
    if (assoc && Gt > 0 && (!a->gt_boxes_h || !a->gt_boxes_o || !a->gt_hoi)) return fail(c, HG_ERR_INVALID, "hg_hoi_detections: gt_boxes_h / gt_boxes_o / gt_hoi missing");
    if (!assoc && (a->det_label || a->det_gt || a->det_max_iou || a->gt_boxes_out))
        return fail(c, HG_ERR_INVALID, "hg_hoi_detections: det_label / det_gt / det_max_iou / gt_boxes_out need ground truth (gt_off)");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    if (B == 0) return HG_OK;
    // workspace: cnt [Pt], bsum [nblk], and one [cap] array for each entry array the association reads that the caller left out
    const size_t nblk = ((size_t)Pt + DET_ROWS - 1) / DET_ROWS;
    DetEntries e{a->det_pair, a->det_verb, a->det_h, a->det_o, a->det_object, a->det_score, a->det_interaction};
    int32_t* det_gt = a->det_gt;
    const int n_sub = assoc ? (!e.h) + (!e.o) + (!e.score) + (!e.interaction) + (!det_gt) : 0;
    int rc = ensure(c, c->det, ((size_t)Pt + nblk + (size_t)n_sub * cap + 1) * 4);
    if (rc) return rc;
    int32_t* cnt = (int32_t*)c->det.p;
    int32_t* bsum = cnt + Pt;
    int32_t* sub = bsum + nblk;
    if (assoc) {
        if (!e.h) { e.h = sub; sub += cap; }
        if (!e.o) { e.o = sub; sub += cap; }
        if (!e.score) { e.score = (float*)sub; sub += cap; }
        if (!e.interaction) { e.interaction = sub; sub += cap; }
        if (!det_gt) { det_gt = sub; sub += cap; }
    }
    HG_HIP(launch_det_compact(db, a->prior, a->scores, a->pair_h, a->pair_o, a->objects, a->conversion, a->n_obj_classes, NC, cap, cnt, bsum,
                              a->det_off, e, a->status, s));
    if (assoc)
        HG_HIP(launch_det_assoc(db, a->boxes, a->gt_boxes_h, a->gt_boxes_o, a->gt_hoi, a->gt_format, a->min_iou, cap, Gt, a->det_off, e, a->det_label,
                                det_gt, a->det_max_iou, a->gt_boxes_out, a->status, s));
    return HG_OK;
}

// ---- CoOp-VAE ---------------------------------------------------------------------------------------------
static int vae_fused_rows(const hg_ctx* c, int R) { return fused_item_rows(c, c->opt_vae_fused, R); }
static int generator_rows(hg_ctx* c, Vae& v, const half_t* z16, int R, float* bias, hipStream_t s) {
    // Generator: relu(z W0^T + b0) W2^T + b2  (main_coop_vae.py:282-296)
    half_t* g1 = (half_t*)c->fc.p;
    HG_HIP(gemm(c, EPI_BIAS_RELU_F16, gemm_args(z16, v.dim, v.g_w0, v.g_b0, g1, v.gh, R, v.gh, v.dim), s));
    HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(g1, v.gh, v.g_w2, v.g_b2, bias, v.dim, R, v.dim, v.gh), s));
    return HG_OK;
}

int hg_vae_forward(hg_ctx* c, int slot, const float* x, const float* eps, int R, float* mean, float* logvar,
                   float* z, float* bias, void* stream) {
    if (!c || slot < 0 || slot >= HG_MAX_SLOTS) return HG_ERR_INVALID;
    Vae& v = c->vae[slot];
    if (!v.enc || (bias && !v.gen)) return fail(c, HG_ERR_NOT_LOADED, "hg_load_vae(slot %d) incomplete", slot);
    if (R == 0) return HG_OK;
    if (R < 0 || !x || !eps) return fail(c, HG_ERR_INVALID, "bad arguments to vae_forward");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const int dim = v.dim;
    // Option vae_fused = 2: the leading rows that fill whole rounds of items (all rows) go through ONE kernel, hidden layers and z on
    // chip (hg_vae_fused.hip).  Default (1): the Encoder stays on the GEMM path - the one kernel computes its hidden layer twice (1 024
    // output columns do not fit a wave's registers) and loses to the GEMMs there: measured 1.94 ms against 1.72 ms for 98 304 rows - and
    // the Generator of those rows runs as the one kernel on the fp16 z the reparameterisation kernel writes (0.86 against 0.92 ms).
    const int Rf = v.wp ? vae_fused_rows(c, R) : 0;
    const bool all_fused = Rf > 0 && c->opt_vae_fused == 2;
    if (all_fused) {
        int rc = ensure(c, c->zpark, vae_fused_park_bytes(Rf));
        if (rc) return rc;
        VaeFusedArgs a{};
        a.x = x; a.eps = eps; a.mean = mean; a.logvar = logvar; a.z = z; a.bias = bias; a.wp = v.wp;
        a.b0e = v.e_b0; a.bml = v.e_bml; a.b0g = v.g_b0; a.b2g = v.g_b2; a.zpark = (half_t*)c->zpark.p;
        a.R = Rf; a.eh = v.eh; a.gh = v.gen ? v.gh : 0; a.mode = bias ? 0 : 1; a.has_enc = true;
        ProfScope ps(c, s, HG_PROF_VAE_FUSED, Rf, bias ? 3 : 2, v.eh);
        HG_HIP(launch_vae_fused(a, s));
    }
    // rows of the call whose Generator runs as the one kernel (hybrid): the chunks below stop at that boundary
    const int Rg = (!all_fused && bias && Rf > 0) ? Rf : 0;
    if (Rg > 0) {      // z of those rows as fp16, for ONE Generator launch behind the chunks (three items per CU instead of three launches)
        int rc = ensure(c, c->zpark, (size_t)rup(Rg, 256) * dim * 2);
        if (rc) return rc;
    }
    for (int r0 = all_fused ? Rf : 0, Rc = 0; r0 < R; r0 += Rc) {
        Rc = chunk_rows(c, R - r0);
        if (r0 < Rg && r0 + Rc > Rg) Rc = Rg - r0;
        const bool gen_fused = r0 < Rg;
        const size_t Rp = rup(Rc, 256);
        int rc = ensure(c, c->h, Rp * dim * 2);
        if (!rc) rc = ensure(c, c->att, Rp * dim * 2);
        if (!rc) rc = ensure(c, c->qkv, Rp * v.eh * 2);
        if (!rc) rc = ensure(c, c->x, Rp * 2 * dim * 4);
        if (!rc && bias && !gen_fused) rc = ensure(c, c->fc, Rp * v.gh * 2);
        if (rc) return rc;
        half_t* x16 = (half_t*)c->h.p;
        const size_t o = (size_t)r0 * dim;
        half_t* z16 = gen_fused ? (half_t*)c->zpark.p + o : (half_t*)c->att.p;
        half_t* h1 = (half_t*)c->qkv.p;
        float* ml = (float*)c->x.p;          // [2][Rp, dim] planes for the halves the caller did not ask for
        float* mean_o = mean ? mean + o : ml;
        float* lv_o = logvar ? logvar + o : ml + Rp * dim;
        HG_HIP(launch_f32_to_f16(x + o, x16, (size_t)Rc * dim, s));
        HG_HIP(gemm(c, EPI_BIAS_RELU_F16, gemm_args(x16, dim, v.e_w0, v.e_b0, h1, v.eh, Rc, v.eh, dim), s));
        // mean | log_var as ONE N = 2*dim GEMM whose two column halves land directly in the caller's tensors
        GemmArgs g = gemm_args(h1, v.eh, v.e_wml, v.e_bml, mean_o, dim, Rc, 2 * dim, v.eh);
        // (The reparameterisation on the accumulators of a row-interleaved mean | log_var GEMM was built and measured in round 3:
        // bit-identical, one launch and 410 MB less per 100 k rows, 0.5-2 % SLOWER - its 56 partial-line stores per wave cost the
        // GEMM what the HBM-speed reparam kernel costs on its own; commit 2b473ec and earlier carry it.)
        g.out_hi = lv_o; g.n_split = dim;
        HG_HIP(gemm(c, EPI_BIAS_F32, g, s));
        HG_HIP(launch_reparam(mean_o, lv_o, eps + o, Rc, dim, z ? z + o : nullptr, z16, dim, s));
        if (bias && !gen_fused) {
            rc = generator_rows(c, v, z16, Rc, bias + o, s);
            if (rc) return rc;
        }
    }
    if (Rg > 0) {
        VaeFusedArgs a{};
        a.x16 = (const half_t*)c->zpark.p; a.bias = bias; a.wp = v.wp; a.b0g = v.g_b0; a.b2g = v.g_b2;
        a.R = Rg; a.eh = v.eh; a.gh = v.gh; a.mode = 2; a.has_enc = true;
        ProfScope ps(c, s, HG_PROF_VAE_FUSED, Rg, 1, v.gh);
        HG_HIP(launch_vae_fused(a, s));
    }
    return HG_OK;
}

int hg_generator(hg_ctx* c, int slot, const float* z, int R, float* bias, void* stream) {
    if (!c || slot < 0 || slot >= HG_MAX_SLOTS) return HG_ERR_INVALID;
    Vae& v = c->vae[slot];
    if (!v.gen) return fail(c, HG_ERR_NOT_LOADED, "generator of slot %d not loaded", slot);
    if (R == 0) return HG_OK;
    if (R < 0 || !z || !bias) return fail(c, HG_ERR_INVALID, "bad arguments to generator");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const int Rf = v.wp ? vae_fused_rows(c, R) : 0;
    if (Rf > 0) {
        VaeFusedArgs a{};
        a.x = z; a.bias = bias; a.wp = v.wp; a.b0g = v.g_b0; a.b2g = v.g_b2;
        a.R = Rf; a.eh = v.enc ? v.eh : 0; a.gh = v.gh; a.mode = 2; a.has_enc = v.enc;
        ProfScope ps(c, s, HG_PROF_VAE_FUSED, Rf, 1, v.gh);
        HG_HIP(launch_vae_fused(a, s));
    }
    for (int r0 = Rf, Rc = 0; r0 < R; r0 += Rc) {
        Rc = chunk_rows(c, R - r0);
        const size_t Rp = rup(Rc, 256);
        int rc = ensure(c, c->att, Rp * v.dim * 2);
        if (!rc) rc = ensure(c, c->fc, Rp * v.gh * 2);
        if (rc) return rc;
        half_t* z16 = (half_t*)c->att.p;
        HG_HIP(launch_f32_to_f16(z + (size_t)r0 * v.dim, z16, (size_t)Rc * v.dim, s));
        rc = generator_rows(c, v, z16, Rc, bias + (size_t)r0 * v.dim, s);
        if (rc) return rc;
    }
    return HG_OK;
}

int hg_mlp_net(hg_ctx* c, int slot, const float* x, int R, float* out, void* stream) {
    if (!c || slot < 0 || slot >= HG_MAX_SLOTS) return HG_ERR_INVALID;
    Mlp& m = c->mlp[slot];
    if (!m.loaded) return fail(c, HG_ERR_NOT_LOADED, "mlp_net slot %d not loaded", slot);
    if (R == 0) return HG_OK;
    if (R < 0 || !x || !out) return fail(c, HG_ERR_INVALID, "bad arguments to mlp_net");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    for (int r0 = 0, Rc = 0; r0 < R; r0 += Rc) {
        Rc = chunk_rows(c, R - r0);
        const size_t Rp = rup(Rc, 256);
        int rc = ensure(c, c->h, Rp * m.in * 2);
        if (!rc) rc = ensure(c, c->att, Rp * m.hid * 2);
        if (!rc) rc = ensure(c, c->qkv, Rp * m.hid * 2);
        if (rc) return rc;
        half_t* x16 = (half_t*)c->h.p;
        half_t* a1 = (half_t*)c->att.p;
        half_t* a2 = (half_t*)c->qkv.p;
        HG_HIP(launch_f32_to_f16(x + (size_t)r0 * m.in, x16, (size_t)Rc * m.in, s));
        HG_HIP(gemm(c, EPI_BIAS_RELU_F16, gemm_args(x16, m.in, m.w0, m.b0, a1, m.hid, Rc, m.hid, m.in), s));
        HG_HIP(gemm(c, EPI_BIAS_RELU_F16, gemm_args(a1, m.hid, m.w2, m.b2, a2, m.hid, Rc, m.hid, m.hid), s));
        HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(a2, m.hid, m.w4, m.b4, out + (size_t)r0 * m.out, m.out, Rc, m.out, m.hid), s));
    }
    return HG_OK;
}

}  // extern "C"
