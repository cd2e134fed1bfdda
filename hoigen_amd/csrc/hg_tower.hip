// The two transformer towers: the plan of a tower call, the block runner and its launch steps, the instance adapter in front of a
// block, and the image / text entry points with their stream-trace hooks.  Host code only.
#include <mutex>

#include "hg_host.h"

namespace {

// The MLP pair launch (hg_mlp_pair.hip) has one workgroup per CU and its workgroups wait for each other: two such launches from different
// streams of this process, each holding part of the CUs, would wait for each other until their bound (both towers of a model run it, and a
// caller may well encode text on one stream and crops on another).  As long as every pair launch of a device comes from ONE stream
// nothing is done.  The first time a second stream shows up the device is synchronised once, and from then on every pair launch waits for
// the previous one's event and records its own: the launches are serial across streams (each fills the chip anyway).  Other processes
// on the same GPU are the deployment's business (option mlp_pair = 0 there).
struct PairGate {
    std::mutex mu;
    bool have_first = false, multi = false, evt_set = false;
    hipStream_t first = nullptr;
    hipEvent_t evt = nullptr;
};
static PairGate g_pair_gate[16];
struct PairGateScope {      // around ONE pair launch on stream s of device dev (the current device)
    PairGate* g;
    hipStream_t s;
    PairGateScope(int dev, hipStream_t s_) : g(&g_pair_gate[dev & 15]), s(s_) {
        g->mu.lock();
        if (!g->have_first) { g->first = s; g->have_first = true; }
        else if (!g->multi && s != g->first) {
            (void)hipDeviceSynchronize();      // (once: whatever the first stream has in flight carries no event)
            if (hipEventCreateWithFlags(&g->evt, hipEventDisableTiming) != hipSuccess) g->evt = nullptr;
            g->multi = true;
        }
        if (g->multi && g->evt && g->evt_set) (void)hipStreamWaitEvent(s, g->evt, 0);
    }
    ~PairGateScope() {
        if (g->multi && g->evt && hipEventRecord(g->evt, s) == hipSuccess) g->evt_set = true;
        g->mu.unlock();
    }
};

// ---- one transformer tower over the residual stream in c->x ------------------------------------------
struct AdapterCall {
    const float* priors = nullptr;   // [n_seq, N, 64] or null
    const uint8_t* mask = nullptr;
    int N = 0;
    bool enabled = false;
};

// One call of run_blocks, filled by name by its two callers (encode_image_impl, text_tail).
// `row0_out` (towers without token outputs): only ONE row of every sequence leaves the tower - row sel[seq] (the EOT
// token of the text tower) or row 0 when sel is null (the class token of the vision tower) - so the LAST block
// computes K and V for all rows but Q, attention, out-proj and the MLP for those n_seq rows only (a dense
// [n_seq, D] stream, returned through *row0_out); all other rows of that block never reach any output.
// Option last_block_row0 = 0 runs the last block on every row like the others.
// `pre_w` / `pre_b` (vision tower): the LayerNorm in front of the first block (ln_pre) has NOT been applied yet; it runs
// here, fused with the first block's folding statistics when folding is on - and, with `pre_pos` / `pre_cls`, with the class
// rows and the positional embedding the patch GEMM left out (clipnet/model.py:223-225 in one pass over the rows)
// `trace` ([layers + 1] entries `trace_stride` floats apart): the stream entering block 0, then after every block - row 0 of every
// sequence, or with `trace_all` (the stream test hooks) all M rows; the last entry of a row0_out block holds its n_seq rows densely
struct TowerCall {
    int n_seq = 0, L = 0, D = 0, heads = 0;
    bool causal = false; hipStream_t s = nullptr;
    float* trace = nullptr; int trace_stride = 0; bool trace_all = false;
    bool trace_entries_only = false;      // no entry behind the last block: the trace holds the stream as it ENTERS every block (hg_encode_text_embeds_save)
    const AdapterCall* ac = nullptr;
    bool ln_fold = false;        // LayerNorm folded into the GEMMs where the shapes allow (ln_fuse_ok)
    bool gamma_act = false;      // ... with the LayerNorm weight in the ACTIVATION copy (text tower, text_ln_fold = 1)
    const int32_t* sel = nullptr;
    const float *pre_w = nullptr, *pre_b = nullptr, *pre_pos = nullptr, *pre_cls = nullptr;
    const float** row0_out = nullptr;
};

// `fused`: LayerNorm folding is on - the stream's centred fp16 copy (c->h), its centre (c->muc) and the folding
// statistics are current; the adapter consumes the copy and its up_proj re-emits all three for the updated stream
// `cat`: the adapter folded into the block's GEMMs altogether - nothing but down_proj and the decoder runs here; the
// centred fp16 copy of the stream is expected in columns 0..D-1 of c->att (row stride D + 64), the decoder writes e beside it and
// turns c->mr into the statistics of x + a; the block's QKV GEMM then takes [x16 | e] x [W'_qkv | W'_qkv Q].  Workspace: plan_tower
// `up_lo`: up_proj as hi + lo where the adapter carries the remainder (towers of more than 224 tokens, hg_load_vit): the tower's calls;
// hg_test_adapter launches the decoder and the one-pass up_proj its float64 check restates
int run_adapter(hg_ctx* c, const AdapterW& a, int n_seq, int L, int D, const AdapterCall& ac, hipStream_t s, bool fused,
                bool cat, half_t* e2, bool up_lo) {
    const int M = n_seq * L;
    float* x = (float*)c->x.p;
    half_t* h = (half_t*)c->h.p;
    AdapterDev ad{};
    ad.down_w = a.down_w; ad.down_b = a.down_b; ad.up_w = a.up_w; ad.up_b = a.up_b; ad.scale = a.scale;
    for (int k = 0; k < 2; ++k) {
        for (int j = 0; j < 12; ++j) ad.dl[k][j] = a.dl[k][j];
        for (int j = 0; j < 6; ++j) ad.w16[k][j] = a.w16[k][j];
    }
    // down = relu(down_proj(x))  (CLIP_models_adapter_prior2.py:184-185) - inside the decoder kernel when it can (folded mode)
    const bool down_fused = cat && adapter_decoder_fused_down_ok(ad, ac.priors != nullptr, L, ac.N);
    const AdapterW::Fold& fold = a.fold[ac.priors ? 0 : 1];
    if (!down_fused) {
        GemmArgs g = gemm_args(h, D, a.down_w, a.down_b, c->ad32.p, 128, M, 128, D);
        if (cat) {   // ... read from the out-proj operand buffer, with x16 Q in the padded columns (no ReLU there)
            g.A = (const half_t*)c->att.p; g.lda = D + 64; g.W = fold.down2; g.n_split = 64;
            g.cs = a.down_cs; g.mu = (const float*)c->muc.p;
            HG_HIP(gemm(c, EPI_MU_BIAS_RELU_F32, g, s));
        } else if (fused) {       // on the centred fp16 copy the residual GEMMs keep current: W (x16 + mu) + b
            g.cs = a.down_cs; g.mu = (const float*)c->muc.p;
            HG_HIP(gemm(c, EPI_MU_BIAS_RELU_F32, g, s));
        } else {
            HG_HIP(launch_f32_to_f16(x, h, (size_t)M * D, s));
            HG_HIP(gemm(c, EPI_BIAS_RELU_F32, g, s));
        }
    }
    // post-norm decoder layer(s) over the 64-wide bottleneck (adapter...:186-200); with adapter_num_layers > 1 the
    // prior path chains mhsa_layers.0 .. N-1, the intermediate activations staying fp32 in place
    const int n_chain = ac.priors ? 1 + (int)a.extra.size() : 1;
    // chained layers exist only in the MFMA decoder (one workgroup per sequence, <= 32 prior tokens): say so up front
    // instead of failing inside the launch
    if (n_chain > 1 && !adapter_decoder_mfma_ok(ad, true, L, ac.N) && !adapter_decoder_long_ok(ad, true, L, ac.N))
        return fail(c, HG_ERR_INVALID, "adapter_num_layers > 1 needs the MFMA decoder path: at most 32 prior tokens (got %d)", ac.N);
    for (int z = 0; z < n_chain; ++z) {
        if (z > 0)
            for (int j = 0; j < 12; ++j) ad.dl[0][j] = a.extra[z - 1].dl[j];
        if (z > 0)
            for (int j = 0; j < 6; ++j) ad.w16[0][j] = a.extra[z - 1].w16[j];
        half_t* d16 = cat ? (half_t*)c->att.p + D : (half_t*)c->ad16.p;
        AdapterFoldDev fd{};
        if (cat) { fd.g16 = fold.g16; fd.qm = fold.qm; fd.mr = (float*)c->mr.p; fd.inv_D = 1.0f / (float)D; fd.e2 = e2; }
        AdapterDownDev dn{};
        if (down_fused && z == 0) {
            dn.x16 = (const half_t*)c->att.p; dn.ldx = D + 64; dn.K = D; dn.w = fold.down2; dn.b = a.down_b; dn.cs = a.down_cs;
            dn.muc = (const float*)c->muc.p;
        }
        hipError_t e = launch_adapter_decoder((const float*)c->ad32.p, ad, ac.priors, ac.mask, n_seq, L, ac.priors ? ac.N : 0,
                                              (float*)c->adkv.p, d16, s,
                                              z + 1 < n_chain ? (float*)c->ad32.p : nullptr, cat ? D + 64 : 64,
                                              cat ? &fd : nullptr, down_fused && z == 0 ? &dn : nullptr);
        if (e != hipSuccess)
            return fail(c, HG_ERR_HIP, "adapter decoder layer %d failed: %s", z, hipGetErrorString(e));
    }
    if (cat) return HG_OK;      // the update itself happens in the block's QKV and out-proj GEMMs
    // x += up_proj(.) * scale   (adapter...:201-202, :456)
    GemmArgs g = gemm_args((const half_t*)c->ad16.p, 64, a.up_w, a.up_b, x, D, M, D, 64);
    g.pos = a.scale;
    if (up_lo && a.up_w_lo) {      // x += ad16 x lo^T * (2^-11 scale), in front of the pass that re-emits the copy
        GemmArgs lo = gemm_args((const half_t*)c->ad16.p, 64, a.up_w_lo, c->vit.lo_scale + D, x, D, M, D, 64);
        lo.pos = a.scale_lo;
        HG_HIP(gemm(c, EPI_SCALE_RESID_F32, lo, s));
    }
    if (fused) {       // ... and re-emit the fp16 copy + row statistics of the updated stream for the folded ln_1
        const int sld = 4 * (D / 256);
        g.out2 = h; g.stats = (float*)c->stats.p; g.stats_ld = sld; g.mu = (const float*)c->mu.p;
        HG_HIP(gemm(c, EPI_SCALE_RESID_LN_F32, g, s));
        HG_HIP(launch_finalize_stats((const float*)c->stats.p, (float*)c->mr.p, (float*)c->mu.p, M, sld, 64, s,
                                     (float*)c->muc.p));
    } else {
        HG_HIP(gemm(c, EPI_SCALE_RESID_F32, g, s));
    }
    return HG_OK;
}

// LayerNorm folded into the GEMMs: the residual GEMMs (out-proj, c_proj) also emit the fp16 copy of the updated
// rows and per-row partial statistics; the consuming GEMMs (QKV, c_fc) read that copy and apply mean / rstd in
// their epilogue.  Used when every GEMM of the block is eligible for the ring kernels and no adapter rewrites
// the stream between the residual GEMM and its LayerNorm.  Option ln_fuse = 0 selects the separate-LayerNorm path.
bool ln_fuse_ok(hg_ctx* c, int M, int D) {
    if (!c->opt_ln_fuse) return false;
    if (D % 256) return false;
    float dummy = 0.f;
    GemmArgs g = gemm_args(nullptr, D, nullptr, nullptr, nullptr, 3 * D, M, 3 * D, D);
    g.cs = &dummy; g.mr = &dummy;
    if (!gemm_ln_ok(EPI_LN_BIAS_F16, g)) return false;
    g.N = 4 * D; g.ldc = 4 * D;
    if (!gemm_ln_ok(EPI_LN_BIAS_QGELU_F16, g)) return false;
    GemmArgs r = gemm_args(nullptr, D, nullptr, nullptr, nullptr, D, M, D, D);
    r.out2 = (half_t*)&dummy; r.stats = &dummy; r.mu = &dummy; r.stats_ld = 4 * (D / 256);
    if (!gemm_ln_ok(EPI_RESID_LN_F32, r)) return false;
    r.K = 4 * D; r.lda = 4 * D;
    return gemm_ln_ok(EPI_RESID_LN_F32, r);
}

// ---- the plan of one tower call: everything run_blocks decides, decided before its first launch; plain data the launch steps read ----
enum class InProj { separate, folded, cat, qkv_attn, qkv_attn_cat, qkv_attn_text };
struct BlockPlan {
    const AdapterW* adapter = nullptr;      // the instance adapter in front of this block (null: none)
    // How the adapter reaches the stream: folded into the block's own GEMMs (default, option adapter_fold = 1, when the shapes allow:
    // QKV takes [x16 | e], out-proj [att | e], ln_1's statistics come from the decoder kernel - no up_proj launch at all), or, null,
    // an up_proj GEMM with a scaled-residual epilogue on the fp32 stream (+ fp16 copy + statistics when folding LayerNorm)
    const AdapterW::Fold* fold = nullptr;
    InProj in_proj = InProj::separate;
    bool row0 = false;       // the tower's last block, on the selected rows only
    bool emits = false;      // c_proj emits the next block's ln_1 copy and statistics (every folded block but the tower's last)
    bool pair = false;       // c_fc -> QuickGELU -> c_proj as ONE persistent launch (hg_mlp_pair.hip)
    bool pair256 = false;    // ... with c_proj on 256 x 256 tiles (hg_mlp_pair256.hip)
    int hl_out = 0, hl_proj = 0;      // GemmArgs::hl of out-proj / c_proj
    bool x_hilo = false;     // behind this block the stream lives in (h, xlo, muc), not in x
    half_t* x16 = nullptr;   // the centred fp16 copy of the stream entering the block (on the hi / lo stream: its hi half), row stride ldx:
    int ldx = 0;             //   beside e in the in_proj operand buffer [x16 | e] (att, D + 64) when the adapter is folded, else h
    half_t *a1 = nullptr, *a2 = nullptr;      // what in_proj / c_fc read: x16 / h - or the copy that carries the LayerNorm weight (gs)
    int lda2 = 0;
};
struct TowerPlan {
    int M = 0, sld = 0, pair_panels = 0;
    bool fuse = false;       // LayerNorm folded into the GEMMs
    // Residual stream as centre + hi + lo between the LayerNorm-emitting residual GEMMs (GemmArgs::hl; option stream_hilo):
    // hi IS the centred fp16 copy those GEMMs write anyway, lo its remainder as bf8 - 6 instead of 10
    // bytes per element through every such epilogue and a third fewer partial-line stores.  The first of them reads the fp32 stream (ln_pre wrote it),
    // the last one writes fp32 again (the plain last c_proj / the class-rows path / ln_post read it); nothing in between
    // touches x.  Variant A, and variant C when EVERY block's adapter is folded into its GEMMs (nothing but the residual GEMMs
    // rewrites the stream): the hi half then lives in the in_proj operand buffer [x16 | e] (row stride D + 64) through the
    // whole block - attention writes into a second operand buffer [att | e] instead of over it, the decoder writes e into both, c_fc
    // reads the copy with that stride.  Only where the GEMMs run on gemm_ring2.
    bool hilo = false, hilo_c = false;      // hilo_c: variant C on it (att holds [x16 = hi | e], att2 [attention output | e])
    // gs (text tower): the LayerNorm weight rides in the activation copy (GemmArgs::gamma), the consumers multiply by the layer's own
    // fp16 weights: no second rounding of W * gamma.  That copy is c->hg behind a producer that keeps h as the stream's hi half
    // (hl 1, 2), h itself otherwise (ln_copy)
    bool gs = false;
    bool pair_on = false;
    float *x = nullptr, *mr = nullptr, *mu = nullptr, *muc = nullptr, *stats = nullptr;
    half_t *h = nullptr, *qkv = nullptr, *att = nullptr, *att_o = nullptr, *fc = nullptr, *hg = nullptr, *xlo = nullptr;
    half_t* pre16 = nullptr;      // where the step in front of block 0 writes the fp16 copy, row stride pre_ld
    int pre_ld = 0;
    std::vector<BlockPlan> blocks;
};

// GemmArgs::hl of the k-th of a call's n LayerNorm-emitting residual GEMMs, in launch order
inline int hl_at(bool hilo, int k, int n) { return !hilo ? 0 : k == 0 ? 1 : k == n - 1 ? 3 : 2; }
inline half_t* ln_copy(const TowerPlan& p, int hl) { return p.gs && (hl == 1 || hl == 2) ? p.hg : p.h; }

// the LayerNorm-emitting form of a residual GEMM: the fp16 copy of the updated rows, their partial statistics, the stream's form on
// both sides (hl) and, in the text tower, the NEXT LayerNorm's weight in the copy its consumer reads
void emit_ln(const TowerPlan& p, GemmArgs& g, half_t* copy, int ld, int hl, const float* gamma) {
    g.out2 = copy; g.ld2 = ld; g.stats = p.stats; g.stats_ld = p.sld; g.mu = p.mu;
    if (p.hilo) { g.hl = hl; g.lo = p.xlo; g.muc = p.muc; }
    if (!p.gs) return;
    g.gamma = gamma;
    if (hl == 1 || hl == 2) { g.out3 = p.hg; g.ld3 = g.N; }
}

GemmArgs fc_args(const TowerPlan& p, const BlockW& w, const BlockPlan& b, int D) {
    if (!p.fuse) return gemm_args(p.h, D, w.w_fc, w.b_fc, p.fc, 4 * D, p.M, 4 * D, D);
    GemmArgs g = gemm_args(b.a2, b.lda2, p.gs ? w.w_fc : w.wf_fc, w.bf_fc, p.fc, 4 * D, p.M, 4 * D, D);
    g.cs = p.gs ? w.csg_fc : w.cs_fc; g.mr = p.mr;
    return g;
}
// (`next`: the plan and the ln_1 weight of the block behind b - read only where b.emits)
GemmArgs proj_args(const TowerPlan& p, const BlockW& w, const BlockPlan& b, int D, const BlockPlan* next, const float* next_ln1_w) {
    GemmArgs g = gemm_args(p.fc, 4 * D, w.w_proj, w.b_proj, p.x, D, p.M, D, 4 * D);
    if (b.emits) emit_ln(p, g, next->x16, next->ldx, b.hl_proj, next_ln1_w);
    return g;
}

// Decides every path of the call and grows every buffer it needs: no ensure() - hipFree, hipMalloc, device synchronise - can fall
// between two launches of a tower call.  The buffer pointers are read once, behind the growth.
int plan_tower(hg_ctx* c, const std::vector<BlockW>& blocks, const TowerCall& t, TowerPlan& p) {
    const int n_seq = t.n_seq, L = t.L, D = t.D, heads = t.heads, M = n_seq * L;
    const size_t nb = blocks.size(), Mp = rup(M, 256);
    const AdapterCall* ac = t.ac;
    const bool adapters = ac && ac->enabled;
    const bool row0 = t.row0_out && c->opt_row0 && !adapters;
    float dummy = 0.f;
    p.M = M; p.sld = 4 * (D / 256);
    p.blocks.assign(nb, BlockPlan{});
    // With adapters the folding survives when the adapter's up_proj can re-emit the fp16 copy and statistics
    // (EPI_SCALE_RESID_LN_F32, duo kernel): option adapter_fuse = 0 selects the separate path (fp32 -> fp16 copy of the stream
    // per adapter, two LayerNorm kernels per block)
    p.fuse = t.ln_fold && ln_fuse_ok(c, M, D);
    if (p.fuse && adapters) {
        GemmArgs u = gemm_args(nullptr, 64, nullptr, nullptr, nullptr, D, M, D, 64);
        u.out2 = (half_t*)&dummy; u.stats = &dummy; u.mu = &dummy; u.pos = &dummy; u.stats_ld = p.sld;
        p.fuse = c->opt_adapter_fuse && gemm_duo_ok(EPI_SCALE_RESID_LN_F32, u);
    }
    bool any_adapter = false, any_cat = false, all_cat = adapters && nb > 0;
    for (size_t i = 0; i < nb; ++i) {
        BlockPlan& b = p.blocks[i];
        if (adapters && c->vit.adapters.size() > i && c->vit.adapters[i].present) b.adapter = &c->vit.adapters[i];
        const AdapterW::Fold* f = b.adapter ? &b.adapter->fold[ac->priors ? 0 : 1] : nullptr;
        if (f && p.fuse && c->opt_adapter_fold && f->wq_cat) {
            AdapterDev ad{};
            for (int k = 0; k < 2; ++k) ad.w16[k][0] = b.adapter->w16[k][0];
            GemmArgs q = gemm_args(nullptr, D + 64, nullptr, nullptr, nullptr, 3 * D, M, 3 * D, D + 64);
            q.cs = &dummy; q.mr = &dummy;
            if (adapter_decoder_mfma_ok(ad, ac->priors != nullptr, L, ac->N) && gemm_ln_ok(EPI_LN_BIAS_F16, q)) b.fold = f;
        }
        any_adapter = any_adapter || b.adapter;
        any_cat = any_cat || b.fold;
        all_cat = all_cat && b.fold;
    }
    const int n_rln = p.fuse ? (row0 ? 2 * ((int)nb - 1) : 2 * (int)nb - 1) : 0;      // LayerNorm-emitting residual GEMMs of the call
    // (a per-block trace of variant C reads the stream's hi half with row stride D: variant C's lives in [x16 | e] with stride D + 64 - no
    // entry point asks for that trace today; should one, it gets the fp32 stream)
    p.hilo = p.fuse && (!adapters || all_cat) && c->opt_stream_hilo && n_rln >= 2 && !(t.trace && adapters);
    if (p.hilo) {
        const int K = adapters ? D + 64 : D;
        p.hilo = gemm_ring2_ok(gemm_args(nullptr, K, nullptr, nullptr, nullptr, D, M, D, K)) &&
                 gemm_ring2_ok(gemm_args(nullptr, 4 * D, nullptr, nullptr, nullptr, D, M, D, 4 * D));
    }
    p.hilo_c = p.hilo && adapters;
    p.gs = t.gamma_act && p.fuse && !adapters && t.pre_w == nullptr;
    // blocks whose in_proj and attention run as one kernel (option qkv_attn): folded LayerNorm, a sequence per row tile
    // (192 < L <= 208), enough sequences to fill the chip
    const bool qa_on = p.fuse && !t.causal && c->opt_qkv_attn && n_seq >= c->opt_qkv_attn_min_seq && qkv_attn_ok(n_seq, L, D, heads, D) &&
                       (c->opt_qkv_attn == 2 || qkv_attn_pays(n_seq, heads, 0));
    // (with a folded adapter - variant C on the hi / lo stream - the same kernel over K = D + 64, [x16 | e] in att -> att2; without the
    // second buffer the attention output overwrites x16 in place, which other work items of the sequence are still reading)
    const bool qa_cat = qa_on && p.hilo_c && c->opt_qkv_attn_c && qkv_attn_ok(n_seq, L, D, heads, D + 64, D + 64);
    // the text tower's form (option qkv_attn_text, hg_qkv_attn_text.hip): causal, L <= 80, folded LayerNorm in either text_ln_fold
    // form, no adapters; a pack of whole sequences per row tile.  Bit-identical to the GEMM + attention_kernel it replaces.
    const bool qat_on = p.fuse && t.causal && !adapters && c->opt_qkv_attn_text && qkv_attn_text_ok(n_seq, L, D, heads, D) &&
                        (c->opt_qkv_attn_text == 2 || qkv_attn_text_pays(n_seq, L, heads, c->n_cu));
    // c_fc and c_proj of a block as ONE persistent launch (option mlp_pair, hg_mlp_pair.hip): LayerNorm-folded blocks without adapters
    // where c_proj is a LayerNorm-emitting residual GEMM on the hi / lo (or fp32) stream (every block but the tower's last)
    p.pair_panels = (int)rup(mlp_pair_ready_words(M), 64);      // words per block: the census, then a counter per 256-row panel
    p.pair_on = p.fuse && !adapters && c->opt_mlp_pair && c->pair_err && nb > 1;

    int rc = 0;
    if (any_cat) keep_first(rc, ensure(c, c->att, Mp * (size_t)(D + 64) * 2));
    if (p.fuse) {
        keep_first(rc, ensure(c, c->mr, Mp * 2 * 4));
        keep_first(rc, ensure(c, c->mu, Mp * 4));
        keep_first(rc, ensure(c, c->stats, Mp * (size_t)p.sld * 2 * 4));
        if (adapters || p.hilo) keep_first(rc, ensure(c, c->muc, Mp * 4));
    }
    if (p.gs) keep_first(rc, ensure(c, c->hg, Mp * (size_t)D * 2));
    if (p.hilo) keep_first(rc, ensure(c, c->xlo, gemm_lo_bytes(M, D)));
    if (p.hilo_c) keep_first(rc, ensure(c, c->att2, Mp * (size_t)(D + 64) * 2));
    if (p.pair_on) keep_first(rc, ensure(c, c->pair_ready, nb * (size_t)p.pair_panels * 4));
    if (any_adapter) {
        keep_first(rc, ensure(c, c->ad32, Mp * 128 * 4));
        keep_first(rc, ensure(c, c->ad16, Mp * 64 * 2));
        keep_first(rc, ensure(c, c->adkv, (size_t)n_seq * (ac->priors ? ac->N : L) * 64 * 4 * 2));
    }
    if (row0 && nb) {
        keep_first(rc, ensure(c, c->cx, (size_t)n_seq * D * 4));
        keep_first(rc, ensure(c, c->ca, rup(n_seq, 256) * D * 2));
        keep_first(rc, ensure(c, c->ch, rup(n_seq, 256) * D * 2));
        keep_first(rc, ensure(c, c->cf, rup(n_seq, 256) * (size_t)4 * D * 2));
        keep_first(rc, ensure(c, c->cq, rup(n_seq, 256) * D * 2));
    }
    if (rc) return rc;
    p.x = (float*)c->x.p; p.h = (half_t*)c->h.p; p.qkv = (half_t*)c->qkv.p; p.att = (half_t*)c->att.p; p.fc = (half_t*)c->fc.p;
    p.att_o = p.hilo_c ? (half_t*)c->att2.p : p.att;      // where the attention output (the out-proj operand) goes
    if (p.fuse) { p.mr = (float*)c->mr.p; p.mu = (float*)c->mu.p; p.stats = (float*)c->stats.p; }
    if (p.fuse && (adapters || p.hilo)) p.muc = (float*)c->muc.p;
    if (p.gs) p.hg = (half_t*)c->hg.p;
    if (p.hilo) p.xlo = (half_t*)c->xlo.p;

    for (size_t i = 0; i < nb; ++i) {
        BlockPlan& b = p.blocks[i];
        b.row0 = row0 && i + 1 == nb;
        b.emits = p.fuse && i + 1 < nb;
        b.hl_out = hl_at(p.hilo, 2 * (int)i, n_rln);
        b.hl_proj = b.emits ? hl_at(p.hilo, 2 * (int)i + 1, n_rln) : 0;
        b.x_hilo = p.hilo && (b.emits ? b.hl_proj : b.hl_out) != 3;
        b.x16 = b.fold ? p.att : p.h;
        b.ldx = b.fold ? D + 64 : D;
        b.a1 = !p.gs ? b.x16 : i == 0 ? p.hg : ln_copy(p, p.blocks[i - 1].hl_proj);
        b.a2 = p.hilo_c ? p.att : ln_copy(p, b.hl_out);
        b.lda2 = p.hilo_c ? D + 64 : D;
        const bool qa = !b.row0 && blocks[i].wp_qkv && (b.fold ? qa_cat && b.fold->wp_qcat : qa_on);
        const bool qat = qat_on && !b.row0 && (p.gs ? blocks[i].wpg_qkv : blocks[i].wp_qkv);
        b.in_proj = !p.fuse ? InProj::separate : b.fold ? (qa ? InProj::qkv_attn_cat : InProj::cat) :
                    qa ? InProj::qkv_attn : qat ? InProj::qkv_attn_text : InProj::folded;
    }
    for (size_t i = 0; p.pair_on && i + 1 < nb; ++i) {    // (the arguments name the next block's copy: behind the loop above)
        const GemmArgs fc = fc_args(p, blocks[i], p.blocks[i], D);
        const GemmArgs proj = proj_args(p, blocks[i], p.blocks[i], D, &p.blocks[i + 1], blocks[i + 1].ln1_w);
        // (the text tower keeps the 128-row kernel in either text_ln_fold form: the 256-row one has no gamma instance and has not been
        // measured at width 512)
        // (... and alone takes calls of fewer than 2 048 rows, where mlp_pair256_min_m lets it)
        p.blocks[i].pair256 = c->opt_mlp_pair256 && !t.causal && mlp_pair256_ok(fc, proj, c->n_cu, c->opt_mlp_pair256_min_m);
        p.blocks[i].pair = p.blocks[i].pair256 || mlp_pair_ok(fc, proj, c->n_cu);
    }
    p.pre16 = !t.pre_w ? (p.gs ? p.hg : p.h) : nb ? p.blocks[0].x16 : p.h;      // (rowstats_cast writes dense rows)
    p.pre_ld = t.pre_w && nb ? p.blocks[0].ldx : D;
    return HG_OK;
}

// a hand-off wait or a range overflow inside an EARLIER tower call: reported by the next one (hg_ctx::pair_err, range_flag)
int check_sticky_flags(hg_ctx* c) {
    if (c->pair_err && *(volatile int32_t*)c->pair_err) {
        *(volatile int32_t*)c->pair_err = 0;
        if (c->range_flag) *(volatile int32_t*)c->range_flag = 0;      // (whatever that call's rows overflowed into is part of the same report)
        return fail(c, HG_ERR_HIP, "a hand-off wait inside the MLP pair kernel of a previous call timed out (a workgroup of its grid never "
                                   "became resident): that call's outputs are invalid; set option mlp_pair = 0 if this device cannot "
                                   "hold one workgroup per compute unit");
    }
    if (c->range_flag && *(volatile int32_t*)c->range_flag) {
        *(volatile int32_t*)c->range_flag = 0;
        return fail(c, HG_ERR_INVALID, "in a previous call activations left the fp16 range inside a tower: a row reached more than 65504 from its "
                                       "centre, which the centred fp16 copy the LayerNorm-folded GEMMs read cannot hold (with option stream_hilo "
                                       "the residual stream itself is held in it) - that call's embeddings of those rows are invalid.  Option "
                                       "ln_fuse = 0 selects the separate-LayerNorm path");
    }
    return HG_OK;
}

// ---- the launch steps of a block: arguments from the plan, then the launch ------------------------------------------------------------
// in_proj + attention in one kernel: q, k, v stay in LDS (hg_qkv_attn.hip; the text tower's: hg_qkv_attn_text.hip); bit-identical to
// the GEMM + attention launch it replaces
QkvAttnArgs qkv_attn_args(hg_ctx* c, const TowerCall& t, const TowerPlan& p, const BlockW& w, const BlockPlan& b) {
    QkvAttnArgs qa{};
    qa.x16 = b.a1; qa.lda = b.ldx; qa.K = b.fold ? t.D + 64 : 0; qa.mr = p.mr; qa.out = p.att_o; qa.ldo = p.hilo_c ? t.D + 64 : t.D;
    qa.wp = b.fold ? b.fold->wp_qcat : p.gs ? w.wpg_qkv : w.wp_qkv;
    qa.bcs = p.gs ? w.bcsg_qkv : w.bcs_qkv;
    qa.n_seq = t.n_seq; qa.L = t.L; qa.D = t.D; qa.heads = t.heads; qa.gsz = t.causal ? 0 : c->opt_qkv_attn_gsz;
    qa.a_bytes = (unsigned)(rup(p.M, 256) * (size_t)b.ldx * 2);
    return qa;
}

int launch_in_proj_attention(hg_ctx* c, const TowerCall& t, const TowerPlan& p, const BlockW& w, const BlockPlan& b) {
    const int D = t.D, K = b.ldx;
    hipStream_t s = t.s;
    // in_proj rows [qoff, 3D): the class-rows-only last block needs K and V of every row but Q of row 0 only
    const size_t qoff = b.row0 ? D : 0;
    GemmArgs g = gemm_args(b.a1, K, w.w_qkv + qoff * D, w.b_qkv + qoff, p.qkv + qoff, 3 * D, p.M, 3 * D - (int)qoff, K);
    switch (b.in_proj) {
    case InProj::qkv_attn: case InProj::qkv_attn_cat: case InProj::qkv_attn_text: {
        const QkvAttnArgs qa = qkv_attn_args(c, t, p, w, b);
        ProfScope ps(c, s, HG_PROF_QKV_ATTN, t.n_seq, t.L, t.heads);
        HG_HIP(b.in_proj == InProj::qkv_attn_text ? launch_qkv_attn_text(qa, s) : launch_qkv_attn(qa, s));
        return HG_OK;
    }
    case InProj::cat:      // ln_1(x + a) W^T: [x16 | e] x [W'_qkv | W'_qkv Q], the statistics are those of x + a
        g.W = b.fold->wq_cat; g.bias = w.bf_qkv; g.cs = w.cs_qkv; g.mr = p.mr;
        HG_HIP(gemm(c, EPI_LN_BIAS_F16, g, s));
        break;
    case InProj::folded:
        if (!p.gs) g.W = w.wf_qkv + qoff * D;
        g.bias = w.bf_qkv + qoff; g.cs = (p.gs ? w.csg_qkv : w.cs_qkv) + qoff; g.mr = p.mr;
        HG_HIP(gemm(c, EPI_LN_BIAS_F16, g, s));
        break;
    case InProj::separate:
        HG_HIP(launch_layernorm_f16(p.x, w.ln1_w, w.ln1_b, p.h, p.M, D, nullptr, 0, 1, s));
        HG_HIP(gemm(c, EPI_BIAS_F16, g, s));
        break;
    }
    if (!b.row0) HG_HIP(attention(c, p.qkv, p.att_o, t.n_seq, t.L, t.heads, t.causal, s, b.fold ? D + 64 : 0));
    return HG_OK;
}

int launch_out_proj(hg_ctx* c, const TowerCall& t, const TowerPlan& p, const BlockW& w, const BlockPlan& b) {
    const int D = t.D, K = b.ldx;
    // with a folded adapter x += [att | e] [W_out | Q]^T + b_out: the adapter's update rides along
    GemmArgs g = gemm_args(p.att_o, K, b.fold ? b.fold->wk_out : w.w_out, w.b_out, p.x, D, p.M, D, K);
    if (!p.fuse) {
        HG_HIP(gemm(c, EPI_BIAS_RESID_F32, g, t.s));
        return HG_OK;
    }
    emit_ln(p, g, p.hilo_c ? p.att : p.h, b.lda2, b.hl_out, w.ln2_w);      // (hilo_c: the copy = the stream's hi half stays in [x16 | e])
    HG_HIP(gemm(c, EPI_RESID_LN_F32, g, t.s));
    HG_HIP(launch_finalize_stats(p.stats, p.mr, p.mu, p.M, p.sld, 64, t.s, p.muc, false, c->range_flag));
    return HG_OK;
}

// c_fc -> QuickGELU -> c_proj: the pair launch, or two GEMMs
int launch_mlp(hg_ctx* c, const TowerCall& t, const TowerPlan& p, const std::vector<BlockW>& blocks, size_t i) {
    const BlockW& w = blocks[i];
    const BlockPlan& b = p.blocks[i];
    const int D = t.D;
    hipStream_t s = t.s;
    if (!p.fuse) HG_HIP(launch_layernorm_f16(p.x, w.ln2_w, w.ln2_b, p.h, p.M, D, nullptr, 0, 1, s));
    const GemmArgs fc = fc_args(p, w, b, D);
    // (the last block is followed by ln_post / ln_final on selected rows: a plain residual GEMM)
    const GemmArgs proj = proj_args(p, w, b, D, b.emits ? &p.blocks[i + 1] : nullptr, b.emits ? blocks[i + 1].ln1_w : nullptr);
    if (b.pair) {
        PairGateScope gate(c->device, s);
        ProfScope ps(c, s, HG_PROF_MLP_PAIR, p.M, 4 * D, D);
        unsigned* ready = (unsigned*)c->pair_ready.p + i * (size_t)p.pair_panels;
        if (b.pair256) ++c->n_pair256_launches;
        if (b.pair256 && c->opt_mlp_pair256_ph2)
            HG_HIP(launch_mlp_pair256p(fc, proj, ready, c->pair_err, c->opt_mlp_pair256_chunk, c->opt_mlp_pair256_ratio, c->n_cu, s, c->opt_mlp_pair_fault));
        else if (b.pair256)
            HG_HIP(launch_mlp_pair256(fc, proj, ready, c->pair_err, c->opt_mlp_pair256_chunk, c->opt_mlp_pair256_ratio, c->n_cu, s, c->opt_mlp_pair_fault));
        else
            HG_HIP(launch_mlp_pair(fc, proj, ready, c->pair_err, c->opt_mlp_pair_chunk, c->opt_mlp_pair_fc_slots, c->n_cu, s, c->opt_mlp_pair_fault));
    } else {
        HG_HIP(gemm(c, p.fuse ? EPI_LN_BIAS_QGELU_F16 : EPI_BIAS_QGELU_F16, fc, s));
        // c_proj as hi + lo (hg_load_vit) behind adapters on a tower of more than 224 tokens: x += fc x lo^T * 2^-11 on the fp32 stream
        // (no adapter is folded there, so the stream is never hi + lo), in FRONT of the pass that emits the next LayerNorm's copy
        if (w.w_proj_lo && b.adapter && !p.hilo) {
            GemmArgs lo = gemm_args(p.fc, 4 * D, w.w_proj_lo, c->vit.lo_scale + D, p.x, D, p.M, D, 4 * D);
            lo.pos = c->vit.lo_scale;
            HG_HIP(gemm(c, EPI_SCALE_RESID_F32, lo, s));
        }
        HG_HIP(gemm(c, b.emits ? EPI_RESID_LN_F32 : EPI_BIAS_RESID_F32, proj, s));
    }
    if (b.emits) HG_HIP(launch_finalize_stats(p.stats, p.mr, p.mu, p.M, p.sld, 64, s, p.muc, false, c->range_flag));
    return HG_OK;
}

// the rest of the tower's last block on the n_seq selected rows (behind in_proj's K and V of every row): a dense [n_seq, D] stream
int launch_row0_block(hg_ctx* c, const TowerCall& t, const TowerPlan& p, const BlockW& w, float* trace_entry) {
    const int n = t.n_seq, L = t.L, D = t.D;
    hipStream_t s = t.s;
    float* cx = (float*)c->cx.p;
    half_t *ca = (half_t*)c->ca.p, *ch = (half_t*)c->ch.p, *cf = (half_t*)c->cf.p, *cq = (half_t*)c->cq.p;
    // Q of the selected rows: ln_1 on those rows, then the first D rows of in_proj
    if (t.sel) HG_HIP(launch_layernorm_f16(p.x, w.ln1_w, w.ln1_b, ch, n, D, t.sel, L, 0, s));
    else HG_HIP(launch_layernorm_f16(p.x, w.ln1_w, w.ln1_b, ch, n, D, nullptr, 0, L, s));
    HG_HIP(gemm(c, EPI_BIAS_F16, gemm_args(ch, D, w.w_qkv, w.b_qkv, cq, D, n, D, D), s));
    HG_HIP(launch_attention_row0(p.qkv, cq, t.sel, ca, n, L, t.heads, t.causal, s));
    HG_HIP(launch_copy_rows(p.x, cx, n, L, D, s, t.sel));
    HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(ca, D, w.w_out, w.b_out, cx, D, n, D, D), s));
    HG_HIP(launch_layernorm_f16(cx, w.ln2_w, w.ln2_b, ch, n, D, nullptr, 0, 1, s));
    HG_HIP(gemm(c, EPI_BIAS_QGELU_F16, gemm_args(ch, D, w.w_fc, w.b_fc, cf, 4 * D, n, 4 * D, D), s));
    HG_HIP(gemm(c, EPI_BIAS_RESID_F32, gemm_args(cf, 4 * D, w.w_proj, w.b_proj, cx, D, n, D, 4 * D), s));
    if (trace_entry) HG_HIP(launch_copy_rows(cx, trace_entry, n, 1, D, s));
    *t.row0_out = cx;
    return HG_OK;
}

// trace entry `entry`: the stream as it stands, from (h, xlo, muc) where it lives there (after finalize_stats muc is the centre the
// stream's hi / lo halves were written with)
hipError_t launch_trace_copy(const TowerCall& t, const TowerPlan& p, int entry, bool x_hilo) {
    float* tr = t.trace + (size_t)entry * t.trace_stride;
    const int rows = t.trace_all ? p.M : t.n_seq, stride = t.trace_all ? 1 : t.L;      // rows a trace entry holds, their stride in the stream
    if (x_hilo) return launch_copy_rows_hilo(p.h, p.xlo, p.muc, tr, rows, stride, t.D, t.s);
    return launch_copy_rows(p.x, tr, rows, stride, t.D, t.s);
}

int run_blocks(hg_ctx* c, const std::vector<BlockW>& blocks, const TowerCall& t) {
    if (t.row0_out) *t.row0_out = nullptr;
    if (int rc = check_sticky_flags(c)) return rc;
    const bool adapters = t.ac && t.ac->enabled;
    if (adapters && !t.pre_w) return fail(c, HG_ERR_INVALID, "a tower with instance adapters needs its ln_pre (the adapters' copy of the stream is written by it)");
    TowerPlan plan;
    if (int rc = plan_tower(c, blocks, t, plan)) return rc;
    const TowerPlan& p = plan;
    const int D = t.D;
    hipStream_t s = t.s;
    float* const muc_pre = adapters ? p.muc : nullptr;
    if (p.fuse && t.pre_w) HG_HIP(launch_layernorm_rowstats(p.x, t.pre_w, t.pre_b, p.pre16, p.mr, p.mu, muc_pre, p.M, D, s, t.pre_pos, t.pre_cls, t.L, p.pre_ld));
    else if (p.fuse) HG_HIP(launch_rowstats_cast(p.x, p.pre16, p.mr, p.mu, p.M, D, s, muc_pre, p.gs ? blocks[0].ln1_w : nullptr));
    else if (t.pre_w) HG_HIP(launch_layernorm_f32(p.x, t.pre_w, t.pre_b, p.x, p.M, D, s, t.pre_pos, t.pre_cls, t.L));
    if (t.trace) HG_HIP(launch_trace_copy(t, p, 0, false));      // (x is the fp32 stream here: the folding kernels only read it)
    if (p.pair_on) HG_HIP(hipMemsetAsync(c->pair_ready.p, 0, blocks.size() * (size_t)p.pair_panels * 4, s));
    for (size_t i = 0; i < blocks.size(); ++i) {
        const BlockPlan& b = p.blocks[i];
        int rc = HG_OK;
        if (b.adapter) rc = run_adapter(c, *b.adapter, t.n_seq, t.L, D, *t.ac, s, p.fuse, b.fold != nullptr, p.hilo_c ? p.att_o + D : nullptr, true);
        if (!rc) rc = launch_in_proj_attention(c, t, p, blocks[i], b);
        const bool tr = t.trace && !(t.trace_entries_only && i + 1 == blocks.size());
        if (!rc && b.row0) return launch_row0_block(c, t, p, blocks[i], tr ? t.trace + (i + 1) * (size_t)t.trace_stride : nullptr);
        if (!rc) rc = launch_out_proj(c, t, p, blocks[i], b);
        if (!rc) rc = launch_mlp(c, t, p, blocks, i);
        if (rc) return rc;
        if (tr) HG_HIP(launch_trace_copy(t, p, (int)i + 1, b.x_hilo));
    }
    return HG_OK;
}

int ensure_tower_ws(hg_ctx* c, int M, int D) {
    const size_t Mp = rup(M, 256);
    int rc = 0;
    keep_first(rc, ensure(c, c->x, Mp * D * 4));
    keep_first(rc, ensure(c, c->h, Mp * D * 2));
    keep_first(rc, ensure(c, c->qkv, Mp * 3 * D * 2));
    keep_first(rc, ensure(c, c->att, Mp * D * 2));
    keep_first(rc, ensure(c, c->fc, Mp * 4 * D * 2));
    return rc;
}

// Crops per pass of the image tower: max_chunk_img (256) for every tower of up to 224 tokens; a longer one gets the ROWS such a pass
// can hold at most (256 x 224 = 57 344: 99 crops of 577 tokens), so no workspace grows beyond what a 224-token tower of the same width
// takes and every GEMM stays far inside gemm_ring_ok's 32-bit byte offsets (Mp x 4096 x 2 < 2^31 at 262 144 rows).  Rows of different
// crops never meet in any kernel, so where the boundary falls does not reach the results.
int image_chunk(const hg_ctx* c, int L) {
    if (L <= ATTN_MAX_L_RESIDENT) return c->max_chunk_img;
    const int n = c->max_chunk_img * ATTN_MAX_L_RESIDENT / L;
    return n > 0 ? n : 1;
}
// `trace_all` (hg_test_image_stream): every row of the stream into `trace`, one entry of B * L rows per block - one chunk only
int encode_image_impl(hg_ctx* c, const float* x_nchw, const float* priors, const uint8_t* mask, int B, int N,
                             float* out, float* out_local, float* trace, bool variant_c, hipStream_t s, bool trace_all = false) {
    if (!c) return HG_ERR_INVALID;
    Vit& v = c->vit;
    if (!v.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_vit has not been called");
    if (B == 0) return HG_OK;
    if (B < 0 || !x_nchw || !out) return fail(c, HG_ERR_INVALID, "bad arguments to encode_image");
    if (variant_c && !out_local) return fail(c, HG_ERR_INVALID, "out_local == NULL");
    if (priors && (N <= 0 || !mask)) return fail(c, HG_ERR_INVALID, "priors given but N <= 0 or mask == NULL");
    HG_ON_DEVICE(c);
    const int D = v.D, L = v.L, G = L - 1, E = v.E;
    if (variant_c && L > adapter_max_tokens(c))      // (a tower loaded with option adapter_long = 1, the option taken back since)
        for (const AdapterW& a : v.adapters)
            if (a.present)
                return fail(c, HG_ERR_INVALID, "instance adapters support at most %d tokens per image: this tower has %d%s", adapter_max_tokens(c),
                            L, adapter_long_hint(c, L));
    const size_t img = (size_t)3 * v.res * v.res;
    const int chunk = image_chunk(c, L);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int Bc = (B - b0 < chunk) ? B - b0 : chunk;
        const int M = Bc * L;
        int rc = ensure_tower_ws(c, M, D);
        if (!rc) rc = ensure(c, c->head16, rup(variant_c ? M : Bc, 256) * D * 2);
        if (!rc && variant_c) rc = ensure(c, c->tok32, (size_t)M * E * 4);
        if (!rc) rc = ensure(c, c->fc, rup((size_t)Bc * G, 256) * (v.Kp > 4 * D ? v.Kp : 4 * D) * 2);
        if (rc) return rc;
        float* x = (float*)c->x.p;
        half_t* patches = (half_t*)c->fc.p;
        // conv1 as GEMM over the patch matrix; epilogue scatters to token rows 1.. and adds pos
        HG_HIP(launch_im2col(x_nchw + (size_t)b0 * img, patches, Bc, v.res, v.patch, s));
        // class rows, positional embedding and ln_pre are one pass over the rows (run_blocks): the GEMM only scatters
        GemmArgs g = gemm_args(patches, v.Kp, v.w_patch, nullptr, x, D, Bc * G, D, v.Kp);
        g.G = G; g.L = L;
        HG_HIP(gemm(c, EPI_PATCH_F32, g, s));
        float* tr = trace ? trace + (trace_all ? 0 : (size_t)b0 * D) : nullptr;      // (row 0 of the trace = after ln_pre: copied inside run_blocks)
        const int tstride = trace_all ? M * D : B * D;
        const AdapterCall ac{priors ? priors + (size_t)b0 * N * 64 : nullptr, mask ? mask + (size_t)b0 * N : nullptr, N, variant_c};
        const float* row0 = nullptr;      // dense class-token rows when the last block ran on them only
        TowerCall t;
        t.n_seq = Bc; t.L = L; t.D = D; t.heads = v.heads; t.s = s;
        t.trace = tr; t.trace_stride = tstride; t.trace_all = trace_all;
        t.ac = &ac; t.ln_fold = true;
        t.pre_w = v.lnpre_w; t.pre_b = v.lnpre_b; t.pre_pos = v.pos; t.pre_cls = v.cls;
        t.row0_out = variant_c ? nullptr : &row0;
        rc = run_blocks(c, v.blocks, t);
        if (rc) return rc;
        half_t* h16 = (half_t*)c->head16.p;
        if (!variant_c) {
            // ln_post(x[:,0,:]) @ proj   (clipnet/model.py:231-234)
            if (row0) HG_HIP(launch_layernorm_f16(row0, v.lnpost_w, v.lnpost_b, h16, Bc, D, nullptr, 0, 1, s));
            else HG_HIP(launch_layernorm_f16(x, v.lnpost_w, v.lnpost_b, h16, Bc, D, nullptr, 0, L, s));
            HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(h16, D, v.w_projT, nullptr, out + (size_t)b0 * E, E, Bc, E, D), s));
        } else {
            // ln_post + proj on all tokens, split into (global, local NCHW)  (adapter...:501-506)
            HG_HIP(launch_layernorm_f16(x, v.lnpost_w, v.lnpost_b, h16, M, D, nullptr, 0, 1, s));
            g = gemm_args(h16, D, v.w_projT, nullptr, c->tok32.p, E, M, E, D);
            HG_HIP(gemm(c, EPI_BIAS_F32, g, s));
            if (v.w_projT_lo) {      // + h16 x lo (hg_load_vit): tok32 += (acc + 0) * 2^-11
                g.W = v.w_projT_lo; g.pos = v.proj_lo_scale; g.bias = v.proj_lo_scale + E;
                HG_HIP(gemm(c, EPI_SCALE_RESID_F32, g, s));
            }
            HG_HIP(launch_split_global_local((const float*)c->tok32.p, out + (size_t)b0 * E,
                                             out_local + (size_t)b0 * E * G, Bc, L, E, s));
        }
    }
    return HG_OK;
}

// ---- text tower -------------------------------------------------------------------------------------------
// A truncation length that does not cover every EOT position (a stale host-side max(EOT)) must not gather
// another sequence's row or read out of bounds: EOT indices are clamped into [0, Leff) on the device; the same flag turns the
// WHOLE output of that call into NaN at its end (the stale call itself is loud: launch_poison_if_flag) and, being sticky and
// host-mapped, makes the NEXT text call fail with HG_ERR_INVALID and an explanation (this call cannot be failed without a sync).
int text_check_flag(hg_ctx* c) {
    if (c->eot_flag && *(volatile int32_t*)c->eot_flag) {
        *(volatile int32_t*)c->eot_flag = 0;
        return fail(c, HG_ERR_INVALID, "a previous encode_text call was given trunc < max(EOT)+1: its EOT rows were clamped and "
                                       "its outputs are invalid (recompute the truncation length from the current token ids)");
    }
    return HG_OK;
}

// Prompts per pass of the text tower: a budget of ROWS, so that a call truncated to the 13-16 tokens its prompts really have (the
// generation pipeline: main_tip_finetune.py:759-824) fills the GEMMs' row tiles like a full-length one does - 640 prompts of 13 tokens
// are 33 row tiles of 256 on 256 CUs.  The budget is 65 536 rows: with D = 512 every GEMM of a block then fills whole rounds (residual
// GEMMs 512 x 2 tiles of 128 x 256 on 2 x 256 workgroups; in_proj 256 x 6 and c_fc 256 x 8 tiles of 256 x 256 on 256) - the 49 280
// rows of 640 full-length prompts leave them at 1.50, 4.52 and 6.03 rounds.  A call longer than one pass is cut into EQUAL passes
// (no small tail pass).  A call that fits one pass is one pass, as before (600 prompts x 77 tokens = 46 200 rows).
int text_chunk_prompts(const hg_ctx* c, int n_prompts, int Leff) {
    const long budget = c->text_rows_budget, L = Leff > 0 ? Leff : 1;
    long per = budget / L;
    if (per < 1) per = 1;
    if (n_prompts <= per) return n_prompts > 0 ? n_prompts : 1;
    const long passes = (n_prompts + per - 1) / per;
    return (int)((n_prompts + passes - 1) / passes);
}

// `trace` (hg_test_text_stream): every row of the stream, [layers + 1][Tc * Leff][D]
// `saved` (hg_encode_text_embeds_save): the stream as it enters every block, [layers][Tc * Leff][D], and behind it the last block's output
// on the EOT rows, [Tc][D] - what the backward recomputes the blocks from.  The same launches otherwise
int text_tail(hg_ctx* c, int Tc, int Leff, const int32_t* eot, float* out, hipStream_t s, float* trace = nullptr, float* saved = nullptr) {
    Text& t = c->text;
    const int D = t.D, E = t.E;
    // option text_ln_fold: 1 (default) folds the LayerNorms with gamma riding in the ACTIVATION copy (6.2e-4 against the reference's
    // fixture, closer than the separate kernels' 6.5e-4, 5.35 -> 5.15 ms for 600 x 77 tokens); 2 folds gamma into the weights (4.8 ms,
    // 7.6e-4, worst prompt 9.6e-4 of the 1e-3 budget); 0 runs the separate kernels
    const float* rows = nullptr;      // dense EOT rows when the last block ran on them only
    if (c->opt_qkv_attn_text && c->opt_text_ln_fold) {
        int rcp = ensure_text_packs(c, t.owned, t.blocks, D, c->opt_text_ln_fold == 1);
        if (rcp) return rcp;
    }
    TowerCall call;
    call.n_seq = Tc; call.L = Leff; call.D = D; call.heads = t.heads; call.causal = true; call.s = s;
    call.trace = saved ? saved : trace; call.trace_stride = Tc * Leff * D; call.trace_all = call.trace != nullptr;
    call.trace_entries_only = saved != nullptr;
    call.ln_fold = c->opt_text_ln_fold != 0; call.gamma_act = c->opt_text_ln_fold == 1;
    call.sel = eot; call.row0_out = &rows;
    int rc = run_blocks(c, t.blocks, call);
    if (rc) return rc;
    half_t* h16 = (half_t*)c->head16.p;
    if (saved) HG_HIP(launch_copy_rows(rows ? rows : (const float*)c->x.p, saved + t.blocks.size() * (size_t)Tc * Leff * D, Tc, rows ? 1 : Leff, D, s,
                                       rows ? nullptr : eot));
    // ln_final, select the EOT row, @ text_projection (clipnet/model.py:346-350); LN is row-wise so
    // selecting before normalising is identical
    if (rows) HG_HIP(launch_layernorm_f16(rows, t.lnf_w, t.lnf_b, h16, Tc, D, nullptr, 0, 1, s));
    else HG_HIP(launch_layernorm_f16((const float*)c->x.p, t.lnf_w, t.lnf_b, h16, Tc, D, eot, Leff, 0, s));
    HG_HIP(gemm(c, EPI_BIAS_F32, gemm_args(h16, D, t.w_projT, nullptr, out, E, Tc, E, D), s));
    return HG_OK;
}

int encode_text_ids_impl(hg_ctx* c, const int32_t* ids, int T, int L, float* out, int trunc, float* trace, void* stream) {
    if (!c) return HG_ERR_INVALID;
    Text& t = c->text;
    if (!t.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_text has not been called");
    if (T == 0) return HG_OK;
    if (T < 0 || !ids || !out || L < 1 || L > t.ctx) return fail(c, HG_ERR_INVALID, "bad arguments to encode_text_ids");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    if (int frc = text_check_flag(c)) return frc;
    const int Leff = (trunc > 0 && trunc < L) ? trunc : L;
    if (Leff < L && c->eot_flag_dev) HG_HIP(hipMemsetAsync(c->eot_flag_dev, 0, 4, s));
    const int chunk = text_chunk_prompts(c, T, Leff);
    if (trace && chunk < T) return fail(c, HG_ERR_INVALID, "hg_test_text_stream: the call is longer than one pass of the text tower");
    for (int t0 = 0; t0 < T; t0 += chunk) {
        const int Tc = (T - t0 < chunk) ? T - t0 : chunk;
        int rc = ensure_tower_ws(c, Tc * Leff, t.D);
        if (!rc) rc = ensure(c, c->head16, rup(Tc, 256) * t.D * 2);
        if (!rc) rc = ensure(c, c->i32, (size_t)(Tc + 4) * 4);
        if (rc) return rc;
        int32_t* eot = (int32_t*)c->i32.p;
        // EOT position = argmax over the FULL row (clipnet/model.py:350); must lie inside Leff
        HG_HIP(launch_eot_argmax(ids + (size_t)t0 * L, Tc, L, eot, nullptr, s));
        if (Leff < L) HG_HIP(launch_clamp_eot(eot, Tc, Leff, eot, c->eot_flag, s, c->eot_flag_dev));
        HG_HIP(launch_embed_tokens(ids + (size_t)t0 * L, L, t.tok, t.pos, (float*)c->x.p, Tc, Leff, t.D, t.vocab, s));
        rc = text_tail(c, Tc, Leff, eot, out + (size_t)t0 * t.E, s, trace);
        if (rc) return rc;
    }
    if (Leff < L) HG_HIP(launch_poison_if_flag(out, (size_t)T * t.E, c->eot_flag_dev, s));
    return HG_OK;
}

}  // namespace

extern "C" {

int hg_encode_image(hg_ctx* c, const float* x_nchw, int B, float* out, void* stream) {
    return encode_image_impl(c, x_nchw, nullptr, nullptr, B, 0, out, nullptr, nullptr, false, (hipStream_t)stream);
}
int hg_encode_image_trace(hg_ctx* c, const float* x_nchw, int B, float* out, float* trace, void* stream) {
    return encode_image_impl(c, x_nchw, nullptr, nullptr, B, 0, out, nullptr, trace, false, (hipStream_t)stream);
}
int hg_test_image_stream(hg_ctx* c, const float* x_nchw, int B, float* out, float* trace, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!c->vit.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_vit has not been called");
    for (const AdapterW& a : c->vit.adapters)
        if (a.present) return fail(c, HG_ERR_INVALID, "hg_test_image_stream: adapters are loaded (under a trace the tower leaves the hi / lo "
                                                      "stream, a path production does not run)");
    if (B < 1 || B > image_chunk(c, c->vit.L) || !trace) return fail(c, HG_ERR_INVALID, "hg_test_image_stream: B must be 1..one chunk, trace != NULL");
    return encode_image_impl(c, x_nchw, nullptr, nullptr, B, 0, out, nullptr, trace, false, (hipStream_t)stream, true);
}
int hg_encode_image_prior(hg_ctx* c, const float* x_nchw, const float* priors, const uint8_t* mask, int B, int N,
                          float* out_global, float* out_local_nchw, void* stream) {
    return encode_image_impl(c, x_nchw, priors, mask, B, priors ? N : 0, out_global, out_local_nchw, nullptr, true,
                             (hipStream_t)stream);
}

// One launch of run_adapter on a caller-supplied stream, the workspace prepared as plan_tower and the step in front of the block leave it:
// ln_pre in front of block 0 (centre = the row's mean) or, with `centre`, the preceding block's last residual GEMM (tests/test_gpu_adapter.py).
// Refuses the shapes run_adapter has no path for; mode 2 takes any number of rows (plan_tower folds from 512 rows on: the launches of
// mode 2 - down_proj on the simple GEMM or inside the decoder, one workgroup per sequence - do not depend on it), without the second
// operand buffer e2 of the hi / lo stream (a second store of the same registers).
int hg_test_adapter(hg_ctx* c, int block, int mode, const float* x, const float* centre, int n_seq, int L, int D, const float* priors,
                    const uint8_t* mask, int N,
                    float* out, float* copy_out, float* mr_out, float* muc_out, float* q_out, int32_t* path, void* stream) {
    if (!c) return HG_ERR_INVALID;
    Vit& v = c->vit;
    if (!v.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_vit has not been called");
    if (block < 0 || block >= (int)v.adapters.size() || !v.adapters[block].present)
        return fail(c, HG_ERR_INVALID, "hg_test_adapter: block %d carries no adapter", block);
    if (mode < 0 || mode > 2) return fail(c, HG_ERR_INVALID, "hg_test_adapter: mode must be 0, 1 or 2 (got %d)", mode);
    if (!x || !out || n_seq < 1 || L < 1) return fail(c, HG_ERR_INVALID, "hg_test_adapter: x, out, n_seq >= 1 and L >= 1 are needed");
    if (L > adapter_max_tokens(c))
        return fail(c, HG_ERR_INVALID, "hg_test_adapter: the adapters serve at most %d tokens (got %d)%s", adapter_max_tokens(c), L, adapter_long_hint(c, L));
    if (mode == 2 && L > ADAPTER_MAX_L)
        return fail(c, HG_ERR_INVALID, "hg_test_adapter: the adapter folded into the block's GEMMs (mode 2) serves at most %d tokens (got %d)", ADAPTER_MAX_L, L);
    if (priors && N < 1) return fail(c, HG_ERR_INVALID, "hg_test_adapter: priors given but N <= 0");
    if (mode >= 1 && (!mr_out || !muc_out || (mode == 1 && !copy_out)))
        return fail(c, HG_ERR_INVALID, "hg_test_adapter: modes 1 and 2 return mr and muc (mode 1: the fp16 copy as well)");
    const AdapterW& a = v.adapters[block];
    if (D != v.D) return fail(c, HG_ERR_INVALID, "hg_test_adapter: the stream is %d wide, the tower %d", D, v.D);
    if (centre && mode == 0) return fail(c, HG_ERR_INVALID, "hg_test_adapter: mode 0 reads the fp32 stream, it has no centre");
    const int M = n_seq * L, sld = 4 * (D / 256);
    if (!priors) N = 0;
    AdapterDev ad{};
    for (int k = 0; k < 2; ++k) ad.w16[k][0] = a.w16[k][0];
    const bool mfma = adapter_decoder_mfma_ok(ad, priors != nullptr, L, N);
    const bool mfma_long = adapter_decoder_long_ok(ad, priors != nullptr, L, N);
    const bool down_fused = mode == 2 && adapter_decoder_fused_down_ok(ad, priors != nullptr, L, N);
    if (mode >= 1 && D % 256) return fail(c, HG_ERR_INVALID, "hg_test_adapter: LayerNorm folding needs a width that is a multiple of 256 (got %d)", D);
    if (mode == 1) {      // plan_tower: folding stays on behind an adapter only where its up_proj can re-emit the copy and the statistics
        float dummy = 0.f;
        GemmArgs u = gemm_args(nullptr, 64, nullptr, nullptr, nullptr, D, M, D, 64);
        u.out2 = (half_t*)&dummy; u.stats = &dummy; u.mu = &dummy; u.pos = &dummy; u.stats_ld = sld;
        if (!gemm_duo_ok(EPI_SCALE_RESID_LN_F32, u))
            return fail(c, HG_ERR_INVALID, "hg_test_adapter: mode 1 needs at least 512 rows (got %d): the scaled residual GEMM that re-emits the copy", M);
    }
    if (mode == 2) {
        if (priors && N > 32) return fail(c, HG_ERR_INVALID, "hg_test_adapter: the folded adapter serves at most 32 prior tokens (got %d)", N);
        if (!mfma || !a.fold[priors ? 0 : 1].wq_cat) return fail(c, HG_ERR_INVALID, "hg_test_adapter: this adapter was loaded without its folded operands");
    }
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t Mp = rup(M, 256);
    int rc = 0;
    keep_first(rc, ensure(c, c->x, Mp * D * 4));
    keep_first(rc, ensure(c, c->h, Mp * D * 2));
    keep_first(rc, ensure(c, c->ad32, Mp * 128 * 4));
    keep_first(rc, ensure(c, c->ad16, Mp * 64 * 2));
    keep_first(rc, ensure(c, c->adkv, (size_t)n_seq * (priors ? N : L) * 64 * 4 * 2));
    if (mode >= 1) {
        keep_first(rc, ensure(c, c->mr, Mp * 2 * 4));
        keep_first(rc, ensure(c, c->mu, Mp * 4));
        keep_first(rc, ensure(c, c->muc, Mp * 4));
        keep_first(rc, ensure(c, c->stats, Mp * (size_t)sld * 2 * 4));
    }
    if (mode == 2) keep_first(rc, ensure(c, c->att, Mp * (size_t)(D + 64) * 2));
    if (rc) return rc;
    HG_HIP(hipMemcpyAsync(c->x.p, x, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    // the centred fp16 copy, its centre and the statistics of the stream as the step in front of the block leaves them
    if (mode >= 1) HG_HIP(launch_rowstats_cast((const float*)c->x.p, (half_t*)c->h.p, (float*)c->mr.p, (float*)c->mu.p, M, D, s, (float*)c->muc.p));
    // ... or, with `centre`, as a preceding block's last residual GEMM + finalize_stats leave them: the copy written with the row's
    // PREVIOUS mean as its centre, muc = that centre, mu = the mean, mr = (mean - centre, rstd)
    if (centre) HG_HIP(launch_recentre_cast((const float*)c->x.p, centre, (half_t*)c->h.p, D, (float*)c->mr.p, (const float*)c->mu.p, (float*)c->muc.p, M, D, s));
    if (mode == 2)      // ... in columns 0 .. D-1 of the in_proj operand buffer [x16 | e]
        HG_HIP(hipMemcpy2DAsync(c->att.p, (size_t)(D + 64) * 2, c->h.p, (size_t)D * 2, (size_t)D * 2, M, hipMemcpyDeviceToDevice, s));
    const AdapterCall ac{priors, priors ? mask : nullptr, N, true};
    if (int r = run_adapter(c, a, n_seq, L, D, ac, s, mode >= 1, mode == 2, nullptr, false)) return r;
    if (path) { path[0] = mfma_long ? 2 : mfma ? 1 : 0; path[1] = down_fused ? 1 : 0; }
    if (mode == 2) {
        HG_HIP(hipMemcpy2DAsync(c->ad16.p, 64 * 2, (const half_t*)c->att.p + D, (size_t)(D + 64) * 2, 64 * 2, M, hipMemcpyDeviceToDevice, s));
        HG_HIP(launch_f16_to_f32((const half_t*)c->ad16.p, out, (size_t)M * 64, s));
        if (q_out) {      // Q as the block's GEMMs hold it: columns D .. D+63 of [W_out | Q] (h is free again: Mp >= 64 rows of D)
            HG_HIP(hipMemcpy2DAsync(c->h.p, 64 * 2, a.fold[priors ? 0 : 1].wk_out + D, (size_t)(D + 64) * 2, 64 * 2, D, hipMemcpyDeviceToDevice, s));
            HG_HIP(launch_f16_to_f32((const half_t*)c->h.p, q_out, (size_t)D * 64, s));
        }
    } else {
        HG_HIP(hipMemcpyAsync(out, c->x.p, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
    }
    if (mode == 1) HG_HIP(launch_f16_to_f32((const half_t*)c->h.p, copy_out, (size_t)M * D, s));
    if (mode >= 1) {
        HG_HIP(hipMemcpyAsync(mr_out, c->mr.p, (size_t)M * 2 * 4, hipMemcpyDeviceToDevice, s));
        HG_HIP(hipMemcpyAsync(muc_out, c->muc.p, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    }
    return HG_OK;
}

int hg_encode_text_ids(hg_ctx* c, const int32_t* ids, int T, int L, float* out, int trunc, void* stream) {
    return encode_text_ids_impl(c, ids, T, L, out, trunc, nullptr, stream);
}
int hg_test_text_stream(hg_ctx* c, const int32_t* ids, int T, int L, int trunc, float* out, float* trace, void* stream) {
    if (c && (T < 1 || !trace)) return fail(c, HG_ERR_INVALID, "hg_test_text_stream: T must be >= 1, trace != NULL");
    return encode_text_ids_impl(c, ids, T, L, out, trunc, trace, stream);
}

static int encode_text_embeds_impl(hg_ctx* c, const float* prompts, const int32_t* eot_idx, int R, int L, float* out, int trunc,
                                   float* saved, void* stream) {
    if (!c) return HG_ERR_INVALID;
    Text& t = c->text;
    if (!t.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_text has not been called");
    if (R == 0) return HG_OK;
    if (R < 0 || !prompts || !eot_idx || !out || L < 1 || L > t.ctx)
        return fail(c, HG_ERR_INVALID, "bad arguments to encode_text_embeds");
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    if (int frc = text_check_flag(c)) return frc;
    const int Leff = (trunc > 0 && trunc < L) ? trunc : L;
    if (Leff < L && c->eot_flag_dev) HG_HIP(hipMemsetAsync(c->eot_flag_dev, 0, 4, s));
    const int chunk = text_chunk_prompts(c, R, Leff);
    if (saved && chunk < R)
        return fail(c, HG_ERR_INVALID, "hg_encode_text_embeds_save: %d prompts of %d tokens are more than one pass of the text tower (a row budget of "
                                       "%d rows: at most %d prompts of this length)", R, Leff, c->text_rows_budget, chunk);
    for (int r0 = 0; r0 < R; r0 += chunk) {
        const int Rc = (R - r0 < chunk) ? R - r0 : chunk;
        int rc = ensure_tower_ws(c, Rc * Leff, t.D);
        if (!rc) rc = ensure(c, c->head16, rup(Rc, 256) * t.D * 2);
        if (rc) return rc;
        HG_HIP(launch_add_pos(prompts + (size_t)r0 * L * t.D, L, t.pos, (float*)c->x.p, Rc, Leff, t.D, s));
        const int32_t* eot = eot_idx + r0;
        if (Leff < L) {
            rc = ensure(c, c->i32, (size_t)(Rc + 4) * 4);
            if (rc) return rc;
            HG_HIP(launch_clamp_eot(eot, Rc, Leff, (int32_t*)c->i32.p, c->eot_flag, s, c->eot_flag_dev));
            eot = (const int32_t*)c->i32.p;
        }
        rc = text_tail(c, Rc, Leff, eot, out + (size_t)r0 * t.E, s, nullptr, saved);
        if (rc) return rc;
    }
    if (Leff < L) HG_HIP(launch_poison_if_flag(out, (size_t)R * t.E, c->eot_flag_dev, s));
    return HG_OK;
}

int hg_encode_text_embeds(hg_ctx* c, const float* prompts, const int32_t* eot_idx, int R, int L, float* out,
                          int trunc, void* stream) {
    return encode_text_embeds_impl(c, prompts, eot_idx, R, L, out, trunc, nullptr, stream);
}
int hg_encode_text_embeds_save(hg_ctx* c, const float* prompts, const int32_t* eot_idx, int R, int L, float* out, int trunc,
                               float* saved, void* stream) {
    if (c && !saved) return fail(c, HG_ERR_INVALID, "hg_encode_text_embeds_save: saved == NULL");
    return encode_text_embeds_impl(c, prompts, eot_idx, R, L, out, trunc, saved, stream);
}

int hg_token_embedding(hg_ctx* c, const int32_t* ids, int n, float* out, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!c->text.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_load_text has not been called");
    if (n < 0 || !ids || !out) return fail(c, HG_ERR_INVALID, "bad arguments to token_embedding");
    HG_ON_DEVICE(c);
    HG_HIP(launch_gather_rows(ids, c->text.tok, out, n, c->text.D, c->text.vocab, (hipStream_t)stream));
    return HG_OK;
}

}  // extern "C"
