// The fused in_proj + causal attention kernel of the text tower (hg_qkv_attn_text.hip), included once per K-tile schedule:
// QT_KERNEL = the kernel's name, SQ_NKMOD = (K / 64) % 3 of the instance (0: D = 768, 2: D = 512).
__global__ __launch_bounds__(512, 2) void QT_KERNEL(const QkvAttnArgs p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int RB = QT_RB, NCB = QT_NCB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nk = p.K >> 6;                       // K-tiles per item: 3 m, or 3 m + 2 in the SQ_NKMOD = 2 instance
    const int HP = p.heads >> 1;
    const int GS = (RB * 16) / p.L;                // sequences per pack: whole sequences in 160 rows
    const int n_pack = (p.n_seq + GS - 1) / GS;    // (the last one may be short)

    // ---- this workgroup's items (pack, head pair), dealt as hg_qkv_attn.hip deals (sequence, head pair): XCD x owns the packs
    // [x * spx, (x + 1) * spx), head-pair-group major, pack next, pair fastest: the pairs of a pack run side by side on one XCD
    const int G = gridDim.x, bid = blockIdx.x;
    const bool xcd_ok = (G & 7) == 0;
    const int cpx = xcd_ok ? (G >> 3) : G;
    const int idx = xcd_ok ? (bid >> 3) : bid;
    const int spx = xcd_ok ? ((n_pack + 7) >> 3) : n_pack;
    const int s0 = xcd_ok ? (bid & 7) * spx : 0;
    int ns = n_pack - s0;
    ns = ns < 0 ? 0 : (ns > spx ? spx : ns);
    const int nx = ns * HP;
    if (idx >= nx) return;
    const int gsz = p.gsz;
    auto decode = [&](int e, int& pk, int& hp) {
        const int per = ns * gsz;
        const int grp = e / per, rem = e - grp * per;
        const int s = rem / gsz;
        pk = s0 + s;
        hp = grp * gsz + (rem - s * gsz);
    };

#define SQ_A_PTR p.x16
#define SQ_A_BYTES p.a_bytes
#define SQ_LDA p.lda
#define SQ_W_PTR p.wp
#define SQ_W_BYTES (unsigned)((size_t)3 * p.D * p.K * 2)
#include "hg_seq_kloop.inc"
    // bias' | cs of the pair (3 KiB: waves 0-2) and (mean - c, rstd) of the pack's rows (160 x 8 B: waves 3 and 4; rows behind the
    // call's last one read as zeros)
    auto issue_extras = [&](int row0, int hp) {
        const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.bcs, 0, (unsigned)(HP * 768 * 4), 0x00020000);
        const __amdgpu_buffer_rsrc_t rsM =
            __builtin_amdgcn_make_buffer_rsrc((void*)p.mr, 0, (unsigned)((size_t)p.n_seq * p.L * 8), 0x00020000);
        if (wave < 3)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (HG_LDS void*)(smem + QT_BCS + wave * 1024), 16, lane * 16,
                                                     hp * 768 * 4 + wave * 1024, 0, 0);
        else if (wave == 3)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsM, (HG_LDS void*)(smem + QT_MR), 16, lane * 16, row0 * 8, 0, 0);
        else if (wave == 4) {
            if (lane < (RB * 16 * 8 - 1024) / 16)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsM, (HG_LDS void*)(smem + QT_MR + 1024), 16, lane * 16, row0 * 8 + 1024, 0, 0);
        }
    };

    // ---- prologue: K-tile 0 of the first item
    int e = idx, pk, hp;
    decode(e, pk, hp);
    seq_prologue(pk * GS * p.L, hp);

    for (;;) {
        const int e_n = e + cpx;
        const bool has_next = e_n < nx;
        int pk_n = pk, hp_n = hp;            // no next item: the run-ahead loads fetch this item's first K-tile again (never read)
        if (has_next) decode(e_n, pk_n, hp_n);
        const int row0 = pk * GS * p.L, row0_n = pk_n * GS * p.L;

        // the attention phases of the previous item have released the shared region: the epilogue's tables, then the K loop
        issue_extras(row0, hp);
        f32x4 acc[RB][NCB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int c = 0; c < NCB; ++c) acc[rb][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const int sq_row0 = row0, sq_pn = hp, sq_row0_n = row0_n, sq_pn_n = hp_n;
#include "hg_seq_kloop_run.inc"
        }
        wait_vm<0>();
        __builtin_amdgcn_s_waitcnt(0xC07F);
        barrier_raw();
#if SQ_NKMOD != 0
        // nk = 3 m + 2: K-tile nk - 2 sat in stage 0 - the next item's first K-tile is fetched into it only now (every wave has left
        // the loop); it lands under the attention phases and is waited for before the item's last barrier
        issue_A(row0_n, 0, SQ_A0);
#endif

        {
            // ---------------- epilogue: LayerNorm fold, fp16 (the expressions of hg_gemm_ring.hip's EPI_LN_BIAS_F16 epilogue)
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            // (an opaque copy of the lane id: the lane constants of these phases are recomputed per item instead of being hoisted
            // above the K loop, where the registers are wanted)
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));
            const int q = lane_e >> 4, r16 = lane_e & 15;
            const int L = p.L;
            unsigned held[RB][NCB][2];
            {
                f32x4 bv[NCB], cv[NCB];
#pragma unroll
                for (int c = 0; c < NCB; ++c) {
                    const int col = (wave * NCB + c) * 16 + 4 * q;
                    bv[c] = *reinterpret_cast<const f32x4*>(smem + QT_BCS + col * 4);
                    cv[c] = *reinterpret_cast<const f32x4*>(smem + QT_BCS + 384 * 4 + col * 4);
                }
                auto cvt2 = [](float a, float b) {      // RNE, one v_cvt_pk_f16_f32
                    const half2v h = __builtin_convertvector(f32x2{a, b}, half2v);
                    return __builtin_bit_cast(unsigned, h);
                };
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    const f32x2 mr = *reinterpret_cast<const f32x2*>(smem + QT_MR + (rb * 16 + r16) * 8);
#pragma unroll
                    for (int c = 0; c < NCB; ++c) {
                        const f32x4 v = (acc[rb][c] - cv[c] * mr[0]) * mr[1] + bv[c];      // rstd * (acc - mean * cs) + bias'
                        held[rb][c][0] = cvt2(v[0], v[1]);
                        held[rb][c][1] = cvt2(v[2], v[3]);
                    }
                }
            }
            // this wave's 3 column blocks -> rows of Q, K or V: block l12 = 3 (wave % 4) + c of the head = matrix l12 / 4,
            // columns 16 (l12 % 4) + 4 q ..  Tile row R = row R - L g of sequence g = R / L of the pack: the sequences sit back to
            // back (row L g), and the 16-byte chunks of a row are XOR-swizzled by its row IN THE SEQUENCE, as attention_kernel's DMA
            // leaves them - the attention phase below then reads sequence g exactly as that kernel reads its own LDS.
            auto write_head = [&]() {
                static_assert(3 * QT_ASTG + QT_OT_BYTES <= SQ_S12_BYTES, "attention operands");
                const int magic = (65536 + L - 1) / L;      // R / L = (R * magic) >> 16 for R < 160, L <= 80
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    const int R = rb * 16 + r16;
                    const int lr = R - ((R * magic) >> 16) * L;
                    const int swk = swz_k(lr), swv = swz_v(lr);
#pragma unroll
                    for (int c = 0; c < NCB; ++c) {
                        const int l12 = (wave & 3) * NCB + c;
                        const int mtx = l12 >> 2, sub = l12 & 3;
                        const int chunk = 2 * sub + (q >> 1);
                        char* dst = smem + QT_ATT + mtx * QT_ASTG + (q & 1) * 8 + R * ROWB + ((chunk ^ (mtx == 2 ? swv : swk)) << 4);
                        *reinterpret_cast<u32x2*>(dst) = u32x2{held[rb][c][0], held[rb][c][1]};
                    }
                }
            };
            // One head: the pack's (sequence, 32-query tile) pairs are dealt round-robin to the 8 waves; a wave runs its tile over the
            // key tiles up to the diagonal with attention_kernel's own tile functions (hg_attn_dev.h: same operations in the same
            // order on the same fp16 q / k / v - bit-identical), bases shifted to the sequence's first row.  What lies behind a
            // sequence's last row - its neighbour, the rows behind the pack, the next matrix - is masked: K by the score mask, V by
            // the VMASK form of tile_softmax_pv, Q rows >= L are computed and never stored.
            auto attend = [&](const int head) {
                const char* Qs = smem + QT_ATT;
                const char* Ks = Qs + QT_ASTG;
                const char* Vs = Ks + QT_ASTG;
                char* const ot = smem + QT_OT + wave * 2048;
                const int nqt = (L + 31) >> 5, rs = (L + 15) & ~15;
                int gp = p.n_seq - pk * GS;
                gp = gp > GS ? GS : gp;
                const int ntask = gp * nqt;
                int ln = lane_e;
                asm volatile("" : "+v"(ln));
                const int qcol = ln & 31, hh = ln >> 5;
                int k_off[4];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) k_off[ks] = qcol * ROWB + (((2 * ks + hh) ^ swz_k(qcol)) << 4);
                const int gi = ln >> 4, l16 = ln & 15;
                const int vq = l16 >> 2, vp = l16 & 3;
                int v_off[2];
                {
                    const int key0 = 4 * (gi >> 1) + vq;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const int chunk = dt * 4 + (gi & 1) * 2 + (vp >> 1);
                        v_off[dt] = key0 * ROWB + ((chunk ^ swz_v(key0)) << 4) + (vp & 1) * 8;
                    }
                }
                const float cexp = 0.125f * 1.4426950408889634f;   // head_dim^-0.5 * log2(e)
                for (int t = wave; t < ntask; t += 8) {
                    const int g = t / nqt, qt = t - g * nqt;
                    const int boff = g * L * ROWB;                  // (a multiple of 128: the transposing reads' address XOR holds)
                    const int qq = qt * 32 + qcol;
                    half8 qf[4];
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const half8*>(Qs + boff + qt * TILEB + k_off[ks]);
                    float m = -1.0e30f, lsum = 0.f;
                    f32x16 o[2];
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
                    for (int kt = 0; kt <= qt; ++kt) {              // causal: key tiles above the diagonal are skipped
                        f32x16 sc;
                        tile_scores(Ks + boff + kt * TILEB, k_off, qf, sc);
                        tile_softmax_pv<true, true>(Vs + boff + kt * TILEB, v_off, sc, kt, qt, qq, L, rs, hh, cexp, m, lsum, o);
                    }
                    lsum += __shfl_xor(lsum, 32, 64);
                    const float inv = 1.0f / lsum;
                    // the wave's 32 x 64 tile leaves through its own 2 KiB of LDS in two halves of 32 columns (16-byte chunks
                    // XOR-swizzled by row), as 64-byte row segments: lane -> (row = l >> 2, chunk = l & 3)
                    half_t* const obase = p.out + (size_t)(pk * GS + g) * L * p.ldo + head * HD;      // (uniform base + 32-bit lane offset)
                    const int cr = ln >> 2, cc = ln & 3;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4) {
                            half4 h;
#pragma unroll
                            for (int e4 = 0; e4 < 4; ++e4) h[e4] = (half_t)(o[dt][g4 * 4 + e4] * inv);
                            *reinterpret_cast<half4*>(ot + qcol * 64 + ((g4 ^ (qcol & 3)) << 4) + hh * 8) = h;
                        }
#pragma unroll
                        for (int r16b = 0; r16b < 32; r16b += 16) {
                            const int row = r16b + cr, qrow = qt * 32 + row;
                            const half8 v = *reinterpret_cast<const half8*>(ot + row * 64 + ((cc ^ (row & 3)) << 4));
                            if (qrow < L) *reinterpret_cast<half8*>(obase + (unsigned)(qrow * p.ldo + dt * 32 + cc * 8)) = v;
                        }
                    }
                }
            };
            if (wave < 4) write_head();
            __builtin_amdgcn_s_waitcnt(0xC07F);
            barrier_raw();
            attend(2 * hp);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            barrier_raw();
            if (wave >= 4) write_head();
            __builtin_amdgcn_s_waitcnt(0xC07F);
            barrier_raw();
            attend(2 * hp + 1);
#if SQ_NKMOD != 0
            wait_vm<0>();      // this wave's pieces of the next item's first K-tile: the barrier publishes them
#endif
            __builtin_amdgcn_s_waitcnt(0xC07F);
            barrier_raw();
        }
        if (!has_next) break;
        e = e_n;
        pk = pk_n;
        hp = hp_n;
    }
#endif
}

