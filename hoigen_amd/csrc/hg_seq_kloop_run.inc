// The K loop itself (hg_seq_dev.h, hg_seq_kloop.inc), expanded where it runs: inside the item loop of the kernel, with `acc`
// (f32x4 [SQ_RB][SQ_NCB]) and the ints sq_row0, sq_pn (this item), sq_row0_n, sq_pn_n (the next one) in scope.
    // The K loop of one item (rows row0.., panel pn); (row0_n, pn_n): the workgroup's next item, whose first K-tile is fetched
    // under the last K-tiles of this one (no next item: pass this item again - the loads are never read).  Before the call:
    // K-tile 0 has landed in stage 0 and the W rings, and the caller's phase has released stages 1 and 2; the caller may have
    // issued further VMEM operations of its own just before (tables for its epilogue: older operations only make the counted
    // waits stricter).  On return the last MFMAs are issued and the next item's first K-tile is in flight: the caller waits
    // vmcnt(0) + barrier before it touches stages 1 and 2 or lets stores enter vmcnt.
    //   (RB = SQ_RB row blocks, NPOS = 2 RB positions per K-tile, PUB = NPOS - 5; 13 row blocks: RB - 3 = 10, PUB = 21; 10: 7 and 15)
    //   position PUB (five reads before the boundary): counted wait for this wave's pieces of stage kt+1, s_barrier (publishes
    //     stage kt+1; every wave has left K-tile kt-1 behind: its stage is free), then the A group of stage kt+2 into it.
    //   VMEM operations of K-tile kt in issue order:   R_0 R_1 R_2 | R_3 R_4 R_5 | A x SQ_NA (one more from waves < SQ_NAX)
    //     R_j: refill of W slot j with K-tile kt+1's fragment, issued once the k-step's fragments are in registers.
    //   Counted waits (vmcnt is in issue order; NCB = 3 refills per k-step, SQ_NA = 3 pieces with 13 row blocks, 2 with 10):
    //     before reading slots 3-5 (k-step 0, row block RB - 3):  R_3-5 of K-tile kt-1 landed; issued since: the A group, R_0-2
    //                                                              -> NCB + SQ_NA (6 / 5)
    //     position PUB:                                            A group of K-tile kt-1 (= stage kt+1) landed; since: R_0-2, R_3-5
    //                                                              -> 2 NCB (6)
    //     before reading slots 0-2 (k-step 1, row block RB - 3):  R_0-2 of this K-tile landed; issued since: R_3-5, the A group
    //                                                              -> NCB + SQ_NA (6 / 5)
    //     (a wave that issued the extra piece has one operation more behind the one it waits for: the same count is stricter for it)
    // KIND 0: first K-tile of an item (primes the ring and reads its W fragments here; stage 1 is issued at the start of the
    // loop), 1: middle, 2: last (stages 1 and 2 of the next item would overlay the caller's phase: no A group, no barrier; the R_j
    // fetch the next item's first K-tile; nothing is read ahead).  PH = kt % 3: the stage, and the ring slot of position 0 (NPOS = 26 or 20
    // positions = 2 mod 6 per K-tile).
    // SQ_NKMOD = nk % 3 (a macro of the including kernel, default 0).  nk = 3 m + 1 (K = 832: the adapter's 64 extra columns): the last
    // K-tile sits in stage 0 itself, so the next item's first K-tile cannot be fetched under this item's last ones: KIND 3 = the
    // second-to-last K-tile, which issues NO activation group at its barrier (the caller fetches the next item's first K-tile into
    // stage 0 behind the loop, under its own phase), KIND 4 = the last K-tile behind it (its one counted wait has three operations
    // fewer in front of it).
    {
        const int row0 = sq_row0, pn = sq_pn, row0_n = sq_row0_n, pn_n = sq_pn_n;
        constexpr int RB = SQ_RB, NCB = SQ_NCB;
        issue_A(row0, 1, stage_base(1));
        constexpr int AR = SQ_AR, NPOS = 2 * RB, PUB = NPOS - (AR - 1);
        half8 wc[NCB], wn[NCB], afr[AR];
        int af_off[2], w_off;      // lane parts of the fragment addresses, recomputed per K-tile (hg_seq_kloop.inc: lane_now)
        auto read_af = [&](int sbase, int ks, int rb, int slot) {
            afr[slot] = *reinterpret_cast<const half8*>(smem + sbase + af_off[ks] + rb * 2048);
        };
        auto read_W = [&](int slot) { return *reinterpret_cast<const half8*>(wring + slot * 1024 + w_off); };
        auto ktile = [&](const int kt, auto KIND_T, auto PH_T) {
            constexpr int KIND = decltype(KIND_T)::value, PH = decltype(PH_T)::value;
            constexpr bool FIRST = KIND == 0, LAST = KIND == 2 || KIND == 4, NO_A = KIND == 3, AFTER_NO_A = KIND == 4;
            constexpr int S0 = (2 * PH) % AR;                     // ring slot of position 0
            // (opaque scalars: the six lane-address sums "stage + lane part" would otherwise be hoisted out of the loop as VGPRs,
            // and spilled - a scratch reload waits for vmcnt(0) and drains the DMA pipeline)
            int sb_cur = stage_base(PH), sb_nxt = stage_base((PH + 1) % 3);
            asm volatile("" : "+s"(sb_cur), "+s"(sb_nxt));
            {
                const int ln = lane_now();
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) af_off[ks] = (ln & 15) * 128 + (((ks * 4 + (ln >> 4)) ^ ((ln >> 1) & 7)) << 4);
                w_off = ln * 16;
            }
            if constexpr (FIRST) {
#pragma unroll
                for (int i = 0; i < AR - 1; ++i) read_af(sb_cur, 0, i, (S0 + i) % AR);
#pragma unroll
                for (int c = 0; c < NCB; ++c) wc[c] = read_W(c);
            }
            // Priority of the MFMA stream: both waves of a SIMD raised, as measured best against none and against only the younger wave
            // w + 4 raised; taking turns position by position was measured 15-20 % slower: profiles/r04_qkv_attn.txt
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    const int pos = ks * RB + rb, pf = pos + AR - 1;
                    if (pos == PUB && !LAST) {
                        SQ_STAMP_B();
                        wait_vm<2 * NCB>();
                        SQ_STAMP_E(0);      // counted wait for stage kt+1
                        SQ_STAMP_B();
                        barrier_raw();
                        SQ_STAMP_E(1);      // barrier
                        const int sb_free = stage_base((PH + 2) % 3);          // stage of K-tile kt-1 = stage of K-tile kt+2
                        if constexpr (!NO_A) {
                            if (kt + 2 < nk) issue_A(row0, kt + 2, sb_free);
                            else issue_A(row0_n, 0, sb_free);                     // kt = nk - 2, stage 0: the next item's first K-tile
                        }
                        asm volatile("" ::: "memory");
                    }
                    if (pf < NPOS) read_af(sb_cur, pf / RB, pf % RB, (S0 + pf) % AR);
                    else if (!LAST) read_af(sb_nxt, 0, pf - NPOS, (S0 + pf) % AR);
                    if (rb == RB - 3 && !(LAST && ks == 1)) {
                        // W fragments of the next k-step (the other half of the ring, or the next K-tile's first half)
                        SQ_STAMP_B();
                        // (behind a K-tile that issued no activation group the refills R_3-5 of K-tile kt - 1 have only R_0-2 behind them)
                        // (... and in that K-tile itself R_0-2 have only R_3-5 behind them at k-step 1)
                        // (otherwise: the three refills and an activation group - SQ_NA pieces from every wave - were issued since)
                        if ((AFTER_NO_A && ks == 0) || (NO_A && ks == 1)) wait_vm<NCB>();
                        else if (!(FIRST && ks == 0)) wait_vm<NCB + SQ_NA>();
                        SQ_STAMP_E(2);      // counted wait for the W slots
#pragma unroll
                        for (int c = 0; c < NCB; ++c) wn[c] = read_W((1 - ks) * NCB + c);
                    }
#pragma unroll
                    for (int c = 0; c < NCB; ++c)
                        acc[rb][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wc[c], afr[(S0 + pos) % AR], acc[rb][c], 0, 0, 0);
                    if (rb == 0) {
                        // the step's W fragments are in registers (the MFMAs above waited for them): refill their slots
                        asm volatile("" ::"v"(wc[0]), "v"(wc[1]), "v"(wc[2]) : "memory");
#pragma unroll
                        for (int c = 0; c < NCB; ++c) {
                            if constexpr (LAST) issue_W(pn_n, 0, ks * NCB + c);
                            else issue_W(pn, kt + 1, ks * NCB + c);
                        }
                        asm volatile("" ::: "memory");
                    }
                }
#pragma unroll
                for (int c = 0; c < NCB; ++c) wc[c] = wn[c];
            }
        };
        using I0 = std::integral_constant<int, 0>;
        using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>;
        using I3 [[maybe_unused]] = std::integral_constant<int, 3>;
        using I4 [[maybe_unused]] = std::integral_constant<int, 4>;
        ktile(0, I0{}, I0{});
#if defined(SQ_NKMOD) && SQ_NKMOD == 2
        // nk = 3 m + 2 (K = 512: the text tower of ViT-B): the last K-tile sits in stage 1 and stage 0 holds K-tile nk-2 until every
        // wave has left it, so - as with 3 m + 1 - the caller fetches the next item's first K-tile behind the loop.  K-tiles 1 .. nk-3
        // (3 m - 1 of them: stages 1 2 | 0 1 2 | ..), then nk-2 (stage 0, no activation group), nk-1 (stage 1)
        for (int kt = 1; kt < nk - 2; kt += 3) {
            ktile(kt, I1{}, I1{});
            ktile(kt + 1, I1{}, I2{});
            if (kt + 2 >= nk - 2) break;
            ktile(kt + 2, I1{}, I0{});
        }
        ktile(nk - 2, I3{}, I0{});
        ktile(nk - 1, I4{}, I1{});
#elif !defined(SQ_NKMOD) || SQ_NKMOD == 0
        for (int kt = 1; kt < nk - 2; kt += 3) {      // K-tiles 1 .. nk-3 (a multiple of 3 of them)
            ktile(kt, I1{}, I1{});
            ktile(kt + 1, I1{}, I2{});
            ktile(kt + 2, I1{}, I0{});
        }
        ktile(nk - 2, I1{}, I1{});
        ktile(nk - 1, I2{}, I2{});
#else      // nk = 3 m + 1: K-tiles 1 .. nk-4 in threes, then nk-3 (stage 1), nk-2 (stage 2, no activation group), nk-1 (stage 0)
        for (int kt = 1; kt < nk - 3; kt += 3) {
            ktile(kt, I1{}, I1{});
            ktile(kt + 1, I1{}, I2{});
            ktile(kt + 2, I1{}, I0{});
        }
        ktile(nk - 3, I1{}, I1{});
        ktile(nk - 2, I3{}, I2{});
        ktile(nk - 1, I4{}, I0{});
#endif
        __builtin_amdgcn_s_setprio(0);
    }
