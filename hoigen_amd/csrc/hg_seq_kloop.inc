// K loop of the sequence-tile GEMMs (hg_seq_dev.h), expanded inside a kernel body.  Expects in scope: `smem` (THE extern
// __shared__ array), `lane`, `wave`, `nk` (K / 64; its residue mod 3 = SQ_NKMOD), and the macros
// SQ_A_PTR / SQ_A_BYTES / SQ_LDA (fp16 activations [rows, lda], bytes readable), SQ_W_PTR / SQ_W_BYTES (packed weight).
// Defines: seq_prologue(row0, pn), stage_base(st), and what hg_seq_kloop_run.inc (the loop itself, expanded inside the item loop) needs.
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(SQ_A_PTR), 0, (SQ_A_BYTES), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)(SQ_W_PTR), 0, (SQ_W_BYTES), 0x00020000);
    const int sq_lda = (SQ_LDA);
    // A pieces of this wave: piece pc = wave + 8 i covers tile rows 8 pc .. 8 pc + 7; lane -> (row = l >> 3, chunk' = l & 7);
    // 64 rows further down the swizzle repeats, so piece i is piece 0 plus a scalar offset
    // (every lane constant of the loop is recomputed from an opaque copy of the lane id where it is used - a few VALU operations
    // per K-tile: kept live across the loop they are what the register allocator spills, and a scratch reload waits for
    // vmcnt(0), i.e. drains the DMA pipeline)
    auto lane_now = [&]() {
        int l = lane;
        asm volatile("" : "+v"(l));
        return l;
    };
    auto stage_base = [&](int st) { return st == 0 ? SQ_A0 : SQ_S12 + (st - 1) * SQ_ASTG; };
    // all pieces of one K-tile of the rows row0 .. row0 + 207 (26 pieces: waves 0 and 1 issue a fourth - an operation more
    // only makes the counted waits below stricter, never looser; 10 row blocks: 20 pieces, two per wave and a third from waves 0-3)
    auto issue_A = [&](int row0, int kt, int sbase) {
        const int soff = (row0 * sq_lda + kt * 64) * 2;
        const int ln = lane_now();
        const int voffA = ((wave * 8 + (ln >> 3)) * sq_lda + (((ln & 7) ^ ((ln >> 4) & 3) ^ ((wave & 1) << 2)) << 3)) * 2;
#pragma unroll
        for (int i = 0; i < SQ_NA; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (HG_LDS void*)(smem + sbase + (wave + 8 * i) * 1024), 16, voffA,
                                                     soff + i * 64 * sq_lda * 2, 0, 0);
        int w_now = wave;      // (opaque: a hoisted copy of this condition is one more value the allocator has to keep across the loop)
        asm volatile("" : "+s"(w_now));
        if (w_now < SQ_NAX)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (HG_LDS void*)(smem + sbase + (wave + 8 * SQ_NA) * 1024), 16, voffA,
                                                     soff + SQ_NA * 64 * sq_lda * 2, 0, 0);
    };
    char* wring = smem + wave * SQ_WSLOT;
    // fragment slot (ks, c) of K-tile kt of panel pn: Wp[pn][2 kt + ks][wave][c][lane][8]
    auto issue_W = [&](int pn, int kt, const int slot) {
        const int ks = slot / SQ_NCB, c = slot % SQ_NCB;
        const int soff = ((((pn * 2 * nk + kt * 2 + ks) * 8 + wave) * SQ_NCB) + c) * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (HG_LDS void*)(wring + slot * 1024), 16, lane_now() * 16, soff, 0, 0);
    };
    // K-tile 0 of the workgroup's first item: fetched, landed and published
    auto seq_prologue = [&](int row0, int pn) {
        issue_A(row0, 0, SQ_A0);
#pragma unroll
        for (int slot = 0; slot < 2 * SQ_NCB; ++slot) issue_W(pn, 0, slot);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        barrier_raw();
    };
