// The list arithmetic of the two MLP pair launches (hg_mlp_pair.hip: c_proj on 128-row tiles; hg_mlp_pair256.hip: c_proj on 256-row
// tiles): which tiles an XCD owns, in which order, and which of them each of its work slots runs.  Plain integer arithmetic, host and
// device: the kernels' schedules and the CPU test of the dealing (tests/test_mlp_pair256_build.py through tools/pair256_deal_check.cpp)
// run this very code.
//
// Both launches: XCD x owns the 256-row panels x, x + 8, ..., their c_fc tiles (MlpFcList) and their c_proj tiles.
//
// 128-row launch: the first `fcs` slots deal the c_fc list by count (MlpFcDeal); the c_proj list - an item is half a panel high - is
// dealt from the last slot down (MlpProjDeal).
//
// 256-row launch (Pair256Deal): the XCD owns T c_fc tiles - positions 0 .. T - 1 of its c_fc list, which completes its row panels in
// order - and P c_proj tiles - items 0 .. P - 1, panel by panel, the column tiles of a panel side by side.  A c_proj tile is `ratio`
// c_fc tiles of work, so the dealing goes by work, not by count:
//   * c_proj: P = pb * cpx + rem.  The LAST rem slots ("heavy") own pb + 1 items, the first nl = cpx - rem ("light") own pb.
//   * c_fc: every slot takes part in hq rounds (position cpx * r + slot), one partial round of R < cpx tiles goes to the slots 0 .. R - 1,
//     and the light slots alone deal d <= ratio more rounds (position cpx * hq + R + j * nl + slot): they own d tiles more than the
//     heavy ones, as much as the c_proj tile they own less weighs.  d shrinks only where T is too small for every slot to own a c_fc tile
//     otherwise (hq >= 1 whenever T >= cpx).
//   * order: a slot runs all its c_fc tiles first.  The heavy slots have the fewest and reach c_proj first, so in every c_proj round
//     (cpx items) they own the first rem items - the XCD's earliest panels of that round -, and the round behind the last full one
//     is theirs alone.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HG_DEAL_FN __host__ __device__ __forceinline__
#else
#define HG_DEAL_FN inline
#endif

namespace hg {

constexpr int MLP_NX = 8;      // XCDs (HW_REG_XCC_ID 0 .. 7): XCD x owns the 256-row panels x, x + 8, ...

// panels of XCD x among pf panels
HG_DEAL_FN int mlp_panels(int pf, int x) { return pf > x ? (pf - x + MLP_NX - 1) / MLP_NX : 0; }

// The XCD's c_fc list: its npx panels in chunks of `ch`, one chunk after the other; inside a chunk column group (cg column tiles: 4, or
// 3, or all tn) by column group, panel by panel, the group's column tiles side by side.
struct MlpFcList {
    int x, ch, tn, cg, npx, nfc;      // XCD, panels per chunk, column tiles, column tiles per group, panels, full chunks
    HG_DEAL_FN MlpFcList(int x_, int ch_, int tn_, int npx_) {
        x = x_; ch = ch_; tn = tn_; npx = npx_;
        cg = tn % 4 == 0 ? 4 : (tn % 3 == 0 ? 3 : tn);
        nfc = npx / ch;
    }
    HG_DEAL_FN int size() const { return npx * tn; }
    // position L -> tile
    HG_DEAL_FN void tile(int L, int& tm, int& tn_) const {
        const int per_c = ch * tn;
        int c = L / per_c, l = L - c * per_c, pc = ch;
        if (c >= nfc) { c = nfc; l = L - nfc * per_c; pc = npx - nfc * ch; }      // (the partial chunk; its panel count worked out here, at
                                                                                  // its use: as a member it changes the 256-row kernel's code)
        const int per_g = pc * cg;                  // inside the chunk: column group, panel, column in the group
        const int grp = l / per_g, rem = l - grp * per_g;
        const int j = rem / cg;
        tn_ = grp * cg + (rem - j * cg);
        tm = x + MLP_NX * (c * ch + j);
    }
};

// ---- 128-row launch.  c_fc: the first `fcs` slots of the XCD deal its list of `len` positions among themselves (cu, cu + fcs, ...)
struct MlpFcDeal {
    int cu, fcs, len, total;
    HG_DEAL_FN MlpFcDeal(int len_, int cu_, int fcs_) {
        cu = cu_; fcs = fcs_; len = len_;
        total = count(len);
    }
    // items of this slot among the first `lim` list positions
    HG_DEAL_FN int count(int lim) const { return cu < fcs && cu < lim ? (lim - cu + fcs - 1) / fcs : 0; }
    HG_DEAL_FN int pos(int r) const { return cu + fcs * r; }
    // tiles this slot owns fewer than the fullest ones
    HG_DEAL_FN int slack() const { return (len + fcs - 1) / fcs - total; }
};
// c_proj: the XCD's list is its panel k, 128-row half, column tile; slot s owns the items cu, cu + cpx, ... with cu = cpx - 1 - s
// (the list is dealt from the LAST slot down: the c_fc list's remainder goes to the first slots, this one's to the last ones - a slot
// owns 10 + 4, 9 + 5 or, two per XCD, 10 + 5 tiles instead of 10 + 5 for twelve: a c_proj tile takes 2.2 c_fc tile times)
struct MlpProjDeal {
    int x, cu, cpx, tn, tx, total;
    HG_DEAL_FN MlpProjDeal(int M, int tn_, int x_, int slot, int cpx_) {
        x = x_; cu = cpx_ - 1 - slot; cpx = cpx_; tn = tn_;
        const int pf = (M + 255) / 256, pq = (M + 127) / 128;
        const int npx = mlp_panels(pf, x);
        // the chip's last panel may have one 128-row half only; it is the last panel of its XCD's list, its missing half the list's tail
        tx = tn * (2 * npx - ((npx > 0 && x + MLP_NX * (npx - 1) == pf - 1 && (pq & 1)) ? 1 : 0));
        total = cu < tx ? (tx - cu + cpx - 1) / cpx : 0;
    }
    HG_DEAL_FN int item(int r) const { return cu + cpx * r; }
    // item i -> tile (tm counts 128-row halves)
    HG_DEAL_FN void tile(int i, int& tm, int& tn_) const {
        const int k = i / (2 * tn), rem = i - k * 2 * tn;
        const int half = rem / tn;
        tn_ = rem - half * tn;
        tm = 2 * (x + MLP_NX * k) + half;
    }
};

// ---- 256-row launch.  The XCD's c_proj list: panel by panel, the column tiles of a panel side by side.  Item i -> tile.
HG_DEAL_FN void pair256_proj_tile(int i, int x, int tn, int& tm, int& tn_) {
    const int k = i / tn;
    tn_ = i - k * tn;
    tm = x + MLP_NX * k;
}

struct Pair256Deal {
    int cpx, slot, T, P, ratio;
    int pb, rem, nl, d, hq, R;
    HG_DEAL_FN Pair256Deal(int T_, int P_, int cpx_, int slot_, int ratio_) {
        cpx = cpx_; slot = slot_; T = T_; P = P_; ratio = ratio_;
        pb = P / cpx;
        rem = P - pb * cpx;
        nl = cpx - rem;
        d = T >= cpx ? (T - cpx) / nl : 0;
        if (d > ratio) d = ratio;
        hq = (T - d * nl) / cpx;
        R = T - hq * cpx - d * nl;
    }
    HG_DEAL_FN bool heavy() const { return slot >= nl; }
    // c_fc tiles of this slot, and the list position of its r-th
    HG_DEAL_FN int n_fc() const { return n_fc_of(slot); }
    HG_DEAL_FN int n_fc_of(int s) const { return hq + (s < R ? 1 : 0) + (s < nl ? d : 0); }
    HG_DEAL_FN int fc_pos(int r) const {
        if (r < hq) return cpx * r + slot;
        const int e = slot < R ? 1 : 0;
        if (r == hq && e) return cpx * hq + slot;
        return cpx * hq + R + (r - hq - e) * nl + slot;
    }
    // c_proj tiles of this slot, and the list item of its j-th
    HG_DEAL_FN int n_proj() const { return n_proj_of(slot); }
    HG_DEAL_FN int n_proj_of(int s) const { return pb + (s >= nl ? 1 : 0); }
    HG_DEAL_FN int proj_item(int j) const { return j * cpx + (heavy() ? slot - nl : rem + slot); }
    // work of a slot in c_fc tile times, the XCD's largest, and this slot's slack against it (the start stagger goes by work)
    HG_DEAL_FN int load_of(int s) const { return n_fc_of(s) + ratio * n_proj_of(s); }
    HG_DEAL_FN int max_load() const {
        int m = load_of(0);      // (the loads take at most four values: light / heavy, with / without a tile of the partial round)
        const int c[3] = {nl - 1, nl < cpx ? nl : 0, cpx - 1};
        for (int i = 0; i < 3; ++i) {
            const int l = load_of(c[i]);
            m = l > m ? l : m;
        }
        return m;
    }
    HG_DEAL_FN int slack() const { return max_load() - load_of(slot); }
};

}  // namespace hg
