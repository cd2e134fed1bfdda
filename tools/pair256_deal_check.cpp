// Host emulation of the dealing of the two MLP pair launches: compiles hoigen_amd/csrc/hg_mlp_pair_deal.h - the code the kernels'
// schedules run - with a host compiler and checks, for every M in [2048, 60000] in steps of 64 (every panel count and every remainder
// of a panel and of a 128-row half) plus the rows around every panel edge and half-panel edge, N_fc in {2048, 3072} with
// N_proj = N_fc / 4 and 32 slots per XCD.
// c_proj on 256-row tiles (hg_mlp_pair256.hip), chunk sizes {1, 3, 8, 32}:
//   * every c_fc tile and every c_proj tile of the chip is dealt exactly once, and nothing outside the tile grid;
//   * no slot is without a c_fc tile as soon as its XCD has a c_fc tile per slot (fewer tiles than slots: the first T slots own one each);
//   * the heavy slots (one c_proj tile more) own no more c_fc tiles than any light slot, and in every c_proj round their items come
//     before every light slot's: the slots that reach c_proj first take the XCD's earliest panels;
//   * a slot's work differs from the XCD's fullest by at most ratio + 1 c_fc tile times where every slot owns a c_fc tile.
// c_proj on 128-row tiles (hg_mlp_pair.hip), chunk sizes {1, 3, 8, 32, 64}, 1, 24 or 32 slots per XCD that run c_fc tiles:
//   * every c_fc tile and every 128-row c_proj tile of the chip is dealt exactly once, and nothing outside the tile grid (at a half-panel
//     edge the chip's last panel has one 128-row half only);
//   * a slot's c_fc positions and its c_proj items lie in list order;
//   * no slot's start stagger is negative (slack() >= 0).
// Prints "ok <cases>" or the first failures.  (tests/test_mlp_pair256_build.py builds and runs it.)
#include <cstdio>
#include <vector>

#include "../hoigen_amd/csrc/hg_mlp_pair_deal.h"

using namespace hg;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL M=%d N_fc=%d ch=%d xcd=%d: ", M, nfc_cols, ch, x); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check(int M, int nfc_cols, int ch, int ratio) {
    const int cpx = 32, tnf = nfc_cols / 256, tnp = nfc_cols / 4 / 256;
    const int pf = (M + 255) / 256;
    std::vector<int> fc_seen((size_t)pf * tnf, 0), proj_seen((size_t)pf * tnp, 0);
    for (int x = 0; x < MLP_NX; ++x) {
        const int npx = mlp_panels(pf, x), T = npx * tnf, P = npx * tnp;
        int max_load = 0, min_load = 1 << 30, min_light_fc = 1 << 30, max_heavy_fc = 0;
        for (int s = 0; s < cpx; ++s) {
            const Pair256Deal d(T, P, cpx, s, ratio);
            const int nf = d.n_fc(), np = d.n_proj();
            CHECK(nf >= 0 && np >= 0, "slot %d: %d c_fc, %d c_proj tiles", s, nf, np);
            if (T >= cpx) CHECK(nf >= 1, "slot %d owns no c_fc tile of %d", s, T);
            else CHECK(nf == (s < T ? 1 : 0), "slot %d owns %d c_fc tiles of %d", s, nf, T);
            int last = -1;
            for (int r = 0; r < nf; ++r) {
                const int L = d.fc_pos(r);
                CHECK(L > last && L < T, "slot %d: c_fc position %d behind %d of %d", s, L, last, T);
                last = L;
                if (L < 0 || L >= T) continue;
                int tm, tn;
                MlpFcList(x, ch, tnf, npx).tile(L, tm, tn);
                CHECK(tm >= 0 && tm < pf && tm % MLP_NX == x && tn >= 0 && tn < tnf, "c_fc position %d -> tile (%d, %d)", L, tm, tn);
                if (tm >= 0 && tm < pf && tn >= 0 && tn < tnf) ++fc_seen[(size_t)tm * tnf + tn];
            }
            for (int j = 0; j < np; ++j) {
                const int i = d.proj_item(j);
                CHECK(i >= 0 && i < P, "slot %d: c_proj item %d of %d", s, i, P);
                if (i < 0 || i >= P) continue;
                int tm, tn;
                pair256_proj_tile(i, x, tnp, tm, tn);
                CHECK(tm >= 0 && tm < pf && tm % MLP_NX == x && tn >= 0 && tn < tnp, "c_proj item %d -> tile (%d, %d)", i, tm, tn);
                if (tm >= 0 && tm < pf && tn >= 0 && tn < tnp) ++proj_seen[(size_t)tm * tnp + tn];
                // the heavy slots' item of a round lies in front of every light slot's
                if (d.heavy()) CHECK(i - j * cpx < d.rem, "heavy slot %d: item %d of round %d", s, i, j);
                else CHECK(i - j * cpx >= d.rem, "light slot %d: item %d of round %d", s, i, j);
            }
            if (d.heavy()) max_heavy_fc = nf > max_heavy_fc ? nf : max_heavy_fc;
            else min_light_fc = nf < min_light_fc ? nf : min_light_fc;
            const int load = d.load_of(s);
            max_load = load > max_load ? load : max_load;
            min_load = load < min_load ? load : min_load;
            CHECK(d.slack() >= 0 && d.slack() == d.max_load() - load, "slot %d: slack %d", s, d.slack());
        }
        if (P % cpx) CHECK(max_heavy_fc <= min_light_fc, "a heavy slot owns %d c_fc tiles, a light one %d", max_heavy_fc, min_light_fc);
        {
            const Pair256Deal d0(T, P, cpx, 0, ratio);
            CHECK(d0.max_load() == max_load, "max_load() %d, largest load %d", d0.max_load(), max_load);
        }
        if (T >= cpx) CHECK(max_load - min_load <= ratio + 1, "loads %d .. %d", min_load, max_load);
    }
    const int x = -1;
    for (size_t i = 0; i < fc_seen.size(); ++i) CHECK(fc_seen[i] == 1, "c_fc tile (%d, %d) dealt %d times", (int)(i / tnf), (int)(i % tnf), fc_seen[i]);
    for (size_t i = 0; i < proj_seen.size(); ++i) CHECK(proj_seen[i] == 1, "c_proj tile (%d, %d) dealt %d times", (int)(i / tnp), (int)(i % tnp), proj_seen[i]);
}

// the 128-row launch: the first fc_slots slots of an XCD deal its c_fc list, all of them its list of 128-row c_proj tiles
static void check128(int M, int nfc_cols, int ch, int fc_slots) {
    const int cpx = 32, tnf = nfc_cols / 256, tnp = nfc_cols / 4 / 256;
    const int pf = (M + 255) / 256, pq = (M + 127) / 128;
    std::vector<int> fc_seen((size_t)pf * tnf, 0), proj_seen((size_t)pq * tnp, 0);
    for (int x = 0; x < MLP_NX; ++x) {
        const MlpFcList list(x, ch, tnf, mlp_panels(pf, x));
        for (int s = 0; s < cpx; ++s) {
            const MlpFcDeal d(list.size(), s, fc_slots);
            CHECK(d.total >= 0 && d.slack() >= 0, "slot %d of %d: %d c_fc tiles, slack %d", s, fc_slots, d.total, d.slack());
            int last = -1;
            for (int r = 0; r < d.total; ++r) {
                const int L = d.pos(r);
                CHECK(L > last && L < list.size(), "slot %d of %d: c_fc position %d behind %d of %d", s, fc_slots, L, last, list.size());
                last = L;
                if (L < 0 || L >= list.size()) continue;
                int tm, tn;
                list.tile(L, tm, tn);
                CHECK(tm >= 0 && tm < pf && tm % MLP_NX == x && tn >= 0 && tn < tnf, "c_fc position %d -> tile (%d, %d)", L, tm, tn);
                if (tm >= 0 && tm < pf && tn >= 0 && tn < tnf) ++fc_seen[(size_t)tm * tnf + tn];
            }
            const MlpProjDeal p(M, tnp, x, s, cpx);
            CHECK(p.total >= 0, "slot %d: %d c_proj tiles", s, p.total);
            last = -1;
            for (int r = 0; r < p.total; ++r) {
                const int i = p.item(r);
                CHECK(i > last && i < p.tx, "slot %d: c_proj item %d behind %d of %d", s, i, last, p.tx);
                last = i;
                if (i < 0 || i >= p.tx) continue;
                int tm, tn;
                p.tile(i, tm, tn);      // (tm counts 128-row halves)
                CHECK(tm >= 0 && tm < pq && (tm >> 1) % MLP_NX == x && tn >= 0 && tn < tnp, "c_proj item %d -> tile (%d, %d)", i, tm, tn);
                if (tm >= 0 && tm < pq && tn >= 0 && tn < tnp) ++proj_seen[(size_t)tm * tnp + tn];
            }
        }
    }
    const int x = -1;
    for (size_t i = 0; i < fc_seen.size(); ++i) CHECK(fc_seen[i] == 1, "c_fc tile (%d, %d) dealt %d times (128-row launch, %d c_fc slots)", (int)(i / tnf), (int)(i % tnf), fc_seen[i], fc_slots);
    for (size_t i = 0; i < proj_seen.size(); ++i) CHECK(proj_seen[i] == 1, "128-row c_proj tile (%d, %d) dealt %d times", (int)(i / tnp), (int)(i % tnp), proj_seen[i]);
}

int main() {
    long cases = 0;
    const int chunks[4] = {1, 3, 8, 32}, widths[2] = {2048, 3072};
    for (int w = 0; w < 2; ++w)
        for (int c = 0; c < 4; ++c) {
            for (int M = 2048; M <= 60000; M += 64, ++cases) check(M, widths[w], chunks[c], 4);
            for (int p = 8; p * 256 <= 60000; ++p)      // the rows around every panel edge and half-panel edge
                for (int dm = -1; dm <= 1; ++dm)
                    for (int h = 0; h < 2; ++h, ++cases) check(p * 256 + h * 128 + dm, widths[w], chunks[c], 4);
        }
    for (int ratio = 1; ratio <= 6; ++ratio)
        for (int M = 2048; M <= 60000; M += 448, ++cases) check(M, 3072, 32, ratio);
    const int chunks128[5] = {1, 3, 8, 32, 64}, fc_slots[3] = {1, 24, 32};
    for (int w = 0; w < 2; ++w)
        for (int c = 0; c < 5; ++c)
            for (int f = 0; f < 3; ++f) {
                for (int M = 2048; M <= 60000; M += 64, ++cases) check128(M, widths[w], chunks128[c], fc_slots[f]);
                for (int p = 8; p * 256 <= 60000; ++p)
                    for (int dm = -1; dm <= 1; ++dm)
                        for (int h = 0; h < 2; ++h, ++cases) check128(p * 256 + h * 128 + dm, widths[w], chunks128[c], fc_slots[f]);
            }
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("ok %ld\n", cases);
    return 0;
}
