// Stand-alone host program around hoigen_amd/csrc/hg_preproc_geom.h, the geometry and weight-table functions the batched crop
// pre-processing kernels evaluate on the device (tests/test_preproc_batch_host.py builds it with the host compiler, once plain and once
// with -fsanitize=address,undefined).  Standard input: one crop per line, "n_px flags background x0 y0 x1 y1 image B".  Standard
// output per crop: a line "H" with the 24 header words; for an accepted crop two more lines "T", one per axis, with the axis' table
// bounds[n_px][2] | kk[n_px][ks] - each table in an allocation of exactly that size, so that a write past it is the sanitizer's.
#include <stdio.h>

#include <vector>

#include "hg_preproc_geom.h"

int main() {
    int n_px, flags, image, B;
    unsigned background;
    int32_t bx[4];
    while (scanf("%d %d %u %d %d %d %d %d %d", &n_px, &flags, &background, &bx[0], &bx[1], &bx[2], &bx[3], &image, &B) == 9) {
        if (n_px < 1 || n_px > hg::PREB_MAX_NPX) return 2;
        int32_t h[hg::PREB_HDR];
        const int status = hg::preb_geometry(bx, image, B, n_px, flags, background, h);
        printf("H");
        for (int i = 0; i < hg::PREB_HDR; ++i) printf(" %d", h[i]);
        printf("\n");
        if (status) continue;
        for (int axis = 0; axis < 2; ++axis) {
            const int ks = axis ? h[9] : h[8];
            std::vector<int32_t> bounds((size_t)2 * n_px), kk((size_t)n_px * ks);
            for (int i = 0; i < n_px; ++i) hg::preb_fill_index(h, axis, i, bounds.data() + 2 * i, kk.data() + (size_t)i * ks);
            printf("T");
            for (int32_t v : bounds) printf(" %d", v);
            for (int32_t v : kk) printf(" %d", v);
            printf("\n");
        }
    }
    return 0;
}
