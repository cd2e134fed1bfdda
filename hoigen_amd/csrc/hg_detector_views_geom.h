// Sizes and tiling of the detector's two views of a batch (hg_detector_views.hip), as __host__ __device__ inline
// functions: the host sizes every buffer and validates every image with them, the kernels derive a workgroup's band from them, and
// tests/detector_views_model.py restates them.  The size rule is get_size_with_aspect_ratio (detr/datasets/transforms_clip.py:142-161)
// in IEEE double, one rounding per operation: whatever includes this is compiled with -ffp-contract=off.
#pragma once
#include "hg_preproc_geom.h"

namespace hg {

// ---- limits of one hg_detector_views call ---------------------------------------------------------------------------------------------
static constexpr int DV_MAX_IMAGES = 64;      // images per call: the image table travels as a kernel argument
static constexpr int DV_MAX_SIDE = 2048;      // output side at most
static constexpr int DV_MAX_TAPS = PREB_MAX_TAPS;      // taps per output index on either axis: downscales up to 16
static constexpr int DV_MAX_CLIP_PX = PREB_MAX_NPX;
static constexpr int DV_BAND = 32;            // output rows of a workgroup at most
static constexpr int DV_STRIP = 64;           // output columns of a strip: a lane each
static constexpr int DV_STRIPS = 4;           // strips of a workgroup
static constexpr int DV_WIN_ROWS = 72;        // rows of the LDS window of horizontally resampled rows: a band of one row needs at most DV_MAX_TAPS
static constexpr int DV_VW_WORDS = 512;       // words of LDS for the vertical weights of a band: band rows * taps stays below
// reasons hg_detector_view_shapes refuses an image with
static constexpr int DV_ZERO_SIDE = 1, DV_SIDE_ABOVE = 2, DV_TAPS = 3, DV_INPUT = 4;

// get_size_with_aspect_ratio((w, h), size, max_size) -> (oh, ow); max_size 0: None.  Returns 0, or the reason the image is refused with
// (then oh, ow hold nothing to be used).  1 <= h, w; 1 <= size <= DV_MAX_SIDE; 0 <= max_size <= DV_MAX_SIDE: checked by the caller.
HG_GEOM_FN int dv_out_size(int h, int w, int size, int max_size, int* oh, int* ow) {
#pragma clang fp contract(off)
    *oh = *ow = 0;
    if (max_size > 0) {
        const double mn = (double)(w < h ? w : h), mx = (double)(w < h ? h : w);
        if (mx / mn * (double)size > (double)max_size) size = (int)nearbyint((double)max_size * mn / mx);      // Python's round: half to even
    }
    double dh, dw;
    if ((w <= h && w == size) || (h <= w && h == size)) { dh = (double)h; dw = (double)w; }
    else if (w < h) { dw = (double)size; dh = floor((double)((long long)size * h) / (double)w); }
    else { dh = (double)size; dw = floor((double)((long long)size * w) / (double)h); }
    if (dh < 1.0 || dw < 1.0) return DV_ZERO_SIDE;                              // Pillow raises "height and width must be > 0"
    if (dh > (double)DV_MAX_SIDE || dw > (double)DV_MAX_SIDE) return DV_SIDE_ABOVE;
    *oh = (int)dh; *ow = (int)dw;
    if (preb_taps(w, *ow) > DV_MAX_TAPS || preb_taps(h, *oh) > DV_MAX_TAPS) return DV_TAPS;
    return 0;
}

// output rows of one band of an image resized from in_h to out_h rows: the source rows a band of bh output rows reaches number at most
// (bh - 1) * scale + 4 * filterscale + 2 <= DV_WIN_ROWS, and its bh * taps vertical weights fit DV_VW_WORDS
HG_GEOM_FN int dv_band_rows(int in_h, int out_h) {
#pragma clang fp contract(off)
    const double sc = (double)in_h / (double)out_h, fs = sc < 1.0 ? 1.0 : sc;
    const double f = ((double)DV_WIN_ROWS - 4.0 * fs - 2.0) / sc;
    int bh = f >= (double)(DV_BAND - 1) ? DV_BAND : (int)f + 1;
    if (bh < 1) bh = 1;
    const int ks = preb_taps(in_h, out_h);
    while (bh > 1 && bh * ks > DV_VW_WORDS) --bh;
    return bh;
}
// bands of an image inside a padded extent of hmax rows: those of its own rows, then whole bands of padding
HG_GEOM_FN int dv_bands(int in_h, int out_h, int hmax) {
    const int bh = dv_band_rows(in_h, out_h);
    return (out_h + bh - 1) / bh + (hmax - out_h + DV_BAND - 1) / DV_BAND;
}
// words of one image's weight tables: hb [ow][2] | hk [ow][ks_h] | vb [oh][2] | vk [oh][ks_v]
HG_GEOM_FN size_t dv_table_words(int h, int w, int oh, int ow) {
    return (size_t)ow * (2 + preb_taps(w, ow)) + (size_t)oh * (2 + preb_taps(h, oh));
}

}  // namespace hg
