// Geometry and weight tables of the batched crop pre-processing (hg_preproc_batch.hip), as __host__ __device__ inline functions: the
// kernels evaluate them per crop on the device, and a stand-alone host program (tests/preproc_geom_main.cpp) runs the same text.
// The expressions are those hg_preprocess_crops evaluates on the host (hg_api.hip) and preproc_tables_kernel on the device
// (hg_preproc.hip), in the same types and order: torchvision's Resize / CenterCrop (clipnet/clip.py:75-82), expand2square
// (utils_tip_cache_and_union_finetune.py:201-212), Pillow's precompute_coeffs / normalize_coeffs_8bpc.  IEEE double, one rounding per
// operation: whatever includes this is compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HG_GEOM_FN __host__ __device__ inline
#else
#define HG_GEOM_FN inline
#endif

namespace hg {

// ---- limits of one hg_preprocess_batch call -----------------------------------------------------------------------------------------
static constexpr int PREB_MAX_IMAGES = 64;      // images per call: the image table travels as a kernel argument
static constexpr int PREB_MAX_N = 4096;         // crops per call
static constexpr int PREB_MAX_NPX = 518;        // output side
static constexpr int PREB_MAX_TAPS = 65;        // taps per output index on either axis: downscales up to 16 (ceil(2 * 16) * 2 + 1)
static constexpr int PREB_MAX_COORD = 1 << 20;  // |box coordinate| at most: every product below stays inside int32 / exact double
static constexpr int PREB_BAND = 16;            // output rows per band at most
static constexpr int PREB_WIN_ROWS = 72;        // rows of the LDS window: a band of one row needs at most PREB_MAX_TAPS of them
static constexpr int PREB_HCACHE_NPX = 336, PREB_HCACHE_TAPS = 13;      // horizontal weights of a crop kept in LDS: up to this output side, this many taps
static constexpr int PREB_HDR = 24;             // header words per crop
// status bits
static constexpr int PREB_EMPTY = 1, PREB_TAPS = 2, PREB_IMAGE = 4;
// header words: 0 x0  1 y0  2 crop_w  3 crop_h  4 pad_x  5 pad_y  6 src_w  7 src_h  8 ks_h  9 ks_v  10 row_lo  11 n_rows  12 band height
// 13 background (0x00BBGGRR)  14 resized_w  15 resized_h  16 left  17 top  18 col_lo  19 n_cols  20 status  21 image  (22, 23 reserved)
// (0 .. 11 and 13 .. 17 are the words of hg_preprocess_crops' header; 12 is its scratch offset, which does not exist here)

// columns of the virtual source one output row can need at most, and the bytes of LDS the kernel is launched with
HG_GEOM_FN int preb_max_cols(int n_px) { return 16 * n_px + 49; }
HG_GEOM_FN int preb_win_stride(int n_px) { return (n_px * 3 + 15) / 16 * 16; }
HG_GEOM_FN int preb_rowbuf_bytes(int n_px) { return (preb_max_cols(n_px) * 3 + 32 + 15) / 16 * 16; }
HG_GEOM_FN int preb_hcache_words(int n_px) { return ((n_px <= PREB_HCACHE_NPX) * n_px * PREB_HCACHE_TAPS + 3) / 4 * 4; }
HG_GEOM_FN int preb_lds_bytes(int n_px) { return 3 * 256 * 4 + PREB_BAND * (PREB_MAX_TAPS + 2) * 4 + PREB_WIN_ROWS * 4 + 64 + preb_rowbuf_bytes(n_px) + PREB_WIN_ROWS * preb_win_stride(n_px) + preb_hcache_words(n_px) * 4; }
// words of one axis' table of one crop: bounds[n_px][2] | kk[n_px][ks], ks <= PREB_MAX_TAPS
HG_GEOM_FN size_t preb_axis_words(int n_px) { return (size_t)n_px * (2 + PREB_MAX_TAPS); }

HG_GEOM_FN double preb_cubic(double x) {      // Pillow's bicubic_filter, a = -0.5
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

HG_GEOM_FN int preb_taps(int in, int outn) {
#pragma clang fp contract(off)
    const double sc = (double)in / (double)outn, fs = sc < 1.0 ? 1.0 : sc;
    return (int)ceil(2.0 * fs) * 2 + 1;
}
HG_GEOM_FN int preb_first_tap(int in, int outn, int idx) {
#pragma clang fp contract(off)
    const double sc = (double)in / (double)outn, fs = sc < 1.0 ? 1.0 : sc;
    const int v = (int)(((double)idx + 0.5) * sc - 2.0 * fs + 0.5);
    return v < 0 ? 0 : v;
}
HG_GEOM_FN int preb_end_tap(int in, int outn, int idx) {
#pragma clang fp contract(off)
    const double sc = (double)in / (double)outn, fs = sc < 1.0 ? 1.0 : sc;
    const int v = (int)(((double)idx + 0.5) * sc + 2.0 * fs + 0.5);
    return v > in ? in : v;
}

// The header of one crop -> h[PREB_HDR]; returns the status (also h[20]).  A refused crop (status != 0) has every geometry word 0:
// nothing may be indexed with them.
HG_GEOM_FN int preb_geometry(const int32_t* bx, int image, int B, int n_px, int flags, uint32_t background, int32_t* h) {
#pragma clang fp contract(off)
    for (int i = 0; i < PREB_HDR; ++i) h[i] = 0;
    int status = 0;
    if (image < 0 || image >= B) status |= PREB_IMAGE;
    const long long cwl = (long long)bx[2] - (long long)bx[0], chl = (long long)bx[3] - (long long)bx[1];
    if (cwl <= 0 || chl <= 0) status |= PREB_EMPTY;
    else
        for (int i = 0; i < 4; ++i)
            if (bx[i] > PREB_MAX_COORD || bx[i] < -PREB_MAX_COORD) status |= PREB_TAPS;      // (no downscale within the tap limit gets there)
    h[13] = (int32_t)background;
    h[21] = image;
    if (!(status & (PREB_EMPTY | PREB_TAPS))) {
        const int cw = (int)cwl, ch = (int)chl;
        int sw = cw, sh = ch, px = 0, py = 0;
        if ((flags & 1) && cw != ch) {                              // expand2square: centred, floor((side - short) / 2)
            if (cw > ch) py = (cw - ch) / 2; else px = (ch - cw) / 2;
            sw = sh = cw > ch ? cw : ch;
        }
        int nw, nh;
        if (flags & 2) { nw = nh = n_px; }                          // IResize([n_px, n_px]): both sides, no centre crop
        else if (sw <= sh) { nw = n_px; nh = (int)((double)((long long)n_px * sh) / (double)sw); }
        else { nw = (int)((double)((long long)n_px * sw) / (double)sh); nh = n_px; }
        const int left = (int)nearbyint((double)(nw - n_px) / 2.0), top = (int)nearbyint((double)(nh - n_px) / 2.0);
        const int ks_h = preb_taps(sw, nw), ks_v = preb_taps(sh, nh);
        if (ks_h > PREB_MAX_TAPS || ks_v > PREB_MAX_TAPS) status |= PREB_TAPS;
        else {
            const int row_lo = preb_first_tap(sh, nh, top), n_rows = preb_end_tap(sh, nh, top + n_px - 1) - row_lo;
            const int col_lo = preb_first_tap(sw, nw, left), n_cols = preb_end_tap(sw, nw, left + n_px - 1) - col_lo;
            // band height: the source rows a band of bh output rows needs number at most (bh - 1) * scale + 4 * filterscale + 2
            const double sc = (double)sh / (double)nh, fs = sc < 1.0 ? 1.0 : sc;
            const double f = ((double)PREB_WIN_ROWS - 4.0 * fs - 2.0) / sc;
            int bh = f >= (double)(PREB_BAND - 1) ? PREB_BAND : (int)f + 1;
            if (bh < 1) bh = 1;
            if (n_cols > preb_max_cols(n_px) || n_cols < 0 || n_rows < 0) status |= PREB_TAPS;      // (cannot happen within the tap limit)
            else if (!status) {                                                                      // (an image index outside the call: words stay 0)
                h[0] = bx[0]; h[1] = bx[1]; h[2] = cw; h[3] = ch; h[4] = px; h[5] = py; h[6] = sw; h[7] = sh;
                h[8] = ks_h; h[9] = ks_v; h[10] = row_lo; h[11] = n_rows; h[12] = bh;
                h[14] = nw; h[15] = nh; h[16] = left; h[17] = top; h[18] = col_lo; h[19] = n_cols;
            }
        }
    }
    h[20] = status;
    return status;
}

// bounds (first tap, count) and the ks fixed-point weights of output index i of one axis (axis 0 horizontal, 1 vertical)
HG_GEOM_FN void preb_fill_index(const int32_t* h, int axis, int i, int32_t* bounds2, int32_t* kk) {
#pragma clang fp contract(off)
    const int in_size = axis ? h[7] : h[6];
    const int out_size = axis ? h[15] : h[14];
    const int first = axis ? h[17] : h[16];
    const int ks = axis ? h[9] : h[8];
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = ((double)(first + i) + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += preb_cubic(((double)(x + xmin) - center + 0.5) * ss);
    for (int x = 0; x < ks; ++x) {
        double w = 0.0;
        if (x < xmax) {
            w = preb_cubic(((double)(x + xmin) - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
        }
        kk[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << 22)) : (int)(0.5 + w * (double)(1 << 22));
    }
    bounds2[0] = xmin;
    bounds2[1] = xmax;
}

}  // namespace hg
