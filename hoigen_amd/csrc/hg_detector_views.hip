// The detector's two views of a batch from raw images (hg_detector_views): for every uint8 [H, W, 3] image of the call
//   RandomResize([size], max_size)        detr/datasets/transforms_clip.py:139-170: a Pillow BICUBIC resize of the whole image
//   ToTensor, Normalize (ImageNet)        utils_tip_cache_and_union_finetune.py:86-89, :109-114
//   nested_tensor_from_tensor_list        detr/util/misc.py:307-329: zero padding to the batch maxima, mask 1 in the padding
// and, of the RESIZED image, IResize([clip_px, clip_px]) + the same normalisation (utils_tip_cache_and_union_finetune.py:193-196) by
// the kernels of hg_preproc_batch.hip.  Every size is known on the host (hg_detector_view_shapes), so the host sizes and places
// everything; the weights and every index come from tables filled on the device.  Two launches of its own, then hg_preprocess_batch's two:
//   1. dv_tables_kernel, grid (256 output indices, axis, image): a lane per output index fills bounds and weights of its axis
//      (preb_fill_index: Pillow's precompute_coeffs / normalize_coeffs_8bpc in IEEE double); one thread per image writes the
//      whole-image box of the resized image and its image number for the CLIP leg;
//   2. dv_resample_kernel, grid (group of DV_STRIPS strips of DV_STRIP output columns, band, image): the bands of an image are those of
//      its own rows (dv_band_rows of them, from the vertical scale) and then bands of DV_BAND rows of padding down to hmax.  Strip by
//      strip, a workgroup resamples the source rows its band's vertical taps reach horizontally, straight from the image (a wave per
//      source row, a lane per output column: neighbouring lanes read neighbouring bytes) into an LDS window of uint8 rows; the vertical
//      pass runs from the window; clip8 after each pass; then the uint8 row, the three fp32 plane rows through the 3 x 256 table (x
//      fastest) and the mask; columns right of the image and the padding bands get 0 and mask 1.
// Compiled with -ffp-contract=off (build.sh), like hg_preproc_batch.hip.
#include "hg_kernels.h"
#include "hg_detector_views_geom.h"

namespace hg {

static constexpr int DV_PREC = 22;
static constexpr int DV_THREADS = 512, DV_WAVES = DV_THREADS / 64;
static constexpr int DV_WSTRIDE = DV_STRIP * 3;      // bytes of a window row
static constexpr int DV_GROUP = DV_STRIP * DV_STRIPS;      // output columns of a workgroup

__device__ __forceinline__ int dv_clip8(int v) {
    v >>= DV_PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// tab: the images' tables at word dv.tab[b] (layout: dv_table_words); boxes [B][4], crop_image [B]: the CLIP leg's arguments
__global__ __launch_bounds__(256) void dv_tables_kernel(DvBatch dv, int32_t* __restrict__ tab, int32_t* __restrict__ boxes,
                                                        int32_t* __restrict__ crop_image) {
#pragma clang fp contract(off)
    const int b = blockIdx.z, axis = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int H = dv.H[b], W = dv.W[b], oh = dv.oh[b], ow = dv.ow[b];
    if (i == 0 && axis == 0) {
        boxes[4 * b] = 0; boxes[4 * b + 1] = 0; boxes[4 * b + 2] = ow; boxes[4 * b + 3] = oh;
        crop_image[b] = b;
    }
    if (i >= (axis ? oh : ow)) return;
    int32_t h[PREB_HDR];      // the words preb_fill_index reads: sizes, taps, no centre-crop offset
    h[6] = W; h[7] = H; h[8] = preb_taps(W, ow); h[9] = preb_taps(H, oh); h[14] = ow; h[15] = oh; h[16] = 0; h[17] = 0;
    int32_t* bounds = tab + dv.tab[b] + (axis ? (size_t)ow * (2 + h[8]) : 0);
    int32_t* kk = bounds + 2 * (size_t)(axis ? oh : ow);
    preb_fill_index(h, axis, i, bounds + 2 * i, kk + (size_t)i * (axis ? h[9] : h[8]));
}

__global__ __launch_bounds__(DV_THREADS) void dv_resample_kernel(DvBatch dv, const int32_t* __restrict__ tab, uint8_t* __restrict__ u8,
                                                                 float* __restrict__ detr, uint8_t* __restrict__ mask) {
    __shared__ float lut[3 * 256];
    __shared__ int32_t vw[DV_VW_WORDS];             // the band's vertical weights [rows][ks_v]
    __shared__ int32_t vbnd[DV_BAND * 2];           // and (first window slot, count) [rows][2]
    __shared__ __attribute__((aligned(16))) uint8_t win[DV_WIN_ROWS * DV_WSTRIDE];
    const int b = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int H = dv.H[b], W = dv.W[b], oh = dv.oh[b], ow = dv.ow[b], hmax = dv.hmax, wmax = dv.wmax;
    const int bh = dv_band_rows(H, oh), nb = (oh + bh - 1) / bh;
    const int band = blockIdx.y;
    const bool own = band < nb;                    // a band of the image's own rows; else of the padding below it
    const int r0 = own ? band * bh : oh + (band - nb) * DV_BAND;
    if (r0 >= hmax) return;
    const int r1 = own ? (r0 + bh < oh ? r0 + bh : oh) : (r0 + DV_BAND < hmax ? r0 + DV_BAND : hmax);
    const int g0 = blockIdx.x * DV_GROUP, g1 = g0 + DV_GROUP < wmax ? g0 + DV_GROUP : wmax;      // the workgroup's columns; g0 < wmax: the grid
    const int ge = own ? (g1 < ow ? g1 : ow) : g0;      // columns [g0, ge) are the image's, [max(g0, ge), g1) padding
    float* planes = detr + (size_t)b * 3 * hmax * wmax;
    uint8_t* mrow = mask + (size_t)b * hmax * wmax;
    if (ge > g0) {
        for (int i = tid; i < 3 * 256; i += DV_THREADS) {      // ToTensor + Normalize as a table: preproc_v_kernel's expression, ImageNet
            const int c = i >> 8;
            const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
            lut[i] = ((float)(i & 255) / 255.0f - mean) / sd;
        }
        const int ksh = preb_taps(W, ow), ksv = preb_taps(H, oh);
        const int32_t* hb = tab + dv.tab[b];
        const int32_t* hk = hb + 2 * (size_t)ow;
        const int32_t* vb = hk + (size_t)ow * ksh;
        const int32_t* vk = vb + 2 * (size_t)oh;
        const uint8_t* img = dv.img[b];
        uint8_t* out_u8 = u8 + (size_t)dv.u8_256[b] * 256;
        const int rlo = vb[2 * r0];
        int nr = vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1] - rlo;
        if (nr > DV_WIN_ROWS) nr = DV_WIN_ROWS;      // (cannot happen: dv_band_rows)
        if (nr < 0) nr = 0;
        for (int i = tid; i < (r1 - r0) * ksv; i += DV_THREADS) vw[i] = vk[(size_t)r0 * ksv + i];      // <= DV_VW_WORDS: dv_band_rows
        for (int i = tid; i < r1 - r0; i += DV_THREADS) {
            const int cnt = vb[2 * (r0 + i) + 1];
            vbnd[2 * i] = vb[2 * (r0 + i)] - rlo;
            vbnd[2 * i + 1] = cnt < ksv ? cnt : ksv;
        }
        for (int x0 = g0; x0 < ge; x0 += DV_STRIP) {      // strip by strip through the one window
            const int xo = x0 + lane;                     // a lane per column of the strip
            const bool live = xo < ge;
            __syncthreads();                              // the strip before has read the window (the first: the tables above are written)
            // horizontal pass: source row rlo + q -> window row q; a wave per row
            if (live) {
                int first = hb[2 * xo], cnt = hb[2 * xo + 1] < ksh ? hb[2 * xo + 1] : ksh;
                if (first < 0) first = 0;
                if (first + cnt > W) cnt = W - first;      // (cannot happen: a table's taps end inside the image)
                const int32_t* k = hk + (size_t)xo * ksh;
                for (int q = wave; q < nr; q += DV_WAVES) {
                    const int iy = rlo + q < H ? rlo + q : H - 1;      // (rlo + q < H, for the same reason)
                    const uint8_t* p = img + ((size_t)iy * W + first) * 3;
                    int a0 = 1 << (DV_PREC - 1), a1 = a0, a2 = a0;
                    for (int j = 0; j < cnt; ++j) {
                        const int w = k[j];
                        a0 += (int)p[3 * j] * w; a1 += (int)p[3 * j + 1] * w; a2 += (int)p[3 * j + 2] * w;
                    }
                    uint8_t* d = win + q * DV_WSTRIDE + lane * 3;
                    d[0] = (uint8_t)dv_clip8(a0); d[1] = (uint8_t)dv_clip8(a1); d[2] = (uint8_t)dv_clip8(a2);
                }
            }
            __syncthreads();
            // vertical pass from the window: a wave per output row, x fastest, so that the fp32 plane stores coalesce
            if (live)
            for (int rr = wave; rr < r1 - r0; rr += DV_WAVES) {
                const int yo = r0 + rr;
                const int first = vbnd[2 * rr], cnt = vbnd[2 * rr + 1];
                const int32_t* k = vw + rr * ksv;
                for (int c = 0; c < 3; ++c) {
                    int acc = 1 << (DV_PREC - 1);
                    for (int j = 0; j < cnt; ++j) {
                        const int slot = first + j;
                        if ((unsigned)slot < (unsigned)nr) acc += (int)win[slot * DV_WSTRIDE + lane * 3 + c] * k[j];
                    }
                    const int u = dv_clip8(acc);
                    out_u8[((size_t)yo * ow + xo) * 3 + c] = (uint8_t)u;
                    planes[((size_t)c * hmax + yo) * wmax + xo] = lut[c * 256 + u];
                }
                mrow[(size_t)yo * wmax + xo] = 0;
            }
        }
    }
    // the padding of these rows: right of the image, or all the workgroup's columns below it
    const int p0 = ge > g0 ? ge : g0;
    for (int rr = wave; rr < r1 - r0; rr += DV_WAVES) {
        const int yo = r0 + rr;
        for (int xo = p0 + lane; xo < g1; xo += 64) {
            for (int c = 0; c < 3; ++c) planes[((size_t)c * hmax + yo) * wmax + xo] = 0.0f;
            mrow[(size_t)yo * wmax + xo] = 1;
        }
    }
}

hipError_t launch_detector_views(const DvBatch& dv, int max_bands, int32_t* tab, int32_t* boxes, int32_t* crop_image, uint8_t* u8,
                                 float* detr, uint8_t* mask, hipStream_t s) {
    int side = 1;
    for (int b = 0; b < dv.B; ++b) {
        if (dv.oh[b] > side) side = dv.oh[b];
        if (dv.ow[b] > side) side = dv.ow[b];
    }
    hipLaunchKernelGGL(dv_tables_kernel, dim3((side + 255) / 256, 2, dv.B), dim3(256), 0, s, dv, tab, boxes, crop_image);
    hipLaunchKernelGGL(dv_resample_kernel, dim3((dv.wmax + DV_GROUP - 1) / DV_GROUP, max_bands, dv.B), dim3(DV_THREADS), 0, s, dv, tab, u8,
                       detr, mask);
    return hipGetLastError();
}

}  // namespace hg

// ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
#include "hg_host.h"

extern "C" {

int hg_detector_view_shapes(const int32_t* heights, const int32_t* widths, int B, int size, int max_size, int32_t* out_sizes,
                            int32_t* hmax, int32_t* wmax, int64_t* u8_off) {
    using namespace hg;
    if (!heights || !widths || !hmax || !wmax) return HG_ERR_INVALID;
    *hmax = -1; *wmax = DV_INPUT;
    if (B < 1 || size < 1 || size > DV_MAX_SIDE || max_size < 0 || max_size > DV_MAX_SIDE) return HG_ERR_INVALID;
    int hm = 0, wm = 0;
    int64_t off = 0;
    for (int b = 0; b < B; ++b) {
        int oh = 0, ow = 0;
        const int why = heights[b] < 1 || widths[b] < 1 ? DV_INPUT : dv_out_size(heights[b], widths[b], size, max_size, &oh, &ow);
        if (why) { *hmax = b; *wmax = why; return HG_ERR_INVALID; }
        if (out_sizes) { out_sizes[2 * b] = oh; out_sizes[2 * b + 1] = ow; }
        if (u8_off) u8_off[b] = off;
        off += ((int64_t)oh * ow * 3 + 255) / 256 * 256;
        if (oh > hm) hm = oh;
        if (ow > wm) wm = ow;
    }
    if (u8_off) u8_off[B] = off;
    *hmax = hm; *wmax = wm;
    return HG_OK;
}

int hg_detector_views(hg_ctx* c, const hg_detector_views_args* a, void* stream) {
    using namespace hg;
    using namespace hg_host;
    if (!c) return HG_ERR_INVALID;
    if (!a) return fail(c, HG_ERR_INVALID, "hg_detector_views: null arguments");
    if (a->B < 1 || a->B > DV_MAX_IMAGES) return fail(c, HG_ERR_INVALID, "hg_detector_views: B must be 1 .. %d (got %d)", DV_MAX_IMAGES, a->B);
    if (a->clip_px < 0 || a->clip_px > DV_MAX_CLIP_PX)
        return fail(c, HG_ERR_INVALID, "hg_detector_views: clip_px must be 0 .. %d (got %d)", DV_MAX_CLIP_PX, a->clip_px);
    if (a->size < 1 || a->size > DV_MAX_SIDE || a->max_size < 0 || a->max_size > DV_MAX_SIDE)
        return fail(c, HG_ERR_INVALID, "hg_detector_views: size must be 1 .. %d and max_size 0 .. %d (got %d, %d)", DV_MAX_SIDE, DV_MAX_SIDE,
                    a->size, a->max_size);
    if (!a->images || !a->heights || !a->widths || !a->detr || !a->mask || (a->clip_px && !a->clip))
        return fail(c, HG_ERR_INVALID, "hg_detector_views: null pointer among images, heights, widths, detr, mask, clip");
    int32_t sizes[2 * DV_MAX_IMAGES], hm = 0, wm = 0;
    int64_t off[DV_MAX_IMAGES + 1];
    if (hg_detector_view_shapes(a->heights, a->widths, a->B, a->size, a->max_size, sizes, &hm, &wm, off)) {
        static const char* const why[] = {"", "an output side of 0", "an output side above 2048", "more than 65 taps on an axis (a downscale above 16)",
                                          "a side <= 0"};
        return fail(c, HG_ERR_INVALID, "hg_detector_views: image %d (%d x %d, h x w): %s", hm, a->heights[hm], a->widths[hm], why[wm]);
    }
    if (a->hmax || a->wmax) {      // a slice of a larger batch: the padded extent is the caller's
        if (a->hmax < hm || a->wmax < wm || a->hmax > DV_MAX_SIDE || a->wmax > DV_MAX_SIDE)
            return fail(c, HG_ERR_INVALID, "hg_detector_views: hmax, wmax must be 0, 0 or %d .. %d, %d .. %d (got %d, %d)", hm, DV_MAX_SIDE, wm,
                        DV_MAX_SIDE, a->hmax, a->wmax);
        hm = a->hmax; wm = a->wmax;
    }
    DvBatch dv = {};
    PreBatch pb = {};
    dv.B = pb.B = a->B; dv.hmax = hm; dv.wmax = wm;
    size_t words = 0;
    int max_bands = 1;
    for (int b = 0; b < a->B; ++b) {
        const int oh = sizes[2 * b], ow = sizes[2 * b + 1];
        if (!a->images[b]) return fail(c, HG_ERR_INVALID, "hg_detector_views: image %d is null", b);
        if (a->clip_px && (preb_taps(ow, a->clip_px) > PREB_MAX_TAPS || preb_taps(oh, a->clip_px) > PREB_MAX_TAPS))
            return fail(c, HG_ERR_INVALID, "hg_detector_views: image %d: its resized image (%d x %d) needs more than 65 taps on an axis at clip_px %d",
                        b, oh, ow, a->clip_px);
        dv.img[b] = a->images[b]; dv.H[b] = a->heights[b]; dv.W[b] = a->widths[b]; dv.oh[b] = oh; dv.ow[b] = ow;
        dv.tab[b] = (int32_t)words;                       // <= 64 * 2 * 2048 * 67 words
        dv.u8_256[b] = (uint32_t)(off[b] / 256);          // <= 64 * 2048 * 2048 * 3 / 256
        words += dv_table_words(dv.H[b], dv.W[b], oh, ow);
        const int nbands = dv_bands(dv.H[b], oh, hm);
        if (nbands > max_bands) max_bands = nbands;
        pb.H[b] = oh; pb.W[b] = ow;
    }
    HG_ON_DEVICE(c);
    // workspace: boxes [64][4] | crop_image [64] | status [64] | tables | the resized images where the caller does not ask for them
    const size_t fixed = (size_t)DV_MAX_IMAGES * 6 * 4, tab_bytes = rup(words * 4, 256);
    int rc = ensure(c, c->dviews, fixed + tab_bytes + (a->resized_u8 ? 0 : (size_t)off[a->B]));
    const size_t head_words = (size_t)a->B * PREB_HDR;
    if (!rc && a->clip_px) rc = ensure(c, c->prebatch, (head_words + (size_t)a->B * 2 * preb_axis_words(a->clip_px)) * 4);
    if (rc) return rc;
    int32_t* boxes = (int32_t*)c->dviews.p;
    int32_t* crop_image = boxes + 4 * DV_MAX_IMAGES;
    int32_t* status = crop_image + DV_MAX_IMAGES;
    int32_t* tab = status + DV_MAX_IMAGES;
    uint8_t* u8 = a->resized_u8 ? a->resized_u8 : (uint8_t*)c->dviews.p + fixed + tab_bytes;
    hipStream_t s = (hipStream_t)stream;
    HG_HIP(launch_detector_views(dv, max_bands, tab, boxes, crop_image, u8, a->detr, a->mask, s));
    if (a->clip_px) {
        for (int b = 0; b < a->B; ++b) pb.img[b] = u8 + off[b];
        int32_t* head = (int32_t*)c->prebatch.p;
        HG_HIP(launch_preprocess_batch(pb, boxes, crop_image, a->B, a->clip_px, HG_PRE_STRETCH | HG_PRE_IMAGENET_NORM, 0, head, head + head_words,
                                       a->clip, nullptr, status, s));
    }
    return HG_OK;
}

}  // extern "C"
