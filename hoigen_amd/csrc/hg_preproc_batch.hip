// Crop pre-processing of a batch of images in one call (hg_preprocess_batch): for every crop i of image crop_image[i]
//   image.crop(box)                       pre_images/crop_images.py:204-219 (PIL: zeros outside the image)
//   [expand2square(crop, background)]     utils_tip_cache_and_union_finetune.py:201-212
//   Resize(n_px, BICUBIC), CenterCrop(n_px), ToTensor, Normalize      clipnet/clip.py:75-82
//   or IResize([n_px, n_px]) + the ImageNet constants: the detector's CLIP view, utils_tip_cache_and_union_finetune.py:105-114
// with the bytes and fp32 bits of hg_preprocess_crops (hg_preproc.hip).  The boxes live in DEVICE memory and the host never reads them,
// so nothing here may be sized from a box: the geometry is worked out on the device (hg_preproc_geom.h), and the intermediate of the
// separable resize - which hg_preprocess_crops writes to a global scratch sized from the boxes - stays in LDS.  Two launches:
//   1. prebatch_tables_kernel, grid (crop, axis): thread 0 works out the crop's header and status; one lane per output index fills the
//      weight table of its axis, in a slot of n_px * (2 + PREB_MAX_TAPS) words laid out bounds[n_px][2] | kk[n_px][ks];
//   2. prebatch_resample_kernel, grid (band slot, crop): a workgroup takes bands of at most PREB_BAND output rows of one crop.  Per band:
//      the source rows [rlo, rhi) its vertical taps reach are loaded from the image once, 16 bytes a lane, into an LDS row buffer (several
//      rows a trip), resampled horizontally into an LDS window of uint8 rows (slot = source row - rlo: the window does not roll, a band
//      whose rows would not fit PREB_WIN_ROWS is shorter - header word 12), and the vertical pass runs from that window; clip8 after
//      each pass; 3 x 256 normalisation table; fp32 plane stores with xo fastest, optional uint8 NHWC.
//      512 threads: a wave per row, a lane per column.  The band's vertical weights, and the crop's horizontal weights where they fit
//      (preb_hcache_words), are read from LDS.
// A refused crop (status != 0) has NaN planes and zero bytes, written from its crop number alone before anything is indexed.
// Compiled with -ffp-contract=off (build.sh), like hg_preproc.hip: the weight tables are IEEE double with one rounding per operation.
#include "hg_kernels.h"
#include "hg_preproc_geom.h"

namespace hg {

static constexpr int PREB_PREC = 22;
static constexpr int PREB_THREADS = 512, PREB_WAVES = PREB_THREADS / 64;      // two workgroups a CU at n_px 224 (78 688 bytes of LDS each): four waves a SIMD

__device__ __forceinline__ int preb_clip8(int v) {
    v >>= PREB_PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// head [n][PREB_HDR], tab [n][2][preb_axis_words(n_px)], status [n]
__global__ __launch_bounds__(256) void prebatch_tables_kernel(const int32_t* __restrict__ boxes, const int32_t* __restrict__ crop_image, int B,
                                                              int n_px, int flags, uint32_t background, int32_t* __restrict__ head,
                                                              int32_t* __restrict__ tab, int32_t* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ int32_t h[PREB_HDR];
    const int crop = blockIdx.x, axis = blockIdx.y;
    if (threadIdx.x == 0) {
        int32_t bx[4];
        for (int i = 0; i < 4; ++i) bx[i] = boxes[4 * (size_t)crop + i];
        preb_geometry(bx, crop_image[crop], B, n_px, flags, background, h);
    }
    __syncthreads();
    if (axis == 0 && threadIdx.x < PREB_HDR) head[(size_t)crop * PREB_HDR + threadIdx.x] = h[threadIdx.x];
    if (axis == 0 && threadIdx.x == 0) status[crop] = h[20];
    if (h[20]) return;
    int32_t* bounds = tab + ((size_t)crop * 2 + axis) * preb_axis_words(n_px);
    int32_t* kk = bounds + 2 * n_px;
    const int ks = axis ? h[9] : h[8];      // <= PREB_MAX_TAPS: checked by preb_geometry
    for (int i = threadIdx.x; i < n_px; i += 256) preb_fill_index(h, axis, i, bounds + 2 * i, kk + (size_t)i * ks);
}

__global__ __launch_bounds__(PREB_THREADS) void prebatch_resample_kernel(PreBatch pb, const int32_t* __restrict__ head, const int32_t* __restrict__ tab,
                                                                int n_px, float* __restrict__ out, uint8_t* __restrict__ out_u8,
                                                                int imagenet_norm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t preb_lds[];
    const int crop = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t* t = head + (size_t)crop * PREB_HDR;
    const size_t plane = (size_t)n_px * n_px;
    if (t[20]) {      // refused: NaN planes, zero bytes, nothing else read
        const float nan = __int_as_float(0x7fc00000);
        for (size_t i = (size_t)blockIdx.x * PREB_THREADS + tid; i < 3 * plane; i += (size_t)gridDim.x * PREB_THREADS) {
            out[(size_t)crop * 3 * plane + i] = nan;
            if (out_u8) out_u8[(size_t)crop * 3 * plane + i] = 0;
        }
        return;
    }
    const int bh = t[12], n_bands = (n_px + bh - 1) / bh;
    if ((int)blockIdx.x >= n_bands) return;
    float* lut = (float*)preb_lds;
    int32_t* vw = (int32_t*)(preb_lds + 3 * 256 * 4);      // the band's vertical weights [bh][ks_v] and (first slot, count) [bh][2]
    int32_t* vbnd = vw + PREB_BAND * PREB_MAX_TAPS;
    int32_t* rowinfo = vbnd + PREB_BAND * 2;               // per row of the trip: its lead (0 .. 15) in the image, 16 in the crop outside the image, 32 padding
    int32_t* geo = rowinfo + PREB_WIN_ROWS;                // 16 words of the crop's geometry: read back per lane (vector registers: the scalar file is full)
    uint8_t* rowbuf = (uint8_t*)(geo + 16);
    const int rowbuf_bytes = preb_rowbuf_bytes(n_px), wstride = preb_win_stride(n_px);
    uint8_t* win = rowbuf + rowbuf_bytes;
    for (int i = tid; i < 3 * 256; i += PREB_THREADS) {      // ToTensor + Normalize as a table: preproc_v_kernel's expression
        const int c = i >> 8;
        // CLIP's own constants (clipnet/clip.py:81), or the detector's CLIP view (utils_tip_cache_and_union_finetune.py:86-89)
        const float mean = imagenet_norm ? (c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f)) : (c == 0 ? 0.48145466f : (c == 1 ? 0.4578275f : 0.40821073f));
        const float sd = imagenet_norm ? (c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f)) : (c == 0 ? 0.26862954f : (c == 1 ? 0.26130258f : 0.27577711f));
        lut[i] = ((float)(i & 255) / 255.0f - mean) / sd;
    }
    const int ksh = t[8], ksv = t[9];
    const int im = t[21];                            // inside [0, B): a crop with status 0
    const uint8_t* img = pb.img[im];
    const int H = pb.H[im], W = pb.W[im];
    const size_t img_bytes = (size_t)H * W * 3;
    // the image columns [ixs, ixe) a source row can need: virtual columns [col_lo, col_lo + n_cols) -> crop columns -> the image
    int n_in;
    {
        const int sx0 = t[0], scw = t[2], spx = t[4], col_lo = t[18], n_cols = t[19];
        int cxs = col_lo - spx, cxe = col_lo + n_cols - spx;
        if (cxs < 0) cxs = 0;
        if (cxe > scw) cxe = scw;
        int sixs = sx0 + cxs, sixe = sx0 + cxe;
        if (sixs < 0) sixs = 0;
        if (sixe > W) sixe = W;
        n_in = sixe > sixs ? sixe - sixs : 0;
        if (tid == 0) {
            geo[0] = sx0; geo[1] = t[1]; geo[2] = scw; geo[3] = t[3]; geo[4] = spx; geo[5] = t[5]; geo[6] = t[13]; geo[7] = sixs; geo[8] = sixe;
            geo[9] = H; geo[10] = W;
        }
    }
    const int32_t* hb = tab + (size_t)crop * 2 * preb_axis_words(n_px);
    const int32_t* hk = hb + 2 * n_px;
    const int32_t* vb = hb + preb_axis_words(n_px);
    const int32_t* vk = vb + 2 * n_px;
    // the crop's horizontal weights in LDS where they fit the region the launch has for them (downscales up to 3 at n_px <= 336):
    // every source row of every band reads them
    int32_t* hc = (int32_t*)(win + PREB_WIN_ROWS * wstride);
    const bool cached = n_px * ksh <= preb_hcache_words(n_px);
    if (cached)
        for (int i = tid; i < n_px * ksh; i += PREB_THREADS) hc[i] = hk[i];
    const int32_t* hku = cached ? hc : hk;
    __syncthreads();
    const int x0 = geo[0], y0 = geo[1], cw = geo[2], ch = geo[3], px = geo[4], py = geo[5], bg = geo[6], ixs = geo[7], ixe = geo[8];
    const int vH = geo[9], vW = geo[10];
    const int lstride = (n_in * 3 + 15) / 16 * 16 + 16;      // bytes of a row of the row buffer: the row's 16-byte chunks, lead included
    const int rows_per_trip = rowbuf_bytes / lstride;          // >= 1: n_in <= n_cols <= preb_max_cols(n_px)

    for (int band = blockIdx.x; band < n_bands; band += gridDim.x) {
        const int r0 = band * bh, r1 = r0 + bh < n_px ? r0 + bh : n_px;
        const int rlo = vb[2 * r0];
        int nr = vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1] - rlo;
        if (nr > PREB_WIN_ROWS) nr = PREB_WIN_ROWS;              // (cannot happen: header word 12)
        if (nr < 0) nr = 0;
        __syncthreads();                                         // the band before has read vw and vbnd
        for (int i = tid; i < (r1 - r0) * ksv; i += PREB_THREADS) vw[i] = vk[(size_t)r0 * ksv + i];      // bh * ks_v <= PREB_BAND * PREB_MAX_TAPS
        for (int i = tid; i < r1 - r0; i += PREB_THREADS) {
            const int cnt = vb[2 * (r0 + i) + 1];
            vbnd[2 * i] = vb[2 * (r0 + i)] - rlo;
            vbnd[2 * i + 1] = cnt < ksv ? cnt : ksv;
        }
        for (int b0 = 0; b0 < nr; b0 += rows_per_trip) {
            const int rb = nr - b0 < rows_per_trip ? nr - b0 : rows_per_trip;
            __syncthreads();                                     // the trip before has read the row buffer; the band before, the window
            // source rows -> row buffer: 16 bytes a lane, from the 16-byte boundary below the row's first byte
            const int nch = lstride / 16;
            for (int q = tid; q < rb; q += PREB_THREADS) {       // rb <= nr <= PREB_WIN_ROWS
                const int cy = rlo + b0 + q - py, iy = y0 + cy;
                int info = 32;
                if (cy >= 0 && cy < ch) info = (iy >= 0 && iy < vH && n_in > 0) ? (int)(((uintptr_t)img + ((size_t)iy * vW + ixs) * 3) & 15) : 16;
                rowinfo[q] = info;
            }
            for (int q = wave; q < rb; q += PREB_WAVES)          // a wave per row, a lane per 16-byte chunk
            for (int k = lane; k < nch; k += 64) {
                const int cy = rlo + b0 + q - py, iy = y0 + cy;
                if (cy < 0 || cy >= ch || iy < 0 || iy >= vH || n_in == 0) continue;
                const size_t off = ((size_t)iy * vW + ixs) * 3;      // first byte of the row inside the image
                const int lead = (int)(((uintptr_t)img + off) & 15);
                if (k * 16 >= lead + n_in * 3) continue;
                const ptrdiff_t c0 = (ptrdiff_t)off - lead + (ptrdiff_t)k * 16;      // chunk start, relative to the image
                uint4 v;
                if (c0 >= 0 && (size_t)c0 + 16 <= img_bytes) v = *(const uint4*)(img + c0);
                else {      // a chunk across either end of the image: byte by byte, 0 outside (those bytes are never used)
                    auto word = [&](ptrdiff_t a) {
                        uint32_t w = 0;
                        for (int e = 0; e < 4; ++e)
                            if (a + e >= 0 && (size_t)(a + e) < img_bytes) w |= (uint32_t)img[a + e] << (8 * e);
                        return w;
                    };
                    v.x = word(c0); v.y = word(c0 + 4); v.z = word(c0 + 8); v.w = word(c0 + 12);
                }
                *(uint4*)(rowbuf + (size_t)q * lstride + k * 16) = v;
            }
            __syncthreads();
            // horizontal pass: one item per (row of the trip, output column), three channels
            for (int q = wave; q < rb; q += PREB_WAVES)          // a wave per row, a lane per output column
            for (int xo = lane; xo < n_px; xo += 64) {
                const int info = rowinfo[q];
                const bool row_in_crop = info != 32, row_in_img = info < 16;
                const uint8_t* src = rowbuf + (size_t)q * lstride + (info & 15);
                const int first = hb[2 * xo], cnt = hb[2 * xo + 1] < ksh ? hb[2 * xo + 1] : ksh;      // (a count is at most ks: Pillow's ksize)
                const int32_t* k = hku + xo * ksh;
                int a0 = 1 << (PREB_PREC - 1), a1 = a0, a2 = a0;
                for (int j = 0; j < cnt; ++j) {
                    const int cx = first + j - px, ix = x0 + cx;                           // column inside the crop, inside the image
                    const bool in_crop = row_in_crop && cx >= 0 && cx < cw;                  // else: padding
                    const bool in_img = in_crop && row_in_img && ix >= ixs && ix < ixe;      // else: 0 (PIL crop outside the image)
                    const uint8_t* p = src + (in_img ? (ix - ixs) * 3 : 0);                  // (offset 0: bytes of the row buffer, unused)
                    const int p0 = in_img ? p[0] : (in_crop ? 0 : bg & 255), p1 = in_img ? p[1] : (in_crop ? 0 : (bg >> 8) & 255),
                              p2 = in_img ? p[2] : (in_crop ? 0 : (bg >> 16) & 255);
                    const int w = k[j];
                    a0 += p0 * w; a1 += p1 * w; a2 += p2 * w;
                }
                uint8_t* d = win + (size_t)(b0 + q) * wstride + xo * 3;
                d[0] = (uint8_t)preb_clip8(a0); d[1] = (uint8_t)preb_clip8(a1); d[2] = (uint8_t)preb_clip8(a2);
            }
        }
        __syncthreads();
        // vertical pass from the window: xo fastest, so that the fp32 plane stores coalesce
        for (int rr = wave; rr < r1 - r0; rr += PREB_WAVES)      // a wave per output row
        for (int c = 0; c < 3; ++c)
        for (int xo = lane; xo < n_px; xo += 64) {
            const int yo = r0 + rr;
            const int o = xo * 3 + c;
            const int first = vbnd[2 * rr], cnt = vbnd[2 * rr + 1];
            const int32_t* k = vw + rr * ksv;
            int acc = 1 << (PREB_PREC - 1);
            for (int j = 0; j < cnt; ++j) {
                const int slot = first + j;
                if ((unsigned)slot < (unsigned)nr) acc += (int)win[(size_t)slot * wstride + o] * k[j];
            }
            const int u = preb_clip8(acc);
            if (out_u8) out_u8[((size_t)crop * n_px + yo) * n_px * 3 + o] = (uint8_t)u;
            out[(((size_t)crop * 3 + c) * n_px + yo) * n_px + xo] = lut[c * 256 + u];
        }
    }
}

hipError_t launch_preprocess_batch(const PreBatch& pb, const int32_t* boxes, const int32_t* crop_image, int n, int n_px, int flags,
                                   uint32_t background, int32_t* head, int32_t* tab, float* out, uint8_t* out_u8, int32_t* status,
                                   hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int lds = preb_lds_bytes(n_px);
    static bool attr_set_d[HG_MAX_DEVICES] = {};
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&prebatch_resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           preb_lds_bytes(PREB_MAX_NPX));
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    hipLaunchKernelGGL(prebatch_tables_kernel, dim3(n, 2), dim3(256), 0, s, boxes, crop_image, pb.B, n_px, flags, background, head, tab, status);
    const int slots = (n_px + PREB_BAND - 1) / PREB_BAND;
    hipLaunchKernelGGL(prebatch_resample_kernel, dim3(slots, n), dim3(PREB_THREADS), lds, s, pb, head, tab, n_px, out, out_u8, (flags & 4) != 0);
    return hipGetLastError();
}

}  // namespace hg
