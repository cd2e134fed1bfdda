// What follows the interaction head, for a whole batch: the detections of UPT.postprocessing
// (upt_tip_cache_model_free_finetune_distill3.py:1408-1427) compacted on the device, and test_hico's association with the ground truth
// (utils_tip_cache_and_union_finetune.py:376-409 with pocket's BoxPairAssociation, pocket/pocket/utils/association.py:17-116) for all
// classes of an image at once.  DESIGN.md §13 has the semantics and the measurements; tests/detections_bound.py restates every
// operation below in numpy and is expected bit for bit.
//
//   det_count_kernel   a wave per pair row: the columns with prior[0][p][c] * prior[1][p][c] != 0 (one fp32 multiply, NaN counts) by
//                      ballot and popcount over chunks of 64 columns; a workgroup takes 64 rows and leaves their sum
//   det_scan_kernel    one workgroup: exclusive prefix over the workgroup sums (256 at a time behind a carry), det_off[b] = the slot of
//                      row pair_off[b], status[b] = bit 2 where the image's entries end behind cap
//   det_write_kernel   the geometry of det_count_kernel: a row's first slot = its workgroup's prefix + the prefix of the rows before it
//                      in the workgroup; the row walks its columns again and writes its entries in column order
//   det_assoc_kernel   one workgroup per image, the ground-truth pairs (recovered boxes, areas, classes) and one 64-bit key per
//                      ground-truth pair in LDS: a thread per detection finds max_iou / max_idx over the pairs of its class, candidates
//                      bid for their ground-truth pair with an LDS atomicMax on (score order, inverted detection index), and the
//                      detection whose index the key holds gets label 1
//
// No slot is decided by the order in which anything arrives: slots come from the two-level prefix, and the maximum of a set of distinct
// keys is the same whatever the order of the atomics.  All arithmetic is fp32 on the VALU, one rounding per operation: this file is
// compiled with -ffp-contract=off (build.sh) - (x2 - x1) * (y2 - y1), cx - 0.5f * w and (area_g + area_d) - inter must not become fused
// multiply-adds.  Nothing here is bound by MFMA rate or by HBM bandwidth: the prior matrix is read twice and everything else is small.
#include <float.h>

#include "hg_kernels.h"

namespace hg {

static constexpr int DET_WAVE_ROWS = DET_ROWS / 4;      // rows per wave of a 256-thread workgroup

__device__ __forceinline__ bool det_finite(float v) { return fabsf(v) <= FLT_MAX; }
// torch.max / torch.min / clamp(min = 0) on elements: a NaN on either side comes out
__device__ __forceinline__ float det_max(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ float det_min(float a, float b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ float det_clamp0(float v) { return v < 0.f ? 0.f : v; }
// nonzero(prior[0] * prior[1]): the product is ONE multiply; NaN != 0
__device__ __forceinline__ bool det_set(float a, float b) {
    const float p = a * b;
    return !(p == 0.f);
}
__device__ __forceinline__ int det_wave_scan(int v, int lane) {      // inclusive
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(256) void det_count_kernel(const float* __restrict__ prior, int Pt, int NC, int32_t* __restrict__ cnt,
                                                        int32_t* __restrict__ bsum) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r0 = blockIdx.x * DET_ROWS + wave * DET_WAVE_ROWS;
    int wsum = 0;
    for (int i = 0; i < DET_WAVE_ROWS; ++i) {
        const int p = r0 + i;
        if (p >= Pt) break;
        const float* a = prior + (size_t)p * NC;
        const float* b = a + (size_t)Pt * NC;
        int n = 0;
        for (int c0 = 0; c0 < NC; c0 += 64) {
            const int c = c0 + lane;
            const bool nz = c < NC && det_set(a[c], b[c]);
            n += __popcll(__ballot(nz));
        }
        if (lane == 0) cnt[p] = n;
        wsum += n;
    }
    if (lane == 0) s_w[wave] = wsum;
    __syncthreads();
    if (tid == 0) bsum[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// bsum [nblk]: sums in, exclusive prefixes out.  det_off [B + 1], status [B] (the later kernels OR their bits into it).
__global__ __launch_bounds__(256) void det_scan_kernel(DetBatch db, int nblk, const int32_t* __restrict__ cnt, int32_t* __restrict__ bsum,
                                                       int cap, int32_t* __restrict__ det_off, int32_t* __restrict__ status) {
    __shared__ int s_part[4];
    __shared__ int s_off[DET_MAX_IMAGES + 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int carry = 0;
    for (int base = 0; base < nblk; base += 256) {
        const int i = base + tid;
        const int v = i < nblk ? bsum[i] : 0;
        const int x = det_wave_scan(v, lane);
        if (lane == 63) s_part[wave] = x;
        __syncthreads();
        int add = carry;
        for (int w = 0; w < wave; ++w) add += s_part[w];
        if (i < nblk) bsum[i] = add + x - v;
        carry += (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
        __syncthreads();
    }
    if (tid <= db.B) {
        const int p = db.pair_off[tid];
        int off = carry;
        if (p < db.Pt) {
            const int blk = p / DET_ROWS;
            off = bsum[blk];
            for (int q = blk * DET_ROWS; q < p; ++q) off += cnt[q];
        }
        det_off[tid] = off;
        s_off[tid] = off;
    }
    __syncthreads();
    if (tid < db.B && status) status[tid] = s_off[tid + 1] > cap ? 4 : 0;
}

__global__ __launch_bounds__(256) void det_write_kernel(DetBatch db, const float* __restrict__ prior, const float* __restrict__ scores,
                                                        const int32_t* __restrict__ pair_h, const int32_t* __restrict__ pair_o,
                                                        const int32_t* __restrict__ objects, const int32_t* __restrict__ conversion,
                                                        int n_obj, int NC, const int32_t* __restrict__ cnt, const int32_t* __restrict__ bsum,
                                                        int cap, DetEntries e, int32_t* __restrict__ status) {
    __shared__ int s_off[DET_ROWS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, Pt = db.Pt;
    if (tid < DET_ROWS) {      // (DET_ROWS == 64: wave 0)
        const int p = blockIdx.x * DET_ROWS + tid;
        const int v = p < Pt ? cnt[p] : 0;
        s_off[tid] = bsum[blockIdx.x] + det_wave_scan(v, lane) - v;
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int i = 0; i < DET_WAVE_ROWS; ++i) {
        const int r = wave * DET_WAVE_ROWS + i, p = blockIdx.x * DET_ROWS + r;
        if (p >= Pt) break;
        int b = 0;
        while (b + 1 < db.B && db.pair_off[b + 1] <= p) ++b;
        const int x = p - db.pair_off[b];
        const int h = pair_h[p], o = pair_o[p], obj = objects[p];
        const bool in_table = obj >= 0 && obj < n_obj;
        const float* pa = prior + (size_t)p * NC;
        const float* pb = pa + (size_t)Pt * NC;
        int slot0 = s_off[r];
        bool bad = false;
        for (int c0 = 0; c0 < NC; c0 += 64) {
            const int c = c0 + lane;
            const bool nz = c < NC && det_set(pa[c], pb[c]);
            const unsigned long long m = __ballot(nz);
            if (nz) {
                int inter = c;
                if (conversion) {
                    inter = in_table ? conversion[(size_t)obj * NC + c] : -1;
                    if (inter < 0) {
                        inter = -1;
                        bad = true;
                    }
                }
                const int slot = slot0 + __popcll(m & lt);
                if (slot < cap) {
                    if (e.pair) e.pair[slot] = x;
                    if (e.verb) e.verb[slot] = c;
                    if (e.h) e.h[slot] = h;
                    if (e.o) e.o[slot] = o;
                    if (e.object) e.object[slot] = obj;
                    if (e.score) e.score[slot] = scores[(size_t)p * NC + c];
                    if (e.interaction) e.interaction[slot] = inter;
                }
            }
            slot0 += __popcll(m);
        }
        if (bad && status) atomicOr(&status[b], 1);
    }
}

// The score's bits as an unsigned whose order is argmax's: NaN above every number, -0 == +0, otherwise the order of the reals.  Never 0.
__device__ __forceinline__ uint32_t det_score_key(float s) {
    if (s != s) return 0xFFFFFFFFu;
    if (s == 0.f) s = 0.f;
    const uint32_t u = (uint32_t)__float_as_int(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void det_assoc_kernel(DetBatch db, const float* __restrict__ boxes, const float* __restrict__ gt_h,
                                                        const float* __restrict__ gt_o, const int32_t* __restrict__ gt_hoi, int gt_format,
                                                        float min_iou, int cap, int Gt, const int32_t* __restrict__ det_off,
                                                        const int32_t* __restrict__ det_h, const int32_t* __restrict__ det_o,
                                                        const float* __restrict__ det_score, const int32_t* __restrict__ det_inter,
                                                        float* __restrict__ det_label, int32_t* __restrict__ det_gt,
                                                        float* __restrict__ det_max_iou, float* __restrict__ gt_out,
                                                        int32_t* __restrict__ status) {
    __shared__ float s_gh[DET_MAX_GT][4];
    __shared__ float s_go[DET_MAX_GT][4];
    __shared__ float s_ah[DET_MAX_GT], s_ao[DET_MAX_GT];
    __shared__ int s_hoi[DET_MAX_GT];
    __shared__ unsigned long long s_key[DET_MAX_GT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int g0 = db.gt_off[b], G = db.gt_off[b + 1] - g0;      // G <= DET_MAX_GT == the workgroup's threads (the host checks)
    if (tid < G) {
        const float wi = (float)db.img_w[b], hi = (float)db.img_h[b];
        bool bad = false;
        for (int k = 0; k < 2; ++k) {
            const float* src = (k ? gt_o : gt_h) + 4 * (size_t)(g0 + tid);
            float x1 = src[0], y1 = src[1], x2 = src[2], y2 = src[3];
            if (gt_format == 1) {      // recover_boxes: box_cxcywh_to_xyxy, then * (w, h, w, h)
                const float cx = x1, cy = y1, hw = 0.5f * x2, hh = 0.5f * y2;
                x1 = (cx - hw) * wi;
                y1 = (cy - hh) * hi;
                x2 = (cx + hw) * wi;
                y2 = (cy + hh) * hi;
            }
            bad |= !(det_finite(x1) && det_finite(y1) && det_finite(x2) && det_finite(y2));
            float* dst = k ? s_go[tid] : s_gh[tid];
            dst[0] = x1; dst[1] = y1; dst[2] = x2; dst[3] = y2;
            (k ? s_ao : s_ah)[tid] = (x2 - x1) * (y2 - y1);
            if (gt_out) {
                float* out = gt_out + 4 * ((size_t)k * Gt + g0 + tid);
                out[0] = x1; out[1] = y1; out[2] = x2; out[3] = y2;
            }
        }
        s_hoi[tid] = gt_hoi[g0 + tid];
        s_key[tid] = 0ull;
        if (bad && status) atomicOr(&status[b], 2);
    }
    __syncthreads();
    const int d0 = det_off[b], d1 = det_off[b + 1] < cap ? det_off[b + 1] : cap;
    const float* bx = boxes + 4 * (size_t)db.box_off[b];
    const uint32_t nbox = (uint32_t)(db.box_off[b + 1] - db.box_off[b]);
    for (int d = d0 + tid; d < d1; d += 256) {
        const int cls = det_inter[d];
        float best = 0.f;
        int bi = -1;
        if (cls >= 0 && (uint32_t)det_h[d] < nbox && (uint32_t)det_o[d] < nbox) {      // (an index outside the image's boxes reads nothing)
            const float* ph = bx + 4 * (size_t)det_h[d];
            const float* po = bx + 4 * (size_t)det_o[d];
            const float hx1 = ph[0], hy1 = ph[1], hx2 = ph[2], hy2 = ph[3], ox1 = po[0], oy1 = po[1], ox2 = po[2], oy2 = po[3];
            const float ah = (hx2 - hx1) * (hy2 - hy1), ao = (ox2 - ox1) * (oy2 - oy1);
            for (int g = 0; g < G; ++g) {
                if (s_hoi[g] != cls) continue;
                const float wh = det_clamp0(det_min(s_gh[g][2], hx2) - det_max(s_gh[g][0], hx1));
                const float hh = det_clamp0(det_min(s_gh[g][3], hy2) - det_max(s_gh[g][1], hy1));
                const float ih = wh * hh;
                const float iou_h = ih / ((s_ah[g] + ah) - ih);
                const float wo = det_clamp0(det_min(s_go[g][2], ox2) - det_max(s_go[g][0], ox1));
                const float ho = det_clamp0(det_min(s_go[g][3], oy2) - det_max(s_go[g][1], oy1));
                const float io = wo * ho;
                const float iou_o = io / ((s_ao[g] + ao) - io);
                const float iou = det_min(iou_h, iou_o);
                // iou.max(0): the first index of the maximum, and a NaN is the maximum from where it first appears
                if (bi < 0 || (best == best && (iou != iou || iou > best))) {
                    best = iou;
                    bi = g;
                }
            }
        }
        if (best != best) best = __int_as_float(0x7FC00000);      // one NaN pattern, whatever the division made
        det_gt[d] = bi;
        if (det_max_iou) det_max_iou[d] = best;
        if (bi >= 0 && best > min_iou)
            atomicMax(&s_key[bi], ((unsigned long long)det_score_key(det_score[d]) << 32) | (unsigned long long)(~(uint32_t)(d - d0)));
    }
    __syncthreads();
    if (det_label)
        for (int d = d0 + tid; d < d1; d += 256) {      // (the same thread wrote det_gt[d])
            const int bi = det_gt[d];
            det_label[d] = (bi >= 0 && (uint32_t)s_key[bi] == ~(uint32_t)(d - d0)) ? 1.f : 0.f;
        }
}

hipError_t launch_det_compact(const DetBatch& db, const float* prior, const float* scores, const int32_t* pair_h, const int32_t* pair_o,
                              const int32_t* objects, const int32_t* conversion, int n_obj, int NC, int cap, int32_t* cnt, int32_t* bsum,
                              int32_t* det_off, const DetEntries& e, int32_t* status, hipStream_t s) {
    const int nblk = (db.Pt + DET_ROWS - 1) / DET_ROWS;
    if (nblk > 0) {
        hipLaunchKernelGGL(det_count_kernel, dim3(nblk), dim3(256), 0, s, prior, db.Pt, NC, cnt, bsum);
        hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(det_scan_kernel, dim3(1), dim3(256), 0, s, db, nblk, cnt, bsum, cap, det_off, status);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess || nblk == 0) return rc;
    hipLaunchKernelGGL(det_write_kernel, dim3(nblk), dim3(256), 0, s, db, prior, scores, pair_h, pair_o, objects, conversion, n_obj, NC, cnt, bsum,
                       cap, e, status);
    return hipGetLastError();
}

hipError_t launch_det_assoc(const DetBatch& db, const float* boxes, const float* gt_h, const float* gt_o, const int32_t* gt_hoi, int gt_format,
                            float min_iou, int cap, int Gt, const int32_t* det_off, const DetEntries& e, float* det_label, int32_t* det_gt,
                            float* det_max_iou, float* gt_out, int32_t* status, hipStream_t s) {
    if (db.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(det_assoc_kernel, dim3(db.B), dim3(256), 0, s, db, boxes, gt_h, gt_o, gt_hoi, gt_format, min_iou, cap, Gt, det_off, e.h, e.o,
                       e.score, e.interaction, det_label, det_gt, det_max_iou, gt_out, status);
    return hipGetLastError();
}

}  // namespace hg
