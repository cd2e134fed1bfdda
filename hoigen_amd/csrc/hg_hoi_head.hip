// The interaction head behind the towers (UPT.compute_roi_embeddings + compute_prior_scores + the score of postprocessing,
// upt_tip_cache_model_free_finetune_distill3.py:959-1268, :806-833, :1408-1427) for a whole batch: four kernels around the branch GEMMs
// that hg_heads.hip issues.  DESIGN.md §11 has the structure and the measurements; tests/hoi_head_bound.py restates every fp32
// operation below in numpy and is expected bit for bit.
//
//   1. hoi_setup_kernel    pair indices, objects, union boxes; per RoI (all boxes, then all union boxes) and per axis the separable
//                          weight vector of the P x P x grid samples of an aligned RoI, the grid count and the support range
//   2. hoi_pool_kernel     mean of the P x P aligned RoI bins = wy^T F_c wx / (count P^2) against a channel chunk of one image's map
//                          staged in LDS, over the RoI's support only
//   3. hoi_feats_kernel    human | object | union (| global) rows L2-normalised: the fp16 A operands of the branch GEMMs and,
//                          optionally, the fp32 rows
//   4. hoi_epilogue_kernel logits = sum_b scale_b branch_b (left to right; a per-image branch read at the pair's image), priors, sigmoid, scores
//
// RoI table, HOI_TAB = 72 words per RoI:  0..31 wy   32..63 wx   64 gy (float; NaN = refused)  65 ylo  66 yhi   67 gx  68 xlo  69 xhi
//
// This file is compiled with -ffp-contract=off (build.sh), as hg_preproc.hip is and for its reason: the coordinates are
// roi_align_kernel's expressions with one rounding per operation, and the contraction is a documented chain of separately rounded
// multiplies and adds.  The one fused operation, the sum of squares of hoi_feats_kernel, is written as fmaf because
// l2_normalize_kernel (hg_elem.hip, compiled with contraction on) has it fused and the rows are held to that kernel bit for bit.
#include <algorithm>

#include "hg_kernels.h"

namespace hg {

// pair p of the batch -> image b, human x, object y (local box indices): pairs of an image are all (x, y), x < n_h, y != x, row-major
// (upt...:1007-1012)
__device__ __forceinline__ void hoi_pair(const HoiBatch& hb, int p, int& b, int& x, int& y) {
    b = 0;
    while (b + 1 < hb.B && hb.pair_off[b + 1] <= p) ++b;
    const int q = p - hb.pair_off[b], n1 = hb.box_off[b + 1] - hb.box_off[b] - 1;
    x = q / n1;
    const int j = q - x * n1;
    y = j < x ? j : j + 1;
}

// torch.min / torch.max of two floats (a NaN wins)
__device__ __forceinline__ float hoi_min(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ float hoi_max(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// One thread per (RoI, axis), axis 0 = y; its 32 weights live in LDS (stride 33) while the samples are walked.
// Operation order of one axis (b1, b2 the box's low and high corner on it, `size` = H or W):
//     s = b1 * scale - 0.5;  e = b2 * scale - 0.5;  r = e - s;  bin = r / P;  g = ceil(r / P)
//     for ph in 0..P-1, i in 0..g-1 (in this order):  y = s + ph * bin + (i + 0.5) * bin / g        roi_align_kernel's expression
//         skipped outside [-1, size]; clamped as roi_align_kernel does;  ly = y - yl;  hy = 1 - ly
//         w[yl] = w[yl] + hy;   then   w[yh] = w[yh] + ly
// support = [smallest yl, largest yh] touched.  A RoI with g beyond HOI_MAX_GRID on an axis (more than 65 536 samples per bin: a box
// hundreds of thousands of cells wide, or a non-finite corner) is refused: g = NaN, and the pooled row is NaN.
__global__ __launch_bounds__(64) void hoi_setup_kernel(HoiBatch hb, const float* __restrict__ boxes, const int32_t* __restrict__ labels,
                                                       float scale, int P, int H, int W, int32_t* __restrict__ pair_h,
                                                       int32_t* __restrict__ pair_o, int32_t* __restrict__ objects,
                                                       float* __restrict__ union_boxes, float* __restrict__ tab) {
    __shared__ float wsh[64 * 33];
    const int t = blockIdx.x * 64 + threadIdx.x;
    const int roi = t >> 1, axis = t & 1;
    if (roi >= hb.N + hb.Pt) return;
    float b1, b2;
    if (roi < hb.N) {
        b1 = boxes[4 * (size_t)roi + 1 - axis];
        b2 = boxes[4 * (size_t)roi + 3 - axis];
    } else {
        const int p = roi - hb.N;
        int b, x, y;
        hoi_pair(hb, p, b, x, y);
        const float* bh = boxes + 4 * (size_t)(hb.box_off[b] + x);
        const float* bo = boxes + 4 * (size_t)(hb.box_off[b] + y);
        const float u0 = hoi_min(bh[0], bo[0]), u1 = hoi_min(bh[1], bo[1]), u2 = hoi_max(bh[2], bo[2]), u3 = hoi_max(bh[3], bo[3]);
        b1 = axis ? u0 : u1;
        b2 = axis ? u2 : u3;
        if (axis == 0) {
            if (pair_h) pair_h[p] = x;
            if (pair_o) pair_o[p] = y;
            if (objects) objects[p] = labels[hb.box_off[b] + y];
            if (union_boxes) {
                union_boxes[4 * (size_t)p] = u0;
                union_boxes[4 * (size_t)p + 1] = u1;
                union_boxes[4 * (size_t)p + 2] = u2;
                union_boxes[4 * (size_t)p + 3] = u3;
            }
        }
    }
    const int size = axis ? W : H;
    const float s1 = b1 * scale - 0.5f, e1 = b2 * scale - 0.5f;
    const float r = e1 - s1;
    const float bin = r / (float)P;
    float gf = ceilf(r / (float)P);
    const bool refused = !(gf <= (float)HOI_MAX_GRID);
    const int g = refused ? 0 : (int)gf;
    if (refused) gf = __builtin_nanf("");
    float* w = wsh + threadIdx.x * 33;
    for (int i = 0; i < HOI_MAX_SIDE; ++i) w[i] = 0.f;
    int lo = size, hi = -1;
    for (int ph = 0; ph < P; ++ph)
        for (int i = 0; i < g; ++i) {
            float y = s1 + (float)ph * bin + ((float)i + 0.5f) * bin / (float)g;
            if (y < -1.0f || y > (float)size) continue;
            if (y <= 0.f) y = 0.f;
            int yl = (int)y, yh;
            if (yl >= size - 1) { yh = yl = size - 1; y = (float)yl; } else yh = yl + 1;
            const float ly = y - (float)yl, hy = 1.f - ly;
            w[yl] = w[yl] + hy;
            w[yh] = w[yh] + ly;
            lo = yl < lo ? yl : lo;
            hi = yh > hi ? yh : hi;
        }
    if (hi < 0) lo = 0;
    float* out = tab + (size_t)roi * HOI_TAB;
    for (int i = 0; i < HOI_MAX_SIDE; ++i) out[32 * axis + i] = w[i];
    out[64 + 3 * axis] = gf;
    out[65 + 3 * axis] = __int_as_float(lo);
    out[66 + 3 * axis] = __int_as_float(hi);
}

// Workgroup (RoI slice, channel chunk, image): the chunk's cn <= CC channels of the image's [C, H, W] map go to LDS with coalesced
// loads, channel c at word c * stride, stride = H W | 1 (odd: the 32 lanes of a ds_read_b32 group hit 32 banks).  A wave takes one
// RoI at a time and a lane one channel; the RoI's 64 weights sit in one register across the wave (lane l: wy[l], lane 32 + l: wx[l])
// and reach every lane through v_readlane.  fp32 VALU, one accumulator per (RoI, channel), in this order:
//     acc = 0;  for y = ylo .. yhi:  for x = xlo .. xhi:   acc = acc + (wy[y] * wx[x]) * f[y][x]             three roundings a tap
//     mean = acc / (max(gy * gx, 1) * (float)(P * P))
// A channel chunk never splits this sum, so the result does not depend on CC, on the slice count or on the batch around the image.
static constexpr int HOI_POOL_WAVES = 8;      // 512 threads: at 24 x 24 the chunk admits one workgroup a CU, and a wave's taps are a dependent chain
__global__ __launch_bounds__(64 * HOI_POOL_WAVES) void hoi_pool_kernel(HoiBatch hb, const float* __restrict__ feat, int C, int H, int W, int CC, int P,
                                                       const float* __restrict__ tab, float* __restrict__ pooled_single,
                                                       float* __restrict__ pooled_union) {
    extern __shared__ float hoi_lds[];
    const int b = blockIdx.z, c0 = blockIdx.y * CC, sl = blockIdx.x, n_slice = gridDim.x;
    const int n = hb.box_off[b + 1] - hb.box_off[b], nr = n + hb.pair_off[b + 1] - hb.pair_off[b];
    if (sl * HOI_POOL_WAVES >= nr) return;      // (the whole workgroup)
    const int HW = H * W, stride = HW | 1;
    const int cn = C - c0 < CC ? C - c0 : CC;
    const float* src = feat + ((size_t)b * C + c0) * HW;
    for (int i = threadIdx.x; i < cn * HW; i += 64 * HOI_POOL_WAVES) {
        const int ch = i / HW;
        hoi_lds[ch * stride + (i - ch * HW)] = src[i];
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float* f = hoi_lds + (lane < cn ? lane : 0) * stride;
    for (int r = sl * HOI_POOL_WAVES + wave; r < nr; r += HOI_POOL_WAVES * n_slice) {
        const bool single = r < n;
        const size_t row = single ? (size_t)(hb.box_off[b] + r) : (size_t)(hb.pair_off[b] + (r - n));
        const float* t = tab + (single ? row : hb.N + row) * HOI_TAB;
        const int wv = __float_as_int(t[lane]);
        const float gy = t[64], gx = t[67];
        const int ylo = __builtin_amdgcn_readfirstlane(__float_as_int(t[65])), yhi = __builtin_amdgcn_readfirstlane(__float_as_int(t[66]));
        const int xlo = __builtin_amdgcn_readfirstlane(__float_as_int(t[68])), xhi = __builtin_amdgcn_readfirstlane(__float_as_int(t[69]));
        float acc = 0.f;
        for (int y = ylo; y <= yhi; ++y) {
            const float wy = __int_as_float(__builtin_amdgcn_readlane(wv, y));
            const float* fr = f + y * W;
            int x = xlo;
            for (; x + 3 <= xhi; x += 4) {      // four taps' loads in flight at once; the additions keep their order
                const float f0 = fr[x], f1 = fr[x + 1], f2 = fr[x + 2], f3 = fr[x + 3];
                const float w0 = wy * __int_as_float(__builtin_amdgcn_readlane(wv, 32 + x));
                const float w1 = wy * __int_as_float(__builtin_amdgcn_readlane(wv, 33 + x));
                const float w2 = wy * __int_as_float(__builtin_amdgcn_readlane(wv, 34 + x));
                const float w3 = wy * __int_as_float(__builtin_amdgcn_readlane(wv, 35 + x));
                acc = acc + w0 * f0;
                acc = acc + w1 * f1;
                acc = acc + w2 * f2;
                acc = acc + w3 * f3;
            }
            for (; x <= xhi; ++x) acc = acc + (wy * __int_as_float(__builtin_amdgcn_readlane(wv, 32 + x))) * fr[x];
        }
        float cnt = gy * gx;
        cnt = cnt < 1.f ? 1.f : cnt;      // (NaN stays NaN)
        const float mean = acc / (cnt * (float)(P * P));
        if (lane < cn) (single ? pooled_single : pooled_union)[row * C + c0 + lane] = mean;
    }
}

// One wave per (pair, segment), segments human, object, union and - with g16 - global.  x / ||x||_2 in l2_normalize_kernel's
// arithmetic (hg_elem.hip): lane l sums v * v over d = l, l + 64, .. fused, wave_sum, 1 / sqrtf, one multiply per element.
__global__ __launch_bounds__(256) void hoi_feats_kernel(HoiBatch hb, const float* __restrict__ pooled_single,
                                                        const float* __restrict__ pooled_union, const float* __restrict__ feat_global,
                                                        int C, int n_seg, float* __restrict__ feats, half_t* __restrict__ ho16,
                                                        half_t* __restrict__ u16, half_t* __restrict__ g16) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= hb.Pt * n_seg) return;
    const int p = item / n_seg, seg = item - p * n_seg;
    int b, x, y;
    hoi_pair(hb, p, b, x, y);
    const float* src = seg == 0 ? pooled_single + (size_t)(hb.box_off[b] + x) * C
                     : seg == 1 ? pooled_single + (size_t)(hb.box_off[b] + y) * C
                     : seg == 2 ? pooled_union + (size_t)p * C : feat_global + (size_t)b * C;
    float q = 0.f;
    for (int d = lane; d < C; d += 64) {
        const float v = src[d];
        q = __builtin_fmaf(v, v, q);
    }
    const float inv = 1.0f / sqrtf(wave_sum(q));
    float* o32 = feats && seg < 3 ? feats + ((size_t)p * 3 + seg) * C : nullptr;
    half_t* base16 = seg < 2 ? ho16 : (seg == 2 ? u16 : g16);      // (all null in a call without branches)
    half_t* o16 = !base16 ? nullptr : seg < 2 ? base16 + ((size_t)p * 2 + seg) * C : base16 + (size_t)p * C;
    for (int d = lane; d < C; d += 64) {
        const float v = src[d] * inv;
        if (o32) o32[d] = v;
        if (o16) o16[d] = (half_t)v;
    }
}

// One workgroup per pair.  logits = branch_0 * scale_0 + branch_1 * scale_1 + .., every product rounded, summed left to right
// (upt...:1195-1196, and :1205-1207 with the DINO row); a per-image branch (HG_HOI_SRC_IMAGE) holds one row per image and is read at row
// b(p) instead of row p - the reference's dino_logits[i] broadcast over the image's pairs (:1184-1207); prior[0] = scores[x]^p and prior[1] = scores[y]^p on the columns obj2target[labels[y]] sets (:806-833; p == 1
// leaves the score as it is, as torch's pow does; any other p goes through double); score = sigmoid(logits) * (prior[0] * prior[1]) (:1417-1423).
__global__ __launch_bounds__(128) void hoi_epilogue_kernel(HoiBatch hb, HoiEpilogue e, const float* __restrict__ scores,
                                                           const int32_t* __restrict__ labels, const uint8_t* __restrict__ obj2target,
                                                           int n_obj, int NC, float score_pow, float* __restrict__ logits,
                                                           float* __restrict__ prior, float* __restrict__ out_scores) {
    const int p = blockIdx.x;
    int b, x, y;
    hoi_pair(hb, p, b, x, y);
    const bool want_prior = prior || out_scores;
    float sh = 0.f, so = 0.f;
    int lab = -1;
    __shared__ float pw[2];
    if (want_prior) {      // (the same for the whole workgroup)
        sh = scores[hb.box_off[b] + x];
        so = scores[hb.box_off[b] + y];
        lab = labels[hb.box_off[b] + y];
        // in double, rounded once: the result is the correctly rounded power up to the double routine's own error, 2^-29 of an fp32 ulp
        // per ulp of it - a bound from the formats, not from a single-precision routine's accuracy (tests/hoi_head_bound.py).  Two
        // threads of the workgroup raise the two scores, the others read the results.
        if (score_pow != 1.0f) {
            if (threadIdx.x < 2) pw[threadIdx.x] = (float)pow((double)(threadIdx.x ? so : sh), (double)score_pow);
            __syncthreads();
            sh = pw[0];
            so = pw[1];
        }
    }
    const bool known = lab >= 0 && lab < n_obj;
    for (int k = threadIdx.x; k < NC; k += 128) {
        const size_t at = (size_t)p * NC + k;
        float acc = 0.f;
        for (int i = 0; i < e.n; ++i) {
            const float v = e.per_image[i] ? e.branch[i][(size_t)b * NC + k] : e.branch[i][at];
            if (e.per_image[i] && e.slab[i]) e.slab[i][at] = v;
            const float t = v * e.scale[i];
            acc = i == 0 ? t : acc + t;
        }
        if (logits) logits[at] = acc;
        if (want_prior) {
            const bool on = known && obj2target[(size_t)lab * NC + k] != 0;
            const float ph = on ? sh : 0.f, po = on ? so : 0.f;
            if (prior) {
                prior[at] = ph;
                prior[(size_t)hb.Pt * NC + at] = po;
            }
            if (out_scores) out_scores[at] = (1.0f / (1.0f + expf(-acc))) * (ph * po);
        }
    }
}

int hoi_pool_chunk(int H, int W) { return (size_t)64 * ((H * W) | 1) * 4 <= HOI_LDS_MAX ? 64 : 32; }

hipError_t launch_hoi_setup(const HoiBatch& hb, const float* boxes, const int32_t* labels, float scale, int P, int H, int W,
                            int32_t* pair_h, int32_t* pair_o, int32_t* objects, float* union_boxes, float* tab, hipStream_t s) {
    const int n = 2 * (hb.N + hb.Pt);
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(hoi_setup_kernel, dim3((n + 63) / 64), dim3(64), 0, s, hb, boxes, labels, scale, P, H, W, pair_h, pair_o, objects,
                       union_boxes, tab);
    return hipGetLastError();
}

hipError_t launch_hoi_pool(const HoiBatch& hb, const float* feat, int C, int H, int W, int P, const float* tab, float* pooled_single,
                           float* pooled_union, int n_cu, hipStream_t s) {
    if (hb.N + hb.Pt <= 0) return hipSuccess;
    static bool attr_set_d[HG_MAX_DEVICES] = {};
    bool& attr_set = attr_set_d[current_device_index()];
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hoi_pool_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)HOI_LDS_MAX);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    const int CC = hoi_pool_chunk(H, W);
    const size_t lds = (size_t)CC * ((H * W) | 1) * 4;
    const int n_chunk = (C + CC - 1) / CC;
    int max_nr = 0;
    for (int b = 0; b < hb.B; ++b) {
        const int nr = hb.box_off[b + 1] - hb.box_off[b] + hb.pair_off[b + 1] - hb.pair_off[b];
        max_nr = nr > max_nr ? nr : max_nr;
    }
    // RoI slices: enough workgroups for every CU to hold as many as its LDS admits (at most 4), never fewer than one RoI a wave each
    const int per_cu = (int)std::min<size_t>(4, HOI_LDS_MAX / lds);
    int n_slice = (n_cu * per_cu + hb.B * n_chunk - 1) / (hb.B * n_chunk);
    n_slice = std::max(1, std::min(n_slice, (max_nr + HOI_POOL_WAVES - 1) / HOI_POOL_WAVES));
    hipLaunchKernelGGL(hoi_pool_kernel, dim3(n_slice, n_chunk, hb.B), dim3(64 * HOI_POOL_WAVES), lds, s, hb, feat, C, H, W, CC, P, tab, pooled_single,
                       pooled_union);
    return hipGetLastError();
}

hipError_t launch_hoi_feats(const HoiBatch& hb, const float* pooled_single, const float* pooled_union, const float* feat_global, int C,
                            float* feats, half_t* ho16, half_t* u16, half_t* g16, hipStream_t s) {
    if (hb.Pt <= 0) return hipSuccess;
    const int n_seg = g16 ? 4 : 3;
    hipLaunchKernelGGL(hoi_feats_kernel, dim3((hb.Pt * n_seg + 3) / 4), dim3(256), 0, s, hb, pooled_single, pooled_union, feat_global, C,
                       n_seg, feats, ho16, u16, g16);
    return hipGetLastError();
}

hipError_t launch_hoi_epilogue(const HoiBatch& hb, const HoiEpilogue& e, const float* scores, const int32_t* labels,
                               const uint8_t* obj2target, int n_obj, int NC, float score_pow, float* logits, float* prior,
                               float* out_scores, hipStream_t s) {
    if (hb.Pt <= 0) return hipSuccess;
    hipLaunchKernelGGL(hoi_epilogue_kernel, dim3(hb.Pt), dim3(128), 0, s, hb, e, scores, labels, obj2target, n_obj, NC, score_pow, logits,
                       prior, out_scores);
    return hipGetLastError();
}

}  // namespace hg
