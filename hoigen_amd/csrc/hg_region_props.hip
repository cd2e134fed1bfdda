// What sits between the detector and the encoders, for a whole batch: UPT.prepare_region_proposals (class-aware NMS + the instance
// selection, upt_tip_cache_model_free_finetune_distill3.py:1361-1406), get_prior with prior_type 'cbe' (:1445-1495) and priors_downproj =
// MLP(E + 5, hidden, 64, 3) (:40-52, :520).  DESIGN.md §12 has the semantics and the measurements; tests/props_bound.py restates every
// fp32 operation below in numpy and is expected bit for bit.
//
//   props_select_kernel   one workgroup per image: torchvision's coordinate-trick NMS in its own fp32 arithmetic, the stable order by
//                         counting, one suppression bit row per sorted box, the greedy walk by one wave, the selection rule
//   prior_pack_kernel     load time: a linear's [N, K] weight as [K, N] (lanes run along n everywhere below)
//   prior_table_kernel    load time and every update: T[c][n] = sum_k object_embedding[c][k] * W0[n][5 + k] - 512 of a prior row's 517
//                         columns depend on the label alone
//   prior_mlp_kernel      workgroup (image, 16 rows): the row, layer 0 five multiply-adds deep on top of T, layers 1 and 2
//
// All of it is fp32 on the VALU, one rounding per operation: this file is compiled with -ffp-contract=off (build.sh), as hg_hoi_head.hip
// is and for its reason.  Every sum runs over k ascending into ONE accumulator per (row, n), whatever the row's position, its row group
// or the batch around it.  No MFMA: 25 k multiply-adds per row, and the launch is bound by latency, not by arithmetic.
#include <float.h>

#include "hg_kernels.h"

namespace hg {

__device__ __forceinline__ bool props_finite(float v) { return fabsf(v) <= FLT_MAX; }
// (comparisons spelt out: a NaN behaves as in the restatement's np.where, whatever fmaxf would make of it)
__device__ __forceinline__ float props_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float props_min(float a, float b) { return a < b ? a : b; }

// Per image (Q <= PROPS_MAX_Q boxes, rows q_off[b] .. q_off[b + 1] - 1 of the inputs):
//   m = max over the 4 Q coordinates;  t = m + 1.0f;  off_i = (float)label_i * t;  every coordinate c + off_i;  area = (x2 - x1) * (y2 - y1)
//   rank_i = #{j : s_j > s_i or (s_j == s_i and j < i)}: the stable order by descending score
//   bit (i, j), j > i in that order:  w = max(min(x2) - max(x1), 0);  h likewise;  inter = w * h;  inter / ((area_i + area_j) - inter) > thr
//   greedy walk: a box still alive removes every later box whose bit it holds; a removed box removes nothing
//   selection over the survivors in order: h, o = humans / others with score >= box_score_thresh; of each kind the first
//   k = (count < min ? min(min, all of the kind) : count > max ? max : count); output = humans, then the others
// counts [B][4] = n, n_human, status, survivors.  status bit 0: a non-finite score or coordinate, bit 1: a label outside the prior
// table (n_classes > 0 only) - either leaves n = 0.  Slots n .. cap - 1: keep -1, box 0, score 0, label -1.
__global__ __launch_bounds__(256) void props_select_kernel(PropsBatch pb, PropsSelect ps, const float* __restrict__ scores,
                                                           const int32_t* __restrict__ labels, const float* __restrict__ boxes,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ keep,
                                                           float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                           int32_t* __restrict__ out_labels, int32_t* __restrict__ survivors) {
    __shared__ float s_sc[PROPS_MAX_Q];
    __shared__ int s_lb[PROPS_MAX_Q];
    __shared__ int s_ord[PROPS_MAX_Q];
    __shared__ float s_bx[PROPS_MAX_Q * 4];      // offset boxes in sorted order
    __shared__ float s_area[PROPS_MAX_Q];
    __shared__ uint32_t s_bits[PROPS_MAX_Q * PROPS_WORDS];
    __shared__ uint32_t s_rem[PROPS_WORDS];
    __shared__ float s_red[4];
    __shared__ int s_flag;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int q0 = pb.q_off[b], Q = pb.q_off[b + 1] - q0;
    const int W = (Q + 31) >> 5;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    float m = -FLT_MAX;
    int bad = 0;
    for (int i = tid; i < Q; i += 256) {
        const float s = scores[q0 + i];
        const int lb = labels[q0 + i];
        const float4 bx = *reinterpret_cast<const float4*>(boxes + 4 * (size_t)(q0 + i));
        if (!(props_finite(s) && props_finite(bx.x) && props_finite(bx.y) && props_finite(bx.z) && props_finite(bx.w))) bad |= 1;
        if (ps.n_classes > 0 && (lb < 0 || lb >= ps.n_classes)) bad |= 2;
        m = props_max(m, props_max(props_max(bx.x, bx.y), props_max(bx.z, bx.w)));
        s_sc[i] = s;
        s_lb[i] = lb;
    }
    if (bad) atomicOr(&s_flag, bad);
    for (int d = 32; d > 0; d >>= 1) m = props_max(m, __shfl_xor(m, d));
    if (lane == 0) s_red[tid >> 6] = m;
    __syncthreads();
    const float t = props_max(props_max(s_red[0], s_red[1]), props_max(s_red[2], s_red[3])) + 1.0f;
    const int flag = s_flag;
    for (int i = tid; i < Q; i += 256) {
        const float si = s_sc[i];
        int r = 0;
        for (int j = 0; j < Q; ++j) {
            const float sj = s_sc[j];
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        s_ord[r] = i;
    }
    __syncthreads();
    if (!flag) {      // (with a non-finite score the ranks above collide and s_ord has holes: nothing below reads it then)
        for (int r = tid; r < Q; r += 256) {
            const int i = s_ord[r];
            const float4 bx = *reinterpret_cast<const float4*>(boxes + 4 * (size_t)(q0 + i));
            const float off = (float)s_lb[i] * t;
            const float x1 = bx.x + off, y1 = bx.y + off, x2 = bx.z + off, y2 = bx.w + off;
            s_bx[4 * r] = x1;
            s_bx[4 * r + 1] = y1;
            s_bx[4 * r + 2] = x2;
            s_bx[4 * r + 3] = y2;
            s_area[r] = (x2 - x1) * (y2 - y1);
        }
    }
    __syncthreads();
    if (!flag) {
        for (int it = tid; it < Q * W; it += 256) {
            const int i = it / W, w = it - i * W;
            uint32_t bits = 0;
            if (32 * w + 31 > i) {
                const float ix1 = s_bx[4 * i], iy1 = s_bx[4 * i + 1], ix2 = s_bx[4 * i + 2], iy2 = s_bx[4 * i + 3], ia = s_area[i];
                for (int jj = 0; jj < 32; ++jj) {
                    const int j = 32 * w + jj;
                    if (j <= i || j >= Q) continue;
                    const float dx = props_min(ix2, s_bx[4 * j + 2]) - props_max(ix1, s_bx[4 * j]);
                    const float dy = props_min(iy2, s_bx[4 * j + 3]) - props_max(iy1, s_bx[4 * j + 1]);
                    const float inter = (dx > 0.f ? dx : 0.f) * (dy > 0.f ? dy : 0.f);
                    const float iou = inter / ((ia + s_area[j]) - inter);
                    if (iou > ps.nms_thr) bits |= 1u << jj;
                }
            }
            s_bits[i * PROPS_WORDS + w] = bits;
        }
    }
    __syncthreads();
    if (tid < 64) {      // the greedy walk: lane l holds word l of the removed set
        uint32_t removed = 0;
        if (!flag)
            for (int i = 0; i < Q; ++i) {
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)removed, i >> 5);
                if (!((r >> (i & 31)) & 1u)) removed |= lane < W ? s_bits[i * PROPS_WORDS + lane] : 0u;
            }
        if (lane < PROPS_WORDS) s_rem[lane] = removed;
    }
    __syncthreads();
    if (tid >= 64) return;
    int n_surv = 0, h_pre = 0, o_pre = 0, h_all = 0, o_all = 0;
    if (!flag)
        for (int c = 0; c < Q; c += 64) {
            const int r = c + lane;
            const bool in = r < Q;
            const bool alive = in && !((s_rem[in ? r >> 5 : 0] >> (r & 31)) & 1u);
            const int i = in ? s_ord[r] : 0;
            const bool hum = s_lb[i] == ps.human_idx, pre = s_sc[i] >= ps.score_thr;
            n_surv += __popcll(__ballot(alive));
            h_all += __popcll(__ballot(alive && hum));
            o_all += __popcll(__ballot(alive && !hum));
            h_pre += __popcll(__ballot(alive && hum && pre));
            o_pre += __popcll(__ballot(alive && !hum && pre));
        }
    const int kh = h_pre < ps.min_inst ? (ps.min_inst < h_all ? ps.min_inst : h_all) : (h_pre > ps.max_inst ? ps.max_inst : h_pre);
    const int ko = o_pre < ps.min_inst ? (ps.min_inst < o_all ? ps.min_inst : o_all) : (o_pre > ps.max_inst ? ps.max_inst : o_pre);
    const int n = kh + ko;      // <= 2 max_inst = cap (min_inst <= max_inst: the host checks)
    const size_t ob = (size_t)b * ps.cap;
    if (!flag) {
        const unsigned long long lt = (1ull << lane) - 1ull;
        int a_base = 0, h_base = 0, o_base = 0;
        for (int c = 0; c < Q; c += 64) {
            const int r = c + lane;
            const bool in = r < Q;
            const bool alive = in && !((s_rem[in ? r >> 5 : 0] >> (r & 31)) & 1u);
            const int i = in ? s_ord[r] : 0;
            const bool hum = s_lb[i] == ps.human_idx;
            const unsigned long long mA = __ballot(alive), mH = __ballot(alive && hum), mO = __ballot(alive && !hum);
            int slot = -1;
            if (alive) {
                if (survivors) survivors[q0 + a_base + __popcll(mA & lt)] = i;
                if (hum) {
                    const int k = h_base + __popcll(mH & lt);
                    if (k < kh) slot = k;
                } else {
                    const int k = o_base + __popcll(mO & lt);
                    if (k < ko) slot = kh + k;
                }
            }
            if (slot >= 0) {
                keep[ob + slot] = i;
                *reinterpret_cast<float4*>(out_boxes + 4 * (ob + slot)) = *reinterpret_cast<const float4*>(boxes + 4 * (size_t)(q0 + i));
                out_scores[ob + slot] = s_sc[i];
                out_labels[ob + slot] = s_lb[i];
            }
            a_base += __popcll(mA);
            h_base += __popcll(mH);
            o_base += __popcll(mO);
        }
    }
    if (lane >= n && lane < ps.cap) {      // (cap <= 64: one lane per slot)
        keep[ob + lane] = -1;
        *reinterpret_cast<float4*>(out_boxes + 4 * (ob + lane)) = make_float4(0.f, 0.f, 0.f, 0.f);
        out_scores[ob + lane] = 0.f;
        out_labels[ob + lane] = -1;
    }
    if (lane < 4) counts[4 * b + lane] = lane == 0 ? n : lane == 1 ? kh : lane == 2 ? flag : n_surv;
}

// out [K][N] = in [N][K]
__global__ __launch_bounds__(256) void prior_pack_kernel(const float* __restrict__ in, int N, int K, float* __restrict__ out) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)N * K) return;
    const int k = (int)(at / N), n = (int)(at - (size_t)k * N);
    out[at] = in[(size_t)n * K + k];
}

// One workgroup per class, lane along n:  acc = 0;  for k = 0 .. E - 1:  acc = acc + emb[c][k] * W0[n][5 + k]   (w0t = W0 as [5 + E][hid])
__global__ __launch_bounds__(256) void prior_table_kernel(const float* __restrict__ emb, const float* __restrict__ w0t, int E, int hid,
                                                          float* __restrict__ T) {
    const int c = blockIdx.x, n = threadIdx.x;
    if (n >= hid) return;
    const float* e = emb + (size_t)c * E;
    const float* w = w0t + (size_t)5 * hid + n;
    float acc = 0.f;
    for (int k = 0; k < E; ++k) acc = acc + e[k] * w[(size_t)k * hid];
    T[(size_t)c * hid + n] = acc;
}

__device__ __forceinline__ float props_relu(float v) { return v < 0.f ? 0.f : v; }

// Workgroup (image b, rows r0 .. r0 + 15 of its cap), 256 threads, lanes along n; a row's activations sit in LDS and reach the lanes as
// broadcast reads, a weight is read once per workgroup (coalesced along n from the [K][N] copies) and used for the 16 rows from a
// register - there is no second use that staging it in LDS would serve.
//   row i < n_b:  x = (score, x1 / w, y1 / h, x2 / w, y2 / h), t = T[label];   row i >= n_b: x = 0, t = 0 (the MLP of a zero row)
//   layer 0:  relu(((((t[n] + b0[n]) + x0 * W0[n][0]) + x1 * W0[n][1]) + x2 * W0[n][2]) + x3 * W0[n][3]) + x4 * W0[n][4])
//   layer 1:  acc = b1[n];  for k = 0 .. hid - 1:  acc = acc + h0[k] * W1[n][k];  relu
//   layer 2:  acc = b2[n];  for k = 0 .. hid - 1:  acc = acc + h1[k] * W2[n][k]
__global__ __launch_bounds__(256) void prior_mlp_kernel(PropsBatch pb, PriorDev pw, int cap, const int32_t* __restrict__ counts,
                                                        const float* __restrict__ sel_boxes, const float* __restrict__ sel_scores,
                                                        const int32_t* __restrict__ sel_labels, float* __restrict__ priors,
                                                        uint8_t* __restrict__ mask) {
    __shared__ float s_x[PRIOR_ROWS][8];
    __shared__ int s_lab[PRIOR_ROWS];
    __shared__ float s_h0[PRIOR_ROWS][PROPS_MAX_HID];
    __shared__ float s_h1[PRIOR_ROWS][PROPS_MAX_HID];
    const int b = blockIdx.x, r0 = blockIdx.y * PRIOR_ROWS, tid = threadIdx.x, hid = pw.hid;
    const int n_b = counts[4 * b];
    if (tid < PRIOR_ROWS) {
        const int r = r0 + tid;
        const bool valid = r < cap && r < n_b;
        float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f, x4 = 0.f;
        int lab = -1;
        if (valid) {
            const size_t at = (size_t)b * cap + r;
            const float4 bx = *reinterpret_cast<const float4*>(sel_boxes + 4 * at);
            const float h = pb.img_h[b], w = pb.img_w[b];
            x0 = sel_scores[at];
            x1 = bx.x / w;
            x2 = bx.y / h;
            x3 = bx.z / w;
            x4 = bx.w / h;
            lab = sel_labels[at];
        }
        s_x[tid][0] = x0; s_x[tid][1] = x1; s_x[tid][2] = x2; s_x[tid][3] = x3; s_x[tid][4] = x4;
        s_lab[tid] = lab;
        if (r < cap) mask[(size_t)b * cap + r] = r >= n_b ? 1 : 0;
    }
    __syncthreads();
    if (tid < hid) {
        const int n = tid;
        const float b0 = pw.b0[n];
        const float w0 = pw.w0t[n], w1 = pw.w0t[hid + n], w2 = pw.w0t[2 * hid + n], w3 = pw.w0t[3 * hid + n], w4 = pw.w0t[4 * hid + n];
        for (int r = 0; r < PRIOR_ROWS; ++r) {
            const int lab = s_lab[r];
            const float t = lab >= 0 ? pw.T[(size_t)lab * hid + n] : 0.f;
            float v = t + b0;
            v = v + s_x[r][0] * w0;
            v = v + s_x[r][1] * w1;
            v = v + s_x[r][2] * w2;
            v = v + s_x[r][3] * w3;
            v = v + s_x[r][4] * w4;
            s_h0[r][n] = props_relu(v);
        }
    }
    __syncthreads();
    if (tid < hid) {
        const int n = tid;
        float acc[PRIOR_ROWS];
        const float b1 = pw.b1[n];
#pragma unroll
        for (int r = 0; r < PRIOR_ROWS; ++r) acc[r] = b1;
        const float* w = pw.w1t + n;
#pragma unroll 4
        for (int k = 0; k < hid; ++k) {
            const float wk = w[(size_t)k * hid];
#pragma unroll
            for (int r = 0; r < PRIOR_ROWS; ++r) acc[r] = acc[r] + s_h0[r][k] * wk;
        }
#pragma unroll
        for (int r = 0; r < PRIOR_ROWS; ++r) s_h1[r][n] = props_relu(acc[r]);
    }
    __syncthreads();
    {
        const int n = tid & 63, g = tid >> 6;      // four rows a wave
        constexpr int RW = PRIOR_ROWS / 4;
        float acc[RW];
        const float b2 = pw.b2[n];
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[r] = b2;
        const float* w = pw.w2t + n;
#pragma unroll 4
        for (int k = 0; k < hid; ++k) {
            const float wk = w[(size_t)k * PROPS_OUT];
#pragma unroll
            for (int r = 0; r < RW; ++r) acc[r] = acc[r] + s_h1[g * RW + r][k] * wk;
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int row = r0 + g * RW + r;
            if (row < cap) priors[((size_t)b * cap + row) * PROPS_OUT + n] = acc[r];
        }
    }
}

hipError_t launch_props_select(const PropsBatch& pb, const PropsSelect& ps, const float* scores, const int32_t* labels, const float* boxes,
                               int32_t* counts, int32_t* keep, float* out_boxes, float* out_scores, int32_t* out_labels,
                               int32_t* survivors, hipStream_t s) {
    if (pb.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(props_select_kernel, dim3(pb.B), dim3(256), 0, s, pb, ps, scores, labels, boxes, counts, keep, out_boxes, out_scores,
                       out_labels, survivors);
    return hipGetLastError();
}

hipError_t launch_prior_pack(const float* in, int N, int K, float* out, hipStream_t s) {
    const size_t n = (size_t)N * K;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(prior_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, N, K, out);
    return hipGetLastError();
}

hipError_t launch_prior_table(const float* emb, const float* w0t, int n_classes, int E, int hid, float* T, hipStream_t s) {
    if (n_classes <= 0) return hipSuccess;
    hipLaunchKernelGGL(prior_table_kernel, dim3(n_classes), dim3(256), 0, s, emb, w0t, E, hid, T);
    return hipGetLastError();
}

hipError_t launch_prior_mlp(const PropsBatch& pb, const PriorDev& pw, int cap, const int32_t* counts, const float* sel_boxes,
                            const float* sel_scores, const int32_t* sel_labels, float* priors, uint8_t* mask, hipStream_t s) {
    if (pb.B <= 0 || cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(prior_mlp_kernel, dim3(pb.B, (cap + PRIOR_ROWS - 1) / PRIOR_ROWS), dim3(256), 0, s, pb, pw, cap, counts, sel_boxes,
                       sel_scores, sel_labels, priors, mask);
    return hipGetLastError();
}

}  // namespace hg
