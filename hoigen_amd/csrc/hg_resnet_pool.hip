// Global average pool + L2 normalisation behind a ResNet's last block (torchvision's avgpool + flatten with fc = Identity, then
// x / x.norm(dim=-1, keepdim=True): upt_tip_cache_model_free_finetune_distill3.py:1617-1618) on the fp32 NHWC stream [B, HW, C] as
// resnet_run_blocks leaves it in the workspace: the channel is the fastest index, so the lanes of a wave read consecutive words, and no
// NCHW copy of the map is made.
//
// One workgroup of RESNET_POOL_THREADS threads per image; thread t owns the channels t, t + RESNET_POOL_THREADS, .. (at most
// RESNET_MAX_C / RESNET_POOL_THREADS = 8 of them, in registers).  Arithmetic (tests/dino_bound.py restates it):
//     per (image, channel):  acc = 0;  for p = 0 .. HW - 1:  acc = acc + x[b][p][c];   pooled = acc / (float)HW        adds only: nothing
//                            to contract, so the sum is the same under any -ffp-contract
//     per image:             q = sum_c pooled^2 (per thread fused, then the 64 lanes by xor butterfly, then the waves in order);
//                            inv = 1 / sqrtf(q);  features = pooled * inv
// A zero row gives 0 * Inf = NaN, as the reference's 0 / 0 does.  An image's rows depend on that image alone.
#include "hg_kernels.h"

namespace hg {

static constexpr int RESNET_POOL_CH = RESNET_MAX_C / RESNET_POOL_THREADS;      // channels a thread holds at most

__global__ __launch_bounds__(RESNET_POOL_THREADS) void resnet_pool_kernel(const float* __restrict__ x, int HW, int C,
                                                                          float* __restrict__ pooled, float* __restrict__ features) {
    __shared__ float part[RESNET_POOL_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* src = x + (size_t)b * HW * C;
    float acc[RESNET_POOL_CH];
#pragma unroll
    for (int j = 0; j < RESNET_POOL_CH; ++j) acc[j] = 0.f;
    for (int p = 0; p < HW; ++p) {
        const float* row = src + (size_t)p * C;
#pragma unroll
        for (int j = 0; j < RESNET_POOL_CH; ++j) {
            const int c = tid + j * RESNET_POOL_THREADS;
            if (c < C) acc[j] = acc[j] + row[c];
        }
    }
    const float n = (float)HW;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < RESNET_POOL_CH; ++j) {
        const int c = tid + j * RESNET_POOL_THREADS;
        if (c < C) {
            acc[j] = acc[j] / n;
            q = __builtin_fmaf(acc[j], acc[j], q);
            if (pooled) pooled[(size_t)b * C + c] = acc[j];
        }
    }
    if (!features) return;      // (the whole workgroup)
    q = wave_sum(q);
    if ((tid & 63) == 0) part[tid >> 6] = q;
    __syncthreads();
    float total = part[0];
#pragma unroll
    for (int w = 1; w < RESNET_POOL_THREADS / 64; ++w) total = total + part[w];
    const float inv = 1.0f / sqrtf(total);
#pragma unroll
    for (int j = 0; j < RESNET_POOL_CH; ++j) {
        const int c = tid + j * RESNET_POOL_THREADS;
        if (c < C) features[(size_t)b * C + c] = acc[j] * inv;
    }
}

bool resnet_pool_ok(const float* x, int B, int HW, int C, const float* pooled, const float* features) {
    if (!x || (!pooled && !features)) return false;
    if (B < 1 || B > RESNET_MAX_B || C < 64 || C % 64 || C > RESNET_MAX_C) return false;
    return HW >= 1 && (long long)HW <= (long long)RESNET_MAX_SIDE * RESNET_MAX_SIDE;
}

hipError_t launch_resnet_pool(const float* x, int B, int HW, int C, float* pooled, float* features, hipStream_t s) {
    if (!resnet_pool_ok(x, B, HW, C, pooled, features)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resnet_pool_kernel, dim3((unsigned)B), dim3(RESNET_POOL_THREADS), 0, s, x, HW, C, pooled, features);
    return hipGetLastError();
}

}  // namespace hg
