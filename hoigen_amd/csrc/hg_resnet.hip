// The bottleneck stages of a ResNet on the HIP path (torchvision's Bottleneck under the reference's FrozenBatchNorm2d,
// detr/models/backbone.py:19-55, :83-93): the weight loader, the output-shape rule and the block runner; and the stem in front of them
// (conv1, bn1, ReLU, max-pool): its loader, shape rule, hg_resnet_stem and hg_resnet_body; and hg_resnet_features, the whole network
// with the global average pool and the L2 normalisation behind the last block (the DINO backbone).  Host code only; the kernels are in
// hg_resnet_conv.hip, hg_resnet_stem.hip and hg_resnet_pool.hip.
#include "hg_host.h"

namespace {

const char* const kConvName[4] = {"conv1", "conv2", "conv3", "downsample.0"};
const char* const kNormName[4] = {"bn1", "bn2", "bn3", "downsample.1"};

const hg_resnet_conv& conv_of(const hg_resnet_block& b, int k) { return k == 0 ? b.conv1 : k == 1 ? b.conv2 : k == 2 ? b.conv3 : b.down_conv; }
const hg_resnet_norm& norm_of(const hg_resnet_block& b, int k) { return k == 0 ? b.bn1 : k == 1 ? b.bn2 : k == 2 ? b.bn3 : b.down_bn; }

// what the kernel covers, from the descriptor's integers alone
int check_conv(hg_ctx* c, int blk, const char* name, const hg_resnet_conv& v) {
    const char* f = "hg_load_resnet_stages: blocks[%d].%s: ";
    char head[96];
    snprintf(head, sizeof head, f, blk, name);
    if (v.kh != v.kw || (v.kh != 1 && v.kh != 3)) return fail(c, HG_ERR_INVALID, "%sa %d x %d kernel; only 1 x 1 and 3 x 3 are implemented", head, v.kh, v.kw);
    if (v.dil_h != 1 || v.dil_w != 1)
        return fail(c, HG_ERR_INVALID, "%sdilation (%d, %d); only dilation 1 is implemented (the reference's --dilation, DC5, is off by default)", head,
                    v.dil_h, v.dil_w);
    if (v.groups != 1) return fail(c, HG_ERR_INVALID, "%sgroups = %d; only groups = 1 is implemented", head, v.groups);
    if (v.has_bias) return fail(c, HG_ERR_INVALID, "%sthe convolution has a bias; a ResNet's convolutions have none", head);
    if (v.stride_h != v.stride_w || (v.stride_h != 1 && v.stride_h != 2))
        return fail(c, HG_ERR_INVALID, "%sstride (%d, %d); only 1 and 2, the same on both axes, are implemented", head, v.stride_h, v.stride_w);
    if (v.pad_h != (v.kh - 1) / 2 || v.pad_w != (v.kh - 1) / 2)
        return fail(c, HG_ERR_INVALID, "%spadding (%d, %d) under a %d x %d kernel; only (k - 1) / 2 is implemented", head, v.pad_h, v.pad_w, v.kh, v.kw);
    if (v.cin < 64 || v.cin % 64 || v.cin > RESNET_MAX_C || v.cout < 64 || v.cout % 64 || v.cout > RESNET_MAX_C)
        return fail(c, HG_ERR_INVALID, "%s%d -> %d channels; both must be multiples of 64 up to %d", head, v.cin, v.cout, RESNET_MAX_C);
    if (v.kh == 3 && v.cin > RESNET_MAX_C3) return fail(c, HG_ERR_INVALID, "%sa 3 x 3 kernel over %d input channels, at most %d", head, v.cin, RESNET_MAX_C3);
    return HG_OK;
}

int check_blocks(hg_ctx* c, const hg_resnet_weights* w) {
    if (!w || !w->blocks) return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: weights are required");
    if (w->n_blocks < 1 || w->n_blocks > RESNET_MAX_BLOCKS)
        return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: %d blocks, 1 .. %d", w->n_blocks, RESNET_MAX_BLOCKS);
    for (int i = 0; i < w->n_blocks; ++i) {
        const hg_resnet_block& b = w->blocks[i];
        for (int k = 0; k < (b.has_downsample ? 4 : 3); ++k) {
            int rc = check_conv(c, i, kConvName[k], conv_of(b, k));
            if (rc) return rc;
        }
        if (b.conv2.cin != b.conv1.cout || b.conv3.cin != b.conv2.cout)
            return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: blocks[%d]: the channels do not chain (conv1 %d -> %d, conv2 %d -> %d, conv3 %d -> %d)", i,
                        b.conv1.cin, b.conv1.cout, b.conv2.cin, b.conv2.cout, b.conv3.cin, b.conv3.cout);
        const int stride = b.conv1.stride_h * b.conv2.stride_h * b.conv3.stride_h;
        if (!b.has_downsample) {
            if (b.conv3.cout != b.conv1.cin || stride != 1)
                return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: blocks[%d] has no downsample, and maps %d channels to %d at stride %d: the identity does not fit",
                            i, b.conv1.cin, b.conv3.cout, stride);
        } else if (b.down_conv.cin != b.conv1.cin || b.down_conv.cout != b.conv3.cout || b.down_conv.stride_h != stride || b.down_conv.kh != 1) {
            return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: blocks[%d].downsample.0 is %d x %d, %d -> %d at stride %d; the block needs 1 x 1, %d -> %d at stride %d",
                        i, b.down_conv.kh, b.down_conv.kw, b.down_conv.cin, b.down_conv.cout, b.down_conv.stride_h, b.conv1.cin, b.conv3.cout, stride);
        }
        if (i && b.conv1.cin != w->blocks[i - 1].conv3.cout)
            return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: blocks[%d] takes %d channels, blocks[%d] gives %d", i, b.conv1.cin, i - 1,
                        w->blocks[i - 1].conv3.cout);
        for (int k = 0; k < (b.has_downsample ? 4 : 3); ++k) {
            const hg_resnet_norm& n = norm_of(b, k);
            if (!conv_of(b, k).weight || !n.weight || !n.bias || !n.running_mean || !n.running_var)
                return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: blocks[%d]: missing tensor of %s / %s", i, kConvName[k], kNormName[k]);
            if (!(n.eps >= 0.0) || n.eps > 1.0) return fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: blocks[%d].%s: eps = %g", i, kNormName[k], n.eps);
        }
    }
    return HG_OK;
}

// one convolution and its norm: the packed fp16 weight, and scale / bias made in double and rounded to fp32 (backbone.py:45-55)
int load_conv(hg_ctx* c, std::vector<void*>& owned, const hg_resnet_conv& v, const hg_resnet_norm& n, int* flag, ResnetConvW& d) {
    d.cin = v.cin; d.cout = v.cout; d.R = v.kh; d.stride = v.stride_h;
    const size_t nw = (size_t)v.cout * v.cin * v.kh * v.kh;
    const bool stem = v.kh == 7;      // hg_load_resnet_stem: hg_resnet_stem.hip's fragment order
    void *pw, *ps, *pb;
    int rc = dev_alloc(c, owned, stem ? RESNET_STEM_W_HALFS * 2 : nw * 2, &pw);
    if (!rc) rc = dev_alloc(c, owned, (size_t)v.cout * 4, &ps);
    if (!rc) rc = dev_alloc(c, owned, (size_t)v.cout * 4, &pb);
    if (rc) return rc;
    if (stem) HG_HIP(launch_resnet_stem_pack(v.weight, (half_t*)pw, flag, 0));
    else HG_HIP(launch_resnet_pack(v.weight, (half_t*)pw, v.cout, v.cin, v.kh, flag, 0));
    std::vector<float> h[4], scale(v.cout), bias(v.cout);
    const float* src[4] = {n.weight, n.bias, n.running_mean, n.running_var};
    for (int k = 0; k < 4; ++k) {
        h[k].resize(v.cout);
        HG_HIP(hipMemcpy(h[k].data(), src[k], (size_t)v.cout * 4, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < v.cout; ++i) {
        const double s = (double)h[0][i] / sqrt((double)h[3][i] + n.eps);
        scale[i] = (float)s;
        bias[i] = (float)((double)h[1][i] - (double)h[2][i] * s);
    }
    HG_HIP(hipMemcpy(ps, scale.data(), (size_t)v.cout * 4, hipMemcpyHostToDevice));
    HG_HIP(hipMemcpy(pb, bias.data(), (size_t)v.cout * 4, hipMemcpyHostToDevice));
    d.w = (half_t*)pw; d.scale = (float*)ps; d.bias = (float*)pb;
    return HG_OK;
}

struct Hw {
    int H, W;
};
Hw conv_out(Hw in, int R, int stride) { return Hw{resnet_out_size(in.H, R, stride), resnet_out_size(in.W, R, stride)}; }

// the stages' workspace (include/hoigen_amd.h states the rule): the fp32 stream in and out, the downsample's output, the fp16 copies,
// conv1's and conv2's outputs.  x32[0] / x16[0] take the input of block `first`.
struct ResnetWs {
    float* x32[2];
    float* ds32;
    half_t* x16[2];
    half_t *t1, *t2;
};
int resnet_workspace(hg_ctx* c, int B_, Hw in, int first, int last, ResnetWs& w) {
    const ResnetStages& r = c->resnet;
    const size_t B = (size_t)B_;
    // walk the range once for the largest buffers
    size_t E = B * in.H * in.W * r.blocks[first].c1.cin, T1 = 0, T2 = 0;
    Hw s0 = in;
    for (int i = first; i <= last; ++i) {
        const ResnetBlockW& b = r.blocks[i];
        const Hw s1 = conv_out(s0, b.c1.R, b.c1.stride), s2 = conv_out(s1, b.c2.R, b.c2.stride), s3 = conv_out(s2, b.c3.R, b.c3.stride);
        T1 = std::max(T1, B * s1.H * s1.W * b.c1.cout);
        T2 = std::max(T2, B * s2.H * s2.W * b.c2.cout);
        E = std::max(E, B * s3.H * s3.W * b.c3.cout);
        s0 = s3;
    }
    E = rup(E, 64); T1 = rup(T1, 64); T2 = rup(T2, 64);
    int rc = ensure(c, c->resnet_ws, 2 * 4 * E + 2 * 2 * E + 4 * E + 2 * T1 + 2 * T2);
    if (rc) return rc;
    char* ws = (char*)c->resnet_ws.p;
    w.x32[0] = (float*)ws; w.x32[1] = (float*)(ws + 4 * E);
    w.ds32 = (float*)(ws + 8 * E);
    w.x16[0] = (half_t*)(ws + 12 * E); w.x16[1] = (half_t*)(ws + 14 * E);
    w.t1 = (half_t*)(ws + 16 * E); w.t2 = (half_t*)(ws + 16 * E + 2 * T1);
    return HG_OK;
}

// blocks first .. last on the NHWC pair in w.x32[0] / w.x16[0] (B x in.H x in.W x cin of `first`): every block is torchvision's
// Bottleneck.forward.  The one block loop of hg_resnet_stages, hg_resnet_body and hg_resnet_features (`who` names the caller in a
// message).  `out` nullable: no exit launch.  `last_nhwc` / `last_hw` nullable: the fp32 NHWC stream behind block `last` and its size.
int resnet_run_blocks(hg_ctx* c, const char* who, int B, Hw cur, int first, int last, const ResnetWs& w, float* out, const int64_t* out_stride,
                      float* const* trace, hipStream_t s, const float** last_nhwc = nullptr, Hw* last_hw = nullptr) {
    const ResnetStages& r = c->resnet;
    auto conv = [&](const ResnetConvW& cw, const half_t* x, Hw in, Hw o, int epi, const float* identity, float* o32, half_t* o16) -> int {
        ResnetConvArgs k{};
        k.x = x; k.w = cw.w; k.scale = cw.scale; k.bias = cw.bias; k.identity = identity; k.out32 = o32; k.out16 = o16;
        k.B = B; k.H = in.H; k.W = in.W; k.Cin = cw.cin; k.Ho = o.H; k.Wo = o.W; k.Cout = cw.cout; k.R = cw.R; k.stride = cw.stride; k.epi = epi;
        ProfScope ps(c, s, HG_PROF_RESNET_CONV, B * o.H * o.W, cw.cout, cw.R * cw.R * cw.cin);
        hipError_t he = launch_resnet_conv(k, s);
        ps.finish();
        if (he != hipSuccess) return fail(c, HG_ERR_HIP, "%s: convolution launch failed: %s", who, hipGetErrorString(he));
        return HG_OK;
    };
    int p = 0, rc;
    for (int i = first; i <= last; ++i) {
        const ResnetBlockW& b = r.blocks[i];
        const Hw s1 = conv_out(cur, b.c1.R, b.c1.stride), s2 = conv_out(s1, b.c2.R, b.c2.stride), s3 = conv_out(s2, b.c3.R, b.c3.stride);
        // out = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x)))))))) + identity)      (torchvision's Bottleneck.forward)
        if ((rc = conv(b.c1, w.x16[p], cur, s1, 1, nullptr, nullptr, w.t1))) return rc;
        if ((rc = conv(b.c2, w.t1, s1, s2, 1, nullptr, nullptr, w.t2))) return rc;
        const float* identity = w.x32[p];
        if (b.down) {
            const Hw sd = conv_out(cur, b.cd.R, b.cd.stride);
            if (sd.H != s3.H || sd.W != s3.W)
                return fail(c, HG_ERR_INVALID, "%s: blocks[%d]: the downsample gives %d x %d, the block %d x %d", who, i, sd.H, sd.W, s3.H, s3.W);
            if ((rc = conv(b.cd, w.x16[p], cur, sd, 2, nullptr, w.ds32, nullptr))) return rc;
            identity = w.ds32;
        }
        if ((rc = conv(b.c3, w.t2, s2, s3, 3, identity, w.x32[p ^ 1], w.x16[p ^ 1]))) return rc;
        p ^= 1;
        cur = s3;
        float* tr = trace ? trace[i - first] : nullptr;
        if (tr) HG_HIP(launch_resnet_exit(w.x32[p], B, b.c3.cout, cur.H * cur.W, tr, (long long)b.c3.cout * cur.H * cur.W, (long long)cur.H * cur.W, s));
    }
    if (out) HG_HIP(launch_resnet_exit(w.x32[p], B, r.blocks[last].c3.cout, cur.H * cur.W, out, out_stride[0], out_stride[1], s));
    if (last_nhwc) *last_nhwc = w.x32[p];
    if (last_hw) *last_hw = cur;
    return HG_OK;
}

// what hg_resnet_stem.hip covers, from the descriptor's integers alone
int check_stem(hg_ctx* c, const hg_resnet_stem_weights* w) {
    if (!w) return fail(c, HG_ERR_INVALID, "hg_load_resnet_stem: weights are required");
    const hg_resnet_conv& v = w->conv1;
    const char* head = "hg_load_resnet_stem: conv1: ";
    if (v.kh != 7 || v.kw != 7) return fail(c, HG_ERR_INVALID, "%sa %d x %d kernel; only 7 x 7 is implemented", head, v.kh, v.kw);
    if (v.dil_h != 1 || v.dil_w != 1) return fail(c, HG_ERR_INVALID, "%sdilation (%d, %d); only dilation 1 is implemented", head, v.dil_h, v.dil_w);
    if (v.groups != 1) return fail(c, HG_ERR_INVALID, "%sgroups = %d; only groups = 1 is implemented", head, v.groups);
    if (v.has_bias) return fail(c, HG_ERR_INVALID, "%sthe convolution has a bias; a ResNet's convolutions have none", head);
    if (v.stride_h != 2 || v.stride_w != 2) return fail(c, HG_ERR_INVALID, "%sstride (%d, %d); only (2, 2) is implemented", head, v.stride_h, v.stride_w);
    if (v.pad_h != 3 || v.pad_w != 3) return fail(c, HG_ERR_INVALID, "%spadding (%d, %d); only (3, 3) is implemented", head, v.pad_h, v.pad_w);
    if (v.cin != 3 || v.cout != 64) return fail(c, HG_ERR_INVALID, "%s%d -> %d channels; only 3 -> 64 is implemented", head, v.cin, v.cout);
    if (w->pool_kernel != 3 || w->pool_stride != 2 || w->pool_padding != 1 || w->pool_dilation != 1 || w->pool_ceil_mode)
        return fail(c, HG_ERR_INVALID, "hg_load_resnet_stem: maxpool: kernel %d, stride %d, padding %d, dilation %d, ceil_mode %d; "
                    "only 3 / 2 / 1 with dilation 1 and ceil_mode off is implemented", w->pool_kernel, w->pool_stride, w->pool_padding, w->pool_dilation, w->pool_ceil_mode);
    const hg_resnet_norm& n = w->bn1;
    if (!v.weight || !n.weight || !n.bias || !n.running_mean || !n.running_var)
        return fail(c, HG_ERR_INVALID, "hg_load_resnet_stem: missing tensor of conv1 / bn1");
    if (!(n.eps >= 0.0) || n.eps > 1.0) return fail(c, HG_ERR_INVALID, "hg_load_resnet_stem: bn1: eps = %g", n.eps);
    return HG_OK;
}

// B, Hi, Wi of a stem call, and the pooled size
int check_stem_shape(hg_ctx* c, const char* who, int B, int Hi, int Wi, Hw& pooled) {
    if (B < 1 || B > RESNET_MAX_B) return fail(c, HG_ERR_INVALID, "%s: B = %d images, 1 .. %d", who, B, RESNET_MAX_B);
    if (Hi < 1 || Wi < 1 || Hi > 4 * RESNET_MAX_SIDE || Wi > 4 * RESNET_MAX_SIDE)
        return fail(c, HG_ERR_INVALID, "%s: Hi x Wi = %d x %d, 1 .. %d each (a pooled map of at most %d a side)", who, Hi, Wi, 4 * RESNET_MAX_SIDE,
                    RESNET_MAX_SIDE);
    pooled = Hw{resnet_stem_pool_size(resnet_stem_conv_size(Hi)), resnet_stem_pool_size(resnet_stem_conv_size(Wi))};
    return HG_OK;
}

int launch_stem(hg_ctx* c, const char* who, const float* x, const int64_t* xs, int B, int Hi, int Wi, float* o32, half_t* o16, hipStream_t s) {
    const ResnetConvW& w = c->resnet_stem.conv;
    ResnetStemArgs k{};
    k.x = x; k.sb = xs[0]; k.sc = xs[1]; k.sr = xs[2]; k.w = w.w; k.scale = w.scale; k.bias = w.bias; k.out32 = o32; k.out16 = o16;
    k.B = B; k.Hi = Hi; k.Wi = Wi; k.Hc = resnet_stem_conv_size(Hi); k.Wc = resnet_stem_conv_size(Wi);
    k.Hp = resnet_stem_pool_size(k.Hc); k.Wp = resnet_stem_pool_size(k.Wc);
    ProfScope ps(c, s, HG_PROF_RESNET_STEM, B * k.Hp * k.Wp, 64, 147);
    hipError_t he = launch_resnet_stem(k, s);
    ps.finish();
    if (he == hipErrorInvalidValue) return fail(c, HG_ERR_INVALID, "%s: the launcher refuses this call (x must be 4-byte aligned)", who);
    if (he != hipSuccess) return fail(c, HG_ERR_HIP, "%s: stem launch failed: %s", who, hipGetErrorString(he));
    return HG_OK;
}

}  // namespace

extern "C" {

// torchvision's Bottleneck (conv1, bn1, conv2, bn2, conv3, bn3, downsample) for every block of layer1 .. layer4 (backbone.py:83-93)
int hg_load_resnet_stages(hg_ctx* c, const hg_resnet_weights* w) {
    if (!c) return HG_ERR_INVALID;
    int rc = check_blocks(c, w);
    if (rc) return rc;
    HG_ON_DEVICE(c);
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    ResnetStages n;
    n.blocks.resize(w->n_blocks);
    void* flags = nullptr;
    rc = dev_alloc(c, n.owned, (size_t)w->n_blocks * 4 * sizeof(int), &flags);
    if (!rc) {
        hipError_t e = hipMemset(flags, 0, (size_t)w->n_blocks * 4 * sizeof(int));
        if (e != hipSuccess) rc = fail(c, HG_ERR_HIP, "hg_load_resnet_stages: hipMemset failed: %s", hipGetErrorString(e));
    }
    for (int i = 0; !rc && i < w->n_blocks; ++i) {
        const hg_resnet_block& b = w->blocks[i];
        ResnetBlockW& d = n.blocks[i];
        d.down = b.has_downsample != 0;
        ResnetConvW* dst[4] = {&d.c1, &d.c2, &d.c3, &d.cd};
        for (int k = 0; !rc && k < (d.down ? 4 : 3); ++k) rc = load_conv(c, n.owned, conv_of(b, k), norm_of(b, k), (int*)flags + 4 * i + k, *dst[k]);
    }
    std::vector<int> hf((size_t)w->n_blocks * 4, 0);
    if (!rc) {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(hf.data(), flags, hf.size() * sizeof(int), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, HG_ERR_HIP, "hg_load_resnet_stages: reading the weights failed: %s", hipGetErrorString(e));
    }
    for (size_t i = 0; !rc && i < hf.size(); ++i)
        if (hf[i])
            rc = fail(c, HG_ERR_INVALID, "hg_load_resnet_stages: blocks[%d].%s.weight holds a value that is not finite or rounds beyond fp16's range (65504)",
                      (int)(i / 4), kConvName[i % 4]);
    if (rc) {
        (void)hipDeviceSynchronize();
        free_all(n.owned);
        return rc;
    }
    free_all(c->resnet.owned);
    c->resnet = std::move(n);
    c->resnet.loaded = true;
    return HG_OK;
}

int hg_resnet_out_shape(const hg_resnet_weights* w, int first_block, int last_block, int H, int W, int32_t* C, int32_t* Ho, int32_t* Wo) {
    if (!w || !w->blocks || first_block < 0 || last_block < first_block || last_block >= w->n_blocks || H < 1 || W < 1) return HG_ERR_INVALID;
    Hw s{H, W};
    for (int i = first_block; i <= last_block; ++i) {
        const hg_resnet_block& b = w->blocks[i];
        for (int k = 0; k < 3; ++k) {
            const hg_resnet_conv& v = conv_of(b, k);
            if (v.stride_h < 1 || v.stride_w < 1) return HG_ERR_INVALID;
            s = Hw{(s.H + 2 * v.pad_h - v.dil_h * (v.kh - 1) - 1) / v.stride_h + 1, (s.W + 2 * v.pad_w - v.dil_w * (v.kw - 1) - 1) / v.stride_w + 1};
            if (s.H < 1 || s.W < 1) return HG_ERR_INVALID;
        }
    }
    if (C) *C = w->blocks[last_block].conv3.cout;
    if (Ho) *Ho = s.H;
    if (Wo) *Wo = s.W;
    return HG_OK;
}

// layer1 .. layer4 of backbone.py:83-93 under IntermediateLayerGetter (:69-73): every block is torchvision's Bottleneck.forward
int hg_resnet_stages(hg_ctx* c, const hg_resnet_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    const ResnetStages& r = c->resnet;
    if (!r.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_resnet_stages: no stages loaded (hg_load_resnet_stages)");
    if (!a || !a->x || !a->out) return fail(c, HG_ERR_INVALID, "hg_resnet_stages: x and out are required");
    if (a->B < 1 || a->B > RESNET_MAX_B) return fail(c, HG_ERR_INVALID, "hg_resnet_stages: B = %d images, 1 .. %d", a->B, RESNET_MAX_B);
    if (a->H < 1 || a->W < 1 || a->H > RESNET_MAX_SIDE || a->W > RESNET_MAX_SIDE)
        return fail(c, HG_ERR_INVALID, "hg_resnet_stages: H x W = %d x %d, 1 .. %d each", a->H, a->W, RESNET_MAX_SIDE);
    const int nb = (int)r.blocks.size(), first = a->first_block, last = a->last_block;
    if (first < 0 || last < first || last >= nb)
        return fail(c, HG_ERR_INVALID, "hg_resnet_stages: blocks %d .. %d of %d loaded", first, last, nb);
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    ResnetWs w;
    int rc = resnet_workspace(c, a->B, Hw{a->H, a->W}, first, last, w);
    if (rc) return rc;
    HG_HIP(launch_resnet_entry(a->x, a->x_stride[0], a->x_stride[1], a->x_stride[2], a->B, r.blocks[first].c1.cin, a->H, a->W, w.x32[0], w.x16[0], s));
    return resnet_run_blocks(c, "hg_resnet_stages", a->B, Hw{a->H, a->W}, first, last, w, a->out, a->out_stride, a->trace, s);
}

// conv1, bn1, relu, maxpool of torchvision's ResNet (backbone.py:83-93) for hg_resnet_stem.hip
int hg_load_resnet_stem(hg_ctx* c, const hg_resnet_stem_weights* w) {
    if (!c) return HG_ERR_INVALID;
    int rc = check_stem(c, w);
    if (rc) return rc;
    HG_ON_DEVICE(c);
    HG_HIP(hipDeviceSynchronize());      // a call in flight may still read the weights this load replaces
    ResnetStem n;
    void* flag = nullptr;
    rc = dev_alloc(c, n.owned, 16, &flag);
    if (!rc) {
        hipError_t e = hipMemset(flag, 0, 16);
        if (e != hipSuccess) rc = fail(c, HG_ERR_HIP, "hg_load_resnet_stem: hipMemset failed: %s", hipGetErrorString(e));
    }
    if (!rc) rc = load_conv(c, n.owned, w->conv1, w->bn1, (int*)flag, n.conv);
    int hf = 0;
    if (!rc) {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(&hf, flag, sizeof hf, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, HG_ERR_HIP, "hg_load_resnet_stem: reading the weights failed: %s", hipGetErrorString(e));
    }
    if (!rc && hf) rc = fail(c, HG_ERR_INVALID, "hg_load_resnet_stem: conv1.weight holds a value that is not finite or rounds beyond fp16's range (65504)");
    if (rc) {
        (void)hipDeviceSynchronize();
        free_all(n.owned);
        return rc;
    }
    free_all(c->resnet_stem.owned);
    c->resnet_stem = std::move(n);
    c->resnet_stem.loaded = true;
    return HG_OK;
}

int hg_resnet_stem_out_shape(int Hi, int Wi, int32_t* Hp, int32_t* Wp) {
    if (Hi < 1 || Wi < 1) return HG_ERR_INVALID;
    if (Hp) *Hp = resnet_stem_pool_size(resnet_stem_conv_size(Hi));
    if (Wp) *Wp = resnet_stem_pool_size(resnet_stem_conv_size(Wi));
    return HG_OK;
}

// maxpool(relu(bn1(conv1(images)))) as fp32 [B, 64, Hp, Wp]: what hg_resnet_stages takes as x
int hg_resnet_stem(hg_ctx* c, const hg_resnet_stem_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    if (!c->resnet_stem.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_resnet_stem: no stem loaded (hg_load_resnet_stem)");
    if (!a || !a->x || !a->out) return fail(c, HG_ERR_INVALID, "hg_resnet_stem: x and out are required");
    Hw p;
    int rc = check_stem_shape(c, "hg_resnet_stem", a->B, a->Hi, a->Wi, p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    const size_t E = rup((size_t)a->B * p.H * p.W * 64, 64);
    if ((rc = ensure(c, c->resnet_stem_ws, 4 * E + 2 * E))) return rc;
    float* o32 = (float*)c->resnet_stem_ws.p;
    half_t* o16 = (half_t*)((char*)c->resnet_stem_ws.p + 4 * E);
    if ((rc = launch_stem(c, "hg_resnet_stem", a->x, a->x_stride, a->B, a->Hi, a->Wi, o32, o16, s))) return rc;
    HG_HIP(launch_resnet_exit(o32, a->B, 64, p.H * p.W, a->out, a->out_stride[0], a->out_stride[1], s));
    return HG_OK;
}

// the body of backbone.py:69-73 from the images: the stem kernel writes the stages' NHWC pair, then blocks 0 .. last_block
int hg_resnet_body(hg_ctx* c, const hg_resnet_body_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    const ResnetStages& r = c->resnet;
    if (!c->resnet_stem.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_resnet_body: no stem loaded (hg_load_resnet_stem)");
    if (!r.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_resnet_body: no stages loaded (hg_load_resnet_stages)");
    if (!a || !a->x || !a->out) return fail(c, HG_ERR_INVALID, "hg_resnet_body: x and out are required");
    if (c->resnet_stem.conv.cout != r.blocks[0].c1.cin)
        return fail(c, HG_ERR_INVALID, "hg_resnet_body: the stem gives %d channels, blocks[0] takes %d", c->resnet_stem.conv.cout, r.blocks[0].c1.cin);
    Hw p;
    int rc = check_stem_shape(c, "hg_resnet_body", a->B, a->Hi, a->Wi, p);
    if (rc) return rc;
    const int nb = (int)r.blocks.size(), last = a->last_block;
    if (last < 0 || last >= nb) return fail(c, HG_ERR_INVALID, "hg_resnet_body: blocks 0 .. %d of %d loaded", last, nb);
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    ResnetWs w;
    if ((rc = resnet_workspace(c, a->B, p, 0, last, w))) return rc;
    if ((rc = launch_stem(c, "hg_resnet_body", a->x, a->x_stride, a->B, a->Hi, a->Wi, w.x32[0], w.x16[0], s))) return rc;
    return resnet_run_blocks(c, "hg_resnet_body", a->B, p, 0, last, w, a->out, a->out_stride, a->trace, s);
}

// The DINO backbone of upt_tip_cache_model_free_finetune_distill3.py:1617-1618 from the images: the stem, every loaded block, then the
// pool + normalise kernel on the NHWC stream the last block left in the workspace (hg_resnet_pool.hip)
int hg_resnet_features(hg_ctx* c, const hg_resnet_features_args* a, void* stream) {
    if (!c) return HG_ERR_INVALID;
    const ResnetStages& r = c->resnet;
    if (!c->resnet_stem.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_resnet_features: no stem loaded (hg_load_resnet_stem)");
    if (!r.loaded) return fail(c, HG_ERR_NOT_LOADED, "hg_resnet_features: no stages loaded (hg_load_resnet_stages)");
    if (!a || !a->x) return fail(c, HG_ERR_INVALID, "hg_resnet_features: x is required");
    if (!a->pooled && !a->features && !a->map_out) return fail(c, HG_ERR_INVALID, "hg_resnet_features: one of pooled, features and map_out is required");
    if (c->resnet_stem.conv.cout != r.blocks[0].c1.cin)
        return fail(c, HG_ERR_INVALID, "hg_resnet_features: the stem gives %d channels, blocks[0] takes %d", c->resnet_stem.conv.cout, r.blocks[0].c1.cin);
    Hw p;
    int rc = check_stem_shape(c, "hg_resnet_features", a->B, a->Hi, a->Wi, p);
    if (rc) return rc;
    const int last = (int)r.blocks.size() - 1;
    hipStream_t s = (hipStream_t)stream;
    HG_ON_DEVICE(c);
    ResnetWs w;
    if ((rc = resnet_workspace(c, a->B, p, 0, last, w))) return rc;
    if ((rc = launch_stem(c, "hg_resnet_features", a->x, a->x_stride, a->B, a->Hi, a->Wi, w.x32[0], w.x16[0], s))) return rc;
    const float* nhwc = nullptr;
    Hw o{};
    if ((rc = resnet_run_blocks(c, "hg_resnet_features", a->B, p, 0, last, w, a->map_out, a->map_stride, nullptr, s, &nhwc, &o))) return rc;
    if (!a->pooled && !a->features) return HG_OK;
    const int C = r.blocks[last].c3.cout;
    ProfScope ps(c, s, HG_PROF_RESNET_POOL, a->B, C, o.H * o.W);
    hipError_t he = launch_resnet_pool(nhwc, a->B, o.H * o.W, C, a->pooled, a->features, s);
    ps.finish();
    if (he != hipSuccess) return fail(c, HG_ERR_HIP, "hg_resnet_features: pool launch failed: %s", hipGetErrorString(he));
    return HG_OK;
}

}  // extern "C"
