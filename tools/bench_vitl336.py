#!/usr/bin/env python3
"""Throughput of CLIP ViT-L/14@336px `encode_image` (577 tokens per crop, 24 blocks of width 1024) and the long-sequence attention
kernel next to torch's scaled_dot_product_attention.  One JSON line on stdout; human-readable tables on stderr.

    python tools/bench_vitl336.py [--batch 64] [--steps 20] [--warmup 5] [--attn-batch 32] [--repeats 5]
    python tools/bench_vitl336.py --adapters [--batch 64] [--steps 10] [--warmup 3] [--repeats 5]

* `every_row` (option last_block_row0 = 0: every row of every block) and `class_rows` (the default: the last block on the class
  rows only): warm-up steps, then timed steps with a hipEvent on the compute stream between them (as bench.py); crops/s from the
  median step, fraction of the 2516.6 TFLOP/s MFMA peak at 381.92 GFLOP per crop (algorithmic, multiply-add = 2).
* `kernels`: every GEMM / attention launch of one step with its time (hipEvent pairs, hg_profile_begin(HG_PROF_ALL)), summed by
  (kind, M, N, K): which kernels the 24 blocks run.
* `attention`: per layer, the fp16 q | k | v of that layer (ln_1 and in_proj of the HIP path's own stream entering the block,
  rounded to fp16) through attention_long_kernel (hg_test_attention, the kernel alone between a hipEvent pair) and through
  torch.nn.functional.scaled_dot_product_attention on the same values, alternating, `--repeats` times each.  Both legs are timed
  between a hipEvent pair around the one launch, queued behind the same fp32 -> fp16 conversion of qkv (so that the host's launch
  latency falls into the conversion's run time for both).
* `--adapters` (instead of all of the above): the detector's tower - variant C with instance adapters in front of every block, option
  adapter_long = 1 (hg_adapter_long.hip) - with priors (N = 14) and with the sequence as the adapters' memory, beside variant C
  without adapters: the three alternating `--repeats` times in one process, `--steps` timed steps each time; the median over the
  repeats' median steps, min .. max beside it.  Under `rocprofv3 --kernel-trace --stats` the same run gives the decoder kernels' own
  times (`--batch 99`: one full pass of 99 x 577 rows).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hoigen_amd import _lib, synth  # noqa: E402
from hoigen_amd.model import build_model  # noqa: E402

MFMA_PEAK_TFLOPS = 2516.6
GFLOP_PER_CROP = 381.92
HG_PROF_ALL, HG_PROF_ATTENTION = -2, 100
L, D, HEADS, LAYERS = 577, 1024, 16, 24


def timed_steps(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))


def summary(per_step, batch):
    med = statistics.median(per_step)
    cps = batch / med * 1e3
    return {"ms_per_step": {"median": round(med, 3), "p10": round(per_step[len(per_step) // 10], 3),
                            "p90": round(per_step[(len(per_step) * 9) // 10 - (len(per_step) % 10 == 0)], 3)},
            "crops_per_s": round(cps, 1), "tflops": round(cps * GFLOP_PER_CROP / 1e3, 1),
            "frac_of_peak": round(cps * GFLOP_PER_CROP / 1e3 / MFMA_PEAK_TFLOPS, 4)}


def bench_adapters(args):
    dev = torch.device("cuda:0")
    raw = synth.clip_state_dict(synth.VIT_L14_336, 0)
    plain = build_model(synth.to_torch(raw), use_adapter=False).to(dev).visual
    raw.update(synth.adapter_state_dict(synth.VIT_L14_336, 1))
    adapted = build_model(synth.to_torch(raw), use_adapter=True).to(dev).visual
    adapted.set_option("adapter_long", 1)
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.batch, 3, 336, 336, device=dev, generator=gen)
    pri, mask = synth.priors(args.batch, n=14, dim=64, n_pad=4, seed=99)
    prior = (torch.from_numpy(pri).to(dev), torch.from_numpy(mask).to(dev))
    legs = {"c_without_adapters": lambda: plain(x, None), "c_adapters_priors": lambda: adapted(x, prior),
            "c_adapters_self": lambda: adapted(x, None)}
    meds = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            meds[k].append(statistics.median(timed_steps(fn, args.steps, args.warmup)))
    res = {"metric": "vitl14_336_variant_c_adapters", "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
    for k, v in meds.items():
        res[k] = {"ms_per_step": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                  "crops_per_s": round(args.batch / statistics.median(v) * 1e3, 1)}
        print(f"{k:22s} {res[k]['ms_per_step']:9.3f} ms ({res[k]['min']:.3f} .. {res[k]['max']:.3f})  {res[k]['crops_per_s']:8.1f} crops/s",
              file=sys.stderr)
    base = res["c_without_adapters"]["ms_per_step"]
    for k in ("c_adapters_priors", "c_adapters_self"):
        res[k]["over_without"] = round(res[k]["ms_per_step"] / base, 4)
        res[k]["ms_per_adapter"] = round((res[k]["ms_per_step"] - base) / LAYERS, 4)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--attn-batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--adapters", action="store_true", help="variant C with instance adapters (option adapter_long) beside variant C without")
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    if args.adapters:
        return bench_adapters(args)
    dev = torch.device("cuda:0")
    model = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_L14_336, 0))).to(dev)
    vis = model.visual
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.batch, 3, 336, 336, device=dev, generator=gen)
    out = torch.empty(args.batch, 768, device=dev)
    res = {"metric": "vitl14_336_encode_image", "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
           "gflop_per_crop": GFLOP_PER_CROP, "peak_tflops": MFMA_PEAK_TFLOPS, "device": torch.cuda.get_device_name(0)}
    for name, row0 in (("every_row", 0), ("class_rows", 1)):
        vis.set_option("last_block_row0", row0)
        res[name] = summary(timed_steps(lambda: vis.encode_into(x, out), args.steps, args.warmup), args.batch)
    assert torch.isfinite(out).all()

    # ---- which kernels a step runs
    _, recs = _lib.profile(vis._ctx.handle, HG_PROF_ALL, 512, lambda: (vis.encode_into(x, out), torch.cuda.synchronize()))
    table = {}
    for kind, M, N, K, ms in recs:
        e = table.setdefault((kind, M, N, K), [0, 0.0])
        e[0] += 1
        e[1] += ms
    res["kernels"] = [{"kind": k[0], "M": k[1], "N": k[2], "K": k[3], "launches": n, "ms": round(ms, 3)}
                      for k, (n, ms) in sorted(table.items(), key=lambda kv: -kv[1][1])]
    res["kernels_ms_total"] = round(sum(r["ms"] for r in res["kernels"]), 3)

    # ---- attention per layer: the kernel next to torch's SDPA on the same fp16 q, k, v
    B = args.attn_batch
    vis.set_option("last_block_row0", 0)
    _, tr = vis.forward_stream_trace(x[:B])
    vis.set_option("last_block_row0", 1)
    lib, h = _lib.lib(), vis._ctx.handle
    att_out = torch.empty(B * L, D, device=dev)
    layers = []
    for i, blk in enumerate(vis.transformer.resblocks):
        hln = torch.nn.functional.layer_norm(tr[i], (D,), blk.ln_1.weight.float(), blk.ln_1.bias.float(), 1e-5)
        qkv16 = (hln.half() @ blk.attn.in_proj_weight.half().t() + blk.attn.in_proj_bias.half()).contiguous()      # [B*L, 3D] fp16
        qkv32 = qkv16.float()
        q, k, v = (qkv16.view(B, L, 3, HEADS, 64)[:, :, j].permute(0, 2, 1, 3).contiguous() for j in range(3))
        hip_ms, sdpa_ms = [], []
        for r in range(args.repeats + 1):
            def run():
                rc = lib.hg_test_attention(h, qkv32.data_ptr(), None, None, B, L, HEADS, 0, att_out.data_ptr(), None)
                assert rc == 0, lib.hg_last_error(h)
                torch.cuda.synchronize()
            _, rec = _lib.profile(h, HG_PROF_ATTENTION, 4, run)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            filler = qkv32.half()                   # the same conversion hg_test_attention queues in front of its kernel: both legs are
            a.record()                              # dispatched while the GPU is busy, neither interval holds host launch latency
            o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
            b.record()
            torch.cuda.synchronize()
            del filler
            if r:                                   # (the first round of a layer is its warm-up)
                hip_ms.append(rec[0][4])
                sdpa_ms.append(a.elapsed_time(b))
        if i == 0:
            want = o.permute(0, 2, 1, 3).reshape(B * L, D).float()
            err = float((att_out - want).abs().max() / want.abs().max())
            res["attention_max_abs_diff_vs_sdpa_rel"] = round(err, 6)
        layers.append({"layer": i, "hip_ms": round(statistics.median(hip_ms), 4), "hip_min": round(min(hip_ms), 4),
                       "hip_max": round(max(hip_ms), 4), "sdpa_ms": round(statistics.median(sdpa_ms), 4),
                       "sdpa_min": round(min(sdpa_ms), 4), "sdpa_max": round(max(sdpa_ms), 4)})
        del hln, qkv16, qkv32, q, k, v
    hip_t, sd_t = sum(r["hip_ms"] for r in layers), sum(r["sdpa_ms"] for r in layers)
    flop = B * HEADS * 4.0 * L * L * 64
    res["attention"] = {"batch": B, "items": B * HEADS, "repeats": args.repeats, "layers": layers,
                        "hip_ms_sum": round(hip_t, 3), "sdpa_ms_sum": round(sd_t, 3), "hip_over_sdpa": round(hip_t / sd_t, 3),
                        "hip_tflops": round(flop * LAYERS / hip_t / 1e9, 1), "sdpa_tflops": round(flop * LAYERS / sd_t / 1e9, 1)}
    print(f"{'layer':>5} {'hip ms (min..max)':>28} {'sdpa ms (min..max)':>28}", file=sys.stderr)
    for r in layers:
        print(f"{r['layer']:5d} {r['hip_ms']:10.4f} ({r['hip_min']:.4f}..{r['hip_max']:.4f}) "
              f"{r['sdpa_ms']:10.4f} ({r['sdpa_min']:.4f}..{r['sdpa_max']:.4f})", file=sys.stderr)
    print(f"{'kind':>5} {'M':>7} {'N':>6} {'K':>6} {'launches':>8} {'ms':>9}", file=sys.stderr)
    for r in res["kernels"]:
        print(f"{r['kind']:5d} {r['M']:7d} {r['N']:6d} {r['K']:6d} {r['launches']:8d} {r['ms']:9.3f}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
