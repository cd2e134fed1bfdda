#!/usr/bin/env python3
"""Times the DETR encoder on the HIP path (hoigen_amd/detr.py) against the same layers as torch's own modules.

Three cases: B = 1 and B = 4 on a 25 x 38 grid (950 tokens), B = 2 on 38 x 38 (1 444 tokens: the chunked form of the attention
kernel); image 0 unpadded, the others padded on the right and at the bottom.  For each case:

  * the whole call: hg_detr_encoder, torch's modules in fp32 (what the reference runs) and under fp16 autocast.  The three are run in
    turn, round after round, each timed with a pair of events around `--inner` calls; the median over the rounds and the spread
    (min .. max) are reported;
  * per layer, the attention kernel and the GEMM launches from the library's own event pairs (hg_profile_begin), median over layers and
    rounds;
  * the attention kernel alone (hg_test_detr_attention) with the slab sized from the launch and fixed at 1, 2 and 4 query tiles, against
    torch.nn.functional.scaled_dot_product_attention on the same fp16 q, k, v and mask - again in turn, round after round.

Seeded default-initialised weights (timing does not depend on their values).  Prints a report and one JSON line.
    python tools/bench_detr_encoder.py [--rounds 7] [--inner 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hoigen_amd import _lib  # noqa: E402
from hoigen_amd.detr import TransformerEncoder  # noqa: E402

D, H, F, NL = 256, 8, 2048, 6
CASES = (("B1_25x38", 1, 25, 38), ("B4_25x38", 4, 25, 38), ("B2_38x38", 2, 38, 38))


class Layer(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(D, H, dropout=0.1)
        self.linear1, self.linear2 = nn.Linear(D, F), nn.Linear(F, D)
        self.norm1, self.norm2 = nn.LayerNorm(D), nn.LayerNorm(D)
        self.activation, self.normalize_before = torch.nn.functional.relu, False

    def forward(self, src, kpm, pos):
        q = k = src + pos
        src = self.norm1(src + self.self_attn(q, k, value=src, key_padding_mask=kpm)[0])
        return self.norm2(src + self.linear2(self.activation(self.linear1(src))))


class Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([Layer() for _ in range(NL)])
        self.norm = None

    def forward(self, src, mask=None, src_key_padding_mask=None, pos=None):
        for l in self.layers:
            src = l(src, src_key_padding_mask, pos)
        return src


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def in_turn(variants, rounds, inner):
    """{name: fn} -> {name: (median ms, min, max)}: one warm-up each, then the variants in turn, round after round"""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def fmt(x):
    return f"{x[0]:8.3f} ms ({x[1]:.3f} .. {x[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    ref = Encoder().to(dev).eval()
    enc = TransformerEncoder.from_module(ref)
    result = {}
    for name, B, gh, gw in CASES:
        S = gh * gw
        src, pos = torch.randn(S, B, D, device=dev), torch.randn(S, B, D, device=dev)
        kpm = torch.zeros(B, gh, gw, dtype=torch.bool, device=dev)
        for b in range(1, B):
            kpm[b, gh - 3 * b:], kpm[b, :, gw - 4 * b:] = True, True
        kpm = kpm.flatten(1)

        def hip():
            return enc(src, src_key_padding_mask=kpm, pos=pos)

        def t32():
            return ref(src, src_key_padding_mask=kpm, pos=pos)

        def t16():
            with torch.autocast("cuda", dtype=torch.float16):
                return ref(src, src_key_padding_mask=kpm, pos=pos)

        err = float((hip() - t32()).norm() / t32().norm())
        call = in_turn({"hip": hip, "torch_fp32": t32, "torch_fp16_autocast": t16}, args.rounds, args.inner)
        # per-kernel times of the call from the library's own event pairs
        handle = enc._ctx.get(dev)
        att, gemm = [], []
        for _ in range(args.rounds):
            _, recs = _lib.profile(handle, _lib.HG_PROF_ALL, 64, hip)
            torch.cuda.synchronize()
            a = [r[4] for r in recs if r[0] == _lib.HG_PROF_ATTENTION]
            g = [r[4] for r in recs if r[0] != _lib.HG_PROF_ATTENTION]
            assert len(a) == NL and len(g) % NL == 0, (len(a), len(g))
            per = len(g) // NL          # GEMM launches a layer
            first_layer = recs[:per + 1]
            att += a
            gemm += [sum(g[per * i:per * i + per]) for i in range(NL)]
        # the attention kernel alone against SDPA on the same fp16 operands
        q32, k32, v32 = (torch.randn(B * S, D, device=dev).half().float() for _ in range(3))
        mask8 = kpm.to(torch.uint8).contiguous()
        out = torch.empty(B * S + 8, D, device=dev)
        hd = lambda t: t.half().view(B, S, H, 32).permute(0, 2, 1, 3).contiguous()
        q16, k16, v16 = hd(q32), hd(k32), hd(v32)
        amask = (~kpm)[:, None, None, :]
        lib = _lib.lib()
        alone = {}
        for waves in (0, 1, 2, 4):
            enc.set_option("detr_attn_waves", waves)
            ts = []
            for _ in range(args.rounds + 1):
                _, recs = _lib.profile(handle, _lib.HG_PROF_ATTENTION, 4, lambda: lib.hg_test_detr_attention(
                    handle, q32.data_ptr(), k32.data_ptr(), v32.data_ptr(), mask8.data_ptr(), B, S, S, H, -1, 0, 0, out.data_ptr(),
                    torch.cuda.current_stream(dev).cuda_stream))
                torch.cuda.synchronize()
                ts.append(recs[0][4])
            ts = ts[1:]
            alone[f"waves_{waves}"] = (statistics.median(ts), min(ts), max(ts))
        enc.set_option("detr_attn_waves", 0)
        sdpa = in_turn({"sdpa_fp16": lambda: torch.nn.functional.scaled_dot_product_attention(q16, k16, v16, attn_mask=amask)},
                       args.rounds, args.inner)
        alone.update(sdpa)
        r = {"call": call, "attention_per_layer": (statistics.median(att), min(att), max(att)),
             "gemms_per_layer": (statistics.median(gemm), min(gemm), max(gemm)), "attention_alone": alone, "rel_l2_vs_torch_fp32": err}
        result[name] = r
        print(f"== {name}: B {B}, {gh} x {gw} = {S} tokens, {NL} layers; rel L2 against torch fp32 {err:.2e}")
        for k, v in call.items():
            print(f"   call {k:20s} {fmt(v)}")
        print(f"   per layer: attention kernel {fmt(r['attention_per_layer'])}   GEMM launches {fmt(r['gemms_per_layer'])}")
        print("   launches of layer 0 (kind, M, N, K, ms): " + "  ".join(f"({r[0]}, {r[1]}, {r[2]}, {r[3]}, {r[4]:.3f})" for r in first_layer))
        for k, v in alone.items():
            print(f"   attention alone {k:10s} {fmt(v)}")
        print(f"   hip / torch fp32 = {call['hip'][0] / call['torch_fp32'][0]:.2f}   hip / torch fp16 autocast = "
              f"{call['hip'][0] / call['torch_fp16_autocast'][0]:.2f}")
    print(json.dumps({"bench": "detr_encoder", "rounds": args.rounds, "inner": args.inner, "cases": result}))


if __name__ == "__main__":
    main()
