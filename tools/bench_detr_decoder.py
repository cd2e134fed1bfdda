#!/usr/bin/env python3
"""Times the DETR decoder on the HIP path (hoigen_amd/detr.py) against the same layers as torch's own modules.

Three cases: B = 1 and B = 4 on a 25 x 38 memory grid (950 tokens), B = 2 on 38 x 38 (1 444 tokens), 100 queries; image 0 unpadded, the
others padded on the right and at the bottom.  For each case:

  * the whole call: hg_detr_decoder with the default FFN rule, with the two GEMMs (option detr_ffn = 1) and with the split kernel
    (detr_ffn = 2), torch's modules in fp32 (what the reference runs) and under fp16 autocast.  The variants are run in turn, round after
    round, each timed with a pair of events around `--inner` calls that end in a synchronise; median and min .. max over the rounds;
  * per layer, from the library's own event pairs (hg_profile_begin): the self-attention launch, the cross-attention launch, the five
    small GEMMs, the FFN (the split kernel, or the two GEMMs) and the row kernels; and the launches in front of the layers;
  * the workspace bytes.

Then the FFN alone through hg_test_detr_ffn at M = 100, 200, 400, 800, 950, 2888: the split kernel + its tail against the two GEMMs +
theirs, per launch from the event pairs, alternating in one process; and the whole call at B = 1, 2, 4, 8 (M = 100 B) under both.

Seeded default-initialised weights (timing does not depend on their values).  Prints a report and one JSON line.
    python tools/bench_detr_decoder.py [--rounds 7] [--inner 5]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hoigen_amd import _lib  # noqa: E402
from hoigen_amd.detr import TransformerDecoder  # noqa: E402

D, H, F, NL, Q = 256, 8, 2048, 6, 100
CASES = (("B1_25x38", 1, 25, 38), ("B4_25x38", 4, 25, 38), ("B2_38x38", 2, 38, 38))
FFN_M = (100, 200, 400, 800, 950, 2888)


class Layer(nn.Module):
    def __init__(self):
        super().__init__()
        self.self_attn, self.multihead_attn = nn.MultiheadAttention(D, H, dropout=0.1), nn.MultiheadAttention(D, H, dropout=0.1)
        self.linear1, self.linear2 = nn.Linear(D, F), nn.Linear(F, D)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(D), nn.LayerNorm(D), nn.LayerNorm(D)
        self.activation, self.normalize_before = torch.nn.functional.relu, False

    def forward(self, tgt, memory, kpm, pos, qp):
        q = k = tgt + qp
        tgt = self.norm1(tgt + self.self_attn(q, k, value=tgt)[0])
        tgt = self.norm2(tgt + self.multihead_attn(tgt + qp, memory + pos, value=memory, key_padding_mask=kpm)[0])
        return self.norm3(tgt + self.linear2(self.activation(self.linear1(tgt))))


class Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([Layer() for _ in range(NL)])
        self.norm = nn.LayerNorm(D)
        self.return_intermediate = True

    def forward(self, tgt, memory, memory_key_padding_mask=None, pos=None, query_pos=None):
        out = []
        for l in self.layers:
            tgt = l(tgt, memory, memory_key_padding_mask, pos, query_pos)
            out.append(self.norm(tgt))
        return torch.stack(out)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def in_turn(variants, rounds, inner):
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, inner))
    return {k: stat(v) for k, v in t.items()}


def stat(v):
    return (statistics.median(v), min(v), max(v))


def fmt(x):
    return f"{x[0]:8.4f} ms ({x[1]:.4f} .. {x[2]:.4f})"


def with_option(dec, value, fn):
    def run():
        dec.set_option("detr_ffn", value)
        try:
            return fn()
        finally:
            dec.set_option("detr_ffn", 0)
    return run


def layer_shares(recs, S):
    """records of one call -> ms per layer of each group (summed over the call, divided by the layers), and in front of the layers"""
    g = {"self_attention": 0.0, "cross_attention": 0.0, "small_gemms": 0.0, "ffn": 0.0, "rows": 0.0, "entry_and_kv": 0.0}
    for i, (kind, M, N, K, ms) in enumerate(recs):
        if i < 4:      # memory entry, the two stacked K / V GEMMs, the decoder entry
            g["entry_and_kv"] += ms
        elif kind == _lib.HG_PROF_ATTENTION:
            g["cross_attention" if N == S and S != Q else "self_attention"] += ms
        elif kind == _lib.HG_PROF_DETR_FFN or (kind in (2, 3) and F in (N, K)):
            g["ffn"] += ms
        elif kind == _lib.HG_PROF_DETR_ROWS:
            g["rows"] += ms
        else:
            g["small_gemms"] += ms
    return {k: (v if k == "entry_and_kv" else v / NL) for k, v in g.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    ref = Decoder().to(dev).eval()
    dec = TransformerDecoder.from_module(ref)
    lib = _lib.lib()
    result = {"cases": {}, "ffn": {}, "calls_by_rows": {}}

    def operands(B, gh, gw):
        S = gh * gw
        mem, pos = torch.randn(S, B, D, device=dev), torch.randn(S, B, D, device=dev)
        qp = torch.randn(Q, D, device=dev).unsqueeze(1).repeat(1, B, 1)
        kpm = torch.zeros(B, gh, gw, dtype=torch.bool, device=dev)
        for b in range(1, B):
            kpm[b, gh - 3 * (b % 4):], kpm[b, :, gw - 4 * (b % 4):] = True, True
        return mem, pos, qp, kpm.flatten(1), torch.zeros(Q, B, D, device=dev)

    for name, B, gh, gw in CASES:
        S = gh * gw
        mem, pos, qp, kpm, tgt = operands(B, gh, gw)
        hip = lambda: dec(tgt, mem, memory_key_padding_mask=kpm, pos=pos, query_pos=qp)
        t32 = lambda: ref(tgt, mem, memory_key_padding_mask=kpm, pos=pos, query_pos=qp)

        def t16():
            with torch.autocast("cuda", dtype=torch.float16):
                return ref(tgt, mem, memory_key_padding_mask=kpm, pos=pos, query_pos=qp)

        err = float((hip() - t32()).norm() / t32().norm())
        call = in_turn({"hip": hip, "hip_ffn_gemms": with_option(dec, 1, hip), "hip_ffn_split": with_option(dec, 2, hip), "torch_fp32": t32,
                        "torch_fp16_autocast": t16}, args.rounds, args.inner)
        handle = dec._ctx.get(dev)
        shares = {}
        for label, opt in (("split", 2), ("gemms", 1)):
            acc = []
            for _ in range(args.rounds):
                _, recs = _lib.profile(handle, _lib.HG_PROF_ALL, 128, with_option(dec, opt, hip))
                torch.cuda.synchronize()
                acc.append(layer_shares(recs, S))
            shares[label] = {k: statistics.median(a[k] for a in acc) for k in acc[0]}
        ws = C.c_uint64()
        lib.hg_workspace_bytes(handle, C.byref(ws))
        result["cases"][name] = {"call": call, "per_layer": shares, "workspace_bytes": int(ws.value), "rel_l2_vs_torch_fp32": err}
        print(f"== {name}: B {B}, {gh} x {gw} = {S} memory tokens, {Q} queries, {NL} layers; rel L2 against torch fp32 {err:.2e}; "
              f"workspace {ws.value / 2 ** 20:.1f} MiB")
        for k, v in call.items():
            print(f"   call {k:20s} {fmt(v)}")
        print(f"   hip / torch fp32 = {call['hip'][0] / call['torch_fp32'][0]:.2f}   hip / torch fp16 autocast = "
              f"{call['hip'][0] / call['torch_fp16_autocast'][0]:.2f}")
        for label, sh in shares.items():
            tot = sum(v for k, v in sh.items() if k != "entry_and_kv")
            print(f"   per layer, FFN as {label:5s}: " + "  ".join(f"{k} {v * 1000:.1f} us ({100 * v / tot:.0f} %)" for k, v in sh.items()
                                                                  if k != "entry_and_kv") + f"   | in front of the layers {sh['entry_and_kv'] * 1000:.1f} us")

    # the FFN alone, per launch, alternating
    handle = dec._ctx.get(dev)
    l0 = ref.layers[0]
    w = [t.detach().float().contiguous() for t in (l0.linear1.weight, l0.linear1.bias, l0.linear2.weight, l0.linear2.bias, l0.norm3.weight, l0.norm3.bias)]
    print("== FFN alone (hg_test_detr_ffn), us per launch: split kernel + tail | linear1 GEMM + linear2 GEMM + tail")
    for M in FFN_M:
        x, y = torch.randn(M, D, device=dev), torch.empty(M, D, device=dev)
        t = {1: [], 2: []}
        parts = {1: [], 2: []}
        for r in range(args.rounds + 1):
            for opt in (2, 1):
                lib.hg_set_option(handle, b"detr_ffn", opt)
                _, recs = _lib.profile(handle, _lib.HG_PROF_ALL, 8, lambda: lib.hg_test_detr_ffn(
                    handle, x.data_ptr(), *[a.data_ptr() for a in w], M, D, F, y.data_ptr(), None, torch.cuda.current_stream(dev).cuda_stream))
                torch.cuda.synchronize()
                assert len(recs) == (2 if opt == 2 else 3), recs
                if r:
                    t[opt].append(sum(rec[4] for rec in recs))
                    parts[opt].append([rec[4] for rec in recs])
        lib.hg_set_option(handle, b"detr_ffn", 0)
        med = {o: [statistics.median(p[i] for p in parts[o]) * 1000 for i in range(len(parts[o][0]))] for o in (1, 2)}
        result["ffn"][M] = {"split": stat(t[2]), "gemms": stat(t[1]), "split_launches_us": med[2], "gemm_launches_us": med[1]}
        print(f"   M {M:5d}: split {fmt(stat(t[2]))} = " + " + ".join(f"{v:.1f}" for v in med[2]) + f"   gemms {fmt(stat(t[1]))} = " +
              " + ".join(f"{v:.1f}" for v in med[1]))
    print("== whole call by rows (25 x 38 memory), FFN as split kernel | two GEMMs")
    for B in (1, 2, 4, 8):
        mem, pos, qp, kpm, tgt = operands(B, 25, 38)
        hip = lambda: dec(tgt, mem, memory_key_padding_mask=kpm, pos=pos, query_pos=qp)
        call = in_turn({"split": with_option(dec, 2, hip), "gemms": with_option(dec, 1, hip)}, args.rounds, args.inner)
        result["calls_by_rows"][100 * B] = call
        print(f"   M {100 * B:4d}: split {fmt(call['split'])}   gemms {fmt(call['gemms'])}")
    print(json.dumps({"bench": "detr_decoder", "rounds": args.rounds, "inner": args.inner, **result}))


if __name__ == "__main__":
    main()
