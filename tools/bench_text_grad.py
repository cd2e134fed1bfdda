#!/usr/bin/env python
"""Time the differentiable text tower in one process: forward + backward of vae.TextEncoder(differentiable=True)
(hg_encode_text_embeds_save + hg_text_backward_embeds) against torch autograd over torch's own modules (nn.MultiheadAttention,
nn.LayerNorm, nn.Linear) holding the same weights in fp32 on the same GPU, for 256 prompts of 16 and of 77 tokens on ViT-B/16's text
tower (width 512, 12 blocks).

    python tools/bench_text_grad.py [--reps 30] [--out profiles/text_grad.txt]

Device events around each arm, arms alternating within a round, every shape warmed up for 5 rounds, median and range (min .. max) over
--reps rounds.  The events bracket the Python call, so a figure includes the host's time to enqueue the call's launches.  Then one
profiled native call per shape (hg_profile_begin / hg_profile_end around every GEMM, attention, attention-backward and row launch): the
share of each kind of launch in the sum of the launch times, forward and backward together."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from hoigen_amd import _lib, synth, vae      # noqa: E402
from hoigen_amd.model import build_model     # noqa: E402

KINDS = {0: "GEMM fp16 out (qkv, u, df, da)", 1: "GEMM QuickGELU fp16 out", 3: "GEMM residual fp32", 4: "GEMM fp32 out (dh1, dh2, tail)",
         8: "GEMM folded LN fp16 out", 9: "GEMM folded LN QuickGELU", 10: "GEMM residual + LN emit", 100: "attention forward",
         101: "fused in_proj + attention", 103: "MLP pair launch (c_fc, QuickGELU, c_proj)", 110: "attention backward", 111: "row / elementwise (backward)"}


class TorchBlock(nn.Module):
    def __init__(self, D, heads):
        super().__init__()
        self.ln_1, self.ln_2 = nn.LayerNorm(D), nn.LayerNorm(D)
        self.attn = nn.MultiheadAttention(D, heads, batch_first=True)
        self.c_fc, self.c_proj = nn.Linear(D, 4 * D), nn.Linear(4 * D, D)

    def forward(self, x, mask):
        h = self.ln_1(x)
        x = x + self.attn(h, h, h, need_weights=False, attn_mask=mask)[0]
        u = self.c_fc(self.ln_2(x))
        return x + self.c_proj(u * torch.sigmoid(1.702 * u))


class TorchText(nn.Module):
    """the text tower of clipnet/model.py:339-352 on embedded prompts, torch modules, fp32"""

    def __init__(self, m):
        super().__init__()
        D, heads = m.transformer.width, m.transformer.heads
        self.blocks = nn.ModuleList(TorchBlock(D, heads) for _ in range(m.transformer.layers))
        self.ln_final = nn.LayerNorm(D)
        sd = {k: v.float() for k, v in m.state_dict().items()}
        with torch.no_grad():
            for i, b in enumerate(self.blocks):
                p = f"transformer.resblocks.{i}."
                b.ln_1.weight.copy_(sd[p + "ln_1.weight"]); b.ln_1.bias.copy_(sd[p + "ln_1.bias"])
                b.ln_2.weight.copy_(sd[p + "ln_2.weight"]); b.ln_2.bias.copy_(sd[p + "ln_2.bias"])
                b.attn.in_proj_weight.copy_(sd[p + "attn.in_proj_weight"]); b.attn.in_proj_bias.copy_(sd[p + "attn.in_proj_bias"])
                b.attn.out_proj.weight.copy_(sd[p + "attn.out_proj.weight"]); b.attn.out_proj.bias.copy_(sd[p + "attn.out_proj.bias"])
                b.c_fc.weight.copy_(sd[p + "mlp.c_fc.weight"]); b.c_fc.bias.copy_(sd[p + "mlp.c_fc.bias"])
                b.c_proj.weight.copy_(sd[p + "mlp.c_proj.weight"]); b.c_proj.bias.copy_(sd[p + "mlp.c_proj.bias"])
            self.ln_final.weight.copy_(sd["ln_final.weight"]); self.ln_final.bias.copy_(sd["ln_final.bias"])
        self.pos = nn.Parameter(sd["positional_embedding"].clone())
        self.proj = nn.Parameter(sd["text_projection"].clone())

    def forward(self, prompts, eot):
        L = prompts.shape[1]
        x = prompts + self.pos[:L]
        mask = torch.full((L, L), float("-inf"), device=x.device).triu(1)
        for b in self.blocks:
            x = b(x, mask)
        return self.ln_final(x[torch.arange(x.shape[0], device=x.device), eot]) @ self.proj


def timed(arms, reps, warmup=5):
    out = {k: [] for k in arms}
    for r in range(warmup + reps):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                out[k].append(a.elapsed_time(b))
    return out


def cell(v):
    return f"{statistics.median(v):8.3f} ({min(v):7.3f} .. {max(v):7.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(synth.VIT_B16, vision_layers=1)
    m = build_model(synth.to_torch(synth.clip_state_dict(cfg, 0))).float().to(dev)
    m.requires_grad_(False)
    ref = TorchText(m).to(dev)
    ref.requires_grad_(False)
    te = vae.TextEncoder(m, differentiable=True)
    lines = ["TextEncoder forward + backward to the prompts, ViT-B/16 text tower (width 512, 12 blocks), 256 prompts: ms, median (min .. max) of "
             f"{args.reps}; torch = autograd over nn.MultiheadAttention / nn.LayerNorm / nn.Linear, fp32, the same weights",
             "  tokens |                         native                          torch torch/native   rel L2 of the gradients"]
    R = 256
    for L in (16, 77):
        gen = torch.Generator().manual_seed(L)
        ids = torch.randint(1, 49000, (R, 77), generator=gen)
        ids[:, L - 1] = 49407
        ids[:, L:] = 0
        ids = ids.to(dev)
        eot = ids.argmax(-1)
        with torch.no_grad():
            prompts = m.token_embedding(ids).float()
        go = (torch.randn(R, cfg["embed_dim"], generator=gen) / R).to(dev)
        grads = {}

        def native():
            p = prompts.detach().requires_grad_()
            te(p, ids).backward(go)
            grads["native"] = p.grad

        def torch_arm():
            p = prompts.detach().requires_grad_()
            ref(p[:, :L], eot).backward(go)
            grads["torch"] = p.grad

        with torch.enable_grad():
            t = timed({"native": native, "torch": torch_arm}, args.reps)
            a, b = grads["native"][:, :L].double(), grads["torch"][:, :L].double()
            lines.append(f"  {L:6d} | {cell(t['native'])} {cell(t['torch'])} {statistics.median(t['torch']) / statistics.median(t['native']):12.2f}"
                         f"   {float((a - b).norm() / b.norm()):.2e}")
            _, recs = _lib.profile(m._ctx.handle, _lib.HG_PROF_ALL, 4096, native)
        total = sum(r[4] for r in recs)
        by = {}
        for kind, _, _, _, ms in recs:
            by.setdefault(kind, [0, 0.0])
            by[kind][0] += 1
            by[kind][1] += ms
        lines.append(f"    one profiled native call at {L} tokens: {len(recs)} launches, {total:.3f} ms in launches")
        for kind, (n, ms) in sorted(by.items(), key=lambda kv: -kv[1][1]):
            lines.append(f"      {KINDS.get(kind, 'kind %d' % kind):38s} {n:4d} launches {ms:8.3f} ms {100 * ms / total:5.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
