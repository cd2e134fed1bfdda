"""Timing of option mlp_pair256 by call size: ms per encode_image of the synthetic ViT-B/16 (every row of every block) for the pair launch
with c_proj on 128-row tiles (mlp_pair256 = 0) and on 256-row tiles (1), alternating, hipEvents around 20 calls each, three rounds;
bit-equality checked first.  PAIR256_CROPS: crop counts (default: from the smallest call the pair launch takes up to the headline's);
PAIR256_CHUNKS: values of mlp_pair256_chunk to time beside the default.  The threshold option mlp_pair256_min_m comes from this table
(profiles/mlp_pair256.txt)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from hoigen_amd import synth
from hoigen_amd.model import build_model

torch.set_grad_enabled(False)
d = torch.device("cuda:0")
m = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).to(d)
v = m.visual
v.set_option("last_block_row0", 0)
v(torch.zeros(1, 3, 224, 224, device=d))
default_chunk = v.get_option("mlp_pair256_chunk")
chunks = [int(c) for c in os.environ.get("PAIR256_CHUNKS", "").split()] or [default_chunk]
configs = [("128-row tiles", 0, default_chunk)] + [(f"256-row tiles chunk {c}", 1, c) for c in chunks]
for B in (int(b) for b in os.environ.get("PAIR256_CROPS", "11 16 24 40 64 96 128 192 256").split()):
    x = torch.randn(B, 3, 224, 224, device=d)
    v.set_option("mlp_pair256_min_m", 2048)
    v.set_option("mlp_pair", 0)
    want = m.encode_image(x)
    v.set_option("mlp_pair", 1)
    times = {name: [] for name, _, _ in configs}
    for rnd in range(3):
        for name, on, ch in configs:
            v.set_option("mlp_pair256", on); v.set_option("mlp_pair256_chunk", ch)
            n0 = v.get_option("mlp_pair256_launches")
            same = bool(torch.equal(m.encode_image(x), want))
            ran = v.get_option("mlp_pair256_launches") - n0
            for _ in range(3): m.encode_image(x)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20): m.encode_image(x)
            e1.record(); torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / 20)
            assert same and ran == (11 if on else 0), (B, name, same, ran)
    print(f"{B:3d} crops ({B * 197:5d} rows): " + " | ".join(f"{n}: {sorted(t)[1]:.3f} ms ({min(t):.3f} .. {max(t):.3f})" for n, t in times.items()), flush=True)
v.set_option("mlp_pair256", 1); v.set_option("mlp_pair256_chunk", default_chunk)
