#!/usr/bin/env python3
"""launch_plans.json: what one tower call launches - the ordered (kind, M, N, K) records of hg_profile (HG_PROF_ALL: every GEMM,
attention, fused in_proj + attention and MLP pair launch) and hg_workspace_bytes after the call - for every path the tower runner can
take (hoigen_amd/csrc/hg_tower.hip).  Three-block towers: the fewest that show the first, middle and last form of the residual GEMMs.

The dispatch depends on the device's compute units (qkv_attn_pays, qkv_attn_text_pays, mlp_pair_ok), so this runs on an MI355X
(256 CUs), with the library built from the commit whose dispatch is to be pinned:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_launch_plans.py
tests/test_gpu_launch_plan.py imports CASES and record() from here and compares against the file.
"""
import ctypes
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from hoigen_amd import _lib, clip, synth  # noqa: E402
from hoigen_amd import model as hm  # noqa: E402

FIXTURE = os.path.join(HERE, "launch_plans.json")
B16_3 = dict(synth.VIT_B16, vision_layers=3, transformer_layers=3)
L336_3 = dict(synth.VIT_L14_336, vision_layers=3, transformer_layers=1)

# (name, model, call, size, options).  Calls: image B crops; prior / self: variant C with / without prior tokens; text T prompts x 77
# tokens; text_trunc: T prompts truncated to max(EOT) + 1 = 13 tokens; embeds_trunc: encode_text_embeds, truncated; image_stream /
# text_stream: the stream-trace hooks
CASES = [
    ("vision B2 separate LayerNorm", "b16", "image", 2, {}),
    ("vision B3 folded, no qkv_attn", "b16", "image", 3, {}),
    ("vision B40", "b16", "image", 40, {}),
    ("vision B40 qkv_attn=0", "b16", "image", 40, {"qkv_attn": 0}),
    ("vision B40 qkv_attn=2", "b16", "image", 40, {"qkv_attn": 2}),
    ("vision B40 ln_fuse=0", "b16", "image", 40, {"ln_fuse": 0}),
    ("vision B40 stream_hilo=0", "b16", "image", 40, {"stream_hilo": 0}),
    ("vision B40 mlp_pair=0", "b16", "image", 40, {"mlp_pair": 0}),
    ("vision B40 last_block_row0=0", "b16", "image", 40, {"last_block_row0": 0}),
    ("vision L336 B2", "l336", "image", 2, {}),
    ("variant C B40 priors", "b16c", "prior", 40, {}),
    ("variant C B40 self", "b16c", "self", 40, {}),
    ("variant C B40 adapter_fold=0", "b16c", "prior", 40, {"adapter_fold": 0}),
    ("variant C B40 adapter_fuse=0", "b16c", "prior", 40, {"adapter_fuse": 0}),
    ("variant C B40 stream_hilo=0", "b16c", "prior", 40, {"stream_hilo": 0}),
    ("variant C B40 qkv_attn_c=0", "b16c", "prior", 40, {"qkv_attn_c": 0}),
    ("variant C B40 adapters on blocks 0, 2", "b16c02", "prior", 40, {}),
    ("text 8x77", "b16", "text", 8, {}),
    ("text 600x13", "b16", "text_trunc", 600, {}),
    ("text 600x13 text_ln_fold=0", "b16", "text_trunc", 600, {"text_ln_fold": 0}),
    ("text 600x13 text_ln_fold=2", "b16", "text_trunc", 600, {"text_ln_fold": 2}),
    ("text 600x13 qkv_attn_text=2", "b16", "text_trunc", 600, {"qkv_attn_text": 2}),
    ("text 600x13 qkv_attn_text=2 text_ln_fold=2", "b16", "text_trunc", 600, {"qkv_attn_text": 2, "text_ln_fold": 2}),
    ("text 8x77 qkv_attn_text=2", "b16", "text", 8, {"qkv_attn_text": 2}),
    ("text 600x13 qkv_attn_text=1", "b16", "text_trunc", 600, {"qkv_attn_text": 1}),
    ("text 600x13 mlp_pair=0", "b16", "text_trunc", 600, {"mlp_pair": 0}),
    ("text 600x13 last_block_row0=0", "b16", "text_trunc", 600, {"last_block_row0": 0}),
    ("text embeds 600x13", "b16", "embeds_trunc", 600, {}),
    ("image stream trace B40", "b16", "image_stream", 40, {}),
    ("image stream trace B40 last_block_row0=0", "b16", "image_stream", 40, {"last_block_row0": 0}),
    ("image stream trace B40 stream_hilo=0", "b16", "image_stream", 40, {"stream_hilo": 0}),
    ("text stream trace 600x13", "b16", "text_stream", 600, {}),
    ("text stream trace 600x13 last_block_row0=0", "b16", "text_stream", 600, {"last_block_row0": 0}),
]

_models = {}
_crops = {}


def _variant_c(cfg, layers):
    sd = synth.to_torch(synth.clip_state_dict(cfg, 0))
    sd.update(synth.to_torch(synth.adapter_state_dict(cfg, 1, layers=layers)))
    for key in ("input_resolution", "context_length", "vocab_size"):
        sd.pop(key, None)
    m = hm.CLIP(**hm._infer_config(sd), variant_c=True, adapter_layers=list(layers))
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if "adaptermlp" in k], (unexpected, missing)
    return m


def model(name):
    if name not in _models:
        if name == "b16":
            m = hm.build_model(synth.to_torch(synth.clip_state_dict(B16_3, 0))).float()
        elif name == "l336":
            m = hm.build_model(synth.to_torch(synth.clip_state_dict(L336_3, 0))).float()
        elif name == "b16c":
            m = _variant_c(B16_3, range(3))
        else:
            m = _variant_c(B16_3, [0, 2])
        _models[name] = m.to(torch.device("cuda:0")).eval()
    return _models[name]


def release():
    for m in _models.values():
        for owner in (m.visual, m):
            owner._ctx.close()
    _models.clear()
    _crops.clear()


def _prompts(n):
    g0 = json.load(open(os.path.join(HERE, "g0_tokens.json")))
    return clip.tokenize(g0["hoi600"]["text"][:n]).to(torch.device("cuda:0"))


@torch.no_grad()
def record(case):
    """Run the case's one call in a FRESH native context (weights loaded, options applied, workspace empty) under the profiler.
    -> {"launches": [[kind, M, N, K], ...], "workspace_bytes": bytes}"""
    _, mname, call, n, opts = case
    m = model(mname)
    dev = torch.device("cuda:0")
    vision = call in ("image", "prior", "self", "image_stream")
    owner = m.visual if vision else m
    for o in (m.visual, m):      # a fresh context for this case: weights are handed over again on the next call
        o._ctx.close()
        o._ctx.options = dict(opts)
    m.visual._loaded_sig = m.visual._adapter_sig = m._text_sig = None
    if vision:
        res = m.visual.input_resolution
        if (n, res) not in _crops:
            _crops[n, res] = torch.from_numpy(synth.crops(n, res, seed=300 + n)).to(dev)
        x = _crops[n, res]
        prior = None
        if call == "prior":
            pri, mask = synth.priors(n, n=14, dim=64, n_pad=4, seed=99)
            prior = (torch.from_numpy(pri).to(dev), torch.from_numpy(mask).to(dev))
        handle = m.visual._sync(dev)
        if call == "image_stream":
            fn = lambda: m.visual.forward_stream_trace(x)
        elif call == "image":
            fn = lambda: m.visual(x)
        else:
            fn = lambda: m.visual(x, prior)
    else:
        ids = _prompts(n)
        handle = m._sync_text(dev)
        m.truncate_text = call != "text"
        if call == "text_stream":
            fn = lambda: m.encode_text_stream_trace(ids, True)
        elif call == "embeds_trunc":
            emb = m.token_embedding(ids).float()
            fn = lambda: m.encode_text_embeds(emb, ids)
        else:
            fn = lambda: m.encode_text(ids)
    try:
        _, recs = _lib.profile(handle, _lib.HG_PROF_ALL, 512, fn)
        torch.cuda.synchronize()
    finally:
        m.truncate_text = True
    assert handle == owner._ctx.handle
    ws = ctypes.c_uint64()
    owner._ctx.check(_lib.lib().hg_workspace_bytes(handle, ctypes.byref(ws)), "hg_workspace_bytes")
    for o in (m.visual, m):
        o._ctx.options = {}
    return {"launches": [list(r[:4]) for r in recs], "workspace_bytes": int(ws.value)}


def main():
    out = {}
    for case in CASES:
        out[case[0]] = record(case)
        print(f"{case[0]}: {len(out[case[0]]['launches'])} launches, {out[case[0]]['workspace_bytes']} workspace bytes", flush=True)
    release()
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in out.items()) + "\n}\n")
    print("wrote", FIXTURE)


if __name__ == "__main__":
    main()
