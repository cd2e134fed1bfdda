"""A call's result must not depend on the calls before it, NON-FINITE ones included.  Every native entry point works in grow-only
workspaces the context keeps between calls, several entry points share them, and the kernels read tile pad rows, padded K columns and
masked keys that the current call did not write: what an earlier, larger call left there.  Where such a leak goes through an exact
zero - a masked probability times a stale V row, a zero weight column, a zero-padded K step - finite stale data leaves every bit as it
is (tests/test_nonfinite_history_model.py), so the finite histories of tests/test_gpu_history_independence.py and of the entry points'
own "history" tests cannot see it; 0 * NaN and 0 * Inf are NaN.  One corrupt image or one overflowing batch in a long-lived process is
that history.

Every case (tests/history_cases.py: run_case): the clean call on a context that has run nothing else -> the reference, finite; on a
second fresh context poison calls whose floating-point data operands are all NaN (second parametrisation: +Inf - Inf - Inf and 0 * Inf
take other routes), then the clean call: finite and torch.equal to the reference in every returned tensor, traces included.  No
tolerance anywhere.  Asserted in every case as well: each poison call's outputs are non-finite in every row, and hg_workspace_bytes
does not change over the clean call (else ensure() would have re-zeroed a buffer).  The poison is the issue's large call - its rows lie
directly behind the clean call's last row in every buffer both use - followed, for the towers and the VAE family, by a NaN call of one
sequence / row more than the clean call: the same path as the clean call takes (a small call leaves the LayerNorm-folded path and
uses buffers of its own), so its rows lie directly behind the clean ones there too.  Boxes, labels, scores, token ids, masks, sizes,
positional inputs and counts stay valid: they steer addresses, loops and sorts.  With Inf the towers may raise their range report
(a row's reach bounded through its statistics; NaN compares false, Inf does not everywhere): the next tower call delivers
it, the case consumes it before the clean call and prints whether it came.

Models: hoigen_amd/synth.py's, cut to 2 or 3 blocks; sizes: M no multiple of 32, 128, 208 or 256.
  image tower A (ViT-B/16, 3 blocks)  poison 48 crops; clean 1 (M = 197: below the folded path), 11 (2 167), 33 crops; forms default,
                                      stream_hilo = 0, last_block_row0 = 0, qkv_attn = 0, mlp_pair = 0, mlp_pair256_min_m = 2048 (the
                                      launch counter shows the 256-row kernel ran); every row of the stream after every block
  variant C (adapters, 14 priors, a padding mask)  poison 48 crops and priors; clean 3 and 33; qkv_attn_c 0 and 1
  ViT-L/14@336px geometry (577 tokens, 2 blocks)   poison 6; clean 1 and 3; variant A, and variant C on the long adapter (option adapter_long = 1,
                                      without which hg_load_vit refuses adapters on 577 tokens)
  text tower                          prompt embeddings: poison 64 prompts of 77 tokens; clean 1, 5, 27 prompts, 77 tokens and truncated;
                                      text_ln_fold 0, 1, 2 x qkv_attn_text 0, 1; ids (with the stream trace) behind an image-tower
                                      poison on a context both towers share
  VAE (vae_fused 0, 1, 2), generator, mlp_net, cache logits   poison 4 000 rows; clean 1, 100, 300; with a finite poison that overflows
                                      fp16 behind the family's ReLU as well (PAST_RELU below says why)
  cross-entry, one context            tower poison -> VAE; VAE poison -> tower; tower poison -> mlp_net and cache logits (the clean
                                      call runs once, on finite data, before the poison: the buffers only it owns have their size)
  interaction head                    poison 2 images of 12 boxes, NaN map and global features; clean 1 image of 3 boxes, with
                                      branches (every output / logits only: the rest stays in the workspace) and without
  DETR encoder, decoder (d_model 256, 384)   poison 3 images of 13 x 17 tokens (decoder: Q = 100, tgt too); clean 2 images of 5 x 7
                                      with a key-padding mask on one, and 1 x 1 (decoder: Q = 7 and 100); detr_ffn 1 and 2 (384: the
                                      split kernel does not exist, 1 only)
  DETR neck (d_model 256: the only width above 128 it loads)   Cin 2 048, split 8 and 4; poison 3 images, clean 1
  ResNet (resnet_cases.small_resnet, both stride placements)   stages, stem, NativeBody(native_stem=True): poison 3 maps of 26 x 36 /
                                      images of 104 x 140; clean 2 x 64 x 13 x 18 and 1 x 64 x 1 x 1 / 2 x 3 x 52 x 72 and 1 x 3 x 1 x 1
Left out: region priors, detections, crop pre-processing, detector views, DETR heads - their inputs are integers, uint8 pixels or floats
that steer selection (scores, boxes), which the NaN families of their own tests do not feed either."""
import json
import os
import types

import numpy as np
import pytest
import torch

import detr_decoder_cases as dd
import detr_encoder_cases as ec
import detr_neck_cases as nc
import history_cases as hc
import hoi_head_bound as hb
import resnet_cases as rc
import roi_bound as rb
from history_cases import POISONS, dev, fresh_context, run_case
from hoigen_amd import _lib, clip, synth
from hoigen_amd.detr import TransformerDecoder, TransformerEncoder
from hoigen_amd.model import build_model
from hoigen_amd.resnet import NativeBody, ResNetStages, ResNetStem

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = pytest.mark.parametrize("poison", list(POISONS))
TOWER_OPTS = ("mlp_pair", "mlp_pair256", "mlp_pair256_min_m", "stream_hilo", "last_block_row0", "qkv_attn", "qkv_attn_c", "qkv_attn_text",
              "text_ln_fold", "adapter_long")


def randn(*shape, seed):
    return torch.randn(*shape, device=dev(), generator=torch.Generator(device=dev()).manual_seed(seed))


def full(shape, poison):
    return torch.full(tuple(shape), POISONS[poison], device=dev())


class Options:
    """the options of a façade model for the length of a test: set on entry (they survive fresh_context), the defaults back on exit"""

    def __init__(self, model, defaults, opts):
        self.model, self.defaults, self.opts = model, defaults, opts

    def __enter__(self):
        for k, v in {**self.defaults, **self.opts}.items():
            self.model.set_option(k, v)
        return {**self.defaults, **self.opts}

    def __exit__(self, *exc):
        for k, v in self.defaults.items():
            self.model.set_option(k, v)
        return False


def with_defaults(m):
    m.visual(torch.zeros(1, 3, m.visual.input_resolution, m.visual.input_resolution, device=dev()), *((None,) if m.visual.returns_local else ()))
    m.encode_text(torch.zeros(1, m.context_length, dtype=torch.int32, device=dev()))      # (creates the native contexts)
    return m, {k: m.get_option(k) for k in TOWER_OPTS}


# ---- image tower, variant A ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tower_a():
    cfg = dict(synth.VIT_B16, vision_layers=3, transformer_layers=3)
    m = build_model(synth.to_torch(synth.clip_state_dict(cfg, 0))).float().to(dev())
    m, defaults = with_defaults(m)
    yield m, defaults, randn(33, 3, 224, 224, seed=41)
    for k, v in defaults.items():
        m.set_option(k, v)


A_FORMS = {"default": {}, "fp32_stream": {"stream_hilo": 0}, "all_rows_last": {"last_block_row0": 0}, "gemm_attention": {"qkv_attn": 0},
           "two_mlp_launches": {"mlp_pair": 0}, "pair256": {"mlp_pair256_min_m": 2048}}


def image_case(m, opts, x, n, bad, key, what, poison, extra_poisons=()):
    """the clean call: n crops through encode_image (the first call behind the poison), then through forward_stream_trace ->
    (embeddings, embeddings, every row after ln_pre and every block); returns the 256-row pair kernel's launches of the traced call"""
    seen = {}

    def clean():
        prod = m.visual(x[:n])
        n0 = m.visual.get_option("mlp_pair256_launches")
        out, tr = m.visual.forward_stream_trace(x[:n])
        if opts["last_block_row0"]:
            tr[-1][n:] = 0      # (rows the hook leaves unwritten)
        seen["pair256"] = m.visual.get_option("mlp_pair256_launches") - n0
        return prod, out, tr

    run_case(key, what, lambda: fresh_context(m.visual), clean, [lambda: m.visual(bad), lambda: m.visual(bad[:n + 1]), *extra_poisons],
             lambda: m.visual._ctx.handle, report=poison == "inf")
    return seen["pair256"]


@POISON
@pytest.mark.parametrize("form", list(A_FORMS))
def test_image_tower(tower_a, form, poison):
    m, defaults, x = tower_a
    bad = full((48, 3, 224, 224), poison)
    with Options(m, defaults, A_FORMS[form]) as opts:
        for n in (1, 11, 33):
            launches = image_case(m, opts, x, n, bad, ("A", form, n), f"image tower A, {form}, {n} crops behind 48 {poison} crops", poison)
            if form == "pair256":
                assert launches == (2 if n * 197 >= 2048 else 0), f"{n} crops: {launches} launches of the 256-row pair kernel"


# ---- variant C ------------------------------------------------------------------------------------------------------------------------------
def variant_c(cfg, seed):
    raw = synth.clip_state_dict(cfg, 0)
    raw.update(synth.adapter_state_dict(cfg, seed))
    return build_model(synth.to_torch(raw), use_adapter=True).float().to(dev()).eval()


def prior_inputs(n, seed):
    mask = torch.zeros(n, 14, dtype=torch.bool, device=dev())
    mask[::2, 10:] = True
    mask[1::3, 13:] = True
    return randn(n, 14, 64, seed=seed), mask


def prior_case(m, x, pri, mask, n, n_bad, key, what, poison):
    res = m.visual.input_resolution
    bad, bad_p = full((n_bad, 3, res, res), poison), full((n_bad, 14, 64), poison)
    run_case(key, what, lambda: fresh_context(m.visual), lambda: m.visual(x[:n], (pri[:n], mask[:n])),
             [lambda: m.visual(bad, (bad_p, mask[:n_bad])), lambda: m.visual(bad[:n + 1], (bad_p[:n + 1], mask[:n + 1]))],
             lambda: m.visual._ctx.handle, report=poison == "inf")


@pytest.fixture(scope="module")
def tower_c():
    m, defaults = with_defaults(variant_c(dict(synth.VIT_B16, vision_layers=3, transformer_layers=1, vocab_size=512), 1))
    pri, mask = prior_inputs(48, 43)
    yield m, defaults, randn(33, 3, 224, 224, seed=42), pri, mask
    for k, v in defaults.items():
        m.set_option(k, v)


@POISON
@pytest.mark.parametrize("qkv_attn_c", (1, 0))
def test_variant_c(tower_c, qkv_attn_c, poison):
    m, defaults, x, pri, mask = tower_c
    with Options(m, defaults, {"qkv_attn_c": qkv_attn_c}):
        for n in (3, 33):
            prior_case(m, x, pri, mask, n, 48, ("C", qkv_attn_c, n), f"variant C, qkv_attn_c {qkv_attn_c}, {n} crops behind 48 {poison} crops", poison)


# ---- 577 tokens -------------------------------------------------------------------------------------------------------------------------------
L14 = dict(synth.VIT_L14_336, vision_layers=2, transformer_layers=1, vocab_size=512)


@pytest.fixture(scope="module")
def long_a():
    m, defaults = with_defaults(build_model(synth.to_torch(synth.clip_state_dict(L14, 0))).float().to(dev()))
    yield m, defaults, randn(3, 3, 336, 336, seed=44)


@pytest.fixture(scope="module")
def long_c():
    m = variant_c(L14, 32)
    m.set_option("adapter_long", 1)      # (hg_load_vit refuses adapters on 577 tokens without it)
    m, defaults = with_defaults(m)
    pri, mask = prior_inputs(6, 46)
    yield m, defaults, randn(3, 3, 336, 336, seed=45), pri, mask
    for k, v in defaults.items():
        m.set_option(k, v)


@POISON
def test_577_token_tower(long_a, poison):
    m, defaults, x = long_a
    bad = full((6, 3, 336, 336), poison)
    with Options(m, defaults, {}) as opts:
        for n in (1, 3):
            image_case(m, opts, x, n, bad, ("L", n), f"577-token tower, {n} crops behind 6 {poison} crops", poison)


@POISON
def test_577_token_variant_c_on_the_long_adapter(long_c, poison):
    m, defaults, x, pri, mask = long_c
    with Options(m, defaults, {}):
        for n in (1, 3):
            prior_case(m, x, pri, mask, n, 6, ("LC", n), f"577-token variant C (adapter_long 1), {n} crops behind 6 {poison} crops", poison)


# ---- text tower ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prompts(tower_a):
    m = tower_a[0]
    ids = clip.tokenize(json.load(open(f"{G}/g0_tokens.json"))["hoi600"]["text"][:64]).to(dev())
    return ids, m.token_embedding.weight.detach()[ids].float().contiguous()      # (plain indexing: no native call)


@POISON
@pytest.mark.parametrize("qkv_attn_text", (1, 0))
@pytest.mark.parametrize("text_ln_fold", (0, 1, 2))
def test_text_tower_prompt_embeddings(tower_a, prompts, text_ln_fold, qkv_attn_text, poison):
    m, defaults, _ = tower_a
    ids, emb = prompts
    bad = full(emb.shape, poison)
    was = m.truncate_text

    def embeds(p, t, truncate):
        m.truncate_text = truncate
        return m.encode_text_embeds(p, t)

    try:
        with Options(m, defaults, {"text_ln_fold": text_ln_fold, "qkv_attn_text": qkv_attn_text}):
            for truncate in (False, True):
                for n in (1, 5, 27):
                    run_case(("T", text_ln_fold, qkv_attn_text, truncate, n),
                             f"text tower, text_ln_fold {text_ln_fold}, qkv_attn_text {qkv_attn_text}, {n} prompts "
                             f"{'truncated' if truncate else 'of 77 tokens'} behind 64 {poison} prompts",
                             lambda: fresh_context(m), lambda: embeds(emb[:n], ids[:n], truncate),
                             [lambda: embeds(bad, ids, False), lambda: embeds(bad[:n + 1], ids[:n + 1], truncate)],
                             lambda: m._ctx.handle, report=poison == "inf")
    finally:
        m.truncate_text = was


@POISON
def test_text_ids_behind_an_image_tower_poison_on_a_shared_context(tower_a, prompts, poison):
    """both towers of the model on ONE native context (they share x, h, att, qkv, fc ...): 48 poisoned crops, then token ids"""
    m, defaults, x = tower_a
    ids, _ = prompts
    bad = full((48, 3, 224, 224), poison)
    own = m._ctx

    def fresh():
        fresh_context(m.visual)
        m._text_sig = None

    def clean(n):
        out, tr = m.encode_text_stream_trace(ids[:n], True)
        tr[-1][n:] = 0      # (last_block_row0 = 1: the n EOT rows, the hook leaves the rest unwritten)
        return out, tr

    try:
        m._ctx = m.visual._ctx
        with Options(m, defaults, {}):
            for n in (5, 27):
                run_case(("T-shared", n), f"text ids, {n} prompts behind 48 {poison} crops on the same context", fresh, lambda: clean(n),
                         [lambda: m.visual(bad)], lambda: m._ctx.handle, warm=lambda: clean(n), report=poison == "inf")
    finally:
        m._ctx = own
        m._text_sig = None
        fresh_context(m.visual)


# ---- VAE family, cache logits -----------------------------------------------------------------------------------------------------------------
class Raw:
    """a native context of the test's own that `fresh` replaces by a new, loaded one"""

    def __init__(self, loader):
        self.h, self.loader = None, loader

    def fresh(self):
        self.close()
        self.h = _lib.lib().hg_create(0)
        assert self.h
        self.loader(self.h)

    def close(self):
        if self.h:
            torch.cuda.synchronize()
            _lib.lib().hg_destroy(self.h)
        self.h = None


@pytest.fixture(scope="module")
def rows():
    return hc.family_rows(300, 70)


# The family's ReLU is a hardware max, which returns 0 for NaN (tests/test_gpu_vae_fused.py says so of the fused kernel and of the GEMM
# epilogue): behind it a NaN or Inf call is finite again, and what it leaves in the hidden-layer buffers is zeros.  So of a NaN / Inf
# call only the outputs no ReLU stands in front of must be non-finite (the VAE's z = mean + eps * std; cache logits have no ReLU), and
# every case adds a FINITE poison that overflows fp16 behind the ReLU: +-6e4 in every element puts a hidden unit at N(0, 2.7e4) (mlp_net:
# 6e4), of a row's 2 048 or more about 16 beyond 65 504 -> +Inf, which max keeps.
# Of that call too only what no ReLU fed with NaN stands in front of: the VAE's mean, log_var and z (its Generator output comes from the
# NaN z through a ReLU), the generator's output; mlp_net's second hidden layer turns the first one's Inf - Inf into 0 again, so no call
# can make its output non-finite: its cases assert the workspace condition and the result alone.
PAST_RELU = {"vae": (2,), "generator": (), "mlp_net": (), "cache": (0,)}
PAST_RELU_OVERFLOW = {"vae": (0, 1, 2), "generator": (0,), "mlp_net": ()}


def overflowing(n):
    return torch.where(randn(n, hc.DIM, seed=77) > 0, 6.0e4, -6.0e4).contiguous()


FAMILY = (("vae", 0), ("vae", 1), ("vae", 2), ("generator", None), ("mlp_net", None), ("cache", None))


@POISON
@pytest.mark.parametrize("entry,vae_fused", FAMILY, ids=[e if f is None else f"{e}-fused{f}" for e, f in FAMILY])
def test_vae_family_and_cache_logits(rows, entry, vae_fused, poison):
    x, eps = rows
    bad, over = full((4000, hc.DIM), poison), overflowing(4000)
    raw = Raw(lambda h: hc.load_family(h, vae_fused))
    call = lambda a, keep=None: hc.family_call(raw.h, entry, a, a, keep)
    try:
        for n in (1, 100, 300):
            poisons = [lambda: call(bad, PAST_RELU[entry]), lambda: call(bad[:n + 1], PAST_RELU[entry])]
            if entry != "cache":      # (no ReLU, no fp16 hidden layer: nothing overflows, and the NaN call is non-finite in every output)
                poisons += [lambda: call(over, PAST_RELU_OVERFLOW[entry]), lambda: call(over[:n + 1], PAST_RELU_OVERFLOW[entry])]
            run_case(("F", entry, vae_fused, n), f"{entry} (vae_fused {vae_fused}), {n} rows behind 4000 {poison} rows", raw.fresh,
                     lambda: hc.family_call(raw.h, entry, x[:n], eps[:n]), poisons, lambda: raw.h)
    finally:
        raw.close()


# ---- one entry point poisons, another runs clean: one context ------------------------------------------------------------------------------------
def shared_fresh(m, vae_fused=None):
    fresh_context(m.visual)
    hc.load_family(m.visual._sync(dev()), vae_fused)      # (the tower's weights and the family's in one context; nothing has run)


@POISON
@pytest.mark.parametrize("vae_fused", (0, 2))
def test_tower_poison_then_vae(tower_a, rows, vae_fused, poison):
    m, defaults, _ = tower_a
    x, eps = rows
    bad = full((48, 3, 224, 224), poison)
    with Options(m, defaults, {}):
        for n in (100, 300):
            clean = lambda: hc.family_call(m.visual._ctx.handle, "vae", x[:n], eps[:n])
            run_case(("X-vae", vae_fused, n), f"VAE (vae_fused {vae_fused}), {n} rows behind 48 {poison} crops of the image tower",
                     lambda: shared_fresh(m, vae_fused), clean, [lambda: m.visual(bad)], lambda: m.visual._ctx.handle, warm=clean)
    fresh_context(m.visual)      # (an Inf poison's range report dies with the context)


@POISON
def test_tower_poison_then_mlp_net_and_cache_logits(tower_a, rows, poison):
    m, defaults, _ = tower_a
    x, _ = rows
    bad = full((48, 3, 224, 224), poison)
    with Options(m, defaults, {}):
        for n in (100, 300):
            clean = lambda: hc.family_call(m.visual._ctx.handle, "mlp_net", x[:n]) + hc.family_call(m.visual._ctx.handle, "cache", x[:n])
            run_case(("X-mlp-cache", n), f"mlp_net and cache logits, {n} rows behind 48 {poison} crops of the image tower",
                     lambda: shared_fresh(m), clean, [lambda: m.visual(bad)], lambda: m.visual._ctx.handle, warm=clean)
    fresh_context(m.visual)


@POISON
def test_vae_poison_then_tower(tower_a, poison):
    m, defaults, x = tower_a
    bad, over = full((4000, hc.DIM), poison), overflowing(4000)
    with Options(m, defaults, {}) as opts:
        for n in (1, 11):
            def clean():
                out, tr = m.visual.forward_stream_trace(x[:n])
                if opts["last_block_row0"]:
                    tr[-1][n:] = 0      # (rows the hook leaves unwritten)
                return out, tr

            run_case(("X-tower", n), f"image tower A, {n} crops behind 4000 {poison} rows of the VAE", lambda: shared_fresh(m, 0), clean,
                     [lambda: hc.family_call(m.visual._ctx.handle, "vae", bad, bad, PAST_RELU["vae"]),
                      lambda: hc.family_call(m.visual._ctx.handle, "vae", over, over, PAST_RELU_OVERFLOW["vae"]),
                      lambda: hc.family_call(m.visual._ctx.handle, "mlp_net", over, None, PAST_RELU_OVERFLOW["mlp_net"])],
                     lambda: m.visual._ctx.handle, warm=clean)
    fresh_context(m.visual)


# ---- interaction head -----------------------------------------------------------------------------------------------------------------------------
HOI_C, HOI_NC, HOI_S = 64, 24, 40
HOI_BRANCHES = (("human_object", 0.5), ("union", 1.0), ("text", 2.0), ("human", 0.7), ("object", 1.3), ("global", 0.3))


def hoi_batch(sizes, humans, seed):
    b = hb.make_batch(sizes, humans, 14, 14, HOI_C, 224, seed=seed, num_classes=HOI_NC)
    # (seeded uniform boxes alone: a zero-width box pools nothing, so its rows would not show the poison)
    b["boxes"] = np.ascontiguousarray(np.concatenate([hb.image_boxes(14, 224, n, seed + 31 * i, families=False) for i, n in enumerate(sizes)]))
    b["scale"] = rb.SCALES["1/16"]
    b["feat_global"] = np.random.RandomState(seed).randn(b["B"], HOI_C).astype(np.float32)
    return b


def load_hoi_branches(h):
    """the six branches of tests/test_gpu_hoi_head.py (every source; the text branch a linear map) in cache slots 0 .. 5 of the context h"""
    g = torch.Generator().manual_seed(HOI_C)
    out, keep = [], []
    for slot, (src, scale) in enumerate(HOI_BRANCHES):
        K = 2 * HOI_C if src == "human_object" else HOI_C
        w = torch.randn(HOI_S if src != "text" else HOI_NC, K, generator=g)
        w = (w / w.norm(dim=1, keepdim=True)).to(dev()).contiguous()
        cw = _lib.hg_cache_weights()
        cw.weight, cw.S, cw.K, cw.C, cw.post_div = _lib.tensor(w), w.shape[0], K, 0, 1.0
        if src != "text":
            lab = (torch.rand(HOI_S, HOI_NC, generator=g) < 0.2).float()
            ts = [t.to(dev()).contiguous() for t in (-torch.ones(HOI_S), lab, lab.sum(0).clamp_min(1.0))]
            cw.bias, cw.labels, cw.sample_lens = (_lib.tensor(t) for t in ts)
            cw.C, cw.post_div = HOI_NC, 2.0 if src == "human_object" else 1.0
            keep += ts
        hc.ok(h, _lib.lib().hg_load_cache(h, slot, _lib.C.byref(cw)), "hg_load_cache")
        out.append(("union" if src == "text" else src, types.SimpleNamespace(slot=slot), scale))
    torch.cuda.synchronize()
    return out


HOI_FORMS = {"every_output": (True, True), "logits_only": (True, False), "pooling_only": (False, True)}


@POISON
@pytest.mark.parametrize("form", list(HOI_FORMS))
def test_interaction_head(form, poison):
    from test_gpu_hoi_head import call
    with_branches, outputs = HOI_FORMS[form]
    small, big = hoi_batch((3,), (1,), 91), hoi_batch((12, 12), (4, 4), 92)
    big["feat"] = np.full_like(big["feat"], POISONS[poison])
    big["feat_global"] = np.full_like(big["feat_global"], POISONS[poison])
    box = {}
    raw = Raw(lambda h: box.update(branches=load_hoi_branches(h)))

    def head(b, branches, outputs, keys=None):
        rc, res, intact = call(b, branches, 2.8, outputs=outputs, ctx=raw.h)
        assert rc == 0 and intact, (rc, intact, _lib.lib().hg_last_error(raw.h))
        return res if keys is None else {k: v for k, v in res.items() if k in keys}

    data = ("pooled_single", "pooled_union", "feats", "branch_logits", "logits")      # (prior comes from the scores alone: finite)
    try:
        poisons = [lambda: head(big, box["branches"] if with_branches else [], outputs, data)]
        if not with_branches:      # (the pooled means of this form go to the caller: dirty the workspace's copies as well)
            poisons.insert(0, lambda: head(big, box["branches"], False, data))
        run_case(("HOI", form), f"interaction head, {form}: 1 image of 3 boxes behind 2 images of 12 boxes with a {poison} map", raw.fresh,
                 lambda: head(small, box["branches"] if with_branches else [], outputs), poisons, lambda: raw.h)
    finally:
        raw.close()


# ---- DETR ---------------------------------------------------------------------------------------------------------------------------------------
DETR_CFG = {256: dict(d_model=256, heads=8, d_ff=2048, layers=2), 384: dict(ec.wide(384), layers=2)}
BIG_GRID, SMALL_GRID = (3, 13, 17), (2, 5, 7)


def small_mask():
    m = np.zeros((2, 35), np.uint8)
    m[1, 20:] = 1      # image 1: padding behind token 20
    return hc.to_dev(m)


@pytest.fixture(scope="module")
def detr_modules():
    out = {}
    for D, cfg in DETR_CFG.items():
        enc = TransformerEncoder(D, cfg["heads"], cfg["layers"], cfg["d_ff"])
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in ec.weights(cfg, 60 + D).items()})
        dec = TransformerDecoder(D, cfg["heads"], cfg["layers"], cfg["d_ff"], True)
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in dd.weights(cfg, 61 + D).items()})
        out[D] = (enc.to(dev()).eval(), dec.to(dev()).eval())
    return out


@POISON
@pytest.mark.parametrize("d_model", list(DETR_CFG))
def test_detr_encoder(detr_modules, d_model, poison):
    enc = detr_modules[d_model][0]
    _, big_pos = (hc.to_dev(a) for a in ec.inputs(*BIG_GRID, d_model, 601))
    bad = full(big_pos.shape, poison)
    for (B, gh, gw), mask in ((SMALL_GRID, small_mask()), ((1, 1, 1), None)):
        src, pos = (hc.to_dev(a) for a in ec.inputs(B, gh, gw, d_model, 602 + gh))
        run_case(("ENC", d_model, gh), f"DETR encoder d_model {d_model}, {B} images of {gh} x {gw} behind 3 {poison} images of 13 x 17",
                 lambda: fresh_context(enc), lambda: enc.forward_trace(src, src_key_padding_mask=mask, pos=pos),
                 [lambda: enc.forward_trace(bad, pos=big_pos)], lambda: enc._ctx.handle)


@POISON
@pytest.mark.parametrize("d_model,detr_ffn", ((256, 1), (256, 2), (384, 1)))
def test_detr_decoder(detr_modules, d_model, detr_ffn, poison):
    dec = detr_modules[d_model][1]
    qe, _, big_pos = (hc.to_dev(a) for a in dd.inputs(*BIG_GRID, 100, d_model, 611))
    bad_mem, bad_tgt = full(big_pos.shape, poison), full((100, 3, d_model), poison)
    _, mem, pos = (hc.to_dev(a) for a in dd.inputs(*SMALL_GRID, 100, d_model, 612))
    mask = small_mask()
    was = dec.get_option("detr_ffn")
    dec.set_option("detr_ffn", detr_ffn)
    try:
        for Q in (7, 100):
            run_case(("DEC", d_model, detr_ffn, Q), f"DETR decoder d_model {d_model}, detr_ffn {detr_ffn}, Q {Q} on 2 images of 5 x 7 behind Q 100 "
                     f"on 3 {poison} images of 13 x 17", lambda: fresh_context(dec),
                     lambda: dec.forward_trace(None, mem, memory_key_padding_mask=mask, pos=pos, query_pos=qe[:Q]),
                     [lambda: dec.forward_trace(bad_tgt, bad_mem, pos=big_pos, query_pos=qe)], lambda: dec._ctx.handle)
    finally:
        dec.set_option("detr_ffn", was)


@POISON
@pytest.mark.parametrize("split", (8, 4))
def test_detr_neck(split, poison):
    from test_gpu_detr_neck import load, run, set_split
    small = nc.make_case("relu", "rect", 1, 2048, 5, 7, 256, 71)
    big = nc.make_case("relu", "rect", 3, 2048, 13, 17, 256, 72)
    big.update(w=small["w"], bias=small["bias"], x=np.full_like(big["x"], POISONS[poison]))

    def loader(h):
        load(h, small)
        set_split(h, split)

    raw = Raw(loader)
    as_tensors = lambda out: {k: torch.from_numpy(v) for k, v in out.items()}
    try:
        run_case(("NECK", split), f"DETR neck, Cin 2048 in {split} slices, 1 image of 5 x 7 behind 3 {poison} images of 13 x 17", raw.fresh,
                 lambda: as_tensors(run(raw.h, small)), [lambda: torch.from_numpy(run(raw.h, big)["src"])], lambda: raw.h)
    finally:
        raw.close()


# ---- ResNet ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=(False, True), ids=("stride_on_conv2", "stride_on_conv1"))
def resnet(request):
    net = rc.small_resnet(stride_on_conv1=request.param)
    return (request.param, ResNetStages.from_module(net).to(dev()), ResNetStem.from_module(net).to(dev()),
            NativeBody.from_module(net, native_stem=True).to(dev()))


def images(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev())


@POISON
def test_resnet_stages(resnet, poison):
    s1, stages, _, _ = resnet
    bad = full((3, 64, 26, 36), poison)
    for shape in ((2, 64, 13, 18), (1, 64, 1, 1)):
        x = rc.stage_input(*shape, seed=81).to(dev())
        run_case(("RS", s1, shape), f"ResNet stages, {shape} behind {poison} maps (3, 64, 26, 36)", lambda: fresh_context(stages),
                 lambda: stages.forward_trace(x), [lambda: stages.forward_trace(bad)], lambda: stages._ctx.handle)


@POISON
def test_resnet_stem(resnet, poison):
    s1, _, stem, _ = resnet
    bad = full((3, 3, 104, 140), poison)
    for shape in ((2, 3, 52, 72), (1, 3, 1, 1)):
        x = images(*shape, seed=82)
        run_case(("RT", s1, shape), f"ResNet stem, images {shape} behind {poison} images (3, 3, 104, 140)", lambda: fresh_context(stem),
                 lambda: stem(x), [lambda: stem(bad)], lambda: stem._ctx.handle)


@POISON
def test_resnet_body(resnet, poison):
    s1, _, _, body = resnet
    bad = full((3, 3, 104, 140), poison)
    for shape in ((2, 3, 52, 72), (1, 3, 1, 1)):
        x = images(*shape, seed=83)
        run_case(("RB", s1, shape), f"ResNet body, images {shape} behind {poison} images (3, 3, 104, 140)",
                 lambda: fresh_context(body.stages, body.native_stem), lambda: body._run_body(x, want_trace=True),
                 [lambda: body._run_body(bad, want_trace=True)], lambda: body.stages._ctx.handle)
