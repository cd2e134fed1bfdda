"""The MLP pair launch with c_proj on 256 x 256 tiles (hg_mlp_pair256.hip, option mlp_pair256) against the two launches (mlp_pair = 0)
and against the pair launch on ring2's 128-row tiles (mlp_pair256 = 0): every row of the residual stream after every block, bit for bit,
and the embeddings - through hg_test_image_stream / hg_test_text_stream and encode_image.

A three-block ViT-B/16 (synthetic weights): its two pair launches are the stream's forms - with the hi / lo stream block 0 takes and
leaves hi + lo (hl 2) and block 1 returns the stream to fp32 for the last block (hl 3); with stream_hilo = 0 both are fp32 (hl 0).
Crop counts: 11 (2 167 rows: the chip's last panel is ONE ragged 128-row half), 12 (2 364: a ragged second half), 13 (2 561: a last
panel of one row), 40 (7 880: the shape the launch plans pin).  Every case asserts through the read-only option mlp_pair256_launches that
the new kernel really ran (its profiler record is the pair launch's).  The text tower keeps the 128-row kernel - no gamma form in the
new one -, and its cases say so in their names."""
import json
import os

import pytest
import torch

from hoigen_amd import clip, synth
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPTS = ("mlp_pair", "mlp_pair256", "mlp_pair256_min_m", "mlp_pair256_chunk", "mlp_pair256_ratio", "mlp_pair_chunk", "mlp_pair_fc_slots", "stream_hilo", "last_block_row0", "text_ln_fold")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model():
    cfg = dict(synth.VIT_B16, vision_layers=3, transformer_layers=3)
    m = build_model(synth.to_torch(synth.clip_state_dict(cfg, 0))).float().to(dev())
    m.visual(torch.zeros(1, 3, 224, 224, device=dev()))      # (creates the native contexts)
    m.encode_text(torch.zeros(1, 77, dtype=torch.int32, device=dev()))
    defaults = {k: m.get_option(k) for k in OPTS}
    yield m, defaults
    for k, v in defaults.items():
        m.set_option(k, v)


def set_opts(m, defaults, opts):
    for k, v in {**defaults, **opts}.items():
        m.set_option(k, v)


def vision_trace(m, defaults, x, opts):
    """-> (embeddings, trace, launches of the new kernel during the call)"""
    set_opts(m, defaults, opts)
    n0 = m.visual.get_option("mlp_pair256_launches")
    out, tr = m.visual.forward_stream_trace(x)
    if {**defaults, **opts}["last_block_row0"]:
        tr[-1][x.shape[0]:] = 0      # (rows the hook leaves unwritten)
    return out, tr, m.visual.get_option("mlp_pair256_launches") - n0


def first_difference(a, b):
    for e in range(a.shape[0]):
        rows = (a[e] != b[e]).any(dim=-1).nonzero()
        if rows.numel():
            r = int(rows[0])
            return f"entry {e}, row {r} (256-row panel {r // 256}, XCD {r // 256 % 8}, 128-row half {r // 128})"
    return "no row"


@pytest.mark.parametrize("B", [11, 12, 13, 40])
@pytest.mark.parametrize("form", [{}, {"stream_hilo": 0}, {"last_block_row0": 0}], ids=["hilo", "fp32", "hilo-allrows"])
def test_pair256_equals_two_launches_and_pair128_every_row(model, B, form):
    m, defaults = model
    x = torch.from_numpy(synth.crops(B, 224, seed=500 + B)).to(dev())
    want_out, want, n = vision_trace(m, defaults, x, {**form, "mlp_pair": 0})
    assert n == 0
    out128, tr128, n = vision_trace(m, defaults, x, {**form, "mlp_pair": 1, "mlp_pair256": 0})
    assert n == 0
    assert torch.equal(tr128, want) and torch.equal(out128, want_out)
    out, tr, n = vision_trace(m, defaults, x, {**form, "mlp_pair": 1, "mlp_pair256": 1, "mlp_pair256_min_m": 2048})
    assert n == 2, f"{n} launches of mlp_pair256_kernel, expected one per block but the last"
    assert torch.equal(tr, want), f"B={B} {form}: differs from the two launches first at {first_difference(tr, want)}"
    assert torch.equal(out, want_out)
    set_opts(m, defaults, {})


def test_pair256_other_chunks_and_work_ratios(model):
    """(mlp_pair256_chunk, mlp_pair256_ratio) away from the defaults - the panels complete in another order, the slots own other tiles -
    and the 128-row kernel's own knobs, which the new kernel ignores: the same bits."""
    m, defaults = model
    x = torch.from_numpy(synth.crops(40, 224, seed=540)).to(dev())
    want_out, want, _ = vision_trace(m, defaults, x, {"mlp_pair": 0})
    for chunk, ratio in ((1, 4), (3, 1), (32, 8)):
        out, tr, n = vision_trace(m, defaults, x, {"mlp_pair256_min_m": 2048, "mlp_pair256_chunk": chunk, "mlp_pair256_ratio": ratio,
                                                   "mlp_pair_chunk": 3, "mlp_pair_fc_slots": 24})
        assert n == 2
        assert torch.equal(tr, want), f"chunk {chunk} ratio {ratio}: differs first at {first_difference(tr, want)}"
        assert torch.equal(out, want_out)
    set_opts(m, defaults, {})


def test_pair256_min_m_keeps_small_calls_on_pair128(model):
    m, defaults = model
    x = torch.from_numpy(synth.crops(11, 224, seed=511)).to(dev())
    _, want, _ = vision_trace(m, defaults, x, {"mlp_pair": 0})
    _, tr, n = vision_trace(m, defaults, x, {"mlp_pair256_min_m": 2168})
    assert n == 0 and torch.equal(tr, want)
    _, tr, n = vision_trace(m, defaults, x, {"mlp_pair256_min_m": 2167})
    assert n == 2 and torch.equal(tr, want)
    set_opts(m, defaults, {})


def test_pair256_inside_encode_image(model):
    m, defaults = model
    x = torch.from_numpy(synth.crops(40, 224, seed=541)).to(dev())
    set_opts(m, defaults, {"mlp_pair": 0})
    want = m.encode_image(x)
    set_opts(m, defaults, {"mlp_pair256_min_m": 2048})
    n0 = m.visual.get_option("mlp_pair256_launches")
    got = m.encode_image(x)
    assert m.visual.get_option("mlp_pair256_launches") - n0 == 2
    assert torch.equal(got, want)
    set_opts(m, defaults, {})


@pytest.mark.parametrize("T,truncate", [(600, True), (27, False)], ids=["600x13", "27x77"])
@pytest.mark.parametrize("fold", [1, 2])
def test_text_tower_stays_on_pair128_with_mlp_pair256_on(model, T, truncate, fold):
    """The text tower (width 512) with the next LayerNorm's weight in the activation copy (text_ln_fold = 1: the gamma instances of
    hg_mlp_pair.hip) or folded into the weights (2).  Option mlp_pair256 = 1 must leave it on that kernel (no launch of the new one) and
    on its bits."""
    m, defaults = model
    ids = clip.tokenize(json.load(open(f"{G}/g0_tokens.json"))["hoi600"]["text"][:T]).to(dev())
    set_opts(m, defaults, {"text_ln_fold": fold, "mlp_pair": 0})
    want_out, want = m.encode_text_stream_trace(ids, truncate)
    set_opts(m, defaults, {"text_ln_fold": fold, "mlp_pair": 1, "mlp_pair256": 1, "mlp_pair256_min_m": 2048})
    n0 = m.get_option("mlp_pair256_launches")
    out, tr = m.encode_text_stream_trace(ids, truncate)
    n = m.get_option("mlp_pair256_launches") - n0
    want[-1][T:] = 0      # (last_block_row0 = 1: the last entry holds the T EOT rows, the hook leaves the rest unwritten)
    tr[-1][T:] = 0
    assert torch.equal(out, want_out) and torch.equal(tr, want)
    assert n == 0, "the text tower is left on the 128-row kernel"
    set_opts(m, defaults, {})
