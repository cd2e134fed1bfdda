"""The MLP pair launch with c_proj on 256 x 256 tiles and the two-phase K loop (hg_mlp_pair256p.hip, option mlp_pair256_ph2 = 1) against
the same launch on the four-phase loop (hg_mlp_pair256.hip, mlp_pair256_ph2 = 0): every row of the residual stream after every block -
through hg_test_image_stream, which returns the stream as fp32 whatever its form, so its fp16 copy, the old and new centres (mu, muc) and
the statistics (mr) of a block all show in the next block's rows - and the embeddings.  Equality, no tolerance.

Crop counts: 3 (591 rows: 3 panels, the last ragged at 79 rows, five XCDs without a panel), 11 (2 167: 9 panels, one XCD owns two),
40 (7 880: 31 panels, slots with 0, 1 and 2 c_proj tiles).  Forms: the fp32 stream (hl 0 in every pair launch); the hi / lo stream on a
three-block tower (block 0 takes and leaves hi + lo, hl 2; block 1 returns it to fp32 for the last block, hl 3); a two-block
tower whose only pair launch goes hi / lo -> fp32 (hl 3).  Every case asserts through mlp_pair256_launches that a 256-row pair launch
really ran in both arms."""
import pytest
import torch

from hoigen_amd import synth
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
OPTS = ("mlp_pair", "mlp_pair256", "mlp_pair256_ph2", "mlp_pair256_min_m", "mlp_pair256_chunk", "mlp_pair256_ratio", "stream_hilo", "last_block_row0")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def make(layers):
    cfg = dict(synth.VIT_B16, vision_layers=layers, transformer_layers=layers)
    m = build_model(synth.to_torch(synth.clip_state_dict(cfg, 0))).float().to(dev())
    m.visual(torch.zeros(1, 3, 224, 224, device=dev()))      # (creates the native context)
    return m, {k: m.visual.get_option(k) for k in OPTS}


@pytest.fixture(scope="module")
def models():
    ms = {2: make(2), 3: make(3)}
    yield ms
    for m, defaults in ms.values():
        for k, v in defaults.items():
            m.visual.set_option(k, v)


def trace(m, defaults, x, opts):
    """-> (embeddings, trace, 256-row pair launches during the call)"""
    for k, v in {**defaults, **opts}.items():
        m.visual.set_option(k, v)
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


FORMS = {"fp32": (3, {"stream_hilo": 0}), "hilo": (3, {"stream_hilo": 1}), "hilo-to-fp32": (2, {"stream_hilo": 1})}


def both_arms(models, B, form, extra=None):
    layers, opts = FORMS[form]
    m, defaults = models[layers]
    x = torch.from_numpy(synth.crops(B, 224, seed=700 + B)).to(dev())
    opts = {**opts, **(extra or {}), "mlp_pair": 1, "mlp_pair256": 1, "mlp_pair256_min_m": 256}
    want_out, want, n4 = trace(m, defaults, x, {**opts, "mlp_pair256_ph2": 0})
    out, tr, n2 = trace(m, defaults, x, {**opts, "mlp_pair256_ph2": 1})
    for k, v in defaults.items():
        m.visual.set_option(k, v)
    assert n4 == layers - 1 and n2 == layers - 1, f"{n4} / {n2} 256-row pair launches, expected one per block but the last"
    assert torch.equal(tr, want), f"B={B} {form} {extra}: the two-phase loop differs first at {first_difference(tr, want)}"
    assert torch.equal(out, want_out)


@pytest.mark.parametrize("B", [3, 11, 40])
@pytest.mark.parametrize("form", list(FORMS))
def test_two_phase_c_proj_equals_four_phase_every_row(models, B, form):
    both_arms(models, B, form)


@pytest.mark.parametrize("chunk,ratio", [(1, 3), (1, 5)])
@pytest.mark.parametrize("form", list(FORMS))
def test_two_phase_c_proj_other_chunk_and_work_ratios(models, form, chunk, ratio):
    """Panels complete in another order and the slots own other tiles: the same bits."""
    both_arms(models, 11, form, {"mlp_pair256_chunk": chunk, "mlp_pair256_ratio": ratio})


@pytest.mark.parametrize("row0", [0, 1])
def test_two_phase_c_proj_inside_encode_image_at_128_crops(models, row0):
    """128 crops (25 216 rows) take the 256-row pair launch at the default mlp_pair256_min_m: the embeddings of both loop forms."""
    m, defaults = models[3]
    x = torch.from_numpy(synth.crops(128, 224, seed=828)).to(dev())
    got = {}
    for ph2 in (0, 1):
        for k, v in {**defaults, "last_block_row0": row0, "mlp_pair256_ph2": ph2}.items():
            m.visual.set_option(k, v)
        n0 = m.visual.get_option("mlp_pair256_launches")
        got[ph2] = m.encode_image(x)
        assert m.visual.get_option("mlp_pair256_launches") - n0 == 2
    for k, v in defaults.items():
        m.visual.set_option(k, v)
    assert torch.equal(got[1], got[0])
