"""The crop pre-processing kernels (hg_preproc.hip) through CropPreprocessor, bit for bit against oracle/preprocess_oracle.py on every
case of tests/preproc_cases.py: n_px 31 .. 518 (one, two and three trips of the tables loop), up- and downscales side by side in one
call, identity passes, boxes across and outside every image edge, square padding with a three-valued background, stretch, both
normalisations, 1 and 33 boxes, with and without the uint8 output.

    uint8 crops   array_equal
    fp32 planes   array_equal (as int32 bit patterns): the kernel's 3 x 256 table is the oracle's ((u / 255) - mean) / sd

tests/test_preproc_model.py proves on the CPU which wrong kernels these cases reject.  File total on an MI355X: about 6 s, nearly all
of it the oracle on the CPU; the slowest case (geo257) takes 1.4 s."""
import numpy as np
import pytest
import torch

import preproc_cases as pc
from hoigen_amd import preprocess

pytestmark = pytest.mark.gpu


def run(c, dev, return_u8):
    pre = preprocess.CropPreprocessor(c["n_px"], c["pad_square"], c["background"], c["stretch"], c["imagenet_norm"])
    img = torch.from_numpy(pc.image(c["image"])).to(dev)
    got = pre(img, c["boxes"], return_u8=return_u8)
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES])
def test_bit_for_bit(name):
    c = pc.BY_NAME[name]
    dev = torch.device("cuda:0")
    want_u8, want_f = pc.expected(name)
    if c["return_u8"]:
        out, u8 = run(c, dev, True)
        bad = int((u8.cpu().numpy() != want_u8).sum())
        assert bad == 0, f"{bad} uint8 values differ from the oracle"
    else:
        out = run(c, dev, False)
    assert out.shape == want_f.shape and out.dtype == torch.float32
    got = out.cpu().numpy()
    bad = got.view(np.int32) != want_f.view(np.int32)
    assert not bad.any(), (f"{int(bad.sum())} fp32 values are not the oracle's bits; first at {np.argwhere(bad)[0].tolist()}: "
                           f"{got[bad][0]!r} for {want_f[bad][0]!r}")


@pytest.mark.parametrize("name", ["geo31", "pad257_stretch"])
def test_return_u8_changes_nothing(name):
    """the fp32 planes of a call without the uint8 output are those of the call with it"""
    c = pc.BY_NAME[name]
    dev = torch.device("cuda:0")
    with_u8, _ = run(c, dev, True)
    assert torch.equal(with_u8.view(torch.int32), run(c, dev, False).view(torch.int32))


def test_calls_do_not_depend_on_the_scratch_left_behind():
    """a small call behind a large one (the scratch and the tables keep the large call's bytes) and the large one again"""
    dev = torch.device("cuda:0")
    for name in ("pad257_stretch", "one_box_31", "mixed31_stretch", "pad257_stretch"):
        c = pc.BY_NAME[name]
        _, u8 = run(c, dev, True)
        assert np.array_equal(u8.cpu().numpy(), pc.expected(name)[0]), name
