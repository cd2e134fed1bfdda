"""The instance adapter of variant C (hg_adapter.hip; run_adapter in hg_tower.hip) launch by launch against float64, through hg_test_adapter:
every path (separate / LayerNorm-folded / folded into the block's GEMMs; MFMA decoder / fp32 one-lane-per-token kernels; down_proj as its
own GEMM / inside the decoder), sequence lengths 1 .. 224, prior counts 1 .. 64 and masks that are no suffix.

Reference: oracle.clip_oracle.adapter in float64 (CLIP_models_adapter_prior2.py:183-203).  What is compared is the UPDATE a = y - x (mode 2:
a = Q e), row by row, never the stream.  Bound: tests/test_adapter_rounding_model.py restates the design with fp16 roundings where the
kernels stage fp16; a kernel may show twice that model's worst-row error and 1.5 x its median row on the same inputs (`rule`), the LayerNorm
statistics the same against the kernels' own formulas in float32 numpy.  Every case is launched twice (bit-identical) and its sequences
again one by one (mode 1, which needs 512 rows: every sequence one place on).  Modes 1 and 2 run with the fp16 copy centred on the row's
mean (as in front of a tower's first block) and on a centre away from it (as behind every other block's residual GEMM).

Worst ratios seen on an MI355X over all cases below (kernel error / model error: worst row, median row; allowed 2.0, 1.5) - the table
in DESIGN.md 4:

    mode  decoder  update a     z            mean         rstd
    0     MFMA     1.00  1.01   -            -            -
    0     lanes    1.00  1.00   -            -            -
    1     MFMA     1.05  1.00   -            1.56  1.09   1.52  1.11
    1     lanes    1.00  1.00   -            1.30  1.11   1.32  1.10
    2     MFMA     1.13  1.01   1.11  1.02   1.15  1.18   1.04  1.04

The errors themselves: a row of the update is 4e-4 .. 1.2e-3 off float64 (median 5e-4 .. 8e-4) on unit-normal and small-spread streams.  With
three channels 67 x the rest and the sequence as its own memory single rows are far worse, in the kernel and in the model alike (ratio 1.00):
worst row 2.5e-2 in mode 0 at L = 65 (1.4e-2 at L = 197) and 1.3e-2 / 1.0e-2 in modes 1 and 2, whose centred copy rounds the outlier
channels better; medians 7e-4 .. 9e-4.  That is the fp16 design, not an error of a kernel.  Statistics: 1e-8 .. 3e-5 of a normalised
value (mean), 1e-7 .. 1.6e-4 (rstd; the 1e-4 are the small-spread stream through the folded update).
The file (169 tests) takes 7 s on an MI355X.
"""
import numpy as np
import pytest
import torch

import test_adapter_rounding_model as rm
from hoigen_amd import synth
from hoigen_amd.model import build_model

pytestmark = pytest.mark.gpu
P0 = rm.PRE.format(0)
LENGTHS = (1, 5, 16, 17, 31, 32, 33, 64, 65, 100, 160, 161, 192, 193, 197, 223, 224)
SEEN = {}          # (mode, decoder, observable) -> [worst ratio, median ratio]
PATHS = set()      # (mode, mfma, down_fused) exercised


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _tower(width, num_layers=1):
    cfg = dict(synth.TINY, vision_width=width)
    raw = synth.clip_state_dict(cfg, 10)
    raw.update(synth.adapter_state_dict(cfg, 13, num_layers=num_layers))
    m = build_model(synth.to_torch(raw), use_adapter=True, adapter_pos="all", adapter_num_layers=num_layers).float().to(dev())
    sd, pre = rm.weights(cfg, 13, num_layers)
    assert pre == P0
    return m.visual, sd


@pytest.fixture(scope="module")
def t256():
    return _tower(256)


@pytest.fixture(scope="module")
def t256x2():
    return _tower(256, 2)


@pytest.fixture(scope="module")
def t768():
    return _tower(768)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nadapter: worst kernel / model ratios (worst row, median row)")
    for k in sorted(SEEN):
        print(f"  mode {k[0]} {k[1]:5s} {k[2]:6s} {SEEN[k][0]:.2f} {SEEN[k][1]:.2f}")
    print("  paths (mode, mfma, down_fused):", sorted(PATHS))


def n_seq_for(mode, L):
    return max(3, -(-512 // L)) if mode == 1 else 3


def judge(key, kernel_rows, model_rows, what):
    ok, rw, rmed = rm.rule(kernel_rows, model_rows)
    s = SEEN.setdefault(key, [0.0, 0.0])
    s[0], s[1] = max(s[0], rw), max(s[1], rmed)
    print(f"\n{what} {key[2]}: kernel worst {np.max(kernel_rows):.3e} median {np.median(kernel_rows):.3e} | model worst "
          f"{np.max(model_rows):.3e} median {np.median(model_rows):.3e} | ratios {rw:.2f} {rmed:.2f}")
    assert ok, (f"{what} {key[2]}: worst row {np.max(kernel_rows):.3e} = {rw:.2f} x the model's (allowed {rm.WORST}), median "
                f"{np.median(kernel_rows):.3e} = {rmed:.2f} x (allowed {rm.MEDIAN})")


def launch(vis, mode, x, prior, centre=None):
    xd = x.to(dev())
    pd = None if prior is None else (prior[0].to(dev()), prior[1].to(dev()))
    res = vis.adapter_launch(0, mode, xd, pd, None if centre is None else centre.to(dev()))
    torch.cuda.synchronize()
    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def same(r1, r2, rows=slice(None), rows2=slice(None)):
    per_row = [k for k in r1 if isinstance(r1[k], torch.Tensor) and k != "q"]      # (q belongs to the weights, not to a row)
    return all(torch.equal(r1[k][rows], r2[k][rows2]) for k in per_row) and ("q" not in r1 or torch.equal(r1["q"], r2["q"]))


def run_case(tower, mode, x, prior, what, mfma=True, fused=False, centre=None):
    vis, sd = tower
    n_seq, L, D = x.shape
    res = launch(vis, mode, x, prior, centre)
    assert (res["mfma"], res["down_fused"]) == (mfma, fused), f"{what}: ran mfma={res['mfma']} down_fused={res['down_fused']}"
    PATHS.add((mode, mfma, fused))
    # ---- determinism: the same launch again, and every sequence apart from its neighbours
    assert same(res, launch(vis, mode, x, prior, centre)), f"{what}: two launches differ"
    if mode == 1:      # (512 rows are needed: every sequence one place on, among other neighbours)
        rot = launch(vis, mode, x.roll(1, 0), None if prior is None else (prior[0].roll(1, 0), prior[1].roll(1, 0)),
                     None if centre is None else centre.roll(1, 0))
        for i in range(n_seq):
            j = (i + 1) % n_seq
            assert same(res, rot, slice(i * L, i * L + L), slice(j * L, j * L + L)), f"{what}: sequence {i} depends on its place"
    else:
        for i in range(n_seq):
            one = launch(vis, mode, x[i:i + 1], None if prior is None else (prior[0][i:i + 1], prior[1][i:i + 1]),
                         None if centre is None else centre[i:i + 1])
            assert same(res, one, slice(i * L, i * L + L)), f"{what}: sequence {i} differs from a launch of it alone"
    # ---- the update against float64
    z_ref, a_ref = rm.oracle_parts(x, sd, P0, prior)
    mdl = rm.model(x, sd, P0, prior, mode, lanes=not mfma, centre=centre)
    dec = "mfma" if mfma else "lanes"
    x2 = x.reshape(-1, D)
    if mode == 2:
        e = res["out"].double()
        assert torch.equal(e[:, 63], torch.ones(n_seq * L, dtype=torch.float64)), f"{what}: e[63] != 1"
        # Q as the block's GEMMs hold it: the float64 Q (tests/test_adapter_fold_math.py) from the fp16 up_proj weight, one fp16 rounding
        # of an fp32 product away - the odd entry rounds the other way than the float64 value does, so the device's own Q it is
        q16, q64 = res["q"].double(), rm.q_matrix(sd, P0, prior, rnd=False, w_up16=True)
        qtol = q64.abs() * 2.0 ** -11 + 2.0 ** -25 + 1e-6      # (1e-6: the 64-term fp32 sum of column 63, terms of 1e-2)
        assert bool(((q16 - q64).abs() <= qtol).all()), f"{what}: Q is off its float64 value by {float(((q16 - q64).abs() / qtol).max()):.2f} roundings"
        a = e @ q16.T
        z = torch.cat([e[:, :63], -e[:, :63].sum(1, keepdim=True)], 1)
        judge((mode, dec, "z"), rm.row_errors(z, z_ref), rm.row_errors(mdl["z"], z_ref), what)
    else:
        a = res["out"].double() - x2.double()
    judge((mode, dec, "a"), rm.row_errors(a, a_ref), rm.row_errors(mdl["a"], a_ref), what)
    # ---- the LayerNorm statistics handed to the block, against those of what its GEMM will normalise
    if mode == 2:
        y = x2.double() + a
        model_stats = rm.fold_stats_f32(x2.numpy(), res["out"].numpy(), q16.numpy(), None if centre is None else centre.numpy())
        if centre is not None:      # the copy was read with the centre it was given
            assert torch.equal(res["muc"], centre.reshape(-1)), f"{what}: muc is not the centre handed in"
    elif mode == 1:
        y = res["out"].double()
        model_stats = rm.group_stats_f32(res["out"].numpy())
    if mode >= 1:
        want = rm.true_stats(y.numpy())
        got = (res["mr"][:, 0].double().numpy() + res["muc"].double().numpy(), res["mr"][:, 1].double().numpy())
        ke, me = rm.stat_errors(got, want), rm.stat_errors(model_stats, want)
        judge((mode, dec, "mean"), ke[0], me[0], what)
        judge((mode, dec, "rstd"), ke[1], me[1], what)
    if mode == 1:      # the re-emitted copy: fp16 of the row minus its centre, one rounding (and the fp32 subtraction in front of it)
        yk, c = res["out"].double(), res["muc"].double()[:, None]
        err = (res["copy"].double() + c - yk).abs()
        tol = (yk - c).abs() * 2.0 ** -11 + 2.0 ** -25 + (yk.abs() + c.abs()) * 2.0 ** -23
        assert bool((err <= tol).all()), f"{what}: fp16 copy + muc is off y by {float((err / tol).max()):.2f} x one rounding"
    return res


def stream(kind, mode, L, D=256, seed=0):
    return rm.make_stream(kind, n_seq_for(mode, L), L, D, 900 + 7 * L + seed)


# (mode 1 needs 512 rows: with at most eight sequences that is L >= 64; its shorter lengths are a refusal, below)
@pytest.mark.parametrize("mode,memory,L", [(mode, memory, L) for mode in (0, 1, 2) for memory in ("self", "prior") for L in LENGTHS
                                           if mode != 1 or L >= 64])
def test_sequence_lengths(t256, mode, memory, L):
    """The partly filled last 32-token tile, multiples of 16 and 32 +- 1, the L >= 161 switch of down_proj into the decoder, L = 224."""
    x = stream("unit", mode, L)
    prior = rm.make_prior(x.shape[0], 17, "suffix", 717) if memory == "prior" else None
    run_case(t256, mode, x, prior, f"mode {mode} {memory} L={L}", True, mode == 2 and L >= 161)


def test_mode_1_refuses_fewer_than_512_rows(t256):
    with pytest.raises(RuntimeError, match="at least 512 rows"):
        launch(t256[0], 1, stream("unit", 0, 33), None)
    with pytest.raises(RuntimeError, match="at least 512 rows"):
        launch(t256[0], 1, rm.make_stream("unit", 7, 73, 256, 1), rm.make_prior(7, 17, "none", 1))      # 511


def test_a_stream_of_another_width_and_a_centre_in_mode_0_are_refused(t256):
    with pytest.raises(RuntimeError, match="the stream must be"):
        launch(t256[0], 0, rm.make_stream("unit", 3, 33, 128, 1), None)
    x = stream("unit", 0, 33)
    with pytest.raises(RuntimeError, match="has no centre"):
        launch(t256[0], 0, x, None, rm.make_centre(x, 1))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_more_than_224_tokens_are_refused(t256, mode):
    with pytest.raises(RuntimeError, match="at most 224 tokens"):
        launch(t256[0], mode, stream("unit", mode, 225), None)


@pytest.mark.parametrize("N", [1, 6, 17, 30, 31, 32, 33, 40, 64])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_prior_counts_and_masks(t256, mode, N):
    """MFMA decoder up to 32 prior tokens, the fp32 one-lane-per-token kernels beyond; none / suffix / prefix / every third key / only key 0 /
    only key N - 1 valid, different in every sequence of the launch."""
    if mode == 2 and N > 32:
        with pytest.raises(RuntimeError, match="at most 32 prior tokens"):
            launch(t256[0], 2, stream("unit", 2, 33), rm.make_prior(3, N, "none", 1))
        return
    L = 64 if mode == 1 else 33
    x = stream("unit", mode, L, seed=N)
    for kind in rm.MASKS:
        prior = rm.make_prior(x.shape[0], N, kind, 700 + N)
        assert not prior[1].all(dim=1).any()
        run_case(t256, mode, x, prior, f"mode {mode} N={N} mask={kind}", N <= 32, False)


@pytest.mark.parametrize("L", [33, 160, 161, 224])
@pytest.mark.parametrize("mode", [0, 2])
def test_chained_layers(t256x2, mode, L):
    """adapter_num_layers = 2 with priors: mhsa_layers.0 -> .1 through the fp32 chain buffer; from L = 161 on together with down_proj inside
    the first layer's launch (mode 2)."""
    x = stream("unit", mode, L, seed=2)
    run_case(t256x2, mode, x, rm.make_prior(3, 17, "third", 742), f"2 layers, mode {mode} L={L}", True, mode == 2 and L >= 161)


def test_chained_layers_refuse_more_than_32_prior_tokens(t256x2):
    with pytest.raises(RuntimeError, match="at most 32 prior tokens"):
        launch(t256x2[0], 0, stream("unit", 0, 33), rm.make_prior(3, 40, "none", 1))


def test_folding_modes_refuse_a_width_that_is_no_multiple_of_256():
    vis, _ = _tower(128)
    x = rm.make_stream("unit", 3, 33, 128, 5)
    assert launch(vis, 0, x, None)["out"].shape == (99, 128)
    for mode in (1, 2):
        with pytest.raises(RuntimeError, match="multiple of 256"):
            launch(vis, mode, x, None)


@pytest.mark.parametrize("kind", ["small", "outlier"])
@pytest.mark.parametrize("memory", ["self", "prior"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_small_spread_and_outlier_streams(t256, mode, memory, kind):
    """Rows of mean 30 and spread 0.02 (var_y = var_x + dv is all dv; the centred copy is what keeps down_proj alive) and rows with three
    channels 67 x the rest, below and above the fused-down_proj switch."""
    for L in (65, 197):
        x = stream(kind, mode, L, seed=3)
        prior = rm.make_prior(x.shape[0], 30, "third", 730) if memory == "prior" else None
        run_case(t256, mode, x, prior, f"mode {mode} {memory} {kind} L={L}", True, mode == 2 and L >= 161)


@pytest.mark.parametrize("kind", rm.STREAMS)
@pytest.mark.parametrize("mode,memory", [(1, "self"), (1, "prior"), (1, "prior40"), (2, "self"), (2, "prior"), (2, "chain")])
def test_centre_away_from_the_mean(t256, t256x2, mode, memory, kind):
    """As every block of a tower but the first is entered: behind a residual GEMM + finalize_stats the fp16 copy is centred on the row's
    PREVIOUS mean and mr[:, 0] = mean - centre is not zero.  Live then: the mu * cs correction of down_proj with a centre that is not
    the mean (both modes), -old[0] * sa in the variance update and old[0] + in the new mean (mode 2), the re-emitted copy's centre =
    the mean, not the centre read (mode 1)."""
    N = {"self": 0, "prior": 30, "prior40": 40, "chain": 17}[memory]
    for L in (65, 197):
        x = stream(kind, mode, L, seed=5)
        centre = rm.make_centre(x, 50 + L)
        prior = rm.make_prior(x.shape[0], N, "third", 730 + N) if N else None
        res = run_case(t256x2 if memory == "chain" else t256, mode, x, prior, f"centred, mode {mode} {memory} {kind} L={L}", N <= 32,
                       mode == 2 and L >= 161, centre)
        if mode == 1:
            mean = x.double().reshape(-1, x.shape[-1]).mean(-1)
            assert float((res["muc"].double() - mean).abs().max()) <= 1e-5 * float(x.abs().max()), "the new copy is not centred on x's mean"
            assert not torch.equal(res["muc"], centre.reshape(-1))


@pytest.mark.parametrize("mode,memory", [(0, "self"), (0, "prior"), (0, "prior40"), (1, "self"), (1, "prior"), (1, "prior40"),
                                         (2, "self"), (2, "prior")])
def test_width_768(t768, mode, memory):
    """ViT-B/16's width: twelve K-tiles of down_proj, three 256-column tiles of up_proj."""
    for L in (33, 197):
        if mode == 1 and L < 64:
            continue
        x = stream("unit" if L == 197 else "outlier", mode, L, 768, seed=4)
        N = 40 if memory == "prior40" else 17
        prior = None if memory == "self" else rm.make_prior(x.shape[0], N, "prefix", 768)
        run_case(t768, mode, x, prior, f"width 768, mode {mode} {memory} L={L}", N <= 32, mode == 2 and L >= 161)


def test_every_path_is_reported(t256):
    """Each mode on both decoders where it admits them, down_proj inside the decoder and apart from it: what the hook says it ran."""
    for mode, L, N, mfma, fused in ((0, 33, 17, True, False), (0, 33, 40, False, False), (1, 64, 17, True, False), (1, 64, 40, False, False),
                                    (2, 160, 17, True, False), (2, 161, 17, True, True), (2, 160, 0, True, False), (2, 161, 0, True, True),
                                    (0, 224, 0, True, False), (1, 224, 0, True, False)):
        x = stream("unit", mode, L)
        res = launch(t256[0], mode, x, rm.make_prior(x.shape[0], N, "none", 1) if N else None)
        assert (res["mfma"], res["down_fused"]) == (mfma, fused), (mode, L, N)
