"""The instance adapter at 225 .. 640 tokens (hoigen_amd/csrc/hg_adapter_long.hip, option adapter_long = 1) launch by launch against
float64, through hg_test_adapter and with the judge of tests/test_gpu_adapter.py (`run_case`: float64 oracle, the rounding model's rule
2.0 / 1.5, two launches bit-equal, every sequence alone equal to its place in the batch).

What is new beyond 224 tokens: a sequence is cut into query chunks (one workgroup each), and a sequence that is its own memory streams
its K / V through LDS in key chunks of 224 with a running maximum.  Lengths: one key past a chunk (225, 449), full chunks (448), the
padded last 32-key block (257, 577, 639), the limit (640).  tests/test_adapter_long_model.py shows which inputs catch a dropped chunk, a
doubled boundary key and a missing rescale: unit and ramp, at every length.  With priors a token's arithmetic is the short kernel's:
checked bit for bit against it.

Worst ratios seen on an MI355X over all cases below (kernel error / model error: worst row, median row; allowed 2.0, 1.5), printed at
the end of the module - the table in DESIGN.md 4:

    mode  decoder  update a     mean         rstd
    0     long     1.04  1.00   -            -
    0     lanes    1.00  1.00   -            -
    1     long     1.06  1.01   1.54  1.05   1.15  1.03
    1     lanes    1.00  1.00   1.13  1.03   1.09  1.01

The file (62 tests) takes 5 s on an MI355X.
"""
import pytest
import torch

import adapter_long_model as alm
import test_adapter_rounding_model as rm
import test_gpu_adapter as ga

pytestmark = pytest.mark.gpu
LENGTHS = (225, 256, 257, 448, 449, 577, 639, 640)
SEEN = {}          # (mode, decoder, observable) -> [worst ratio, median ratio]


def _long_tower(width, num_layers=1):
    vis, sd = ga._tower(width, num_layers)
    assert vis.get_option("adapter_long") == 0, "the option's default is 0"
    vis.set_option("adapter_long", 1)
    return vis, sd


@pytest.fixture(scope="module")
def t256():
    return _long_tower(256)


@pytest.fixture(scope="module")
def t256x2():
    return _long_tower(256, 2)


@pytest.fixture(scope="module")
def t1024():
    return _long_tower(1024)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nadapter, 225 .. 640 tokens: worst kernel / model ratios (worst row, median row)")
    for k in sorted(SEEN):
        print(f"  mode {k[0]} {k[1]:5s} {k[2]:6s} {SEEN[k][0]:.2f} {SEEN[k][1]:.2f}")


def run_case(tower, mode, x, prior, what, decoder=2):
    """ga.run_case with this module's table of ratios; `decoder`: 2 the long MFMA decoder, 0 the fp32 one-lane-per-token kernels"""
    seen, ga.SEEN = ga.SEEN, {}
    try:
        res = ga.run_case(tower, mode, x, prior, what, decoder != 0, False)
        for (m, _, obs), v in ga.SEEN.items():
            s = SEEN.setdefault((m, "long" if decoder == 2 else "lanes", obs), [0.0, 0.0])
            s[0], s[1] = max(s[0], v[0]), max(s[1], v[1])
    finally:
        ga.SEEN = seen
    assert res["decoder"] == decoder, f"{what}: decoder {res['decoder']} ran"
    return res


def stream(kind, L, D=256, seed=0, n_seq=3):
    return alm.make_stream(kind, n_seq, L, D, 900 + 7 * L + seed)


@pytest.mark.parametrize("mode,memory,L", [(mode, memory, L) for mode in (0, 1) for memory in ("self", "prior") for L in LENGTHS])
def test_sequence_lengths(t256, mode, memory, L):
    x = stream("unit", L)
    prior = rm.make_prior(3, 17, "suffix", 717) if memory == "prior" else None
    run_case(t256, mode, x, prior, f"long, mode {mode} {memory} L={L}")


@pytest.mark.parametrize("kind", ["unit", "ramp", "outlier", "small"])
@pytest.mark.parametrize("mode", [0, 1])
def test_input_families_at_577_tokens(t256, mode, kind):
    run_case(t256, mode, stream(kind, 577, seed=3), None, f"long, mode {mode} self {kind} L=577")


@pytest.mark.parametrize("L", [225, 449, 640])
def test_ramp_at_the_chunk_edges(t256, L):
    """the family whose maximum moves in every key chunk, where a chunk holds one key (225, 449) and at the limit"""
    run_case(t256, 0, stream("ramp", L, seed=1), None, f"long, mode 0 self ramp L={L}")


@pytest.mark.parametrize("N", [1, 17, 32, 40])
@pytest.mark.parametrize("mode", [0, 1])
def test_prior_counts_and_masks(t256, mode, N):
    x = stream("unit", 257, seed=N)
    for kind in rm.MASKS:
        prior = rm.make_prior(3, N, kind, 700 + N)
        assert not prior[1].all(dim=1).any()
        run_case(t256, mode, x, prior, f"long, mode {mode} N={N} mask={kind}", 2 if N <= 32 else 0)


@pytest.mark.parametrize("L", [257, 577])
@pytest.mark.parametrize("mode", [0, 1])
def test_chained_layers(t256x2, mode, L):
    run_case(t256x2, mode, stream("unit", L, seed=2), rm.make_prior(3, 17, "third", 742), f"long, 2 layers, mode {mode} L={L}")


@pytest.mark.parametrize("memory", ["self", "prior"])
def test_width_1024(t1024, memory):
    x = stream("unit", 577, 1024, seed=4)
    prior = None if memory == "self" else rm.make_prior(3, 17, "prefix", 768)
    run_case(t1024, 0, x, prior, f"long, width 1024, mode 0 {memory} L=577")


@pytest.mark.parametrize("n_seq,L,parts", [(2, 448, 2), (1, 640, 5)])
def test_with_priors_the_long_decoder_is_the_short_one_bit_for_bit(t256, n_seq, L, parts):
    """tokens attend only to the priors: a long sequence is `parts` short ones with the same priors and mask"""
    x = stream("unit", L, seed=7, n_seq=n_seq)
    pri, mask = rm.make_prior(n_seq, 17, "third", 731)
    long_ = ga.launch(t256[0], 0, x, (pri, mask))
    short = ga.launch(t256[0], 0, x.reshape(n_seq * parts, L // parts, 256),
                      (pri.repeat_interleave(parts, 0), mask.repeat_interleave(parts, 0)))
    assert (long_["decoder"], short["decoder"]) == (2, 1)
    assert torch.equal(long_["out"], short["out"])


@pytest.mark.parametrize("memory", ["self", "prior"])
def test_a_non_finite_sequence_stays_alone(t256, memory):
    x = stream("unit", 577, seed=9)
    prior = rm.make_prior(3, 17, "suffix", 717) if memory == "prior" else None
    want = ga.launch(t256[0], 0, x, prior)
    bad = x.clone()
    bad[1, 5, 3], bad[1, 300, 7], bad[1, 576, 0] = float("nan"), float("inf"), float("-inf")
    got = ga.launch(t256[0], 0, bad, prior)
    for i in (0, 2):
        assert torch.equal(got["out"][i * 577:(i + 1) * 577], want["out"][i * 577:(i + 1) * 577]), f"sequence {i} saw its neighbour"
    assert torch.equal(ga.launch(t256[0], 0, x, prior)["out"], want["out"]), "a finite launch behind a non-finite one differs"


def test_refusals(t256, t256x2):
    vis = t256[0]
    with pytest.raises(RuntimeError, match="at most 640 tokens"):
        ga.launch(vis, 0, stream("unit", 641), None)
    with pytest.raises(RuntimeError, match=r"mode 2\) serves at most 224 tokens"):
        ga.launch(vis, 2, stream("unit", 225), None)
    with pytest.raises(RuntimeError, match="at most 32 prior tokens"):
        ga.launch(t256x2[0], 0, stream("unit", 257), rm.make_prior(3, 40, "none", 1))
    vis.set_option("adapter_long", 0)
    try:
        with pytest.raises(RuntimeError, match="at most 224 tokens"):
            ga.launch(vis, 0, stream("unit", 225), None)
        assert ga.launch(vis, 0, stream("unit", 224), None)["decoder"] == 1
    finally:
        vis.set_option("adapter_long", 1)
    assert ga.launch(vis, 0, stream("unit", 225), None)["decoder"] == 2
