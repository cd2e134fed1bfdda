"""The host side of the batched crop pre-processing, without a GPU:

* hoigen_amd/csrc/hg_preproc_geom.h - the geometry and weight-table functions the kernels evaluate per crop on the device - compiled with
  the host compiler into the stand-alone program tests/preproc_geom_main.cpp, run on every box and flag set of tests/preproc_cases.py and
  on the limit boxes of tests/preproc_batch_model.py: the header words against preproc_cases.header (and the model's geometry for the
  words the per-image call does not have), the tables against preproc_cases.fill_tables word for word.  Built a second time with
  -fsanitize=address,undefined and run the same way (a program of its own, in the environment as it is; skipped where that
  environment preloads a library into every process, which the sanitizer's runtime does not start behind).
* records.plan_record_batches."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import preproc_batch_model as pbm
import preproc_cases as pc
from hoigen_amd import records

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
BG = 0x00687A74 | 0      # any three distinct channel values


def crops():
    """(n_px, flags, box, image, B) of every committed box, the model's own, and a few refusals"""
    out = []
    for c in pc.CASES + pbm.OWN:
        out += [(c["n_px"], pbm.flags_of(c), tuple(int(v) for v in b), 0, 1) for b in c["boxes"]]
    out += [(31, 0, (5, 5, 5, 9), 0, 1), (31, 0, (9, 9, 5, 5), 0, 1), (31, 0, (0, 0, 9, 9), 1, 1), (31, 0, (0, 0, 9, 9), -1, 3),
            (31, 2, pbm.ABOVE_BOX, 0, 1), (31, 2, pbm.LIMIT_BOX, 0, 1), (224, 0, (0, 0, (1 << 20) + 1, 50), 0, 1),
            (518, 3, (-(1 << 31), -(1 << 31), (1 << 31) - 1, (1 << 31) - 1), 0, 1), (518, 2, (0, 0, 518 * 16, 518 * 16), 0, 1)]
    return out


def build(tmp, name, extra):
    exe = os.path.join(tmp, name)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", *extra,
                        "-I", os.path.join(REPO, "hoigen_amd", "csrc"), os.path.join(REPO, "tests", "preproc_geom_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_and_check(exe):
    todo = crops()
    text = "".join(f"{n_px} {flags} {BG} {b[0]} {b[1]} {b[2]} {b[3]} {im} {B}\n" for n_px, flags, b, im, B in todo)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    at = accepted = 0
    for n_px, flags, b, im, B in todo:
        assert lines[at][0] == "H"
        h = [int(v) for v in lines[at][1:].split()]
        at += 1
        assert len(h) == pbm.HDR
        want_h, want_status = pbm.geometry(b, im, B, n_px, flags, BG)
        assert h == want_h, (n_px, flags, b, h, want_h)
        if want_status:
            assert h[20] == want_status and not any(h[:13]) and not any(h[14:20])
            continue
        accepted += 1
        # the words of the per-image call's header (0 .. 11, 14 .. 17; 13 is the background), as hg_preprocess_crops works them out on the host
        assert pbm.as_dict(h) == pc.header(b, n_px, bool(flags & 1), bool(flags & 2)) and h[13] == BG and h[20] == 0 and h[21] == im
        want = pc.fill_tables(pbm.as_dict(h), n_px)
        got = np.concatenate([np.array(lines[at + a][1:].split(), np.int64) for a in (0, 1)])
        assert lines[at][0] == "T" and lines[at + 1][0] == "T"
        at += 2
        assert got.size == want.size and np.array_equal(got, want), (n_px, flags, b, int((got != want).sum()))
    assert at == len(lines) and accepted >= len(todo) - 8


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("preproc_geom"))


@pytest.mark.skipif(not CXX, reason="no host C++ compiler")
def test_geometry_header_on_the_host(tmp):
    run_and_check(build(tmp, "geom", []))


@pytest.mark.skipif(not CXX, reason="no host C++ compiler")
@pytest.mark.skipif(bool(os.environ.get("LD_PRELOAD")), reason="a library is preloaded into every process here: the sanitizer's runtime must come "
                                                               "first, and the environment stays as it is")
def test_geometry_header_under_address_and_undefined_behaviour_sanitizers(tmp):
    run_and_check(build(tmp, "geom_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))


# ---- records.plan_record_batches ------------------------------------------------------------------------------------------------------
def check_plan(counts, max_crops):
    groups = records.plan_record_batches(counts, max_crops)
    assert [i for a, b in groups for i in range(a, b)] == list(range(len(counts)))      # every image once, in order, never split
    for a, b in groups:
        assert 1 <= b - a <= 64
        crops_ = 3 * sum(counts[a:b])
        assert crops_ <= max_crops or b - a == 1                                         # the caps; one image above max_crops alone
    for (a, b), (_, d) in zip(groups, groups[1:]):                                       # greedy: the next image did not fit
        assert b - a == 64 or 3 * sum(counts[a:b + 1]) > max_crops
    return groups


def test_plan_record_batches():
    assert records.plan_record_batches([]) == []
    assert check_plan([0, 0, 0], 256) == [(0, 3)]
    assert check_plan([1, 2, 0, 100, 3, 0, 0], 30) == [(0, 3), (3, 4), (4, 7)]
    assert check_plan([100], 30) == [(0, 1)]
    assert check_plan([1] * 70, 1000) == [(0, 64), (64, 70)]
    assert check_plan([0] * 130, 1) == [(0, 64), (64, 128), (128, 130)]
    assert check_plan([10, 10], 60) == [(0, 2)] and check_plan([10, 10], 59) == [(0, 1), (1, 2)]
    rng = np.random.RandomState(3)
    for _ in range(50):
        check_plan(rng.randint(0, 30, size=rng.randint(1, 200)).tolist(), int(rng.randint(1, 300)))
    with pytest.raises(ValueError):
        records.plan_record_batches([1, -1])
    with pytest.raises(ValueError):
        records.plan_record_batches([1], 0)
