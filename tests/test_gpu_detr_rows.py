"""The five row kernels of hoigen_amd/csrc/hg_detr_rows.hip, each alone through hg_test_detr_rows, against tests/detr_rows_bound.py: the
entry and exit kernels bit for bit at every layout; the post-norm and the decoder layer's tail inside the per-element bound against
float64 on every family, bit for bit the CPU restatement on the families whose arithmetic is exact, their fp16 copies and trace copy
derived bit for bit from the same launch's fp32 stream (which the bound holds to float64); NaN canaries before and behind every output,
finite guard rows around the stream that is normalised in place; and the launchers' refusals, which write nothing."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import detr_rows_bound as rb
from hoigen_amd import _lib

pytestmark = pytest.mark.gpu

PAD = rb.PAD
MS = (1, 3, 4, 5, 33)
SEED = 23
HG_ERR_INVALID = -1
ENTRY, POSTNORM, EXIT, DEC_ENTRY, DEC_TAIL = range(5)


@pytest.fixture(scope="module")
def ctx():
    h = _lib.lib().hg_create(0)
    assert h
    yield h
    _lib.lib().hg_destroy(h)


def call(ctx, op, ptrs, strides=(), ints=()):
    a = _lib.hg_test_detr_rows_args()
    for k, t in enumerate(ptrs):
        a.p[k] = None if t is None else (t.data_ptr() if isinstance(t, torch.Tensor) else t)
    for k, v in enumerate(strides):
        a.s[k] = v
    for k, v in enumerate(ints):
        a.i[k] = v
    return _lib.lib().hg_test_detr_rows(ctx, op, C.byref(a), None)


def ok(ctx, rc):
    assert rc == 0, _lib.lib().hg_last_error(ctx)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(rows, D, dtype=torch.float32, fill=float("nan")):
    """[PAD + rows + PAD, D] on the device, everything `fill`; the kernels get the middle"""
    return torch.full((2 * PAD + rows, D), fill, dtype=dtype, device="cuda")


def stream(x):
    """the in-place stream: x between GUARD rows"""
    t = padded(x.shape[0], x.shape[1], fill=float(rb.GUARD))
    t[PAD:PAD + x.shape[0]] = torch.from_numpy(x).cuda()
    return t


def back(t, M, guard=False):
    """a padded device buffer -> numpy fp32 [M + PAD, D] (the rows behind M kept for the judge); the rows in front are checked here"""
    if t is None:
        return None
    a = t.float().cpu().numpy()
    front = a[:PAD]
    assert (rb.same_bits(front, np.full_like(front, rb.GUARD)) if guard else np.isnan(front).all()), "rows in front of a buffer were written"
    return np.ascontiguousarray(a[PAD:])


def run_norm(ctx, c, with_pos, with_copy, tail=None, copy_shift=0):
    """one launch of the post-norm (tail None) or of the tail (tail = dict(out layout 'qbc' / 'bqc' / None)) -> rb's result dict"""
    M, D = c["M"], c["D"]
    x = stream(c["x"])
    x16 = padded(M, D, torch.float16)
    xp16 = padded(M, D, torch.float16) if with_pos else None
    copy = None
    if with_copy:      # copy_shift = 1: an address that is 4-byte aligned and no more
        flat = torch.full(((2 * PAD + M) * D + copy_shift,), float("nan"), device="cuda")
        copy = flat[copy_shift:].view(2 * PAD + M, D)
        assert copy.data_ptr() % 16 == 4 * copy_shift
    mid = lambda t: None if t is None else t[PAD:]
    pos = dev(c["qpos" if tail is not None else "pos"]) if with_pos else None
    res = {}
    if tail is None:
        g, b = dev(c["g"]), dev(c["b"])
        ok(ctx, call(ctx, POSTNORM, [mid(x), g, b, pos, mid(x16), mid(xp16), mid(copy)], (), (M, D)))
    else:
        B, Q = tail["BQ"]
        assert B * Q == M
        out = padded(M, D) if tail["out"] else None
        ob, oq = {"qbc": (D, B * D), "bqc": (Q * D, D), None: (0, 0)}[tail["out"]]
        w = {k: dev(c[k]) for k in ("b2", "part", "g3", "be3", "gf", "bef")}
        ok(ctx, call(ctx, DEC_TAIL, [mid(x), w["b2"], w["part"] if c["n_sl"] else None, w["g3"], w["be3"], pos, mid(x16), mid(xp16), mid(copy),
                                     w["gf"] if out is not None else None, w["bef"] if out is not None else None, mid(out)],
                     (ob, oq), (c["n_sl"], Q, M, D)))
        res["out"] = None
        if out is not None:      # back to dense batch-major rows
            o = back(out, M)
            rows = o[:M].reshape(Q, B, D).transpose(1, 0, 2).reshape(M, D) if tail["out"] == "qbc" else o[:M]
            res["out"] = np.concatenate([rows, o[M:]])
    torch.cuda.synchronize()
    res.update(x=back(x, M, guard=True), x16=back(x16, M), xp16=back(xp16, M), copy=back(copy, M))
    return res


@pytest.mark.parametrize("D", (4, 128, 132, 256, 384, 512, 640))
def test_postnorm_every_family_inside_the_bound(ctx, D):
    fails, top = [], 0.0
    for M, family in itertools.product(MS, rb.NORM_FAMILIES):
        c = rb.make_postnorm(family, M, D, SEED)
        want, bound = rb.reference_postnorm(c), rb.bounds_postnorm(c)
        assert np.isfinite(bound).all()
        exact = rb.model_postnorm(c)["x"] if family in rb.BITWISE_FAMILIES else None
        variants = [(True, True, 0), (False, False, 0)] + ([(True, True, 1), (False, True, 0), (True, False, 0)] if family == "randn" else [])
        first = None
        for with_pos, with_copy, shift in variants:
            res = run_norm(ctx, c, with_pos, with_copy, copy_shift=shift)
            f, r = rb.judge_norm(res, M, want, bound, c["pos"] if with_pos else None, exact)
            assert (res["xp16"] is not None) == with_pos and (res["copy"] is not None) == with_copy
            top = max(top, r)
            fails += [f"{family} M {M} pos {with_pos} copy {with_copy} shift {shift}: {m}" for m in f]
            if first is None:
                first = res["x"]
            elif not rb.same_bits(first, res["x"]):
                fails.append(f"{family} M {M}: the stream depends on which copies are asked for")
        if family == "constant" and not rb.same_bits(first[:M], np.broadcast_to(c["b"], (M, D)).copy()):
            fails.append(f"constant M {M}: not the norm's bias bit for bit")
    print(f"DETR_ROWS_RATIO postnorm D {D}: worst |err| / bound {top:.3f}")
    assert not fails, "\n".join(fails[:20])


def split_rows(M):
    return {1: (1, 1), 3: (3, 1), 4: (2, 2), 5: (1, 5), 33: (3, 11)}[M]


@pytest.mark.parametrize("D", (128, 256, 384, 512))
def test_dec_tail_every_family_inside_the_bound(ctx, D):
    fails, top, top_out = [], 0.0, 0.0
    for M, family, n_sl, with_b2 in itertools.product(MS, rb.NORM_FAMILIES, (0, 1, 16), (True, False)):
        c = rb.make_tail(family, M, D, n_sl, SEED, with_b2)
        _, y, o = rb.reference_tail(c)
        _, Ey, Eo = rb.bounds_tail(c)
        assert np.isfinite(Ey).all() and np.isfinite(Eo).all()
        model = rb.model_tail(c) if family in rb.BITWISE_FAMILIES else None
        first = None
        for layout, with_pos in itertools.product(("qbc", "bqc", None), (True, False)):
            what = f"{family} M {M} slices {n_sl} b2 {with_b2} out {layout} xp16 {with_pos}"
            res = run_norm(ctx, c, with_pos, True, tail=dict(BQ=split_rows(M), out=layout))
            out = res.pop("out")
            f, r = rb.judge_norm(res, M, y, Ey, c["qpos"] if with_pos else None, model["x"] if model else None)
            assert (res["xp16"] is not None) == with_pos and (out is not None) == (layout is not None)
            top = max(top, r)
            fails += [f"{what}: {m}" for m in f]
            if out is not None:
                ro = rb.worst_ratio(out[:M], o, Eo)
                top_out = max(top_out, ro)
                if not ro <= 1.0:
                    fails.append(f"{what}: out worst |err| / bound {ro:.3g}")
                if not np.isnan(out[M:]).all():
                    fails.append(f"{what}: rows behind out were written")
                if model and not rb.same_bits(out[:M], model["out"][:M]):
                    fails.append(f"{what}: out is not the restatement's bit for bit")
                if rb.same_bits(out[:M], res["x"][:M]):
                    fails.append(f"{what}: the stream is the final norm's output")
            if first is None:
                first = res["x"]
            elif not rb.same_bits(first, res["x"]):
                fails.append(f"{what}: the stream depends on out / xp16")
        if family == "constant" and not rb.same_bits(first[:M], np.broadcast_to(c["be3"], (M, D)).copy()):
            fails.append(f"constant M {M}: not norm3's bias bit for bit")
    print(f"DETR_ROWS_RATIO dec_tail D {D}: worst |err| / bound: stream {top:.3f}, out {top_out:.3f}")
    assert not fails, "\n".join(fails[:20])


def layouts(B, T, D):
    """name -> (element strides (batch, token), flat size): sequence-first, batch-first, rows 8 elements apart"""
    return {"seq_first": ((D, B * D), B * T * D), "batch_first": ((T * D, D), B * T * D), "gap": ((T * (D + 8), D + 8), B * T * (D + 8))}


def flat_of(logical, strides, size):
    B, T, D = logical.shape
    flat = np.full(size, np.nan, np.float32)
    b, t = np.divmod(np.arange(B * T), T)
    flat[(b * strides[0] + t * strides[1])[:, None] + np.arange(D)[None, :]] = logical.reshape(B * T, D)
    return flat


@pytest.mark.parametrize("D", (4, 128, 260, 512, 516))
def test_entry_dec_entry_and_exit_bit_for_bit(ctx, D):
    fails = []
    for B, T, family in itertools.product((1, 3), (1, 5, 33), ("randn", "f16edge")):
        M = B * T
        src, pos = rb.make_entry(family, B, T, D, SEED)
        for (name, (st, size)), (pname, (pst, psize)) in zip(layouts(B, T, D).items(), list(layouts(B, T, D).items())[1:] + list(layouts(B, T, D).items())[:1]):
            fs, fp = flat_of(src, st, size), flat_of(pos, pst, psize)
            ds, dp = dev(fs), dev(fp)
            # (op, first operand, second operand): the encoder's entry with and without pos, the decoder's with and without tgt
            for op, a, b_ in ((ENTRY, True, True), (ENTRY, True, False), (DEC_ENTRY, True, True), (DEC_ENTRY, False, True)):
                what = f"op {op} {family} B {B} S {T} {name} / {pname} src {a} pos {b_}"
                outs = dict(x=padded(M, D), x16=padded(M, D, torch.float16), xp16=padded(M, D, torch.float16), posb=padded(M, D))
                o = [outs[k][PAD:] for k in ("x", "x16", "xp16", "posb")]
                sa, sb_ = (st if a else (0, 0)), (pst if b_ else (0, 0))
                if op == ENTRY:
                    ok(ctx, call(ctx, op, [ds, dp if b_ else None, *o], (*sa, *sb_), (B, T, D)))
                else:
                    ok(ctx, call(ctx, op, [ds if a else None, dp, *o], (*sa, *sb_), (B, T, D)))
                torch.cuda.synchronize()
                got = {k: back(v, M) for k, v in outs.items()}
                want = rb.model_entry(fs if a else None, fp if b_ else None, *sa, *sb_, B, T, D)
                fails += [f"{what}: {k} differs in {int((rb.bits(got[k][:M]) != rb.bits(want[k][:M])).sum())} elements" for k in want
                          if not rb.same_bits(got[k][:M], want[k][:M])]
                fails += [f"{what}: rows behind {k} were written" for k in rb.pads_intact(got, M, False)]
            # exit: the dense stream to the caller's rows; everything between and around them keeps its NaN
            x = dev(src.reshape(M, D))
            out = torch.full((size + 2 * PAD * D,), float("nan"), device="cuda")
            ok(ctx, call(ctx, EXIT, [x, out[PAD * D:]], st, (B, T, D)))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            if not (np.isnan(got[:PAD * D]).all() and np.isnan(got[PAD * D + size:]).all()):
                fails.append(f"exit {family} B {B} S {T} {name}: written around out")
            want = rb.model_exit(src.reshape(M, D), *st, B, T, D, size)
            inner, gap = got[PAD * D:PAD * D + size], np.isnan(want)
            if not (np.isnan(inner[gap]).all() and rb.same_bits(inner[~gap], want[~gap])):
                fails.append(f"exit {family} B {B} S {T} {name}: out differs (rows or the gaps between them)")
    print(f"DETR_ROWS_RATIO entry, dec_entry, exit D {D}: bit for bit ({'no' if not fails else len(fails)} differences)")
    assert not fails, "\n".join(fails[:20])


def test_refused_calls_write_nothing(ctx):
    lib = _lib.lib()
    M, D = 8, 640
    bufs = {k: torch.full((M, D), float("nan"), device="cuda") for k in ("x", "copy", "out", "posb")}
    h16 = {k: torch.full((M, D), float("nan"), dtype=torch.float16, device="cuda") for k in ("x16", "xp16")}
    w = torch.ones(D, device="cuda")
    part = torch.zeros(M * D, device="cuda")
    x, cp, out, posb, x16, xp16 = bufs["x"], bufs["copy"], bufs["out"], bufs["posb"], h16["x16"], h16["xp16"]
    refused = [
        ("postnorm D % 4", POSTNORM, [x, w, w, posb, x16, xp16, cp], (), (M, 130)),
        ("postnorm D 0", POSTNORM, [x, w, w, posb, x16, xp16, cp], (), (M, 0)),
        ("postnorm M 0", POSTNORM, [x, w, w, posb, x16, xp16, cp], (), (0, 128)),
        ("postnorm xp16 without posb", POSTNORM, [x, w, w, None, x16, xp16, cp], (), (M, 128)),
        ("postnorm no x16", POSTNORM, [x, w, w, posb, None, xp16, cp], (), (M, 128)),
        ("postnorm no weight", POSTNORM, [x, None, w, posb, x16, xp16, cp], (), (M, 128)),
        ("tail D 640", DEC_TAIL, [x, w, part, w, w, posb, x16, xp16, cp, w, w, out], (D, M * D), (1, 1, M, 640)),
        ("tail D % 4", DEC_TAIL, [x, w, part, w, w, posb, x16, xp16, cp, w, w, out], (D, M * D), (1, 1, M, 130)),
        ("tail xp16 without qposb", DEC_TAIL, [x, w, part, w, w, None, x16, xp16, cp, w, w, out], (D, M * D), (1, 1, M, 128)),
        ("tail out without wf", DEC_TAIL, [x, w, part, w, w, posb, x16, xp16, cp, None, w, out], (D, M * D), (1, 1, M, 128)),
        ("tail out without bf", DEC_TAIL, [x, w, part, w, w, posb, x16, xp16, cp, w, None, out], (D, M * D), (1, 1, M, 128)),
        ("tail out with Q 0", DEC_TAIL, [x, w, part, w, w, posb, x16, xp16, cp, w, w, out], (D, M * D), (1, 0, M, 128)),
        ("tail slices without partial", DEC_TAIL, [x, w, None, w, w, posb, x16, xp16, cp, w, w, out], (D, M * D), (1, 1, M, 128)),
        ("tail negative slices", DEC_TAIL, [x, w, part, w, w, posb, x16, xp16, cp, w, w, out], (D, M * D), (-1, 1, M, 128)),
        ("tail M 0", DEC_TAIL, [x, w, part, w, w, posb, x16, xp16, cp, w, w, out], (D, M * D), (1, 1, 0, 128)),
        ("entry no src", ENTRY, [None, w, x, x16, xp16, posb], (0, 0, 0, 0), (1, M, 128)),
        ("entry B 0", ENTRY, [cp, w, x, x16, xp16, posb], (0, 0, 0, 0), (0, M, 128)),
        ("entry no xp16", ENTRY, [cp, w, x, x16, None, posb], (0, 0, 0, 0), (1, M, 128)),
        ("dec_entry no qpos", DEC_ENTRY, [cp, None, x, x16, xp16, posb], (0, 0, 0, 0), (1, M, 128)),
        ("dec_entry Q 0", DEC_ENTRY, [cp, w, x, x16, xp16, posb], (0, 0, 0, 0), (1, 0, 128)),
        ("exit no out", EXIT, [x, None], (0, 128), (1, M, 128)),
        ("exit D 0", EXIT, [x, out], (0, 128), (1, M, 0)),
        ("op 5", 5, [x, out], (), (1, M, 128)),
        ("op -1", -1, [x, out], (), (1, M, 128)),
    ]
    for what, op, ptrs, strides, ints in refused:
        assert call(ctx, op, ptrs, strides, ints) == HG_ERR_INVALID, what
        assert lib.hg_last_error(ctx), what
    assert lib.hg_test_detr_rows(ctx, POSTNORM, None, None) == HG_ERR_INVALID
    torch.cuda.synchronize()
    for k, t in {**bufs, **h16}.items():
        assert torch.isnan(t).all(), f"a refused call wrote into {k}"
    # ... and the same buffers are written by a call that is not refused
    x.fill_(1.0)
    x[:, ::2] = -1.0
    ok(ctx, call(ctx, POSTNORM, [x, w, torch.zeros(D, device="cuda"), None, x16, None, None], (), (M, D)))
    torch.cuda.synchronize()
    assert torch.isfinite(x).all() and torch.isfinite(x16).all() and torch.isnan(xp16).all()
