"""hg_cache_logits / hg_mlp_net (hg_heads.hip) with the host folding of hg_load_cache / hg_load_mlp, through CacheLogits, vae.mlp_net,
option chunk_rows and hg_profile_*, held PER OUTPUT ELEMENT to the float64 reference and the bound of tests/heads_bound.py, and bit for
bit to its exact families:

* K 64 / 256 / 1024 and (S, C) from (1, 1) to (1200, 600): Sp and Cp on both sides of launch_gemm's N % 256 rule, the second GEMM's
  K = Sp below and above 256, so that the simple 128 x 128 kernel AND the ring kernels run inside hg_cache_logits (asserted from the
  dispatcher's rule) - with labels (null-bias fp16 phi, scale epilogue on the zeroed destination) and without;
* chunk_rows 512 and 256 with row counts on both sides of the chunk seam and of its absorbed tail, the chunk rows asserted through
  hg_profile (M of the recorded GEMMs); a ring chunk followed by a simple-kernel chunk in one call; the seam rows again on slots whose
  output is narrower than its padded row (Nout < Np), where a chunk written at r0 * Np or copied with the wrong ld shows;
* every output written through the ABI between NaN canary rows and compared whole;
* update() to a smaller S and C in the same slot and back, two slots with different K alive at once, R = 0, the loader's refusals;
* mlp_net at four width triples, the same row counts.

Every test prints HEADS_RATIO lines (worst |err| / E per family); heads_bound's docstring carries them as a table.
tests/test_heads_rounding_model.py proves on the CPU which wrong kernels the rule rejects.

File total on an MI355X: about 10 s for the 52 cases; none takes more than a second."""
import ctypes as C

import pytest
import torch

import heads_bound as hb
from hoigen_amd import _lib, vae
from hoigen_amd.cache_model import CacheLogits
from hoigen_amd.model import _stream_ptr

pytestmark = pytest.mark.gpu
CANARY = 0x7FC0DEAD          # a quiet NaN with a payload
KS = (64, 256, 1024)
SC = ((1, 1), (77, 24), (129, 117), (256, 128), (300, 256), (512, 256), (1200, 600))
R_SHAPES = 520               # M >= 512: the ring kernels run wherever N and K allow them
CHUNK_ROWS = {512: {1: [1], 511: [511], 512: [512], 513: [513], 1088: [512, 576], 1089: [512, 512, 65]}, 256: {288: [288], 289: [256, 33]}}
MLP_WIDTHS = ((512, 512, 512), (64, 128, 128), (768, 1024, 256), (1536, 256, 128))


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def cache_ctx():
    return _lib.ctx(0)


def get_chunk(handle):
    v = C.c_int32()
    assert _lib.lib().hg_get_option(handle, b"chunk_rows", C.byref(v)) == 0
    return v.value


def set_chunk(handle, v):
    assert _lib.lib().hg_set_option(handle, b"chunk_rows", int(v)) == 0


@pytest.fixture()
def d():
    dv = dev()
    cache_chunk = get_chunk(cache_ctx())
    mlp_chunk = vae.get_option("chunk_rows", dv)
    yield dv
    set_chunk(cache_ctx(), cache_chunk)
    vae.set_option("chunk_rows", mlp_chunk, dv)


class Book:
    def __init__(self, what):
        self.what, self.worst, self.failures = what, {}, []

    def judge(self, c, got, tag, rows=None):
        got = got.cpu()
        mlp = "dims" in c
        want, E = hb.mlp_reference(c, rows) if mlp else hb.cache_reference(c, rows)
        r = hb.worst(got, want, E)
        key = f"{'mlp_net' if mlp else 'labels' if c['has_labels'] else 'linear'} {c['family']}"
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        if not r <= 1.0:
            self.failures.append(f"{tag} {c['family']}: worst |err| / E {r:.3f}")
        if c["family"] in hb.EXACT_FAMILIES:
            exact = hb.mlp_exact(c, rows) if mlp else hb.cache_exact(c, rows)
            if not torch.equal(got, exact):
                self.failures.append(f"{tag} {c['family']}: {int((got != exact).sum())} elements are not the float64 result bit for bit")

    def close(self):
        print()
        for fam, v in sorted(self.worst.items()):
            print(f"HEADS_RATIO {self.what} {fam}: worst |err| / E {v:.3f}")
        assert not self.failures, self.failures


def load(c, dv, into=None):
    """CacheLogits of the case (or `into`.update with it)"""
    t = [c["w"].to(dv), c["b"].to(dv)] + ([c["lab"].to(dv), c["lens"].to(dv)] if c["has_labels"] else [None, None])
    if into is None:
        return CacheLogits(*t, post_div=c["post_div"])
    into.post_div = float(c["post_div"])
    into.update(*t)
    return into


def logits(m, f, book, tag):
    """hg_cache_logits on the object's slot with the output between NaN canary rows -> [R, Nout] (the façade's own call is compared
    with it bit for bit)"""
    R, n_out = f.shape[0], (m.C if m.C else m.S)
    buf = torch.full((R + 2, n_out), CANARY, dtype=torch.int32, device=f.device)
    rc = _lib.lib().hg_cache_logits(_lib.ctx(m.device), m.slot, f.data_ptr(), R, buf[1:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(m.device, rc, "hg_cache_logits")
    torch.cuda.synchronize()
    if not (bool((buf[0] == CANARY).all()) and bool((buf[R + 1] == CANARY).all())):
        book.failures.append(f"{tag}: a row in front of or behind the output was written")
    out = buf[1:R + 1].view(torch.float32)
    if not torch.equal(m(f).view(torch.int32), buf[1:R + 1]):
        book.failures.append(f"{tag}: the façade's call and the direct call differ")
    return out


def test_the_shapes_reach_both_gemm_kernels():
    """launch_gemm's rule applied to the GEMMs of the cases below: both kernels, for both GEMMs, and the second K on both sides of 256"""
    first = {hb.ring_kernel(R_SHAPES, hb.rup(S, 128), K) for K in KS for S, _ in SC}
    second = {hb.ring_kernel(R_SHAPES, hb.rup(Cc, 128), hb.rup(S, 128)) for S, Cc in SC}
    assert first == {True, False} and second == {True, False}
    assert {hb.rup(S, 128) < 256 for S, _ in SC} == {True, False}
    assert hb.ring_kernel(512, 512, 256) and not hb.ring_kernel(65, 512, 256) and not hb.ring_kernel(511, 512, 256)


@pytest.mark.parametrize("S,Cc", SC)
@pytest.mark.parametrize("K", KS)
def test_cache_shapes_and_families(d, K, S, Cc):
    """520 rows (and the first 3 alone) with labels and post_div = 2, and as the linear map; exact and rounded everywhere, every
    family at K = 256"""
    book = Book(f"cache K {K} S {S} C {Cc}")
    fams = hb.CACHE_FAMILIES if K == 256 and (S, Cc) in ((129, 117), (512, 256), (1200, 600)) else ("exact", "rounded", "unit")
    for family in fams:
        for labels in (True, False):
            if not labels and family in ("soft", "sparse"):
                continue
            c = hb.cache_case(family, R_SHAPES, S, Cc, K, labels)
            m = load(c, d)
            f = c["f"].to(d)
            tag = f"{'labels' if labels else 'linear'} R {R_SHAPES}"
            book.judge(c, logits(m, f, book, tag), tag)
            book.judge(c, logits(m, f[:3].contiguous(), book, tag + " first 3"), tag + " first 3", rows=slice(0, 3))
            m.close()
    book.close()


@pytest.mark.parametrize("chunk,R", [(ch, R) for ch, rows in CHUNK_ROWS.items() for R in rows])
def test_chunk_seams(d, chunk, R):
    """K = 256, (S, C) = (512, 256): chunks of 512 rows and more take the ring kernels, shorter ones the simple kernel.  The M of the
    recorded GEMMs must be the chunk rows this test was written for: a change of the chunk rule cannot quietly make it one chunk."""
    set_chunk(cache_ctx(), chunk)
    book = Book(f"cache chunk_rows {chunk} R {R}")
    want_rows = CHUNK_ROWS[chunk][R]
    assert hb.chunks(R, chunk) == want_rows
    for family, labels in (("exact", True), ("rounded", True), ("randn", True), ("soft", True), ("rounded", False), ("randn", False)):
        c = hb.cache_case(family, 1089, 512, 256, 256, labels)
        rows = slice(0, R)
        m = load(c, d)
        f = c["f"][:R].contiguous().to(d)
        tag = f"{'labels' if labels else 'linear'}"
        out, recs = _lib.profile(cache_ctx(), _lib.HG_PROF_ALL, 64, lambda: logits(m, f, book, tag))
        first = [r[1] for r in recs if r[2] == 512 and r[3] == 256]          # the GEMM f W^T: N = Sp, K = 256
        assert first == want_rows + want_rows, f"chunk rows {first[:len(first) // 2]} (direct call, then the façade's), expected {want_rows}"
        if labels:
            second = [r[1] for r in recs if r[0] == 7]
            assert second == want_rows + want_rows, second
        book.judge(c, out, tag, rows=rows)
        m.close()
    book.close()


# (S, C, labels): Nout < Np, so that `out + r0 * Nout` and `out + r0 * Np` are different addresses and copy_cols' ld is not its N
RAGGED = ((300, 256, False), (129, 117, True), (1200, 600, True), (77, 24, True), (77, 24, False))


@pytest.mark.parametrize("S,Cc,labels", RAGGED)
@pytest.mark.parametrize("chunk,R", [(512, 1088), (512, 1089), (256, 289)])
def test_chunk_seams_with_ragged_outputs(d, chunk, R, S, Cc, labels):
    """The seam rows on slots whose output is narrower than its padded row (C % 128 != 0 with labels, S % 128 != 0 without): a later
    chunk written at out + r0 * Np, or copied with another ld than the first, lands in other rows - and in the canary row behind.
    The chunk rows are asserted through hg_profile on the GEMM f W^T (N = Sp, K = 256)."""
    set_chunk(cache_ctx(), chunk)
    book = Book(f"cache ragged chunk_rows {chunk} R {R} S {S} C {Cc}")
    want_rows = CHUNK_ROWS[chunk][R]
    Sp, n_out = hb.rup(S, 128), (Cc if labels else S)
    assert n_out < (hb.rup(Cc, 128) if labels else Sp) and len(want_rows) >= 2
    for family in ("exact", "rounded", "randn"):
        c = hb.cache_case(family, 1089, S, Cc, 256, labels)
        m = load(c, d)
        f = c["f"][:R].contiguous().to(d)
        tag = f"{'labels' if labels else 'linear'}"
        out, recs = _lib.profile(cache_ctx(), _lib.HG_PROF_ALL, 64, lambda: logits(m, f, book, tag))
        first = [r[1] for r in recs if r[0] == (0 if labels else 4) and r[2] == Sp and r[3] == 256]
        assert first == want_rows + want_rows, f"chunk rows {first} (direct call, then the façade's), expected {want_rows} twice"
        assert out.shape == (R, n_out)
        book.judge(c, out, tag, rows=slice(0, R))
        m.close()
    book.close()


def test_update_in_one_slot_and_two_slots(d):
    """(S, C) = (512, 256) -> (77, 24) -> (512, 256) in one slot: no stale padded rows or classes; a second object with another K alive
    beside it the whole time"""
    book = Book("cache update")
    big = hb.cache_case("randn", R_SHAPES, 512, 256, 256, True)
    big_x = hb.cache_case("rounded", R_SHAPES, 512, 256, 256, True)
    small = hb.cache_case("randn", R_SHAPES, 77, 24, 256, True)
    small_x = hb.cache_case("rounded", R_SHAPES, 77, 24, 256, True)
    other = hb.cache_case("rounded", R_SHAPES, 129, 117, 64, True)
    m, o = load(big, d), load(other, d)
    slot = m.slot
    assert o.slot != slot
    for step, c in enumerate((big, small, small_x, big_x, small, big)):
        load(c, d, into=m)
        assert m.slot == slot
        book.judge(c, logits(m, c["f"].to(d), book, f"step {step}"), f"step {step} S {c['S']} C {c['C']}")
        book.judge(other, logits(o, other["f"].to(d), book, f"other at step {step}"), f"the other slot at step {step}")
    m.close()
    o.close()
    book.close()


def test_no_rows_and_refusals(d):
    """R = 0 returns an empty tensor; K % 64 != 0, a missing weight, labels without sample_lens and S <= 0 return HG_ERR_INVALID with a
    message and leave the slot unloaded"""
    c = hb.cache_case("randn", 8, 77, 24, 64, True)
    m = load(c, d)
    assert m(torch.zeros(0, 64, device=d)).shape == (0, 24)
    lib, h = _lib.lib(), cache_ctx()
    w, b, lab, lens = (c[k].to(d) for k in ("w", "b", "lab", "lens"))
    f = c["f"].to(d)
    out = torch.empty(8, 24, device=d)

    def weights(S=77, K=64, Cc=24, weight=w, labels=lab, sample_lens=lens):
        cw = _lib.hg_cache_weights()
        cw.weight, cw.bias, cw.labels, cw.sample_lens = (_lib.tensor(t) for t in (weight, b, labels, sample_lens))
        cw.S, cw.K, cw.C, cw.post_div = S, K, Cc, 1.0
        return cw

    for what, cw in (("K % 64", weights(K=96)), ("no weight", weights(weight=None)), ("labels without sample_lens", weights(sample_lens=None)),
                     ("S = 0", weights(S=0)), ("S < 0", weights(S=-5))):
        assert lib.hg_load_cache(h, m.slot, C.byref(weights())) == 0, what          # a good load first: the refusal must unload it
        rc = lib.hg_load_cache(h, m.slot, C.byref(cw))
        assert rc == -1, (what, rc)                                      # HG_ERR_INVALID
        assert lib.hg_last_error(h), what
        rc = lib.hg_cache_logits(h, m.slot, f.data_ptr(), 8, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == -3, (what, rc)                                      # HG_ERR_NOT_LOADED
    load(c, d, into=m)
    book = Book("cache after refusals")
    book.judge(c, logits(m, f, book, "reloaded"), "reloaded")
    m.close()
    book.close()


class Net:
    def __init__(self, c, dv):
        d_in, hid, d_out = c["dims"]
        self.net = vae.mlp_net(d_in, d_out, hid).to(dv)
        self.net.load_state_dict({"net.0.weight": c["w0"], "net.0.bias": c["b0"], "net.2.weight": c["w2"], "net.2.bias": c["b2"],
                                  "net.4.weight": c["w4"], "net.4.bias": c["b4"]})
        self.net.eval()
        self.dv, self.d_out = dv, d_out
        self.net(c["x"][:1].to(dv))          # (weights loaded outside the profiled calls)

    def __call__(self, x, book, tag):
        """hg_mlp_net on the module's slot between canary rows; the module's own call is compared with it bit for bit"""
        R = x.shape[0]
        buf = torch.full((R + 2, self.d_out), CANARY, dtype=torch.int32, device=self.dv)
        with self.net._slot.session(self.dv) as (ctx, h, slot, fresh):
            assert not fresh
            ctx.check(_lib.lib().hg_mlp_net(h, slot, x.data_ptr(), R, buf[1:].data_ptr(), _stream_ptr(self.dv)), "hg_mlp_net")
        torch.cuda.synchronize()
        if not (bool((buf[0] == CANARY).all()) and bool((buf[R + 1] == CANARY).all())):
            book.failures.append(f"{tag}: a row in front of or behind the output was written")
        if not torch.equal(self.net(x).view(torch.int32), buf[1:R + 1]):
            book.failures.append(f"{tag}: the module's call and the direct call differ")
        return buf[1:R + 1].view(torch.float32)


@pytest.mark.parametrize("dims", MLP_WIDTHS)
def test_mlp_net_widths_rows_chunks(d, dims):
    """chunk_rows = 512 and the row counts of test_chunk_seams (256: 288 and 289): every row of every call judged; the M of the recorded
    GEMMs are the chunk rows, three GEMMs a chunk"""
    book = Book(f"mlp_net {dims}")
    handle = None
    for family in hb.MLP_FAMILIES if dims == (512, 512, 512) else ("exact", "randn"):
        c = hb.mlp_case(family, 1089, *dims)
        net = Net(c, d)
        handle = vae._Slot._pools[d.index or 0]["ctx"].handle
        x = c["x"].to(d)
        for chunk, rows in CHUNK_ROWS.items():
            vae.set_option("chunk_rows", chunk, d)
            for R, want_rows in rows.items():
                tag = f"chunk_rows {chunk} R {R}"
                out, recs = _lib.profile(handle, _lib.HG_PROF_ALL, 64, lambda: net(x[:R].contiguous(), book, tag))
                got_rows = [r[1] for r in recs if r[0] == 4]          # EPI_BIAS_F32: the last GEMM of a chunk
                assert got_rows == want_rows + want_rows, (tag, got_rows)
                assert len(recs) == 6 * len(want_rows), (tag, recs)
                book.judge(c, out, tag, rows=slice(0, R))
    book.close()


def test_mlp_net_no_rows(d):
    c = hb.mlp_case("randn", 1089, 64, 128, 128)
    net = Net(c, d)
    assert net.net(torch.zeros(0, 64, device=d)).shape == (0, 128)
