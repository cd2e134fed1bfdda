"""The CoOp-VAE kernels - hg_vae_fused.hip as one kernel (option vae_fused = 2), the GEMM path (0) and the default hybrid (1) of
hg_heads.hip, launch_reparam of hg_elem.hip - held PER OUTPUT ELEMENT to the float64 CPU reference and the stage-wise rounding bound of
tests/vae_bound.py, and bit for bit to its two exact families, through vae.Encoder / vae.Generator / vae.VAE (direct ABI calls where a
test says so):

* hidden widths (128, 128), (128, 384), (384, 128) - a stream of a few iterations that wraps inside the eight-slot ring, eh != gh in
  both directions - and (2048, 4096), (4096, 2048); 1 .. 257 rows; every input family; the four outputs of VAE, the two of an
  Encoder-only slot, the Generator alone;
* a workgroup that walks the weight stream twice, and the default hybrid on both sides of its row boundaries (with the launch of the one
  kernel confirmed by hg_profile), chunks of 256 rows on the GEMM path;
* hg_generator on a slot that also holds an encoder (the stream offset by the encoder's passes);
* every output set of hg_vae_forward, with NaN canary rows in front of and behind each requested output.

Every test prints VAE_RATIO lines (worst |err| / E per family, path and output); tests/vae_bound.py's docstring carries them as a table.
tests/test_vae_rounding_model.py proves on the CPU which wrong kernels the bound and the exact families reject."""
import ctypes as C

import pytest
import torch

import vae_bound as vb
from hoigen_amd import _lib, vae
from hoigen_amd.model import _stream_ptr

pytestmark = pytest.mark.gpu
R0 = 257
ROWS = (1, 31, 32, 33, 127, 128, 129, 257)
SMALL = [(128, 128), (128, 384), (384, 128)]
LARGE = [(2048, 4096), (4096, 2048)]
CASES = [(eh, gh, f) for eh, gh in SMALL for f in vb.FAMILIES] + [(eh, gh, f) for eh, gh in LARGE for f in ("rounded", "unit", "outlier")]
PATHS = {2: "one", 0: "gemm", 1: "hybrid"}
CANARY = 0x7FC0DEAD          # a quiet NaN with a payload


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture()
def d():
    dv = dev()
    chunk = vae.get_option("chunk_rows", dv)
    yield dv
    vae.set_option("vae_fused", 1, dv)
    vae.set_option("chunk_rows", chunk, dv)


class Nets:
    """Encoder, Generator and VAE of a case on the device, and the case's inputs"""

    def __init__(self, c, dv):
        self.c = c
        self.E, self.G = vae.Encoder(vb.DIM, c["eh"]).to(dv), vae.Generator(vb.DIM, c["gh"]).to(dv)
        self.E.load_state_dict({"net.0.weight": c["e_w0"], "net.0.bias": c["e_b0"], "mean.weight": c["e_wm"], "mean.bias": c["e_bm"],
                                "log_var.weight": c["e_wl"], "log_var.bias": c["e_bl"]})
        self.G.load_state_dict({"net.0.weight": c["g_w0"], "net.0.bias": c["g_b0"], "net.2.weight": c["g_w2"], "net.2.bias": c["g_b2"]})
        self.V = vae.VAE(self.E, self.G)
        self.x, self.eps, self.zg = c["x"].to(dv), c["eps"].to(dv), c["zg"].to(dv)
        self.enc_ref = vb.enc_reference(c)
        self.exact = vb.exact_expected(c) if c["family"] in vb.EXACT_FAMILIES else None

    def enc_rows(self, rows):
        return {n: (w[rows], E[rows]) for n, (w, E) in self.enc_ref.items()}


class Book:
    """worst ratios per (path, output) and the failures of one test"""

    def __init__(self, c):
        self.c, self.worst, self.failures = c, {}, []

    def judge(self, nets, path, got, rows, what, operands=None):
        """got: {name: device tensor of the case's rows `rows`}: in bound, and bit for bit where the family is exact"""
        cpu = {k: v.cpu() for k, v in got.items()}
        ops = {k: v.cpu() for k, v in operands.items()} if operands else None
        r = vb.ratios(self.c, cpu, rows=rows, enc_ref=nets.enc_rows(rows), operands=ops)
        for k, v in r.items():
            self.worst[(path, k)] = max(self.worst.get((path, k), 0.0), v)
            if not v <= 1.0:
                self.failures.append(f"{what} {k}: worst |err| / E {v:.3f}")
        if nets.exact is not None:
            for k in cpu:
                if k in nets.exact and not torch.equal(cpu[k], nets.exact[k][rows]):
                    n_bad = int((cpu[k] != nets.exact[k][rows]).sum())
                    self.failures.append(f"{what} {k}: {n_bad} elements are not the float64 result bit for bit")

    def close(self):
        c = self.c
        print()
        for (path, k), v in sorted(self.worst.items()):
            print(f"VAE_RATIO {c['family']} {path} {k} eh {c['eh']} gh {c['gh']}: worst |err| / E {v:.3f}")
        assert not self.failures, self.failures


def named(t):
    return dict(zip(vb.NAMES, t))


@pytest.mark.parametrize("eh,gh,family", CASES)
def test_widths_rows_families_paths(d, eh, gh, family):
    """VAE, Encoder alone (a slot with [E0 | E1] only, mode 1) and Generator alone (has_enc = false) as one kernel and on the GEMM
    path; the exact families on the default option as well (at these row counts it takes the GEMM path)"""
    c = vb.make_case(family, eh, gh, R0)
    nets, book = Nets(c, d), Book(c)
    for opt in (2, 0, 1) if family in vb.EXACT_FAMILIES else (2, 0):
        vae.set_option("vae_fused", opt, d)
        for R in ROWS if (eh, gh) in SMALL else (1, 129, 257):
            rows, what = slice(0, R), f"option {opt} R {R}"
            book.judge(nets, PATHS[opt], named(nets.V(nets.x[:R], nets.eps[:R])), rows, what + " VAE")
            book.judge(nets, PATHS[opt], dict(zip(("mean", "log_var"), nets.E(nets.x[:R]))), rows, what + " Encoder")
            book.judge(nets, PATHS[opt], {"gen": nets.G(nets.zg[:R])}, rows, what + " Generator")
    book.close()


def tiled(nets, R, seed):
    """R rows drawn (seeded, with repetition) from the case's 257: a row's result does not depend on its position, so every row's
    expectation is known -> (idx, x, eps, zg)"""
    idx = torch.randint(0, R0, (R,), generator=torch.Generator().manual_seed(seed))
    di = idx.to(nets.x.device)
    return idx, nets.x[di], nets.eps[di], nets.zg[di]


def sample_rows(R, must, seed, n):
    extra = torch.randint(0, R, (n,), generator=torch.Generator().manual_seed(seed)).tolist()
    return torch.tensor(sorted({r for r in list(must) + extra if 0 <= r < R}))


def judge_sampled(nets, book, path, got, idx, sample, what):
    ds = sample.to(nets.x.device)
    book.judge(nets, path, {k: v[ds] for k, v in got.items()}, idx[sample], what)
    if nets.exact is not None:      # every row, on the device
        for k, v in got.items():
            if k in nets.exact and not torch.equal(v, nets.exact[k].to(v.device)[idx.to(v.device)]):
                book.failures.append(f"{what} {k}: some row is not the float64 result bit for bit")


@pytest.mark.parametrize("family", ["randn", "rounded"])
def test_a_workgroup_walks_the_stream_twice(d, family):
    """More items than CUs at (128, 384): the stream offset wraps to 0 at the item's end and the next item walks it again from a ring
    position that is not the first one's.  Reference on the first and last row of the first item, of the items on both sides of the
    first round's end and of the last (partly filled) item, and on 64 seeded rows."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R = 128 * n_cu + 129
    c = vb.make_case(family, 128, 384, R0)
    nets, book = Nets(c, d), Book(c)
    idx, x, eps, zg = tiled(nets, R, 11)
    must = [0, 127, 128 * (n_cu - 1), 128 * n_cu - 1, 128 * n_cu, 128 * n_cu + 127, 128 * (n_cu + 1), R - 1]
    sample = sample_rows(R, must, 12, 64)
    vae.set_option("vae_fused", 2, d)
    judge_sampled(nets, book, "one", named(nets.V(x, eps)), idx, sample, f"R {R} VAE")
    judge_sampled(nets, book, "one", dict(zip(("mean", "log_var"), nets.E(x))), idx, sample, f"R {R} Encoder")
    judge_sampled(nets, book, "one", {"gen": nets.G(zg)}, idx, sample, f"R {R} Generator")
    book.close()


@pytest.mark.parametrize("eh,gh,family", [(128, 384, "randn"), (128, 384, "rounded"), (2048, 4096, "randn"), (2048, 4096, "rounded")])
def test_the_default_hybrid(d, eh, gh, family):
    """Option 1 with one full round of items and 129 rows more: Encoder and reparameterisation of every row on the GEMM path in chunks,
    the Generator of the first 128 n_cu rows as the one kernel on the fp16 z that launch_reparam wrote, of the rest as GEMMs.  Rows on
    both sides of that boundary and of row 32 768 (the default chunk size), the first and the last row, 16 seeded rows."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    Rf = 128 * n_cu
    R = Rf + 129
    c = vb.make_case(family, eh, gh, R0)
    nets, book = Nets(c, d), Book(c)
    idx, x, eps, zg = tiled(nets, R, 21)
    sample = sample_rows(R, [0, Rf - 1, Rf, 32767, 32768, R - 1], 22, 16)
    vae.set_option("vae_fused", 1, d)
    nets.V(x[:1], eps[:1])          # (weights packed outside the profiled call)
    handle = vae._Slot._pools[d.index or 0]["ctx"].handle
    got, recs = _lib.profile(handle, 102, 16, lambda: nets.V(x, eps))          # HG_PROF_VAE_FUSED
    assert [r[:4] for r in recs] == [(102, Rf, 1, gh)], f"the Generator of the first {Rf} rows did not run as the one kernel: {recs}"
    judge_sampled(nets, book, "hybrid", named(got), idx, sample, f"R {R} VAE")
    gen, recs = _lib.profile(handle, 102, 16, lambda: nets.G(zg))
    assert [r[:4] for r in recs] == [(102, Rf, 1, gh)], recs
    judge_sampled(nets, book, "hybrid", {"gen": gen}, idx, sample, f"R {R} Generator")
    book.close()


@pytest.mark.parametrize("family", ["randn", "rounded"])
def test_gemm_path_across_chunk_boundaries(d, family):
    """chunk_rows = 256 and 700 rows on the GEMM path: chunks of 256, 256 and 188 rows; every row judged"""
    c = vb.make_case(family, 128, 384, R0)
    nets, book = Nets(c, d), Book(c)
    R = 700
    idx, x, eps, zg = tiled(nets, R, 31)
    vae.set_option("vae_fused", 0, d)
    vae.set_option("chunk_rows", 256, d)
    every = torch.arange(R)
    judge_sampled(nets, book, "gemm", named(nets.V(x, eps)), idx, every, "chunks of 256 VAE")
    judge_sampled(nets, book, "gemm", dict(zip(("mean", "log_var"), nets.E(x))), idx, every, "chunks of 256 Encoder")
    judge_sampled(nets, book, "gemm", {"gen": nets.G(zg)}, idx, every, "chunks of 256 Generator")
    book.close()


def abi_call(nets, dv, fn):
    """fn(lib, handle, slot) on the VAE object's slot, in the session the facade uses (the weights are loaded by a facade call first)"""
    nets.V(nets.x[:1], nets.eps[:1])
    with nets.V._slot.session(dv) as (ctx, h, slot, fresh):
        assert not fresh
        ctx.check(fn(_lib.lib(), h, slot), "direct ABI call")


@pytest.mark.parametrize("eh,gh", [(128, 384), (2048, 4096)])
def test_generator_on_a_slot_that_holds_an_encoder(d, eh, gh):
    """hg_generator on the VAE's slot as one kernel: has_enc = true, the Generator's pass behind the two encoder passes of the stream"""
    vae.set_option("vae_fused", 2, d)
    for family in ("rounded", "randn"):
        c = vb.make_case(family, eh, gh, R0)
        nets, book = Nets(c, d), Book(c)
        for R in (1, 129, 257):
            out = torch.empty(R, vb.DIM, device=d)
            zg = nets.zg[:R].contiguous()
            abi_call(nets, d, lambda l, h, slot: l.hg_generator(h, slot, zg.data_ptr(), R, out.data_ptr(), _stream_ptr(d)))
            book.judge(nets, "one", {"gen": out}, slice(0, R), f"hg_generator on the VAE slot R {R}")
        book.close()


OUTPUT_SETS = [("mean",), ("log_var",), ("z",), ("bias",), ("z", "bias"), vb.NAMES]


@pytest.mark.parametrize("opt", [2, 0])
def test_partial_outputs_and_canaries(d, opt):
    """hg_vae_forward with every output set at (128, 384): each requested output has a row in front of it and 128 rows behind row R
    filled with a NaN bit pattern.  Requested outputs are in bound and equal the all-four call bit for bit; no canary row changes (the one
    kernel drops the rows >= R of an item by the size of its buffer descriptors, and gives a tensor nobody asked for a size of 0)."""
    c = vb.make_case("randn", 128, 384, R0)
    nets, book = Nets(c, d), Book(c)
    vae.set_option("vae_fused", opt, d)
    for R in (1, 33, 129):
        x, eps = nets.x[:R].contiguous(), nets.eps[:R].contiguous()
        full = None
        for names in [vb.NAMES] + OUTPUT_SETS:
            bufs = {n: torch.full((1 + R + 128, vb.DIM), CANARY, dtype=torch.int32, device=d) for n in names}
            ptr = [C.c_void_p(bufs[n][1:].data_ptr()) if n in bufs else None for n in vb.NAMES]
            abi_call(nets, d, lambda l, h, slot: l.hg_vae_forward(h, slot, x.data_ptr(), eps.data_ptr(), R, *ptr, _stream_ptr(d)))
            torch.cuda.synchronize()
            what = f"option {opt} R {R} outputs {'+'.join(names)}"
            got = {}
            for n, b in bufs.items():
                if not (bool((b[0] == CANARY).all()) and bool((b[1 + R:] == CANARY).all())):
                    rows_hit = torch.nonzero((b != CANARY).any(1)).flatten().tolist()
                    book.failures.append(f"{what}: {n} written outside rows [0, {R}): buffer rows {[r - 1 for r in rows_hit if r < 1 or r > R]}")
                got[n] = b[1:1 + R].view(torch.float32)
            if full is None:
                full = got
            for n in names:
                if not torch.equal(got[n].view(torch.int32), full[n].view(torch.int32)):
                    book.failures.append(f"{what}: {n} differs from the call that asked for all four")
            book.judge(nets, PATHS[opt], got, slice(0, R), what, operands=full)
    book.close()
