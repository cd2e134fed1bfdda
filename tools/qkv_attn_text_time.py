"""Diagnostics: the text tower's fused in_proj + causal attention kernel (hg_qkv_attn_text.hip, option qkv_attn_text) against the two
kernels it replaces, same process, alternating.
  kernel : hipEvent pairs around every launch (hg_profile_*) through hg_test_qkv_attn, random operands, a sweep over (sequences, L, heads)
  tower  : encode_text over the 600 HICO prompts (77 tokens / truncated) and encode_text_embeds over a generation step's 14-token prompts,
           option 0 against 2 in both text_ln_fold forms, wall time per call
WHAT="kernel tower" selects; ROUNDS alternations (default 5)."""
import json, os, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import torch
from hoigen_amd import _lib

WHAT = os.environ.get("WHAT", "kernel tower").split()
ROUNDS = int(os.environ.get("ROUNDS", 5))


def kernel_sweep():
    ctx = _lib.ctx(0)
    L_ = _lib.lib()
    shapes = [(600, 77, 8), (512, 77, 8), (300, 77, 8), (128, 77, 8), (64, 77, 8), (198, 77, 12), (600, 13, 8), (1800, 14, 8), (7200, 14, 8)]
    print("kernel level, us per launch (median of the medians over %d alternations; min): separate = folded GEMM (kind 8) + causal attention (100)" % ROUNDS)
    for n_seq, L, heads in shapes:
        D = heads * 64
        g = torch.Generator(device="cuda").manual_seed(1)
        a = torch.randn(n_seq * L, D, device="cuda", generator=g)
        w = torch.randn(3 * D, D, device="cuda", generator=g) * D ** -0.5
        bias = torch.randn(3 * D, device="cuda", generator=g) * 0.3
        cs = w.half().float().sum(1)
        mr = torch.stack([torch.randn(n_seq * L, device="cuda", generator=g) * 0.05, torch.rand(n_seq * L, device="cuda", generator=g) + 0.5], 1).contiguous()
        out = torch.empty(n_seq * L, D, device="cuda")

        def run(fused):
            rc = L_.hg_test_qkv_attn(ctx, a.data_ptr(), w.data_ptr(), bias.data_ptr(), cs.data_ptr(), mr.data_ptr(), n_seq, L, heads, fused,
                                     out.data_ptr(), None)
            assert rc == 0, L_.hg_last_error(ctx)

        def timed(fused, iters=8):
            def body():
                for _ in range(iters):
                    run(fused)
                torch.cuda.synchronize()
            _, recs = _lib.profile(ctx, _lib.HG_PROF_ALL, 4 * iters + 8, body)
            by = {}
            for kind, M, N, K, ms in recs:
                by.setdefault(kind, []).append(ms * 1e3)
            return {k: sorted(v)[len(v) // 2] for k, v in by.items()}

        run(4); run(5)
        sep, gem, att, fus = [], [], [], []
        for _ in range(ROUNDS):
            u = timed(4)
            f = timed(5)
            assert 8 in u and 100 in u and _lib.HG_PROF_QKV_ATTN in f, (sorted(u), sorted(f))      # GEMM epilogue kind 8 (EPI_LN_BIAS_F16), attention 100
            gem.append(u[8]); att.append(u[100]); sep.append(u[8] + u[100]); fus.append(f[_lib.HG_PROF_QKV_ATTN])
        med = lambda v: sorted(v)[len(v) // 2]
        G = 160 // L
        items = (n_seq + G - 1) // G * (heads // 2)
        print(f"  {n_seq:5d} x {L:2d} x {heads:2d} heads ({items:5d} items = {items / 256:6.2f} rounds): GEMM {med(gem):7.1f} + attention {med(att):6.1f} = "
              f"{med(sep):7.1f} (min {min(sep):7.1f})   fused {med(fus):7.1f} (min {min(fus):7.1f})   fused / separate {med(fus) / med(sep):.3f}", flush=True)
        del a, w, out
    torch.cuda.empty_cache()


def wall(fn, n):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def tower():
    from hoigen_amd import clip, synth
    from hoigen_amd.model import build_model
    dev = torch.device("cuda:0")
    m = build_model(synth.to_torch(synth.clip_state_dict(synth.VIT_B16, 0))).to(dev)
    g0 = json.load(open(os.path.join(HERE, "tests", "golden", "g0_tokens.json")))
    ids = clip.tokenize(g0["hoi600"]["text"]).to(dev)
    gen_ids = ids.repeat(12, 1)                       # 7 200 prompts: a generation step's worth (4 iterations x 1 800), truncated to 13 tokens
    gen_emb = m.token_embedding(gen_ids).float()
    cases = [("encode_text 600 x 77", lambda: m.encode_text(ids), False, 20), ("encode_text 600 truncated", lambda: m.encode_text(ids), True, 20),
             ("encode_text_embeds 7200 truncated", lambda: m.encode_text_embeds(gen_emb, gen_ids), True, 10)]
    print("tower level, ms per call, option qkv_attn_text 0 / 2 alternating (%d alternations: median; min .. max)" % ROUNDS)
    for fold in (1, 2):
        m.set_option("text_ln_fold", fold)
        for name, fn, trunc, n in cases:
            m.truncate_text = trunc
            t = {0: [], 2: []}
            for _ in range(ROUNDS):
                for mode in (0, 2):
                    m.set_option("qkv_attn_text", mode)
                    t[mode].append(wall(fn, n))
            med = lambda v: sorted(v)[len(v) // 2]
            print(f"  text_ln_fold {fold} | {name:34s} | 0: {med(t[0]):7.3f} ({min(t[0]):7.3f} .. {max(t[0]):7.3f}) | 2: {med(t[2]):7.3f} "
                  f"({min(t[2]):7.3f} .. {max(t[2]):7.3f}) | 2 / 0 = {med(t[2]) / med(t[0]):.3f}", flush=True)
            # per-launch kernel time inside the tower (hipEvent pairs)
            for mode in (0, 2):
                m.set_option("qkv_attn_text", mode)
                _, recs = _lib.profile(m._ctx.handle, _lib.HG_PROF_ALL, 256, fn)
                by = {}
                for kind, M, N, K, ms in recs:
                    by.setdefault((kind, N if kind < 100 else 0), []).append(ms * 1e3)
                sel = {k: v for k, v in by.items() if k in ((8, 3 * 512), (100, 0), (101, 0))}
                print("      option %d, us per launch (median x count): " % mode +
                      ", ".join(f"kind {k[0]}: {sorted(v)[len(v) // 2]:.1f} x {len(v)}" for k, v in sorted(sel.items())), flush=True)
    m.set_option("qkv_attn_text", 0)
    m.truncate_text = True


if "kernel" in WHAT:
    kernel_sweep()
if "tower" in WHAT:
    tower()
