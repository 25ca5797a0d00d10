"""Windowed training attention timing: forward + backward of
ops.attention_train at B=2, Hq=32, Hkv=8, D=128, W=4096.

    python scripts/bench_swa_train.py
    python scripts/bench_swa_train.py --parent-ext /path/to/parent/_C*.so
    TL_NO_GRAPH=1 rocprofv3 --kernel-trace --stats -d OUT -- \\
        python scripts/bench_swa_train.py --profile

Arms, alternating over --rounds rounds so drift hits all of them:
  window   the windowed HIP route
  plain    the unwindowed HIP route at the same S (window = 0)
  sdpa     the SDPA band-mask composition (TL_NO_SWA_TRAIN=1, read per call)
Each figure is ms per forward + backward (host clock around a device
synchronise), best and worst round; peak memory is per arm, over one call.
--parent-ext loads a second build of the extension (the parent commit's)
and times its unwindowed backward kernels against this build's in the same
rounds, after checking the gradients bit-equal. --profile runs a few calls
of the window and plain arms only, for a kernel trace."""
import argparse, importlib.util, os, sys, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensorlink_amd import _C, ops

ap = argparse.ArgumentParser()
ap.add_argument("--parent-ext", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--lengths", type=int, nargs="+", default=[4096, 8192, 16384])
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"

PARENT = None
if args.parent_ext:
    spec = importlib.util.spec_from_file_location("_C", args.parent_ext)
    PARENT = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(PARENT)

def timeit(fn, iters):
    for _ in range(2): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms

def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20

def run(name, arms, base):
    ts = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            # the O(S^2) composition is seconds per call at 16k
            ts[a].append(timeit(fn, 2 if a == "sdpa" else args.iters))
    print(name)
    for a, t in ts.items():
        print(f"  {a:<12} best {min(t):9.3f} ms  worst {max(t):9.3f} ms"
              f"  {base}/this {min(ts[base]) / min(t):5.2f}x", flush=True)

B, Hq, Hkv, D, W = 2, 32, 8, 128, 4096
sc = D ** -0.5
for S in args.lengths:
    q, k, v = (torch.randn(B, S, h, D, device="cuda", dtype=torch.bfloat16)
               .requires_grad_(True) for h in (Hq, Hkv, Hkv))
    dout = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16)

    def step(window, sdpa=False):
        if sdpa:
            os.environ["TL_NO_SWA_TRAIN"] = "1"
        try:
            out = ops.attention_train(q, k, v, scale=sc, window=window)
        finally:
            os.environ.pop("TL_NO_SWA_TRAIN", None)
        out.backward(dout)
        q.grad = k.grad = v.grad = None

    arms = {"window": lambda: step(W), "plain": lambda: step(0)}
    if args.profile:
        for fn in arms.values():
            for _ in range(3): fn()
        torch.cuda.synchronize()
        continue
    arms["sdpa"] = lambda: step(W, sdpa=True)
    # (query, key) pairs visited: S^2/2 causal, W*S - W^2/2 in the band
    pairs = (S * S / 2) / (W * S - W * W / 2)
    run(f"fwd+bwd S={S} W={W}: causal/band pairs {pairs:.2f}x", arms, "plain")
    print(f"  peak MiB over one call: window {peak_mib(arms['window']):.0f}"
          f"  sdpa {peak_mib(arms['sdpa']):.0f}", flush=True)

    # backward kernels alone: WIN = 1 against WIN = 0 (and the parent's)
    with torch.no_grad():
        def saved(window):
            out, lse = _C.prefill_attn_lse(q, k, v, sc, True, window)
            delta = (dout.float() * out.float()).sum(-1)
            return lse, delta.permute(0, 2, 1).contiguous()
        l0, d0 = saved(0)
        lw, dw = saved(W)
        bw = {"plain": lambda: _C.attn_bwd(q, k, v, dout, l0, d0, sc, True, 0),
              "window": lambda: _C.attn_bwd(q, k, v, dout, lw, dw, sc, True, W)}
        if PARENT:
            bw["parent"] = lambda: PARENT.attn_bwd(q, k, v, dout, l0, d0, sc,
                                                   True)
            for a, b in zip(bw["parent"](), bw["plain"]()):
                assert torch.equal(a, b)
        run(f"backward kernels S={S} W={W}", bw, "plain")
    del q, k, v, dout, l0, d0, lw, dw
    torch.cuda.empty_cache()
