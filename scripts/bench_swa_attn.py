"""Sliding-window attention timing: windowed prefill / decode kernels
against the unwindowed ones.

    python scripts/bench_swa_attn.py
    python scripts/bench_swa_attn.py --parent-ext /path/to/parent/_C*.so

Arms alternate over --rounds rounds so drift hits all of them; each figure
is ms per call (host clock around a device synchronise), best and worst
round. --parent-ext loads a second build of the extension (the parent
commit's) and times its window = 0 kernels in the same rounds, after
checking its outputs bit-equal."""
import argparse, importlib.util, os, sys, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensorlink_amd import _C

ap = argparse.ArgumentParser()
ap.add_argument("--parent-ext", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"

PARENT = None
if args.parent_ext:
    spec = importlib.util.spec_from_file_location("_C", args.parent_ext)
    PARENT = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(PARENT)

def timeit(fn, iters):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms

def run(name, arms):
    ts = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            ts[a].append(timeit(fn, args.iters))
    base = min(ts["plain"])
    print(name)
    for a, t in ts.items():
        print(f"  {a:<12} best {min(t):8.3f} ms  worst {max(t):8.3f} ms"
              f"  plain/this {base / min(t):5.2f}x", flush=True)

# ---- prefill: B=4, Hq=32, Hkv=8, D=128, W=4096 ----
B, Hq, Hkv, D, W = 4, 32, 8, 128, 4096
for S in (4096, 8192, 16384):
    q = torch.randn(B, S, Hq, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, S, Hkv, D, device="cuda", dtype=torch.bfloat16)
    sc = D ** -0.5
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    arms = {
        "plain": lambda: _C.prefill_attn(q, k, v, sc, True, 0),
        "window": lambda: _C.prefill_attn(q, k, v, sc, True, 0, W),
        # the route ops.attention_prefill takes for an unwindowed model here
        "sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(
            qt, kt, vt, is_causal=True, scale=sc, enable_gqa=True),
    }
    if PARENT:
        arms["parent"] = lambda: PARENT.prefill_attn(q, k, v, sc, True, 0)
        assert torch.equal(arms["parent"](), arms["plain"]())
    # keys a row visits: ~S/2 plain, ~W - W^2/(2S) windowed
    keys = W - W * W / (2 * S)
    run(f"prefill S={S} W={W}: keys/row {S / 2:.0f} -> {keys:.0f} "
        f"({S / 2 / keys:.2f}x fewer)", arms)
    del q, k, v, qt, kt, vt

# ---- decode: B=256, Hq=28, Hkv=4, D=128, L=8192 ----
B, Hq, Hkv, D, L = 256, 28, 4, 128, 8192
q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16)
kc = torch.randn(B, Hkv, L, D, device="cuda", dtype=torch.bfloat16)
vc = torch.randn(B, Hkv, L, D, device="cuda", dtype=torch.bfloat16)
lens = torch.full((B,), L, device="cuda", dtype=torch.int32)
sc = D ** -0.5
arms = {"plain": lambda: _C.decode_attn(q, kc, vc, lens, sc, 0, None, 0)}
for w in (1024, 4096):
    arms[f"window {w}"] = (lambda w=w: _C.decode_attn(q, kc, vc, lens, sc, 0,
                                                      None, 0, w))
if PARENT:
    arms["parent"] = lambda: PARENT.decode_attn(q, kc, vc, lens, sc, 0, None, 0)
    assert torch.equal(arms["parent"](), arms["plain"]())
run(f"decode B={B} L={L}", arms)
