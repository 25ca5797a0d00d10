"""CP ring attention on one GPU: the last rank of cp = 4 over local chunks.

    python scripts/bench_cp_attn.py [--tokens 4096] [--rounds 5] [--out f.json]

Three routes over the same four K/V chunks (diagonal chunk first, earlier
chunks descending, as the ring delivers them), timed in alternating rounds
so drift hits all of them:

  (a) torch math   parallel/cp.py with TL_NO_CP_KERNEL=1: a [B,Hq,Sq,Sk] fp32
                   score tensor per step, elementwise (o, m, l) merges
  (b) carried      one carried-state prefill kernel call per step, fp32
                   state updated in place
  (c) one call     _C.prefill_attn with Sq = tokens, Skv = 4 * tokens,
                   q_off = 3 * tokens: the same FLOPs with no state traffic

Peak memory is what each route allocates above the inputs. TF counts the
causal half of the diagonal chunk plus three full chunks."""
import argparse, json, os, sys, time, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tensorlink_amd import ops, _C
from tensorlink_amd.parallel import cp

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=4096, help="tokens per rank")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--iters-math", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the result as JSON")
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_cp_attn.py needs a GPU"
assert "TL_NO_CP_KERNEL" not in os.environ

WORLD, RANK = 4, 3
B, Hq, Hkv, D, sc = 1, 28, 4, 128, args.tokens
scale = D ** -0.5
g = torch.Generator(device="cuda").manual_seed(0)
q = torch.randn(B, sc, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g)
k = torch.randn(B, WORLD * sc, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
v = torch.randn(B, WORLD * sc, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g)
# each ring step's chunk is a buffer of its own, as a received chunk is
chunks = [(c, k[:, c*sc:(c+1)*sc].contiguous(), v[:, c*sc:(c+1)*sc].contiguous())
          for c in range(WORLD)]
steps = [chunks[(RANK - r) % WORLD] for r in range(WORLD)]

def math_route():
    os.environ["TL_NO_CP_KERNEL"] = "1"
    try:
        return cp._ring_accumulate(q, scale, RANK, iter(steps))
    finally:
        del os.environ["TL_NO_CP_KERNEL"]

def carried_route():
    return cp._ring_accumulate(q, scale, RANK, iter(steps))

def one_call():
    return _C.prefill_attn(q, k, v, scale, True, RANK * sc)

def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms

def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2**20

n0 = ops.attn_carry_dispatch_count
o_a, o_b, o_c = math_route().float(), carried_route().float(), one_call().float()
assert ops.attn_carry_dispatch_count == n0 + RANK + 1, "carried route did not run the kernel"
err_b, err_a = (o_b - o_c).abs().max().item(), (o_a - o_c).abs().max().item()
del o_a, o_b, o_c
mem_a, mem_b = peak_mb(math_route), peak_mb(carried_route)

ta, tb, tc = [], [], []
for _ in range(args.rounds):
    ta.append(timeit(math_route, args.iters_math))
    tb.append(timeit(carried_route, args.iters))
    tc.append(timeit(one_call, args.iters))

flops = 2 * 2 * B * Hq * sc * sc * D * (RANK + 0.5)
state_mb = 2 * RANK * (q.numel() * 4 + B * Hq * sc * 8) / 1e6   # stores + loads
tf = lambda ms: flops / ms / 1e9
f = lambda ts: " ".join(f"{t:.3f}" for t in ts)
res = {"tokens_per_rank": sc, "B": B, "Hq": Hq, "Hkv": Hkv, "D": D,
       "math_ms": ta, "carried_ms": tb, "one_call_ms": tc,
       "carried_over_one_call": min(tb) / min(tc),
       "math_over_carried": min(ta) / min(tb),
       "math_peak_mb": mem_a, "carried_peak_mb": mem_b,
       "state_traffic_mb": state_mb,
       "carried_vs_one_call_max_abs": err_b, "math_vs_one_call_max_abs": err_a}
print(f"cp=4 last rank, {sc} tokens/rank, Hq {Hq} Hkv {Hkv} D {D}: {flops/1e12:.2f} TFLOP, "
      f"state traffic {state_mb:.0f} MB"
      f"\n  (a) torch math ms [{f(ta)}]  best {min(ta):.3f} ({tf(min(ta)):.0f} TF)  peak {mem_a:.0f} MB"
      f"\n  (b) carried    ms [{f(tb)}]  best {min(tb):.3f} ({tf(min(tb)):.0f} TF)  peak {mem_b:.0f} MB"
      f"\n  (c) one call   ms [{f(tc)}]  best {min(tc):.3f} ({tf(min(tc)):.0f} TF)"
      f"\n  (b)/(c) {min(tb)/min(tc):.3f}   (a)/(b) {min(ta)/min(tb):.2f}x"
      f"\n  max abs vs (c): carried {err_b:.3e}  torch math {err_a:.3e}", flush=True)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh)
