"""A/B the grouped MXFP4 expert GEMM (ops/csrc/mxfp4_moe_gemm.hip) against
the other ways the project can run the same expert projection, on the
Mixtral-8x7B and Qwen3-30B-A3B expert shapes. Run on a GPU box:

    python scripts/bench_mxfp4_moe.py [--csv logs/mxfp4_moe.csv]

Per shape and token count T (us per call):
  fp4    ops.mxfp4_moe_gemm -> the grouped kernel, one launch
  loop   the route fp4 experts took before it: the per-expert Python loop
         of MoEMLP.forward through ops.mxfp4_linear (gate_up: mask +
         nonzero + row gather per expert, as the block does; down:
         host-known slices of the pair rows, no sync, which flatters it)
  fp8    C.moe_gemm on fp8 e4m3 weights (in-kernel dequant)
  bf16   C.moe_gemm on bf16 weights
  fp4sN  the grouped kernel with the split count forced to N (only with
         --splits, for judging the split policy)
and the rate of the grouped kernel on the fp4 bytes (packed + exponents) of
the experts actually routed to. That is an algorithmic rate, not a share of
peak: experts with one row and experts with many read the same bytes.

Method: every variant is warmed up, then the variants are timed in
interleaved rounds inside this one process with device events around a
batch of calls; the table gives the median and the minimum over rounds.
Routing is drawn uniformly (k distinct experts per token) from a fixed
seed; calls rotate through 17 such routings and through enough copies of
the whole expert set that the pool exceeds twice the 256 MiB Infinity
Cache, so a weight is not met again while it could still be cached.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorlink_amd import ops  # noqa: E402
from tensorlink_amd.models.quant import (quantize_fp8_per_channel,  # noqa: E402
                                         quantize_mxfp4_rows)

DEV = "cuda"
CACHE_BYTES = 256 << 20
ROUNDS = 7
BATCH_MS = 8.0          # target length of one timed batch
N_ROUTES = 17           # prime: stays out of step with the copy rotation

# name, N, K, E, experts per token
SHAPES = [
    ("mixtral_gate_up", 28672, 4096, 8, 2),
    ("mixtral_down", 4096, 14336, 8, 2),
    ("qwen3_gate_up", 1536, 2048, 128, 8),
    ("qwen3_down", 2048, 768, 128, 8),
]
TOKENS = (1, 8, 64, 256)


def batch_ms(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_variants(variants):
    """variants: {name: fn(i)}. Returns {name: (median_us, min_us)}."""
    iters = {}
    for name, fn in variants.items():
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        est = batch_ms(fn, 3) / 3
        iters[name] = int(max(3, min(400, BATCH_MS / max(est, 1e-3))))
        batch_ms(fn, iters[name])                       # warm-up batch
    samples = {name: [] for name in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            samples[name].append(batch_ms(fn, iters[name]) / iters[name] * 1e3)
    return {n: (statistics.median(s), min(s)) for n, s in samples.items()}


def ptrs(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64,
                        device=DEV)


def build_pool(N, K, E):
    """Copies of one random expert set in all three formats, with their
    pointer tables. Returns (pool, fp4 bytes per expert)."""
    gen = torch.Generator(device=DEV).manual_seed(N + K + E)
    base = dict(packed=[], exps=[], w8=[], s8=[], wb=[])
    for _ in range(E):
        w = torch.randn(N, K, device=DEV, generator=gen) / K ** 0.5
        p, e = quantize_mxfp4_rows(w)
        w8, s8 = quantize_fp8_per_channel(w)
        base["packed"].append(p)
        base["exps"].append(e)
        base["w8"].append(w8.contiguous())
        base["s8"].append(s8.float().contiguous())
        base["wb"].append(w.to(torch.bfloat16))
        del w
    expert_bytes = base["packed"][0].numel() + base["exps"][0].numel()
    n_sets = max(2, -(-2 * CACHE_BYTES // (expert_bytes * E)))
    pool = []
    for s in range(n_sets):
        st = base if s == 0 else {k: [t.clone() for t in v]
                                  for k, v in base.items()}
        st = dict(st)
        for k in ("packed", "exps", "w8", "s8", "wb"):
            st[k + "_ptrs"] = ptrs(st[k])
        pool.append(st)
    return pool, expert_bytes


def build_routes(T, E, k, gen):
    """N_ROUTES uniform routings of T tokens to k distinct experts each,
    in the expert-sorted form MoEMLP._fused_forward builds."""
    routes = []
    for _ in range(N_ROUTES):
        idx = torch.rand(T, E, generator=gen).topk(k, dim=1).indices
        fi = idx.reshape(-1)
        order = fi.argsort(stable=True)
        counts = torch.bincount(fi, minlength=E)
        seg = torch.zeros(E + 1, dtype=torch.int32)
        seg[1:] = counts.cumsum(0)
        routes.append(dict(
            idx=idx.to(DEV), seg=seg.to(DEV), seg_host=seg.tolist(),
            tok=(order // k).to(torch.int32).to(DEV),
            routed=int((counts > 0).sum())))
    return routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv", default=None)
    ap.add_argument("--only", default=None,
                    help="comma-separated shape names to run")
    ap.add_argument("--splits", default=None,
                    help="name:N[,N...] — also time the grouped kernel with "
                         "the split count forced, e.g. mixtral_down:2,4")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    C = ops._require_ext()
    forced = {}
    if args.splits:
        name, ns = args.splits.split(":")
        forced[name] = [int(n) for n in ns.split(",")]
    shapes = SHAPES
    if args.only:
        keep = set(args.only.split(","))
        shapes = [s for s in SHAPES if s[0] in keep]
    rows = []
    for name, N, K, E, k in shapes:
        torch.cuda.empty_cache()
        pool, expert_bytes = build_pool(N, K, E)
        split = C.mxfp4_moe_n_split(N, K, E)
        print(f"# {name}: N{N} K{K} E{E} k{k}, {len(pool)} copies of the "
              f"expert set ({expert_bytes * E / 2**20:.0f} MiB fp4 each), "
              f"policy split {split}", flush=True)
        is_down = name.endswith("down")
        gen = torch.Generator().manual_seed(1234)
        for T in TOKENS:
            routes = build_routes(T, E, k, gen)
            P = T * k
            # gate_up reads token rows through tok_idx; down reads the
            # pair rows themselves
            x = torch.randn(P if is_down else T, K, device=DEV,
                            dtype=torch.bfloat16)

            def pick(i):
                return pool[i % len(pool)], routes[i % N_ROUTES]

            def tok_of(r):
                return None if is_down else r["tok"]

            def run_fp4(i):
                st, r = pick(i)
                return ops.mxfp4_moe_gemm(x, tok_of(r), r["seg"],
                                          st["packed_ptrs"], st["exps_ptrs"],
                                          N)

            def make_forced(ns):
                def run(i):
                    st, r = pick(i)
                    return C.mxfp4_moe_gemm(x, tok_of(r), r["seg"],
                                            st["packed_ptrs"],
                                            st["exps_ptrs"], N,
                                            n_split_override=ns)
                return run

            def run_loop(i):
                st, r = pick(i)
                outs = []
                if is_down:
                    sh = r["seg_host"]
                    for e in range(E):
                        if sh[e + 1] > sh[e]:
                            outs.append(ops.mxfp4_linear(
                                x[sh[e]:sh[e + 1]], st["packed"][e],
                                st["exps"][e]))
                    return outs
                idx = r["idx"]
                for e in range(E):
                    tok, _ = (idx == e).nonzero(as_tuple=True)
                    if tok.numel() == 0:
                        continue
                    outs.append(ops.mxfp4_linear(x[tok], st["packed"][e],
                                                 st["exps"][e]))
                return outs

            def run_fp8(i):
                st, r = pick(i)
                return C.moe_gemm(x, tok_of(r), r["seg"], st["w8_ptrs"],
                                  st["s8_ptrs"], N, True)

            def run_bf16(i):
                st, r = pick(i)
                return C.moe_gemm(x, tok_of(r), r["seg"], st["wb_ptrs"],
                                  None, N, False)

            variants = {"fp4": run_fp4, "loop": run_loop, "fp8": run_fp8,
                        "bf16": run_bf16}
            for ns in forced.get(name, []):
                variants[f"fp4s{ns}"] = make_forced(ns)
            with torch.no_grad():
                before = ops.mxfp4_moe_dispatch_count
                got = run_fp4(0).float()
                assert ops.mxfp4_moe_dispatch_count == before + 1
                ref = run_bf16(0).float()
                err = ((got - ref).abs().max() / ref.abs().max()).item()
                t = time_variants(variants)
            routed = statistics.mean(r["routed"] for r in routes)
            tbs = routed * expert_bytes / (t["fp4"][0] * 1e-6) / 1e12
            line = (f"{name:16s} T{T:4d} P{P:5d} routed {routed:6.1f}: " +
                    " | ".join(f"{v} {t[v][0]:8.1f} (min {t[v][1]:8.1f})"
                               for v in variants) +
                    f" us | fp4 {tbs:5.2f} TB/s | vs bf16 relerr {err:.3f}")
            print(line, flush=True)
            rows.append(dict(name=name, T=T, P=P, routed=routed, tbs=tbs,
                             relerr=err, t=t))
        del pool
    if args.csv:
        d = os.path.dirname(args.csv)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.csv, "w") as f:
            f.write("name,T,P,routed,variant,median_us,min_us,fp4_TBps,"
                    "relerr_vs_bf16\n")
            for r in rows:
                for v, (med, mn) in r["t"].items():
                    f.write(f"{r['name']},{r['T']},{r['P']},"
                            f"{r['routed']:.1f},{v},{med:.2f},{mn:.2f},"
                            f"{r['tbs']:.3f},{r['relerr']:.4f}\n")


if __name__ == "__main__":
    main()
