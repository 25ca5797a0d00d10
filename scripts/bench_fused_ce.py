"""Time the fused linear cross-entropy (ops/csrc/head_ce.hip through
ops.linear_cross_entropy) against the torch route it replaces
(ops/reference.py::_ChunkedCELoss, chunk 1024) at the Qwen2.5-7B head:
V = 152064, H = 3584, forward plus backward. Run on a GPU box:

    python scripts/bench_fused_ce.py [--rows 2048,8192,32736] [--out DIR]

Every timed run is a child process of its own under its own time limit,
one at a time; nothing is tried twice, and the first child that fails ends
the script. A child prints one JSON line: median and min wall time per
forward+backward (device-synchronised), and the peak of
torch.cuda.max_memory_allocated above what the operands themselves take.
``--grid`` children time the two kernels alone in both grid orders.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

V, H = 152064, 3584


def _sync_time(fn, iters):
    import torch
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def _operands(rows):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(0)
    w = (torch.randn(V, H, device="cuda", generator=gen) / H ** 0.5).to(
        torch.bfloat16)
    x = torch.randn(rows, H, device="cuda", generator=gen).to(torch.bfloat16)
    labels = torch.randint(0, V, (rows,), device="cuda", generator=gen)
    labels[::17] = -100
    return x, w, labels


def child_route(route, rows, iters):
    import torch
    from tensorlink_amd import ops
    from tensorlink_amd.ops import reference as ref
    assert torch.cuda.is_available(), "needs a GPU"
    ops._require_ext()
    x, w, labels = _operands(rows)
    x.requires_grad_()
    w.requires_grad_()

    def step():
        x.grad = w.grad = None
        if route == "fused":
            loss = ops.linear_cross_entropy(x, w, labels)
        else:
            loss = ref._ChunkedCELoss.apply(x, w, labels, 1024)
        loss.backward()
        return loss

    for _ in range(2):
        loss = step()
    x.grad = w.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ts = _sync_time(step, iters)
    peak = torch.cuda.max_memory_allocated() - base
    print(json.dumps({"route": route, "rows": rows, "ms": statistics.median(ts),
                      "ms_min": min(ts), "ms_max": max(ts),
                      "peak_extra_mb": peak / 2 ** 20, "loss": float(loss)}))


def child_grid(rows, iters):
    import torch
    from tensorlink_amd import ops
    C = ops._require_ext()
    x, w, labels = _operands(rows)
    lse, _ = C.head_ce_stats(x, w, labels)
    scale = torch.full((rows,), 1.0 / rows, device="cuda")
    res = {"grid": True, "rows": rows}
    fl = 2.0 * rows * V * H / 1e9          # GFLOP per kernel
    for rows_fast in (1, 0, 1, 0):
        def stats():
            C.head_ce_stats(x, w, labels, rows_fast=rows_fast)

        def grad():
            C.head_ce_grad(x, w, labels, lse, scale, rows_fast=rows_fast)

        for name, fn in (("stats", stats), ("grad", grad)):
            fn()
            t = statistics.median(_sync_time(fn, iters))
            key = f"{name}_{'rows' if rows_fast else 'panels'}_fast_ms"
            res.setdefault(key, []).append(round(t, 3))
            res[f"{name}_tflops_last"] = round(fl / t, 1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="2048,8192,32736")
    ap.add_argument("--grid-rows", default="4096,8192")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240,
                    help="seconds each child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None)
    args = ap.parse_args()
    if args.child:
        if args.child[0] == "grid":
            child_grid(int(args.child[1]), args.iters)
        else:
            child_route(args.child[0], int(args.child[1]), args.iters)
        return

    jobs = [["grid", r] for r in args.grid_rows.split(",") if r]
    for r in args.rows.split(","):
        jobs += [["torch", r], ["fused", r]]
    lines = []
    for job in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), "--iters",
               str(args.iters), "--child"] + job
        try:
            p = subprocess.run(cmd, capture_output=True, text=True,
                               timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f"{job}: over its {args.limit} s limit; stopping",
                  flush=True)
            sys.exit(124)
        if p.returncode != 0:
            print(f"{job}: exit {p.returncode}; stopping\n{p.stderr[-2000:]}",
                  flush=True)
            sys.exit(p.returncode if p.returncode > 0 else 1)
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "fused_ce.jsonl"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
