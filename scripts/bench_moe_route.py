"""Time one MoE layer's routing glue, gate included and the two grouped
GEMMs left out, at the two served model shapes: the torch glue
(nn.Linear gate + reference router + argsort / scatter_add / cumsum +
gather-multiply + inverse permutation + sum), the default route (same
router, ops.moe_plan + ops.moe_combine) and the opt-in fused router
(ops.moe_route + plan + combine). Run on a GPU box:

    python scripts/bench_moe_route.py [--csv out/moe_route.csv]

Each form is timed eagerly (wall time per call, launches included) and as
a captured graph replay (what decode runs); the forms alternate in one
process, several rounds each, and median / min / max are printed, the
min-max range of a form being the run-to-run spread to hold a difference
against. ``sum(1) bits`` says whether the new combine is bit-equal to the
old one on this torch build (at k = 2 it is by construction).
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorlink_amd import ops  # noqa: E402

MODELS = {"mixtral": (8, 2, 4096), "qwen3-30b-a3b": (128, 8, 2048)}
BF16 = torch.bfloat16


def timeit(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def glue_plan(idx, E, k):
    fi = idx.reshape(-1)
    order = fi.argsort(stable=True)
    counts = torch.zeros(E, device=fi.device, dtype=torch.long)
    counts.scatter_add_(0, fi, torch.ones_like(fi))
    seg = torch.zeros(E + 1, device=fi.device, dtype=torch.int32)
    seg[1:] = counts.cumsum(0)
    return seg, (order // k).to(torch.int32), order


def glue_combine(y, rw, order, T, k):
    y = y * rw.reshape(-1)[order].unsqueeze(1)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(T * k, device=y.device, dtype=order.dtype)
    return y[inv].view(T, k, -1).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ts", default="1,8,64,256,4096")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    ops._require_ext()
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name, (E, k, H) in MODELS.items():
        gw = (torch.randn(E, H, device="cuda", generator=gen)
              / H ** 0.5).to(BF16)
        for T in (int(t) for t in args.ts.split(",")):
            x = torch.randn(T, H, device="cuda", generator=gen).to(BF16)
            y = torch.randn(T * k, H, device="cuda", generator=gen).to(BF16)

            def torch_route():
                rw, idx = ops.moe_topk_router(
                    torch.nn.functional.linear(x, gw), k)
                return rw.to(BF16), idx

            def parent():
                rw, idx = torch_route()
                _, _, order = glue_plan(idx, E, k)
                return glue_combine(y, rw, order, T, k)

            def default():
                rw, idx = torch_route()
                _, _, pos = ops.moe_plan(idx, E)
                return ops.moe_combine(y, rw, pos)

            def fused():
                idx, rw, _ = ops.moe_route(x, gw, k)
                _, _, pos = ops.moe_plan(idx, E)
                return ops.moe_combine(y, rw, pos)

            forms = {"parent": parent, "default": default, "fused": fused}
            same = torch.equal(parent(), default())
            graphs = {}
            for f, fn in forms.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                graphs[f] = g
            t = {(f, m): [] for f in forms for m in ("eager", "graph")}
            for _ in range(args.rounds):
                for f, fn in forms.items():
                    t[f, "eager"].append(timeit(fn, args.iters))
                    t[f, "graph"].append(timeit(graphs[f].replay, args.iters))
            for m in ("eager", "graph"):
                cells = "  ".join(
                    f"{f} {statistics.median(t[f, m]):7.1f}us "
                    f"[{min(t[f, m]):7.1f}, {max(t[f, m]):7.1f}]"
                    for f in forms)
                print(f"{name} E{E} k{k} H{H} T{T:5d} {m}: {cells}  "
                      f"sum(1) bits {same}", flush=True)
                rows.append([name, E, k, H, T, m] + [
                    v for f in forms
                    for v in (statistics.median(t[f, m]), min(t[f, m]),
                              max(t[f, m]))] + [same])
    if args.csv:
        os.makedirs(os.path.dirname(args.csv), exist_ok=True)
        with open(args.csv, "w") as f:
            f.write("model,E,k,H,T,mode," + ",".join(
                f"{n}_{s}_us" for n in ("parent", "default", "fused")
                for s in ("med", "min", "max")) + ",combine_bits_equal\n")
            for r in rows:
                f.write(",".join(str(v) for v in r) + "\n")


if __name__ == "__main__":
    main()
