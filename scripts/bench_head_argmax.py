"""Time the fused greedy head (ops/csrc/head_argmax.hip) against the pair it
replaces — the family GEMM writing [M, N] logits plus ATen's argmax over
them — at the Qwen2.5-7B lm_head shape. Run on a GPU box:

    python scripts/bench_head_argmax.py [--csv out/head_argmax.csv]

Wall times per call (launches included) are printed; for kernel times run
it under ``rocprofv3 --kernel-trace --stats -- python scripts/
bench_head_argmax.py --iters 20`` and read head_argmax_kernel +
head_combine_kernel against gemm_tiled_sq_kernel (skinny_gemm_kernel at
M <= 64) + reduce_kernel. The two forms alternate in one process, several
rounds each, and the median is reported.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorlink_amd import ops  # noqa: E402


def timeit(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=151936)
    ap.add_argument("--k", type=int, default=3584)
    ap.add_argument("--ms", default="256,1,16,64,128,512")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    C = ops._require_ext()
    N, K = args.n, args.k
    assert C.gemm_n_split(N, K) == 1
    gen = torch.Generator(device="cuda").manual_seed(0)
    w = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).to(
        torch.bfloat16)
    rows = []
    for M in (int(m) for m in args.ms.split(",")):
        x = torch.randn(M, K, device="cuda", generator=gen).to(torch.bfloat16)

        def pair():
            return C.skinny_gemm(x, w, None).argmax(-1)

        def fused():
            return C.lm_head_argmax(x, w)

        same = torch.equal(pair(), fused())
        for _ in range(5):
            pair()
            fused()
        t_pair, t_fused = [], []
        for _ in range(args.rounds):
            t_pair.append(timeit(pair, args.iters))
            t_fused.append(timeit(fused, args.iters))
        tp, tf = statistics.median(t_pair), statistics.median(t_fused)
        wb = N * K * 2 / 1e9
        fl = 2.0 * M * N * K / 1e12
        print(f"lm_head M{M:4d} N{N} K{K}: gemm+argmax {tp:7.1f}us "
              f"(min {min(t_pair):7.1f})  fused {tf:7.1f}us "
              f"(min {min(t_fused):7.1f}, {wb / tf * 1e3:5.2f} TB/s W, "
              f"{fl / tf * 1e6:5.0f} TF)  tokens equal {same}", flush=True)
        rows.append((M, N, K, tp, min(t_pair), tf, min(t_fused), same))
    if args.csv:
        os.makedirs(os.path.dirname(args.csv), exist_ok=True)
        with open(args.csv, "w") as f:
            f.write("M,N,K,pair_us,pair_min_us,fused_us,fused_min_us,"
                    "tokens_equal\n")
            for r in rows:
                f.write(",".join(str(v) for v in r) + "\n")


if __name__ == "__main__":
    main()
