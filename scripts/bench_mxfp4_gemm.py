"""A/B the MXFP4 weight-only GEMM (ops/csrc/mxfp4_gemm.hip) against the
other ways the project can run the same projection, on the Qwen2.5-7B
serving shapes. Run on a GPU box:

    python scripts/bench_mxfp4_gemm.py [--csv logs/mxfp4_gemm.csv]

Per shape, four times (us per call):
  fp4   ops.mxfp4_linear -> the new kernel
  bf16  C.skinny_gemm on bf16 weights (streaming / tiled family)
  fp8   Fp8Linear's kernel route (moe_gemm.hip, in-kernel e4m3 dequant)
  old   the former Fp4Linear.forward: fp32 dequant per call + F.linear
and the effective TB/s of the new kernel on the fp4 bytes
(N*K/2 packed + N*K/32 exponents).

Method: every variant is warmed up, then the variants are timed in
interleaved rounds inside this one process with device events around a
batch of calls; the table gives the median and the minimum over rounds.
Weights rotate through enough copies to exceed the 256 MiB Infinity
Cache, as a decode step that walks all layers sees them: a single 8 MB
fp4 panel would otherwise be served from cache and overstate the rate.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorlink_amd import ops  # noqa: E402
from tensorlink_amd.models.quant import (Fp8Linear, dequantize_mxfp4,  # noqa: E402
                                         quantize_fp8_per_channel,
                                         quantize_mxfp4)

DEV = "cuda"
CACHE_BYTES = 256 << 20
ROUNDS = 7
BATCH_MS = 8.0          # target length of one timed batch


def quantize_rows(w, rows=4096):
    """quantize_mxfp4 in row blocks (its argmin temporary is 32 B per
    weight)."""
    ps, es = zip(*(quantize_mxfp4(w[i:i + rows])
                   for i in range(0, w.shape[0], rows)))
    return torch.cat(ps), torch.cat(es)


def n_copies(nbytes):
    return max(1, min(64, -(-2 * CACHE_BYTES // nbytes)))


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


def old_fp4_forward(x, packed, exps):
    w = dequantize_mxfp4(packed, exps, dtype=torch.float32)
    return torch.nn.functional.linear(x.float(), w).to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv", default=None)
    ap.add_argument("--only", default=None,
                    help="comma-separated shape names to run")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    C = ops._require_ext()
    proj = [(4608, 3584, "qkv"), (3584, 3584, "o"),
            (37888, 3584, "gate_up"), (3584, 18944, "down")]
    shapes = [(M, N, K, f"{name}_m{M}") for M in (1, 16, 64)
              for N, K, name in proj]
    shapes += [
        # the serving-M list of scripts/bench_gemm.py
        (256, 4608, 3584, "qkv"),
        (256, 3584, 3584, "o"),
        (256, 37888, 3584, "gate_up"),
        (256, 3584, 18944, "down"),
        (256, 151936, 3584, "lm_head"),
        (512, 4608, 3584, "qkv_m512"),
        (512, 37888, 3584, "gate_up_m512"),
        (512, 3584, 18944, "down_m512"),
        (128, 4608, 3584, "qkv_m128"),
        (96, 4608, 3584, "qkv_m96"),
    ]
    if args.only:
        keep = set(args.only.split(","))
        shapes = [s for s in shapes if s[3] in keep]
    shapes.sort(key=lambda s: (s[2], s[1]))     # one weight set per (N, K)
    rows = []
    cache = {}
    for M, N, K, name in shapes:
        if (N, K) not in cache:
            cache.clear()                       # one weight set at a time
            torch.cuda.empty_cache()
            gen = torch.Generator(device=DEV).manual_seed(N + K)
            w = torch.randn(N, K, device=DEV, generator=gen) / K ** 0.5
            packed, exps = quantize_rows(w)
            w8, s8 = quantize_fp8_per_channel(w)
            wb = w.to(torch.bfloat16)
            del w
            fp4_bytes = packed.numel() + exps.numel()
            cache[(N, K)] = dict(
                fp4=[(packed.clone(), exps.clone())
                     for _ in range(n_copies(fp4_bytes))],
                bf16=[wb.clone() for _ in range(n_copies(wb.numel() * 2))],
                fp8=[Fp8Linear(w8.clone(), s8.clone())
                     for _ in range(n_copies(w8.numel()))],
                fp4_bytes=fp4_bytes)
        c = cache[(N, K)]
        x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
        f4, b16, f8 = c["fp4"], c["bf16"], c["fp8"]

        def run_fp4(i):
            p, e = f4[i % len(f4)]
            return ops.mxfp4_linear(x, p, e)

        def run_bf16(i):
            return C.skinny_gemm(x, b16[i % len(b16)], None)

        def run_fp8(i):
            return f8[i % len(f8)](x)

        def run_old(i):
            p, e = f4[i % len(f4)]
            return old_fp4_forward(x, p, e)

        with torch.no_grad():
            before = ops.mxfp4_dispatch_count
            got = run_fp4(0).float()
            assert ops.mxfp4_dispatch_count == before + 1, "kernel not used"
            ref = old_fp4_forward(x, *f4[0]).float()
            err = ((got - ref).abs().max() / ref.abs().max()).item()
            t = time_variants({"fp4": run_fp4, "bf16": run_bf16,
                               "fp8": run_fp8, "old": run_old})
        tbs = c["fp4_bytes"] / (t["fp4"][0] * 1e-6) / 1e12
        line = (f"{name:14s} M{M:4d} N{N:6d} K{K:6d}: "
                f"fp4 {t['fp4'][0]:8.1f} (min {t['fp4'][1]:8.1f}) us "
                f"{tbs:5.2f} TB/s | bf16 {t['bf16'][0]:8.1f} "
                f"(min {t['bf16'][1]:8.1f}) | fp8 {t['fp8'][0]:8.1f} "
                f"(min {t['fp8'][1]:8.1f}) | old {t['old'][0]:9.1f} "
                f"(min {t['old'][1]:9.1f}) | relerr {err:.4f}")
        print(line, flush=True)
        rows.append((name, M, N, K) + t["fp4"] + (round(tbs, 3),) + t["bf16"]
                    + t["fp8"] + t["old"] + (err,))
    if args.csv:
        d = os.path.dirname(args.csv)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.csv, "w") as f:
            f.write("name,M,N,K,fp4_us,fp4_min_us,fp4_TBps,bf16_us,"
                    "bf16_min_us,fp8_us,fp8_min_us,old_us,old_min_us,"
                    "relerr\n")
            for r in rows:
                f.write(",".join(f"{v:.3f}" if isinstance(v, float) else
                                 str(v) for v in r) + "\n")


if __name__ == "__main__":
    main()
