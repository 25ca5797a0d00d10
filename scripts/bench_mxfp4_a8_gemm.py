"""A/B the MXFP4 x MXFP8 path (ops/csrc/mxfp4_a8_gemm.hip: activation
quantizer + scaled-MFMA GEMM) against today's fp4-dense route and bf16, on
the Qwen2.5-7B projections. Run on a GPU box:

    python scripts/bench_mxfp4_a8_gemm.py [--csv logs/mxfp4_a8_gemm.csv]

Per shape (us per call, median over rounds):
  quant  C.mx_quant_act alone
  gemm   C.mxfp4_a8_gemm alone, on ready codes
  a8     ops.mxfp4_linear(act_quant="mxfp8") with the threshold at 1: both
  fp4    ops.mxfp4_linear as fp4-dense runs it today: mxfp4_gemm.hip up to
         M = 512, per-call dequant + F.linear above
  bf16   ops.linear on bf16 weights
The smallest M of {65, 96, 128, 256} from which a8 beats fp4 on all four
projections is the default of ops.MXFP4_A8_M_MIN (profiles/mxfp4_a8_gemm.md;
M = 64 is listed as the row below every candidate).

Method as in scripts/bench_mxfp4_gemm.py, whose helpers this script uses:
warm-up, interleaved rounds in one process, device events around batches,
weights rotating through copies that exceed the Infinity Cache.

--accuracy adds the cost of quantizing activations: nme of the a8 output
against the weight-only float64 reference on tests/mxfp4_oracle cases.
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import bench_mxfp4_gemm as base  # noqa: E402
from tensorlink_amd import ops  # noqa: E402

DEV = "cuda"
PROJ = [(4608, 3584, "qkv"), (3584, 3584, "o"), (37888, 3584, "gate_up"),
        (3584, 18944, "down")]
MS = (64, 96, 128, 256, 512, 2048, 8192)


def accuracy():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import kernel_oracle as ko
    import mxfp4_oracle as mo
    for N, K in ((320, 1024), (4608, 512), (4608, 3584)):
        c = mo.make_case(513, N, K, bias=False, device=DEV)
        w64 = mo.dequant64(c["packed"], c["exps"])
        ref64, emu = mo.reference(c["x"], w64, None)
        a8 = ops.mxfp4_linear(c["x"], c["packed"], c["exps"],
                              act_quant="mxfp8")
        w4 = ops.mxfp4_linear(c["x"][:512], c["packed"], c["exps"])
        print(f"accuracy N{N} K{K}: nme vs weight-only f64: "
              f"a8 {ko.nme(a8, ref64):.3e}  weight-only kernel "
              f"{ko.nme(w4, ref64[:512]):.3e}  bf16-rounded fp32 "
              f"{ko.nme(emu, ref64):.3e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csv", default=None)
    ap.add_argument("--only", default=None,
                    help="comma-separated projection names to run")
    ap.add_argument("--accuracy", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    C = ops._require_ext()
    ops.MXFP4_A8_M_MIN = 1
    base.ROUNDS = 5
    if args.accuracy:
        accuracy()
    keep = set(args.only.split(",")) if args.only else None
    rows = []
    for N, K, name in PROJ:
        if keep and name not in keep:
            continue
        torch.cuda.empty_cache()
        gen = torch.Generator(device=DEV).manual_seed(N + K)
        w = torch.randn(N, K, device=DEV, generator=gen) / K ** 0.5
        packed, exps = base.quantize_rows(w)
        wb = w.to(torch.bfloat16)
        del w
        f4 = [(packed.clone(), exps.clone()) for _ in range(
            base.n_copies(packed.numel() + exps.numel()))]
        b16 = [wb.clone() for _ in range(base.n_copies(wb.numel() * 2))]
        for M in MS:
            x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
            xq, xs = C.mx_quant_act(x)

            def run_quant(i):
                return C.mx_quant_act(x)

            def run_gemm(i):
                p, e = f4[i % len(f4)]
                return C.mxfp4_a8_gemm(xq, xs, p, e, None)

            def run_a8(i):
                p, e = f4[i % len(f4)]
                return ops.mxfp4_linear(x, p, e, act_quant="mxfp8")

            def run_fp4(i):
                p, e = f4[i % len(f4)]
                return ops.mxfp4_linear(x, p, e)

            def run_bf16(i):
                return ops.linear(x, b16[i % len(b16)])

            with torch.no_grad():
                before = ops.mxfp4_a8_dispatch_count
                run_a8(0)
                assert ops.mxfp4_a8_dispatch_count == before + 1
                t = base.time_variants({"quant": run_quant, "gemm": run_gemm,
                                        "a8": run_a8, "fp4": run_fp4,
                                        "bf16": run_bf16})
            tf = 2.0 * M * N * K / (t["gemm"][0] * 1e-6) / 1e12
            print(f"{name:8s} M{M:5d} N{N:6d} K{K:6d} tile "
                  f"{C.mxfp4_a8_tile(M, N):3d}: quant {t['quant'][0]:7.1f} "
                  f"gemm {t['gemm'][0]:8.1f} ({tf:6.1f} TF) a8 "
                  f"{t['a8'][0]:8.1f} | fp4 {t['fp4'][0]:9.1f} "
                  f"({t['fp4'][0] / t['a8'][0]:5.2f}x) | bf16 "
                  f"{t['bf16'][0]:8.1f} ({t['bf16'][0] / t['a8'][0]:5.2f}x)",
                  flush=True)
            rows.append((name, M, N, K, t["quant"][0], t["gemm"][0],
                         t["a8"][0], t["fp4"][0], t["bf16"][0]))
        del f4, b16, packed, exps, wb
    if args.csv:
        d = os.path.dirname(args.csv)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(args.csv, "w") as f:
            f.write("name,M,N,K,quant_us,gemm_us,a8_us,fp4_us,bf16_us\n")
            for r in rows:
                f.write(",".join(f"{v:.1f}" if isinstance(v, float) else
                                 str(v) for v in r) + "\n")


if __name__ == "__main__":
    main()
