"""Cases, references and wrong-kernel emulations for the grouped MXFP4
expert GEMM (ops/csrc/mxfp4_moe_gemm.hip). Torch only; the CPU tier
(tests/test_mxfp4_moe.py) and the GPU tier (tests/test_mxfp4_moe_gpu.py)
share it.

Weights come from mxfp4_oracle.make_case, one independent seed per expert,
so every expert keeps the per-group exponent jitter, the all-zero group,
code 0x8 and the builder's own asserts. Routing is forced: expert-sorted
pair rows with given segment sizes. x rows that no pair references hold
1e4, so a wrong row index shows.

The acceptance rule is the conformance suite's own (tests/kernel_oracle.py):
``nme(out, ref64) <= MARGIN * E0`` with ref64 = kernel_oracle.moe_grouped in
float64 on the exactly dequantized weights and E0 the nme of the
bf16-rounded fp32 run of the same function. Nothing here comes from the
kernel under test.
"""

from __future__ import annotations

import functools

import torch

import kernel_oracle as ko
import mxfp4_oracle as mo
from tensorlink_amd.models.quant import dequantize_mxfp4

BASE_SEGMENTS = ko.MOE_SEGMENTS          # (130, 64, 0, 6): P = 200, MT = 4
MT1_SEGMENTS = (5, 0, 9, 2)              # P = 16 -> MT = 1
MT2_SEGMENTS = (17, 0, 1, 14)            # P = 32 -> MT = 2
SEGMENT_SETS = {"P200": BASE_SEGMENTS, "P16": MT1_SEGMENTS,
                "P32": MT2_SEGMENTS}
T_ROWS = 48
UNREFERENCED = 1e4


def seg_tensor(segments, device="cpu") -> torch.Tensor:
    seg = torch.zeros(len(segments) + 1, dtype=torch.int32)
    seg[1:] = torch.tensor(segments).cumsum(0)
    return seg.to(device)


def make_case(segments, N: int, K: int, T: int = T_ROWS, seed: int = 0,
              device="cpu"):
    """x [T, K] bf16, per-expert (packed, exps) lists, tok [P] int32, seg
    [E+1] int32. Rows r with r % 4 == 3 are never routed to and, like any
    other row the draw leaves out, hold UNREFERENCED."""
    E = len(segments)
    P = sum(segments)
    gen = torch.Generator().manual_seed(7000 * seed + 13 * N + K + P)
    x = torch.randn(T, K, generator=gen).to(torch.bfloat16)
    allowed = torch.tensor([r for r in range(T) if r % 4 != 3])
    tok = allowed[torch.randint(0, allowed.numel(), (P,), generator=gen)]
    unref = torch.ones(T, dtype=torch.bool)
    unref[tok] = False
    assert int(unref.sum()) >= T // 4
    x[unref] = UNREFERENCED
    packed, exps = [], []
    for e in range(E):
        c = mo.make_case(1, N, K, bias=False, seed=10 * seed + e + 1,
                         device=device)
        packed.append(c["packed"].contiguous())
        exps.append(c["exps"].contiguous())
    return dict(x=x.to(device), tok=tok.to(torch.int32).to(device),
                seg=seg_tensor(segments, device), packed=packed, exps=exps,
                segments=tuple(segments), N=N, K=K)


def exact_weights(case, dtype=ko.F64):
    return [dequantize_mxfp4(p, e).to(dtype)
            for p, e in zip(case["packed"], case["exps"])]


def reference(case, ws=None):
    """(ref64, E0) by kernel_oracle.moe_grouped on the exactly dequantized
    weights (fp32 holds them exactly)."""
    ws = ws if ws is not None else exact_weights(case)
    ref = ko.moe_grouped(case["x"], case["tok"], case["seg"], ws)
    emu = ko.bf16_round(ko.moe_grouped(case["x"], case["tok"], case["seg"],
                                       ws, dtype=torch.float32))
    return ref, ko.nme(emu, ref)


@functools.lru_cache(maxsize=None)
def cpu_case(name: str = "P200", N: int = 128, K: int = 256):
    """A shared CPU case with its reference, computed once."""
    c = make_case(SEGMENT_SETS[name], N, K)
    c["ref"], c["e0"] = reference(c)
    return c


# --------------------------------------------------------------------------
# wrong kernels
# --------------------------------------------------------------------------
MUTANT_EXPERT = 1          # the 64-row segment of the base case
GROUP_MUTANTS = ("last_row_next_expert", "exponents_of_next_expert")
MUTANTS = GROUP_MUTANTS + tuple(f"{m}@e{MUTANT_EXPERT}" for m in mo.MUTANTS)


def mutant_output(name: str, case) -> torch.Tensor:
    """bf16-rounded fp32 output of a plausibly wrong grouped kernel."""
    ws = exact_weights(case, torch.float32)
    E = len(ws)
    flag = False
    if name == "last_row_next_expert":
        flag = True
    elif name == "exponents_of_next_expert":
        # table mismatch: expert e's packed bytes, expert e+1's exponents
        ws = [dequantize_mxfp4(case["packed"][e], case["exps"][(e + 1) % E])
              for e in range(E)]
    else:
        base, at = name.split("@e")
        e = int(at)
        ws[e] = mo.mutant_weights(base, case["packed"][e],
                                  case["exps"][e]).float()
    out = ko.moe_grouped(case["x"], case["tok"], case["seg"], ws,
                         dtype=torch.float32, last_row_next_expert=flag)
    return ko.bf16_round(out)
