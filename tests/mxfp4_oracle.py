"""Cases, references and wrong-kernel emulations ("mutants") for the MXFP4
weight-only GEMM (ops/csrc/mxfp4_gemm.hip). Torch only; the CPU tier
(tests/test_mxfp4_linear.py) and the GPU tier
(tests/test_mxfp4_gemm_gpu.py) share it.

The acceptance rule is the conformance suite's own (tests/kernel_oracle.py):
``nme(out, ref64) <= MARGIN * E0`` with ref64 the float64 linear on the
exactly dequantized weights and E0 the nme of the bf16-rounded fp32 linear
on the same weights. Nothing here comes from the kernel under test.
"""

from __future__ import annotations

import functools

import torch

import kernel_oracle as ko
from tensorlink_amd.models.quant import dequantize_mxfp4, quantize_mxfp4

GROUP = 32
KSTEP = 128               # k per main-loop step of the kernel
# bf16 bit patterns of the e2m1 magnitudes {0,.5,1,1.5,2,3,4,6}
E2M1_BF16_BITS = (0x0000, 0x3F00, 0x3F80, 0x3FC0, 0x4000, 0x4040, 0x4080,
                  0x40C0)


def unpack_codes(packed: torch.Tensor) -> torch.Tensor:
    """[N, K/2] uint8 -> [N, K] 4-bit codes (element 2i = low nibble)."""
    N = packed.shape[0]
    code = torch.empty(N, packed.shape[1] * 2, dtype=torch.uint8,
                       device=packed.device)
    code[:, 0::2] = packed & 0xF
    code[:, 1::2] = packed >> 4
    return code


def dequant64(packed, exponents) -> torch.Tensor:
    """Exact weights in float64 (fp32 already holds them exactly)."""
    return dequantize_mxfp4(packed, exponents).to(ko.F64)


def make_case(M: int, N: int, K: int, bias: bool, seed: int = 0,
              device="cpu"):
    """x ~ N(0,1) bf16; w ~ N(0,1)/sqrt(K) with a per-group scale jitter
    2^U{-12..8} (one row mixes exponents) and one all-zero group per row
    (exponent -42, all codes 0); quantized with quantize_mxfp4 on
    ``device``. The builder checks that the case can show the faults the
    tests are after: code 0x8 present, >= 10 distinct exponents, low and
    high nibbles differing."""
    assert K % GROUP == 0
    gen = torch.Generator().manual_seed(1000 * seed + N + K)
    G = K // GROUP
    x = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    w = torch.randn(N, G, GROUP, generator=gen) / K ** 0.5
    jit = torch.randint(-12, 9, (N, G), generator=gen).float()
    w = w * torch.pow(2.0, jit).unsqueeze(-1)
    zg = torch.randint(0, G, (N,), generator=gen)
    w[torch.arange(N), zg] = 0.0
    b = torch.randn(N, generator=gen).to(torch.bfloat16) if bias else None
    packed, exps = quantize_mxfp4(w.reshape(N, K).to(device))
    code = unpack_codes(packed)
    assert bool((code == 0x8).any()), "no negative-zero code in the case"
    assert exps.unique().numel() >= 10, "too few distinct exponents"
    assert bool((exps[torch.arange(N), zg.to(exps.device)] == -42).all())
    differ = ((packed & 0xF) != (packed >> 4)).float().mean()
    assert float(differ) > 0.5, "nibble positions too often equal"
    dev = packed.device
    return dict(x=x.to(dev), packed=packed, exps=exps,
                b=b.to(dev) if b is not None else None, zero_group=zg)


def reference(x, w_exact, b):
    """(ref64, emu): the float64 linear and the bf16-rounded fp32 linear
    on the same exactly dequantized weights (w_exact: fp32 or fp64)."""
    ref = ko.linear(x, w_exact, b)
    emu = ko.bf16_round(ko.linear(x, w_exact, b, dtype=torch.float32))
    return ref, emu


def onehot_expected(packed, exps, k_lo: int, k_hi: int) -> torch.Tensor:
    """Expected output of one-hot rows k_lo..k_hi-1: dequant(W)^T rows, in
    bf16 (exact)."""
    w = dequantize_mxfp4(packed, exps, dtype=torch.bfloat16)
    return w[:, k_lo:k_hi].t().contiguous()


def onehot_rows(K: int, k_lo: int, k_hi: int, device="cpu") -> torch.Tensor:
    x = torch.zeros(k_hi - k_lo, K, dtype=torch.bfloat16, device=device)
    x[torch.arange(k_hi - k_lo), torch.arange(k_lo, k_hi)] = 1.0
    return x


# --------------------------------------------------------------------------
# emulations: a correct table + exponent-add dequant, and wrong kernels
# --------------------------------------------------------------------------
def table_add_dequant(packed, exps, bypass_zero: bool = True,
                      sign_bit: int = 3) -> torch.Tensor:
    """The in-register dequant a kernel may use: code -> bf16 bits through
    the 8-entry magnitude table, plus an integer add of e into the bf16
    exponent field (e << 7), in 16-bit arithmetic; the sign goes to bit
    15. bypass_zero=False pushes the +-0 codes through the add as well
    (the mutant). Returns bf16 [N, K]."""
    code = unpack_codes(packed).to(torch.int32)
    tbl = torch.tensor(E2M1_BF16_BITS, dtype=torch.int32,
                       device=packed.device)
    mag = tbl[(code & 7).long()]
    e = exps.to(torch.int32).repeat_interleave(GROUP, -1)
    added = (mag + (e << 7)) & 0xFFFF
    if bypass_zero:
        added = torch.where((code & 7) == 0, torch.zeros_like(added), added)
    sign = ((code >> sign_bit) & 1) << 15
    bits = (added | sign) & 0xFFFF
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    return bits.view(torch.bfloat16)


def mutant_weights(name: str, packed, exps) -> torch.Tensor:
    """fp32 [N, K] weights as a plausibly wrong kernel would see them."""
    if name == "swapped_nibbles":
        sw = ((packed >> 4) | (packed << 4)) & 0xFF
        return dequantize_mxfp4(sw.to(torch.uint8), exps)
    if name == "neighbour_exponent":
        return dequantize_mxfp4(packed, torch.roll(exps, 1, dims=1))
    if name == "exponent_off_by_one":
        e = exps.clone()
        e[:, 1] += 1                       # one group of every row
        return dequantize_mxfp4(packed, e)
    if name == "zero_through_add":
        return table_add_dequant(packed, exps, bypass_zero=False).float()
    if name == "sign_from_bit2":
        return table_add_dequant(packed, exps, sign_bit=2).float()
    if name == "last_kstep_dropped":
        w = dequantize_mxfp4(packed, exps).clone()
        w[:, -KSTEP:] = 0.0
        return w
    raise KeyError(name)


MUTANTS = ("swapped_nibbles", "neighbour_exponent", "exponent_off_by_one",
           "zero_through_add", "sign_from_bit2", "last_kstep_dropped")


@functools.lru_cache(maxsize=None)
def cpu_case(M: int = 16, N: int = 64, K: int = 384, bias: bool = True):
    """The shared CPU case with its reference, computed once."""
    c = make_case(M, N, K, bias)
    w32 = dequantize_mxfp4(c["packed"], c["exps"])
    ref, emu = reference(c["x"], w32, c["b"])
    c.update(w32=w32, ref=ref, e0=ko.nme(emu, ref))
    return c
