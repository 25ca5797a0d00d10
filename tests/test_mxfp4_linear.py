"""CPU tier of the MXFP4 weight-only linear: the op-layer route, the
exactness premise of the kernel's dequant, and proof that the acceptance
rule of tests/test_mxfp4_gemm_gpu.py rejects plausibly wrong kernels."""

import pytest
import torch
import torch.nn.functional as F

import kernel_oracle as ko
import mxfp4_oracle as mo
from tensorlink_amd import ops
from tensorlink_amd.models.quant import (Fp4Linear, dequantize_mxfp4,
                                         quantize_mxfp4)


def _old_forward(x, packed, exps, bias):
    """What Fp4Linear.forward computed before the op existed."""
    w = dequantize_mxfp4(packed, exps, dtype=torch.float32)
    y = F.linear(x.float(), w, bias.float() if bias is not None else None)
    return y.to(x.dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("bias", [False, True])
def test_op_equals_dequant_linear_on_cpu(dtype, bias):
    c = mo.cpu_case(bias=bias)
    x = c["x"].to(dtype)
    b = c["b"].to(dtype) if bias else None
    before = ops.mxfp4_dispatch_count
    out = ops.mxfp4_linear(x, c["packed"], c["exps"], b)
    assert out.dtype == dtype and out.shape == (x.shape[0], 64)
    assert torch.equal(out, _old_forward(x, c["packed"], c["exps"], b))
    assert ops.mxfp4_dispatch_count == before, "CPU must not count a kernel"
    # leading dims pass through
    out3 = ops.mxfp4_linear(x.view(2, -1, x.shape[-1]), c["packed"],
                            c["exps"], b)
    assert torch.equal(out3.reshape(out.shape), out)


def test_fp4linear_module_equals_op():
    torch.manual_seed(0)
    lin = torch.nn.Linear(256, 128, bias=True)
    q = Fp4Linear.from_linear(lin)
    x = torch.randn(3, 5, 256)
    with torch.no_grad():
        out = q(x)
        want = _old_forward(x, q.packed, q.exponents, lin.bias)
    assert torch.equal(out, want)
    assert sorted(n for n, _ in q.named_buffers()) == ["exponents", "packed"]


def test_quant_module_still_exports_the_format_functions():
    from tensorlink_amd.models import quant
    from tensorlink_amd.ops import reference
    assert quant.dequantize_mxfp4 is reference.dequantize_mxfp4
    p, e = quant.quantize_mxfp4(torch.randn(4, 64))
    assert p.shape == (4, 32) and p.dtype == torch.uint8
    assert e.shape == (4, 2) and e.dtype == torch.int8


def _wide_exponent_weights():
    """Every code under every exponent in -120..120 (hand-built)."""
    es = torch.arange(-120, 121, dtype=torch.int8)            # 241 groups
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)     # one group
    packed_g = codes[0::2] | (codes[1::2] << 4)               # 16 bytes
    packed = packed_g.repeat(es.numel()).view(1, -1)
    return packed, es.view(1, -1)


def test_dequant_is_exact_in_bf16():
    c = mo.cpu_case()
    w32 = dequantize_mxfp4(c["packed"], c["exps"])
    w16 = dequantize_mxfp4(c["packed"], c["exps"], dtype=torch.bfloat16)
    assert torch.equal(w16.float(), w32)
    p, e = _wide_exponent_weights()
    w32 = dequantize_mxfp4(p, e)
    assert torch.isfinite(w32).all()
    assert float(w32.abs().max()) == 6.0 * 2.0 ** 120
    assert float(w32[w32 != 0].abs().min()) == 0.5 * 2.0 ** -120
    assert torch.equal(dequantize_mxfp4(p, e, dtype=torch.bfloat16).float(),
                       w32)


def test_table_plus_exponent_add_is_exact_with_zero_bypass():
    """The integer dequant (bf16 table + e << 7) equals the float one for
    every code and exponent in range — if +-0 skip the add."""
    p, e = _wide_exponent_weights()
    assert torch.equal(mo.table_add_dequant(p, e).float(),
                       dequantize_mxfp4(p, e))
    c = mo.cpu_case()
    assert torch.equal(mo.table_add_dequant(c["packed"], c["exps"]).float(),
                       c["w32"])


def test_all_zero_group_quantizes_to_exponent_minus_42():
    w = torch.randn(2, 64)
    w[:, 32:] = 0
    p, e = quantize_mxfp4(w)
    assert e[:, 1].tolist() == [-42, -42]
    assert int(p[:, 16:].max()) == 0


def test_true_emulation_meets_the_rule():
    c = mo.cpu_case()
    out = ko.bf16_round(ko.linear(c["x"], c["w32"], c["b"],
                                  dtype=torch.float32))
    assert ko.nme(out, c["ref"]) <= ko.tolerance(c["e0"])
    K = c["x"].shape[1]
    want = mo.onehot_expected(c["packed"], c["exps"], 0, K)
    got = ko.linear(mo.onehot_rows(K, 0, K), c["w32"],
                    dtype=torch.float32).to(torch.bfloat16)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", mo.MUTANTS)
def test_mutant_is_rejected(name):
    c = mo.cpu_case()
    wm = mo.mutant_weights(name, c["packed"], c["exps"])
    out = ko.bf16_round(ko.linear(c["x"], wm, c["b"], dtype=torch.float32))
    err = ko.nme(out, c["ref"])
    tol = ko.tolerance(c["e0"])
    K = c["x"].shape[1]
    want = mo.onehot_expected(c["packed"], c["exps"], 0, K)
    got = ko.linear(mo.onehot_rows(K, 0, K), wm,
                    dtype=torch.float32).to(torch.bfloat16)
    onehot_differs = not torch.equal(got, want)
    print(f"MUTANT {name}: nme {err:.3e} tol {tol:.3e} "
          f"ratio {err / tol:.1f} onehot_differs {onehot_differs}")
    # each one misses the nme rule by >= 2x AND fails the exact layout
    # check (either alone would do)
    assert err >= 2 * tol, (name, err, tol)
    assert onehot_differs, name
