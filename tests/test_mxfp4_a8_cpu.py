"""CPU tier of the MXFP4 x MXFP8 path: the MXFP8 activation format on
hand-worked groups (ops.reference.quantize_mxfp8 is the contract of the
HIP quantizer) and the reference linear behind act_quant="mxfp8"."""

import torch

import mxfp4_oracle as mo
from tensorlink_amd import ops
from tensorlink_amd.ops import reference as ref

BF16 = torch.bfloat16


def _group(**at):
    x = torch.zeros(1, 32)
    for i, v in at.items():
        x[0, int(i[1:])] = v
    return x.to(BF16)


def test_spec_on_hand_worked_groups():
    # amax = 1.0: floor(log2) - 8 + 127 = 119; 1.0 / 2^-8 = 256 = 2^8
    codes, scales = ref.quantize_mxfp8(_group(k0=1.0, k5=-0.5))
    assert scales.tolist() == [[119]]
    assert codes.dtype == torch.uint8 and codes.shape == (1, 32)
    assert codes[0, 0] == (15 << 3) and codes[0, 5] == 0x80 | (14 << 3)
    # all-zero group
    codes, scales = ref.quantize_mxfp8(_group())
    assert scales.tolist() == [[0]] and int(codes.sum()) == 0
    # the top of the binade saturates: 1.99 * 2^5 -> 509 -> 448
    x = _group(k3=1.99 * 2 ** 5, k4=-1.99 * 2 ** 5)
    codes, scales = ref.quantize_mxfp8(x)
    assert scales.tolist() == [[127 + 5 - 8]]
    back = ref.dequantize_mxfp8(codes, scales)
    assert back[0, 3] == 448 * 2.0 ** -3 and back[0, 4] == -448 * 2.0 ** -3
    # ties to even: with amax 256 the unit is 2^0 and [16, 32) steps by 2
    x = _group(k0=256.0, k1=17.0, k2=19.0, k3=21.0)
    codes, scales = ref.quantize_mxfp8(x)
    assert scales.tolist() == [[127]]
    assert ref.dequantize_mxfp8(codes, scales)[0, :4].tolist() == \
        [256.0, 16.0, 20.0, 20.0]


def test_roundtrip_is_exact_where_the_group_fits_e4m3():
    gen = torch.Generator().manual_seed(3)
    # 4-bit significands below the saturating top (15 -> 480 > 448) over
    # seven binades, times a per-group power of two
    vals = torch.randint(8, 15, (5, 4, 32), generator=gen).float()
    vals = vals * torch.pow(2.0, torch.randint(-6, 1, (5, 4, 32),
                                               generator=gen).float())
    vals = vals * torch.where(torch.rand(5, 4, 32, generator=gen) < 0.5,
                              -1.0, 1.0)
    vals[..., 0] = 14.0                         # amax: 448 after scaling
    jit = torch.pow(2.0, torch.randint(-30, 30, (5, 4, 1),
                                       generator=gen).float())
    x = (vals * jit).reshape(5, 128).to(BF16)
    codes, scales = ref.quantize_mxfp8(x)
    assert torch.equal(ref.dequantize_mxfp8(codes, scales, BF16), x)
    assert torch.equal(ref.dequantize_mxfp8(codes, scales, torch.float64),
                       x.double())


def test_cpu_linear_is_the_reference():
    c = mo.cpu_case()
    x, p, e, b = c["x"], c["packed"], c["exps"], c["b"]
    got = ops.mxfp4_linear(x, p, e, b, act_quant="mxfp8")
    want = ref.mxfp4_a8_linear(x, p, e, b)
    assert got.dtype == BF16 and torch.equal(got, want)
    # the quantized path is a different function of x ...
    plain = ops.mxfp4_linear(x, p, e, b)
    assert not torch.equal(got, plain)
    # ... and act_quant=None is today's
    assert torch.equal(plain, ref.mxfp4_linear(x, p, e, b))
    assert torch.equal(plain, ops.mxfp4_linear(x, p, e, b, act_quant=None))
