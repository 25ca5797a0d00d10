"""GPU tier of the MXFP4 x MXFP8 path (ops/csrc/mxfp4_a8_gemm.hip) on
MI355X: quantizer bytes, exact operand layout (one-hot), float64-oracle
conformance under the suite's own rule (tests/kernel_oracle.py), the bit
contract across M, row position and tile instantiation, routing, and the
fp4-dense-a8 model path with captured decode. ``CONF`` lines show with -s."""

import functools
import os

import pytest
import torch

import kernel_oracle as ko
import mxfp4_oracle as mo
from tensorlink_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
M_FULL = 513
ALL_M = (1, 17, 255, 256, 257, 513)
# (N, K) -> the M subset run on it (the large shape subset to stay at seconds)
SHAPES = {
    (64, 128): ALL_M,
    (192, 384): ALL_M,
    (320, 1024): ALL_M,
    (4608, 512): (1, 257, 513),
}


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


@pytest.fixture
def m_min_1(monkeypatch):
    """Every M takes the new path."""
    monkeypatch.setattr(_ops(), "MXFP4_A8_M_MIN", 1)


def _kernel(x, packed, exps, b=None):
    """ops.mxfp4_linear(act_quant="mxfp8"), asserting that the scaled-MFMA
    kernel took the call."""
    ops = _ops()
    before = ops.mxfp4_a8_dispatch_count
    out = ops.mxfp4_linear(x, packed, exps, b, act_quant="mxfp8")
    assert ops.mxfp4_a8_dispatch_count == before + 1, "not the a8 kernel"
    return out


def _forced(x, packed, exps, b, tile):
    C = _ops()._C
    xq, xs = C.mx_quant_act(x.contiguous())
    return C.mxfp4_a8_gemm(xq, xs, packed, exps, b, tile)


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """One 513-row case per shape, with the float64 reference and its fp32
    twin on the MXFP8-dequantized activations, computed once on the GPU."""
    c = mo.make_case(M_FULL, N, K, bias=True, device=DEV)
    w64 = mo.dequant64(c["packed"], c["exps"])
    xq64 = ref.dequantize_mxfp8(*ref.quantize_mxfp8(c["x"]), dtype=ko.F64)
    for tag, b in (("nobias", None), ("bias", c["b"])):
        c["ref_" + tag], c["emu_" + tag] = mo.reference(xq64, w64, b)
    return c


# --------------------------------------------------------------------------
# 1. quantizer bytes
# --------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(1, 128), (17, 384), (257, 1024)])
def test_quantizer_bytes_equal_the_reference(M, K):
    gen = torch.Generator().manual_seed(M + K)
    G = K // 32
    x = torch.randn(M, G, 32, generator=gen)
    x = x * torch.pow(2.0, torch.randint(-20, 21, (M, G, 1),
                                         generator=gen).float())
    rows = torch.arange(M)
    x[rows, rows % G] = 0.0                          # an all-zero group
    x[rows, (rows + 1) % G, 7] = 2.0 ** 25           # amax an exact 2^n
    x = x.reshape(M, K).to(BF16).to(DEV)
    codes, scales = _ops().quantize_mxfp8(x)
    want_c, want_s = ref.quantize_mxfp8(x)
    assert codes.shape == (M, K) and scales.shape == (M, G)
    assert codes.dtype == scales.dtype == torch.uint8
    assert torch.equal(scales, want_s), \
        f"{int((scales != want_s).sum())} scale bytes differ"
    assert torch.equal(codes, want_c), \
        f"{int((codes != want_c).sum())} of {codes.numel()} codes differ"


# --------------------------------------------------------------------------
# 2. exact layout
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 128), (192, 384), (320, 1024)])
def test_scaled_onehot_rows_return_the_dequantized_weights(N, K, m_min_1):
    c = mo.make_case(1, N, K, bias=False, seed=1, device=DEV)
    j = torch.arange(K, device=DEV) % 21 - 10
    sign = torch.where(torch.arange(K, device=DEV) % 2 == 0, 1.0, -1.0)
    s = (sign * torch.pow(2.0, j.float())).to(BF16)  # +-2^j, per row
    for k_lo in range(0, K, 256):
        k_hi = min(K, k_lo + 256)
        x = mo.onehot_rows(K, k_lo, k_hi, device=DEV) * s[k_lo:k_hi, None]
        out = _kernel(x, c["packed"], c["exps"])
        want = mo.onehot_expected(c["packed"], c["exps"], k_lo, k_hi) \
            * s[k_lo:k_hi, None]                     # exact in bf16
        assert out.dtype == BF16 and out.shape == want.shape
        assert torch.equal(out, want), \
            f"N{N} K{K} rows {k_lo}:{k_hi}: " \
            f"{int((out != want).sum())} of {want.numel()} differ"


# --------------------------------------------------------------------------
# 3. oracle conformance
# --------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N,K", list(SHAPES))
def test_conformance(N, K, bias, m_min_1):
    c = _case(N, K)
    tag = "bias" if bias else "nobias"
    b = c["b"] if bias else None
    for M in SHAPES[(N, K)]:
        out = _kernel(c["x"][:M], c["packed"], c["exps"], b)
        assert out.shape == (M, N) and out.dtype == BF16
        ref64, emu = c["ref_" + tag][:M], c["emu_" + tag][:M]
        e0, got = ko.nme(emu, ref64), ko.nme(out, ref64)
        print(f"CONF mxfp4_a8 N{N} K{K} M{M} {tag}: nme={got:.3e} "
              f"E0={e0:.3e}")
        assert got <= ko.tolerance(e0), \
            f"M{M}: nme {got:.3e} > {ko.MARGIN:g} * E0 {e0:.3e}"


# --------------------------------------------------------------------------
# 4. bit contract
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(320, 1024), (4608, 512)])
def test_rows_do_not_depend_on_m_position_tile_or_call(N, K, m_min_1):
    c = _case(N, K)
    x, p, e, b = c["x"], c["packed"], c["exps"], c["b"]
    full = _kernel(x, p, e, b)
    assert torch.equal(full, _kernel(x, p, e, b)), "call-to-call difference"
    for M in (1, 17, 255, 257):
        assert torch.equal(_kernel(x[:M], p, e, b), full[:M]), f"M={M}"
    assert torch.equal(_kernel(x[300:301], p, e, b), full[300:301])
    # both instantiations, forced through the binding's test argument
    assert _ops()._C.mxfp4_a8_tile(M_FULL, N) == 128
    assert _ops()._C.mxfp4_a8_tile(8192, 37888) == 256
    assert torch.equal(_forced(x, p, e, b, 128), full)
    assert torch.equal(_forced(x, p, e, b, 256), full), "256-tile differs"
    assert torch.equal(_forced(x[:17], p, e, None, 256),
                       _forced(x[:17], p, e, None, 128))


# --------------------------------------------------------------------------
# 5. routing
# --------------------------------------------------------------------------
def test_routing():
    ops = _ops()
    c = _case(64, 128)
    x, p, e, b = c["x"], c["packed"], c["exps"], c["b"]

    def counts():
        return ops.mxfp4_a8_dispatch_count, ops.mxfp4_dispatch_count

    assert 64 < ops.MXFP4_A8_M_MIN <= 512            # the measured default
    plain = ops.mxfp4_linear(x[:ops.MXFP4_A8_M_MIN - 1], p, e, b)
    a8, w4 = counts()
    below = ops.mxfp4_linear(x[:ops.MXFP4_A8_M_MIN - 1], p, e, b,
                             act_quant="mxfp8")
    assert counts() == (a8, w4 + 1), "below the threshold: weight-only"
    assert torch.equal(below, plain)
    ops.mxfp4_linear(x[:ops.MXFP4_A8_M_MIN], p, e, b, act_quant="mxfp8")
    assert counts() == (a8 + 1, w4 + 1), "at the threshold: a8"
    ops.mxfp4_linear(x, p, e, b)                     # M = 513, no act_quant
    assert counts() == (a8 + 1, w4 + 1), "act_quant=None reached a kernel"
    for N, K in ((80, 128), (64, 96)):               # today's fallback
        u = mo.make_case(300, N, K, bias=True, seed=2, device=DEV)
        out = ops.mxfp4_linear(u["x"], u["packed"], u["exps"], u["b"],
                               act_quant="mxfp8")
        assert counts() == (a8 + 1, w4 + 1), "kernel took a bad shape"
        assert torch.equal(out, ops.mxfp4_linear(
            u["x"], u["packed"], u["exps"], u["b"]))


# --------------------------------------------------------------------------
# 6. model level (tiny: H=256, I=512 -> every projection is supported)
# --------------------------------------------------------------------------
def _tiny_runner(device, dtype, seed=2):
    from tensorlink_amd.parallel.pipeline import PipelineRunner
    from tensorlink_amd.parallel.planner import plan_for_world
    plan = plan_for_world("tiny", 1)
    return PipelineRunner(plan, 0, 1, device=device, dtype=dtype, seed=seed,
                          quantize="fp4-dense-a8")


def test_fp4_dense_a8_graph_decode_matches_eager(m_min_1):
    from tensorlink_amd.parallel.pipeline import SamplingParams
    ops = _ops()
    r = _tiny_runner(DEV, BF16)
    torch.manual_seed(9)
    ids = torch.randint(0, 1024, (4, 16))
    before = ops.mxfp4_a8_dispatch_count
    out_graph = r.generate(ids, SamplingParams(max_new_tokens=12)).cpu()
    assert r._decode_graph is not None, "graph was not captured"
    assert ops.mxfp4_a8_dispatch_count > before, "projections missed a8"
    r2 = _tiny_runner(DEV, BF16)
    os.environ["TL_NO_GRAPH"] = "1"
    try:
        out_eager = r2.generate(ids, SamplingParams(max_new_tokens=12)).cpu()
        assert r2._decode_graph is None
    finally:
        os.environ.pop("TL_NO_GRAPH", None)
    assert torch.equal(out_graph, out_eager), (out_graph, out_eager)


def test_fp4_dense_a8_logits_close_to_cpu_fp32_in_the_same_mode(m_min_1):
    from tensorlink_amd.models.quant import Fp4Linear
    ops = _ops()
    r_cpu = _tiny_runner("cpu", torch.float32)
    r_gpu = _tiny_runner(DEV, BF16)
    r_gpu.stage.load_state_dict(r_cpu.stage.state_dict())
    torch.manual_seed(33)
    ids = torch.randint(0, 1024, (1, 12))
    pos = torch.arange(12).unsqueeze(0).contiguous()
    before = ops.mxfp4_a8_dispatch_count
    with torch.no_grad():
        l_cpu = r_cpu.stage(ids, pos).float()
        l_gpu = r_gpu.stage(ids.to(DEV), pos.to(DEV)).float().cpu()
    fp4 = [m for m in r_gpu.stage.modules() if isinstance(m, Fp4Linear)]
    assert fp4 and all(m.act_quant == "mxfp8" for m in fp4)
    assert ops.mxfp4_a8_dispatch_count == before + len(fp4)
    cos = torch.nn.functional.cosine_similarity(l_cpu.flatten(),
                                                l_gpu.flatten(), dim=0)
    print(f"CONF fp4-dense-a8 tiny logits: cosine {float(cos):.5f}")
    assert cos > 0.97, float(cos)
