"""GPU tier of the MXFP4 weight-only GEMM (ops/csrc/mxfp4_gemm.hip) on
MI355X: exact layout (one-hot), float64-oracle conformance under the
suite's own rule (tests/kernel_oracle.py), bitwise row M-independence,
fallback routing, and the fp4-dense model path with captured decode.
Cases, references and the mutants the rule rejects: tests/mxfp4_oracle.py
and tests/test_mxfp4_linear.py. ``CONF`` lines are visible with -s."""

import functools
import math
import os

import pytest
import torch

import kernel_oracle as ko
import mxfp4_oracle as mo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
M_FULL = 512
ALL_M = (1, 7, 16, 17, 64, 65, 130, 512)
# (N, K) -> the M subset run on it (large shapes subset to stay at seconds)
SHAPES = {
    (64, 128): ALL_M,
    (192, 384): ALL_M,
    (64, 3584): ALL_M,
    (4608, 512): (1, 17, 64, 130, 512),
    (4608, 3584): (1, 16, 65, 512),
}


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


def _kernel(x, packed, exps, b=None):
    """ops.mxfp4_linear, asserting that the HIP kernel took the call."""
    ops = _ops()
    before = ops.mxfp4_dispatch_count
    out = ops.mxfp4_linear(x, packed, exps, b)
    assert ops.mxfp4_dispatch_count == before + 1, "not the MXFP4 kernel"
    return out


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """One 512-row case per shape, with its float64 reference and fp32
    emulation with and without bias, computed once on the GPU."""
    c = mo.make_case(M_FULL, N, K, bias=True, device=DEV)
    w64 = mo.dequant64(c["packed"], c["exps"])
    for tag, b in (("nobias", None), ("bias", c["b"])):
        c["ref_" + tag], c["emu_" + tag] = mo.reference(c["x"], w64, b)
    return c


def _check(name, out, ref64, emu):
    e0 = ko.nme(emu, ref64)
    got = ko.nme(out, ref64)
    ratio = got / e0 if e0 > 0 else (0.0 if got == 0 else math.inf)
    print(f"CONF {name}: nme={got:.3e} E0={e0:.3e} nme/E0={ratio:.2f}")
    assert got <= ko.tolerance(e0), \
        f"{name}: nme {got:.3e} > {ko.MARGIN:g} * E0 {e0:.3e}"


# --------------------------------------------------------------------------
# 1. exact layout
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 128), (192, 384), (64, 512)])
def test_onehot_rows_return_the_dequantized_weights(N, K):
    c = mo.make_case(1, N, K, bias=False, seed=1, device=DEV)
    for k_lo in range(0, K, 256):
        k_hi = min(K, k_lo + 256)
        x = mo.onehot_rows(K, k_lo, k_hi, device=DEV)
        out = _kernel(x, c["packed"], c["exps"])
        want = mo.onehot_expected(c["packed"], c["exps"], k_lo, k_hi)
        assert out.dtype == BF16 and out.shape == want.shape
        bad = int((out != want).sum())
        assert torch.equal(out, want), \
            f"N{N} K{K} rows {k_lo}:{k_hi}: {bad} of {want.numel()} differ"


# --------------------------------------------------------------------------
# 2. oracle conformance
# --------------------------------------------------------------------------
def test_shape_set_covers_split_and_unsplit():
    C = _ops()._C
    splits = {s: C.mxfp4_n_split(*s) for s in SHAPES}
    print(f"CONF mxfp4 n_split: {splits}")
    assert any(v > 1 for v in splits.values())
    assert any(v == 1 for v in splits.values())
    # (N,K)-pure and stable call to call
    assert splits == {s: C.mxfp4_n_split(*s) for s in SHAPES}


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N,K", list(SHAPES))
def test_conformance(N, K, bias):
    c = _case(N, K)
    tag = "bias" if bias else "nobias"
    b = c["b"] if bias else None
    for M in SHAPES[(N, K)]:
        out = _kernel(c["x"][:M], c["packed"], c["exps"], b)
        assert out.shape == (M, N) and out.dtype == BF16
        _check(f"mxfp4_gemm N{N} K{K} M{M} {tag}", out,
               c["ref_" + tag][:M], c["emu_" + tag][:M])


# --------------------------------------------------------------------------
# 3. row M-independence, bitwise
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 3584), (192, 384)])
def test_rows_are_bitwise_m_independent(N, K):
    C = _ops()._C
    assert (C.mxfp4_n_split(N, K) > 1) == (K == 3584)
    c = _case(N, K)
    x, p, e, b = c["x"], c["packed"], c["exps"], c["b"]
    full = _kernel(x, p, e, b)
    again = _kernel(x, p, e, b)
    assert torch.equal(full, again), "call-to-call difference"
    for M in (1, 16, 17, 64, 65, 130):
        part = _kernel(x[:M], p, e, b)
        assert torch.equal(part, full[:M]), f"M={M} rows differ from M=512"
    row7 = _kernel(x[7:8], p, e, b)
    assert torch.equal(row7, full[7:8])


# --------------------------------------------------------------------------
# 4. fallback routing
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 96), (80, 128)])
def test_unsupported_shape_takes_the_fallback(N, K):
    ops = _ops()
    c = mo.make_case(17, N, K, bias=True, seed=2, device=DEV)
    w64 = mo.dequant64(c["packed"], c["exps"])
    ref, emu = mo.reference(c["x"], w64, c["b"])
    before = ops.mxfp4_dispatch_count
    out = ops.mxfp4_linear(c["x"], c["packed"], c["exps"], c["b"])
    assert ops.mxfp4_dispatch_count == before, "kernel took a bad shape"
    assert out.dtype == BF16 and out.shape == (17, N)
    _check(f"mxfp4 fallback N{N} K{K}", out, ref, emu)


# --------------------------------------------------------------------------
# 5. model level (tiny: H=256, I=512 -> every projection is supported)
# --------------------------------------------------------------------------
def _tiny_runner(device, dtype, seed=2):
    from tensorlink_amd.parallel.pipeline import PipelineRunner
    from tensorlink_amd.parallel.planner import plan_for_world
    plan = plan_for_world("tiny", 1)
    return PipelineRunner(plan, 0, 1, device=device, dtype=dtype, seed=seed,
                          quantize="fp4-dense")


def test_fp4_dense_graph_decode_matches_eager():
    from tensorlink_amd.parallel.pipeline import SamplingParams
    ops = _ops()
    r = _tiny_runner(DEV, BF16)
    assert r._no_graph is False
    torch.manual_seed(9)
    ids = torch.randint(0, 1024, (4, 16))
    before = ops.mxfp4_dispatch_count
    out_graph = r.generate(ids, SamplingParams(max_new_tokens=12)).cpu()
    assert r._decode_graph is not None, "graph was not captured"
    assert r._no_graph is False
    assert ops.mxfp4_dispatch_count > before, "projections missed the kernel"
    r2 = _tiny_runner(DEV, BF16)
    os.environ["TL_NO_GRAPH"] = "1"
    try:
        out_eager = r2.generate(ids, SamplingParams(max_new_tokens=12)).cpu()
        assert r2._decode_graph is None
    finally:
        os.environ.pop("TL_NO_GRAPH", None)
    assert torch.equal(out_graph, out_eager), (out_graph, out_eager)


def test_fp4_dense_logits_close_to_cpu_fp32():
    from tensorlink_amd.models.quant import Fp4Linear
    r_cpu = _tiny_runner("cpu", torch.float32)
    r_gpu = _tiny_runner(DEV, BF16)
    # same seed, same weights: the GPU generator differs from the CPU
    # one, so the CPU stage's parameters and packed weights are copied
    r_gpu.stage.load_state_dict(r_cpu.stage.state_dict())
    torch.manual_seed(33)
    ids = torch.randint(0, 1024, (1, 12))
    pos = torch.arange(12).unsqueeze(0).contiguous()
    ops = _ops()
    before = ops.mxfp4_dispatch_count
    with torch.no_grad():
        l_cpu = r_cpu.stage(ids, pos).float()
        l_gpu = r_gpu.stage(ids.to(DEV), pos.to(DEV)).float().cpu()
    n_fp4 = sum(isinstance(m, Fp4Linear) for m in r_gpu.stage.modules())
    assert n_fp4 > 0
    assert ops.mxfp4_dispatch_count == before + n_fp4
    cos = torch.nn.functional.cosine_similarity(l_cpu.flatten(),
                                                l_gpu.flatten(), dim=0)
    print(f"CONF fp4-dense tiny logits: cosine {float(cos):.5f}")
    assert cos > 0.97, float(cos)
    # no dequantized copy is kept on the module
    for m in r_gpu.stage.modules():
        if isinstance(m, Fp4Linear):
            assert sorted(n for n, _ in m.named_buffers()) == \
                ["exponents", "packed"]
            assert not any(
                torch.is_tensor(v) and v.dtype in (BF16, torch.float32)
                and v.numel() >= m.in_features * m.out_features
                for v in vars(m).values())
