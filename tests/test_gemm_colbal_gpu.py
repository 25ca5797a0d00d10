"""Column-balanced one-pass GEMM (ops/csrc/gemm_colbal.hip) and its fused
SwiGLU variant.

The oracle is the existing family kernel through ``_C.skinny_gemm`` (and
``_C.swiglu_fused`` on top of it): the new kernel walks the same K chain, so
every comparison is ``torch.equal`` on the bf16 output, for every number of
workgroups and every M. Each case is also held against the float64 reference
by the conformance suite's rule, nme <= MARGIN * E0 (tests/kernel_oracle.py).

Shapes are the smallest at which the kernel can go wrong: K = 192 is three
chunks (prologue, steady state, drain of the 3-stage ring), K = 64 a single
chunk, K = 96 one chunk plus the 32-wide tail; N = 16384 deals even column
ranges at 256 workgroups, 16448 uneven ones (1028 tiles, 5/4), 40960 exactly
10 tiles each and 41024 eleven, the multi-pass path; n_blocks = 7 and 64
force long multi-pass and uneven ranges on any device."""

import os
from contextlib import contextmanager

import pytest
import torch

import kernel_oracle as ko
from tensorlink_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
MS = (65, 255, 256, 257, 512)


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _C():
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops._require_ext()


def _blocks():
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return (7, 64, cus)


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _conf(name, out, ref64, emu):
    e0 = ko.nme(emu, ref64)
    got = ko.nme(out, ref64)
    print(f"CONF {name}: nme={got:.3e} E0={e0:.3e}")
    assert got <= ko.tolerance(e0), \
        f"{name}: nme {got:.3e} > {ko.MARGIN:g} * E0 {e0:.3e}"


# ---------------------------------------------------------------------------
# unfused kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [192, 64, 96])
@pytest.mark.parametrize("N", [16384, 16448, 40960, 41024])
def test_colbal_equals_family_and_fp64(N, K):
    C = _C()
    assert C.gemm_n_split(N, K) == 1
    c = ko.gemm_case(max(MS), N, K, False, seed=3)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    ref64 = ko.linear(x, w)
    emu = ko.bf16_round(ko.linear(x, w, dtype=torch.float32))
    for M in MS:
        want = C.skinny_gemm(x[:M].contiguous(), w, None)
        for nb in _blocks():
            got = C.gemm_colbal(x[:M].contiguous(), w, nb)
            assert got.shape == (M, N)
            assert torch.equal(got, want), (M, nb)
        _conf(f"colbal N{N} K{K} M{M}", want, ref64[:M], emu[:M])
    # default n_blocks is the CU count
    assert torch.equal(C.gemm_colbal(x, w), want)


def test_colbal_rows_do_not_depend_on_m():
    C = _C()
    c = ko.gemm_case(257, 16448, 192, False, seed=4)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    big = C.gemm_colbal(x, w)
    small = C.gemm_colbal(x[:65].contiguous(), w)
    assert torch.equal(big[:65], small)


# ---------------------------------------------------------------------------
# fused SwiGLU variant
# ---------------------------------------------------------------------------
def _fused_case(M, I, K, seed):
    gen = torch.Generator().manual_seed(seed + I)
    x = torch.randn(M, K, generator=gen).to(BF)
    w = torch.randn(2 * I, K, generator=gen) / K ** 0.5
    # gate pre-activations with sigma 4: their extremes over M * I draws
    # reach about +-20, where __expf(-g) saturates in both directions
    w[:I] *= 4.0
    return x.to(DEV), w.to(BF).to(DEV)


@pytest.mark.parametrize("I", [8192, 8224, 18944])
def test_colbal_swiglu_equals_chain_and_fp64(I):
    C = _C()
    K = 192
    x, w = _fused_case(257, I, K, seed=5)
    gu64 = ko.linear(x, w)
    assert gu64[:, :I].abs().max() > 18.0
    ref64 = ko.swiglu(gu64[:, :I], gu64[:, I:])
    gu32 = ko.bf16_round(ko.linear(x, w, dtype=torch.float32))
    emu = ko.bf16_round(ko.swiglu(gu32[:, :I], gu32[:, I:],
                                  dtype=torch.float32))
    for M in (65, 256, 257):
        xm = x[:M].contiguous()
        want = C.swiglu_fused(C.skinny_gemm(xm, w, None))
        for nb in _blocks():
            got = C.gemm_colbal_swiglu(xm, w, nb)
            assert got.shape == (M, I)
            assert torch.equal(got, want), (M, nb)
        _conf(f"colbal_swiglu I{I} M{M}", want, ref64[:M], emu[:M])


# ---------------------------------------------------------------------------
# repeatability at the full gate_up shape: a staging race would show as a
# rare differing tile
# ---------------------------------------------------------------------------
def test_colbal_repeats_bitwise_at_gate_up_shape():
    C = _C()
    M, N, K = 256, 37888, 3584
    gen = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(M, K, generator=gen, device=DEV).to(BF)
    w = (torch.randn(N, K, generator=gen, device=DEV) / K ** 0.5).to(BF)
    first = C.gemm_colbal(x, w)
    assert torch.equal(first, C.skinny_gemm(x, w, None))
    first_f = C.gemm_colbal_swiglu(x, w)
    assert torch.equal(first_f, C.swiglu_fused(first))
    for _ in range(19):
        assert torch.equal(C.gemm_colbal(x, w), first)
        assert torch.equal(C.gemm_colbal_swiglu(x, w), first_f)


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------
def test_routing_takes_colbal_for_gateup_class():
    N, K = 16384, 192
    assert "gateup" not in ops._LIB_CLASSES, "default must be the family"
    assert ops._gemm_class(N, K) == "gateup"
    assert ops._use_colbal(65, N, K) and ops._use_colbal(512, N, K)
    assert not ops._use_colbal(64, N, K)
    assert not ops._use_colbal(65, 8192, K)
    c = ko.gemm_case(65, N, K, True, seed=7)
    x, w, b = c["x"].to(DEV), c["w"].to(DEV), c["b"].to(DEV)
    C = _C()
    before = ops.gemm_dispatch_count
    out = ops.linear(x, w)
    act = ops.gate_up_swiglu(x, w)
    assert ops.gemm_dispatch_count == before + 2
    assert torch.equal(out, C.skinny_gemm(x, w, None))
    assert torch.equal(act, C.swiglu_fused(out))
    # a bias keeps the family's own path; M <= 64 falls back to the chain
    assert torch.equal(ops.linear(x, w, b), C.skinny_gemm(x, w, b))
    x64 = x[:64].contiguous()
    assert torch.equal(ops.gate_up_swiglu(x64, w),
                       C.swiglu_fused(C.skinny_gemm(x64, w, None)))
    with _env(TL_NO_GATEUP_FUSION="1", TL_NO_COLBAL="1"):
        assert not ops._use_colbal(65, N, K)
        assert torch.equal(ops.gate_up_swiglu(x, w), act)


# ---------------------------------------------------------------------------
# model level: gate_up_proj has N = 2 * 8192 = 16384, the gateup class
# ---------------------------------------------------------------------------
def test_generate_fused_gate_up_equals_unfused_chain():
    from tensorlink_amd.models.configs import ModelConfig
    from tensorlink_amd.parallel.planner import plan_for_world
    from tensorlink_amd.parallel.pipeline import PipelineRunner, SamplingParams
    cfg = ModelConfig(name="colbal-tiny", vocab_size=256, hidden_size=256,
                      intermediate_size=8192, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=1,
                      max_position_embeddings=64)
    B, S, T = 66, 6, 8            # prefill M = 396, decode M = 66
    plan = plan_for_world(cfg, 1, batch_size=B, seq_len=S + T)
    ids = torch.randint(0, 256, (B, S),
                        generator=torch.Generator().manual_seed(8))
    sp = SamplingParams(max_new_tokens=T)
    r = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    out_graph = r.generate(ids, sp).cpu()
    assert r._decode_graph is not None, "graph was not captured"
    r2 = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    with _env(TL_NO_GRAPH="1"):
        before = ops.gemm_dispatch_count
        out_eager = r2.generate(ids, sp).cpu()
        assert ops.gemm_dispatch_count > before
        with _env(TL_NO_GATEUP_FUSION="1", TL_NO_COLBAL="1"):
            out_chain = r2.generate(ids, sp).cpu()
    assert out_graph.shape == (B, T)
    assert torch.equal(out_graph, out_eager)
    assert torch.equal(out_graph, out_chain)
