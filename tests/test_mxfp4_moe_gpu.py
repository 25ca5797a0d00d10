"""GPU tier of the grouped MXFP4 expert GEMM (ops/csrc/mxfp4_moe_gemm.hip)
on MI355X: exact layout through the pointer tables (one-hot), float64-oracle
conformance under the suite's own rule (tests/kernel_oracle.py), bitwise
independence of a pair's row from the rest of the call, bitwise equality
with the dense MXFP4 kernel where the split counts agree, the MoE block on
both of its paths, and fp4 MoE models with captured decode. Cases,
references and the mutants the rule rejects: tests/mxfp4_moe_oracle.py and
tests/test_mxfp4_moe.py. ``CONF`` lines are visible with -s."""

import functools
import math
import os

import pytest
import torch

import kernel_oracle as ko
import mxfp4_moe_oracle as mmo
import mxfp4_oracle as mo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
# (N, K, E) of the cases below; the two N=128 shapes have equal split counts
# under the grouped and the dense policy (1 and 4)
SHAPES = ((128, 256, 4), (128, 1024, 4), (768, 256, 4), (128, 256, 3),
          (64, 512, 3))


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


def _ptrs(tensors):
    assert all(t.is_contiguous() and t.data_ptr() % 16 == 0
               for t in tensors)
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64,
                        device=DEV)


def _kernel(x, tok, seg, packed, exps):
    """ops.mxfp4_moe_gemm, asserting that the HIP kernel took the call."""
    ops = _ops()
    before = ops.mxfp4_moe_dispatch_count
    out = ops.mxfp4_moe_gemm(x, tok, seg.to(DEV), _ptrs(packed), _ptrs(exps),
                             packed[0].shape[0])
    assert ops.mxfp4_moe_dispatch_count == before + 1, "not the MoE kernel"
    P = x.shape[0] if tok is None else tok.shape[0]
    assert out.shape == (P, packed[0].shape[0]) and out.dtype == BF16
    return out


@functools.lru_cache(maxsize=None)
def _case(name, N, K):
    """One case per (segments, shape) with its float64 reference, E0 and
    the kernel's output, computed once and left unchanged."""
    c = mmo.make_case(mmo.SEGMENT_SETS[name], N, K, device=DEV)
    c["ref"], c["e0"] = mmo.reference(c)
    c["out"] = _kernel(c["x"], c["tok"], c["seg"], c["packed"], c["exps"])
    return c


def _check(name, out, ref64, e0):
    got = ko.nme(out, ref64)
    ratio = got / e0 if e0 > 0 else (0.0 if got == 0 else math.inf)
    print(f"CONF {name}: nme={got:.3e} E0={e0:.3e} nme/E0={ratio:.2f}")
    assert got <= ko.tolerance(e0), \
        f"{name}: nme {got:.3e} > {ko.MARGIN:g} * E0 {e0:.3e}"


def _solo_seg(e, rows, E):
    """Segment offsets with ``rows`` pairs for expert e and none elsewhere."""
    return torch.tensor([0] * (e + 1) + [rows] * (E - e), dtype=torch.int32)


# --------------------------------------------------------------------------
# 1. exact layout
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(128, 256), (64, 512)])
def test_onehot_rows_return_each_experts_dequantized_weights(N, K):
    E = 3
    packed, exps = [], []
    for e in range(E):
        c = mo.make_case(1, N, K, bias=False, seed=20 + e, device=DEV)
        packed.append(c["packed"])
        exps.append(c["exps"])
    for e in range(E):
        for k_lo in range(0, K, 256):
            k_hi = min(K, k_lo + 256)
            rows = k_hi - k_lo
            x = mo.onehot_rows(K, k_lo, k_hi, device=DEV)
            tok = torch.arange(rows, dtype=torch.int32, device=DEV)
            out = _kernel(x, tok, _solo_seg(e, rows, E), packed, exps)
            want = mo.onehot_expected(packed[e], exps[e], k_lo, k_hi)
            bad = int((out != want).sum())
            assert torch.equal(out, want), \
                f"N{N} K{K} expert {e} rows {k_lo}:{k_hi}: {bad} of " \
                f"{want.numel()} differ"


# --------------------------------------------------------------------------
# 2. split policy
# --------------------------------------------------------------------------
def test_shape_set_covers_split_and_unsplit():
    C = _ops()._C
    assert C.mxfp4_moe_n_split(128, 256, 4) == 1
    assert C.mxfp4_moe_n_split(128, 1024, 4) > 1
    splits = {s: C.mxfp4_moe_n_split(*s) for s in SHAPES}
    print(f"CONF mxfp4_moe n_split (N, K, E): {splits}")
    # (N, K, E)-pure and stable call to call
    assert splits == {s: C.mxfp4_moe_n_split(*s) for s in SHAPES}
    # more experts never mean more splits: the grid only grows
    assert C.mxfp4_moe_n_split(128, 1024, 128) == 1


# --------------------------------------------------------------------------
# 3. oracle conformance
# --------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("name", list(mmo.SEGMENT_SETS))
def test_conformance(name, K):
    c = _case(name, 128, K)
    _check(f"mxfp4_moe {name} N128 K{K}", c["out"], c["ref"], c["e0"])


def test_conformance_tiny_moe_gate_up_shape():
    c = _case("P200", 768, 256)
    _check("mxfp4_moe P200 N768 K256", c["out"], c["ref"], c["e0"])


def test_pair_rows_without_tok_idx():
    c = _case("P200", 128, 256)
    rows = c["x"][c["tok"].long()].contiguous()
    out = _kernel(rows, None, c["seg"], c["packed"], c["exps"])
    assert torch.equal(out, c["out"])


# --------------------------------------------------------------------------
# 4. a pair's row does not depend on the rest of the call, bitwise
# --------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 1024])
def test_rows_are_bitwise_independent_of_the_call(K):
    c = _case("P200", 128, K)
    full, tok, E = c["out"], c["tok"], len(c["segments"])
    again = _kernel(c["x"], tok, c["seg"], c["packed"], c["exps"])
    assert torch.equal(again, full), "call-to-call difference"
    seg = c["seg"].tolist()
    for e in range(E):
        a, b = seg[e], seg[e + 1]
        if b == a:
            continue
        solo = _kernel(c["x"], tok[a:b].contiguous(), _solo_seg(e, b - a, E),
                       c["packed"], c["exps"])
        assert torch.equal(solo, full[a:b]), f"expert {e} segment alone"
    # the 6-row segment of expert 3: alone it is a P=6 call (MT=1) ...
    a, b = seg[3], seg[4]
    assert b - a == 6
    # ... and behind 20 rows of expert 0 and 6 of expert 1 a P=32 call (MT=2)
    parts = [(0, 20), (seg[1], seg[1] + 6), (a, b)]
    tok32 = torch.cat([tok[lo:hi] for lo, hi in parts]).contiguous()
    seg32 = torch.tensor([0, 20, 26, 26, 32], dtype=torch.int32)
    out32 = _kernel(c["x"], tok32, seg32, c["packed"], c["exps"])
    want32 = torch.cat([full[lo:hi] for lo, hi in parts])
    assert torch.equal(out32, want32), "rows differ inside a P=32 call"


# --------------------------------------------------------------------------
# 5. bitwise equal to the dense MXFP4 kernel where the splits agree
# --------------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 1024])
@pytest.mark.parametrize("name", list(mmo.SEGMENT_SETS))
def test_rows_equal_the_dense_kernel(name, K):
    C = _ops()._C
    N = 128
    c = _case(name, N, K)
    E = len(c["segments"])
    assert C.mxfp4_moe_n_split(N, K, E) == C.mxfp4_n_split(N, K)
    seg = c["seg"].tolist()
    for e in range(E):
        a, b = seg[e], seg[e + 1]
        if b == a:
            continue
        rows = c["x"][c["tok"][a:b].long()].contiguous()
        dense = C.mxfp4_gemm(rows, c["packed"][e], c["exps"][e], None)
        assert torch.equal(c["out"][a:b], dense), \
            f"{name} K{K}: expert {e} rows differ from mxfp4_gemm"


# --------------------------------------------------------------------------
# 6. block level (tiny-moe: gate_up 768x256, down 256x384)
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block():
    from tensorlink_amd.models.configs import get_config
    from tensorlink_amd.models.dense import MoEMLP
    from tensorlink_amd.models.quant import quantize_experts_fp4
    ops = _ops()
    torch.manual_seed(5)
    mlp = MoEMLP(get_config("tiny-moe"))
    assert quantize_experts_fp4(mlp) == 8
    mlp = mlp.to(device=DEV, dtype=BF16).eval()
    assert mlp._fused_kind() == "fp4"
    gen = torch.Generator().manual_seed(6)
    flat = torch.randn(24, 256, generator=gen).to(BF16).to(DEV)
    with torch.no_grad():
        rw, idx = ops.moe_topk_router(mlp.gate(flat), mlp.top_k)
    return mlp, flat, rw.to(BF16), idx


def _block_reference(mlp, flat, rw, idx, dtype, rnd):
    """The block with the routing given: per (token, slot) gate_up ->
    silu(g)*u -> down, weighted, summed over slots in slot order. ``rnd``
    is applied wherever the GPU paths materialise bf16: gu, act, the pair
    row, the weighted row and the sum."""
    from tensorlink_amd.models.quant import dequantize_mxfp4
    T, H = flat.shape
    x = flat.to(dtype)
    out = torch.zeros(T, H, dtype=dtype, device=flat.device)
    for s in range(mlp.top_k):
        y_s = torch.zeros_like(out)
        for e, ex in enumerate(mlp.experts):
            t = (idx[:, s] == e).nonzero(as_tuple=True)[0]
            if t.numel() == 0:
                continue
            wgu = dequantize_mxfp4(ex.gate_up_proj.packed,
                                   ex.gate_up_proj.exponents).to(dtype)
            wd = dequantize_mxfp4(ex.down_proj.packed,
                                  ex.down_proj.exponents).to(dtype)
            gu = rnd(x[t] @ wgu.t())
            act = rnd(ko.swiglu(gu[:, :ex.inter], gu[:, ex.inter:],
                                dtype=dtype))
            y_s[t] = rnd(act @ wd.t())
        out = out + rnd(y_s * rw[:, s, None].to(dtype))
    return rnd(out)


def test_block_fused_and_loop_paths_meet_the_rule():
    from tensorlink_amd.models.dense import MoEMLP
    ops = _ops()
    mlp, flat, rw, idx = _block()
    ref64 = _block_reference(mlp, flat, rw, idx, ko.F64, lambda v: v)
    emu = _block_reference(mlp, flat, rw, idx, torch.float32, ko.bf16_round)
    e0 = ko.nme(emu, ref64)
    x3 = flat.view(1, *flat.shape)
    with torch.no_grad():
        before = ops.mxfp4_moe_dispatch_count
        fused = mlp(x3)[0]
        assert ops.mxfp4_moe_dispatch_count == before + 2, \
            "block missed the grouped kernel"
        orig = MoEMLP._fused_kind
        MoEMLP._fused_kind = lambda self: None
        try:
            dense_before = ops.mxfp4_dispatch_count
            loop = mlp(x3)[0]
        finally:
            MoEMLP._fused_kind = orig
        assert ops.mxfp4_moe_dispatch_count == before + 2
        assert ops.mxfp4_dispatch_count > dense_before
    _check("fp4 MoE block fused", fused, ref64, e0)
    _check("fp4 MoE block loop", loop, ref64, e0)


def test_block_row_is_bitwise_independent_of_the_batch():
    ops = _ops()
    mlp, flat, rw, idx = _block()
    with torch.no_grad():
        before = ops.mxfp4_moe_dispatch_count
        full = mlp._fused_forward(flat, rw, idx)
        one = mlp._fused_forward(flat[:1], rw[:1], idx[:1])
        assert ops.mxfp4_moe_dispatch_count == before + 4
        assert torch.equal(mlp(flat.view(1, *flat.shape))[0], full)
    assert torch.equal(one[0], full[0])


# --------------------------------------------------------------------------
# 7. model level
# --------------------------------------------------------------------------
def _runner(model, quantize, seed=2):
    from tensorlink_amd.parallel.pipeline import PipelineRunner
    from tensorlink_amd.parallel.planner import plan_for_world
    return PipelineRunner(plan_for_world(model, 1), 0, 1, device=DEV,
                          dtype=BF16, seed=seed, quantize=quantize)


@pytest.mark.parametrize("quantize", ["fp4", "fp4-dense"])
def test_fp4_moe_graph_decode_matches_eager(quantize):
    from tensorlink_amd.models.quant import Fp4Linear
    from tensorlink_amd.parallel.pipeline import SamplingParams
    ops = _ops()
    r = _runner("tiny-moe", quantize)
    assert r._no_graph is False
    n_fp4 = sum(isinstance(m, Fp4Linear) for m in r.stage.modules())
    assert n_fp4 == (32 if quantize == "fp4" else 32 + 8)
    torch.manual_seed(9)
    ids = torch.randint(0, 1024, (4, 16))
    before = ops.mxfp4_moe_dispatch_count
    out_graph = r.generate(ids, SamplingParams(max_new_tokens=12)).cpu()
    assert r._decode_graph is not None, "graph was not captured"
    assert r._no_graph is False
    assert ops.mxfp4_moe_dispatch_count > before, \
        "experts missed the grouped kernel"
    r2 = _runner("tiny-moe", quantize)
    os.environ["TL_NO_GRAPH"] = "1"
    try:
        out_eager = r2.generate(ids, SamplingParams(max_new_tokens=12)).cpu()
        assert r2._decode_graph is None
    finally:
        os.environ.pop("TL_NO_GRAPH", None)
    assert torch.equal(out_graph, out_eager), (out_graph, out_eager)
    # no dequantized copy is kept on an expert or on the block
    for m in r.stage.modules():
        if isinstance(m, Fp4Linear):
            assert sorted(n for n, _ in m.named_buffers()) == \
                ["exponents", "packed"]
            size = m.in_features * m.out_features
        elif type(m).__name__ == "MoEMLP":
            size = 768 * 256
        else:
            continue
        assert not any(
            torch.is_tensor(v) and v.dtype in (BF16, torch.float32)
            and v.numel() >= size for v in vars(m).values())


def test_unsupported_expert_shape_generates_through_the_loop():
    """tiny-qwen3-moe: down K = 192 is no multiple of 128, so the block
    keeps the per-expert loop over the dense MXFP4 kernel's own routing."""
    from tensorlink_amd.parallel.pipeline import SamplingParams
    ops = _ops()
    r = _runner("tiny-qwen3-moe", "fp4")
    assert r.stage.layers[0].mlp._fused_kind() is None
    torch.manual_seed(9)
    ids = torch.randint(0, 1024, (2, 16))
    before = ops.mxfp4_moe_dispatch_count
    dense_before = ops.mxfp4_dispatch_count
    out = r.generate(ids, SamplingParams(max_new_tokens=4))
    assert out.shape == (2, 4)
    assert ops.mxfp4_moe_dispatch_count == before
    assert ops.mxfp4_dispatch_count > dense_before    # gate_up 384x256
