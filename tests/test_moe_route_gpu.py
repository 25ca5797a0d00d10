"""GPU tier of the MoE routing kernels (ops/csrc/moe_route.hip) on MI355X:
the dispatch plan and the weighted combine bit for bit against the torch
glue they replace, the fused router against a float64 product under the
suite's rule (tests/kernel_oracle.py) and against its own emitted logits,
then the MoE block and a captured decode on tiny-moe. ``CONF`` lines are
visible with -s."""

import functools

import pytest
import torch

import kernel_oracle as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


def _routing(T, k, E, seed=0):
    """[T, k] distinct experts per token, int64, as topk returns them."""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(T, E, generator=gen).topk(k, dim=-1).indices.to(DEV)


# --------------------------------------------------------------------------
# 1. dispatch plan: the stable-argsort glue, element for element
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("T,k,E", [(1, 2, 4), (24, 2, 4), (37, 8, 128),
                                   (1100, 2, 3), (300, 1, 8)])
def test_plan_equals_the_stable_argsort_glue(T, k, E, dtype):
    ops = _ops()
    idx = _routing(T, k, E, seed=T)
    if (T, k, E) == (300, 1, 8):
        idx.fill_(5)                   # one expert takes every pair
    P = T * k
    fi = idx.reshape(-1)
    order = fi.argsort(stable=True)
    seg = torch.zeros(E + 1, dtype=torch.int32, device=DEV)
    seg[1:] = torch.bincount(fi, minlength=E).cumsum(0)
    before = ops.moe_plan_dispatch_count
    seg_off, pair_tok, pos = ops.moe_plan(idx.to(dtype), E)
    assert ops.moe_plan_dispatch_count == before + 1
    assert all(t.dtype == torch.int32 for t in (seg_off, pair_tok, pos))
    assert pos.shape == (T, k)
    assert torch.equal(seg_off, seg)
    assert torch.equal(pair_tok, (order // k).int())
    assert torch.equal(pos.view(-1)[order].long(),
                       torch.arange(P, device=DEV))


# --------------------------------------------------------------------------
# 2. combine: bf16 product, fp32 sum in slot order, one rounding
# --------------------------------------------------------------------------
@pytest.mark.parametrize("T,k,H", [(1, 2, 64), (24, 2, 256), (37, 8, 264)])
def test_combine_is_the_fixed_slot_order_sum(T, k, H):
    ops = _ops()
    _, _, pos = ops.moe_plan(_routing(T, k, 2 * k, seed=H), 2 * k)
    gen = torch.Generator().manual_seed(H)
    y = torch.randn(T * k, H, generator=gen).to(BF16).to(DEV)
    w = torch.rand(T, k, generator=gen).to(BF16).to(DEV)
    acc = torch.zeros(T, H, dtype=torch.float32, device=DEV)
    for s in range(k):
        prod = y[pos[:, s].long()].float() * w[:, s, None].float()   # exact
        acc = acc + prod.bfloat16().float()
    before = ops.moe_combine_dispatch_count
    out = ops.moe_combine(y, w, pos)
    assert ops.moe_combine_dispatch_count == before + 1
    assert out.dtype == BF16 and torch.equal(out, acc.bfloat16())


# --------------------------------------------------------------------------
# 3. fused router
# --------------------------------------------------------------------------
ROUTER_CASES = [(1, 256, 4, 2), (70, 96, 8, 2), (37, 2048, 128, 8),
                (33, 128, 3, 1)]


@functools.lru_cache(maxsize=None)
def _router_case(T, H, E, k, tie=False):
    gen = torch.Generator().manual_seed(T + H + E)
    x = torch.randn(T, H, generator=gen).to(BF16)
    gw = (torch.randn(E, H, generator=gen) / H ** 0.5).to(BF16)
    if tie:
        gw[1] *= 2                     # exact; puts the pair on top often
        gw[3] = gw[1]
    ref64 = x.double() @ gw.double().t()
    e0 = ko.nme(ko.bf16_round(x.float() @ gw.float().t()), ref64)
    ops = _ops()
    before = ops.moe_route_dispatch_count
    idx, w, logits = ops.moe_route(x.to(DEV), gw.to(DEV), k)
    assert ops.moe_route_dispatch_count == before + 1
    return dict(x=x.to(DEV), gw=gw.to(DEV), ref64=ref64, e0=e0, idx=idx,
                w=w, logits=logits)


def _check_router(name, c, k):
    idx, w, logits = c["idx"], c["w"], c["logits"]
    T, E = logits.shape
    assert idx.dtype == torch.int32 and idx.shape == (T, k)
    assert w.dtype == BF16 and w.shape == (T, k) and logits.dtype == BF16
    got = ko.nme(logits, c["ref64"])
    print(f"CONF moe_route {name}: nme={got:.3e} E0={c['e0']:.3e}")
    assert got <= ko.tolerance(c["e0"])
    want = logits.float().sort(dim=-1, descending=True, stable=True).indices
    assert torch.equal(idx.long(), want[:, :k])
    sel = logits.double().gather(1, idx.long())
    ref = (sel - sel.amax(-1, keepdim=True)).exp()
    ref = ref / ref.sum(-1, keepdim=True)
    err = ((w.double() - ref).abs() / ref).max().item()
    print(f"CONF moe_route {name}: weight rel err {err:.3e}")
    assert ((w.double() - ref).abs() <= 2.0 ** -8 * ref).all()
    assert ((w.double().sum(-1) - 1).abs() <= k * 2.0 ** -8).all()


@pytest.mark.parametrize("T,H,E,k", ROUTER_CASES)
def test_router_logits_topk_and_weights(T, H, E, k):
    _check_router(f"T{T} H{H} E{E} k{k}", _router_case(T, H, E, k), k)


def test_router_tie_goes_to_the_lower_index():
    c = _router_case(33, 128, 8, 2, tie=True)
    assert torch.equal(c["logits"][:, 1], c["logits"][:, 3])
    _check_router("tie", c, 2)
    first, second = c["idx"][:, 0], c["idx"][:, 1]
    assert (first == 1).any() and not (first == 3).any()
    assert torch.equal(second == 3, first == 1)


def test_router_rows_do_not_depend_on_the_batch():
    ops = _ops()
    c = _router_case(70, 96, 8, 2)
    full = (c["idx"], c["w"], c["logits"])
    for lo, hi in ((0, 1), (69, 70), (53, 70)):
        part = ops.moe_route(c["x"][lo:hi], c["gw"], 2)
        for a, b in zip(part, full):
            assert torch.equal(a, b[lo:hi]), (lo, hi)


# --------------------------------------------------------------------------
# 4. block and model level on tiny-moe
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _block():
    from tensorlink_amd.models.configs import get_config
    from tensorlink_amd.models.dense import MoEMLP
    torch.manual_seed(5)
    mlp = MoEMLP(get_config("tiny-moe")).to(device=DEV, dtype=BF16).eval()
    assert mlp._fused_kind() == "bf16" and mlp.top_k == 2
    gen = torch.Generator().manual_seed(6)
    return mlp, torch.randn(24, 256, generator=gen).to(BF16).to(DEV)


def test_block_default_path_plans_and_equals_the_torch_glue(monkeypatch):
    ops = _ops()
    mlp, flat = _block()
    x3 = flat.view(1, *flat.shape)
    with torch.no_grad():
        before = (ops.moe_plan_dispatch_count, ops.moe_combine_dispatch_count)
        out = mlp(x3)
        assert (ops.moe_plan_dispatch_count,
                ops.moe_combine_dispatch_count) == (before[0] + 1,
                                                    before[1] + 1)
        monkeypatch.setenv("TL_NO_MOE_PLAN", "1")
        glue = mlp(x3)
        assert ops.moe_plan_dispatch_count == before[0] + 1
    # k = 2: the two fp32 adds commute, so the old sum(1) has these bits
    assert torch.equal(out, glue)


def test_block_fused_router_feeds_the_same_forward(monkeypatch):
    ops = _ops()
    mlp, flat = _block()
    with torch.no_grad():
        idx, w, _ = ops.moe_route(flat, mlp.gate.weight, mlp.top_k)
        want = mlp._fused_forward(flat, w, idx)
        before = ops.moe_route_dispatch_count
        monkeypatch.setattr(mlp, "fused_router", True)
        got = mlp(flat.view(1, *flat.shape))[0]
        assert ops.moe_route_dispatch_count == before + 1, "router not taken"
    assert torch.equal(got, want)


def test_captured_decode_with_the_fused_router_matches_eager(monkeypatch):
    from tensorlink_amd.parallel.pipeline import (PipelineRunner,
                                                  SamplingParams)
    from tensorlink_amd.parallel.planner import plan_for_world
    ops = _ops()
    monkeypatch.setenv("TL_MOE_FUSED_ROUTER", "1")
    torch.manual_seed(9)
    ids = torch.randint(0, 1024, (4, 16))
    outs = []
    for no_graph in (False, True):
        if no_graph:
            monkeypatch.setenv("TL_NO_GRAPH", "1")
        r = PipelineRunner(plan_for_world("tiny-moe", 1), 0, 1, device=DEV,
                           dtype=BF16, seed=2, quantize="fp4")
        before = ops.moe_route_dispatch_count
        outs.append(r.generate(ids, SamplingParams(max_new_tokens=12)).cpu())
        assert ops.moe_route_dispatch_count > before, "router not taken"
        assert (r._decode_graph is None) == no_graph
    assert torch.equal(outs[0], outs[1]), outs
