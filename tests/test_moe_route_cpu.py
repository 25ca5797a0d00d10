"""CPU tier of the MoE routing change: off the GPU the block keeps the
reference router and the per-expert loop whatever the opt-in says, and the
served-shape predicates match what ops/csrc/moe_route.hip takes."""

import pytest
import torch

from tensorlink_amd import ops
from tensorlink_amd.models.configs import get_config
from tensorlink_amd.models.dense import MoEMLP


def test_cpu_block_ignores_the_fused_router_opt_in(monkeypatch):
    torch.manual_seed(0)
    mlp = MoEMLP(get_config("tiny-moe")).eval()
    x = torch.randn(1, 5, mlp.gate.in_features)
    with torch.no_grad():
        want = mlp(x)
        monkeypatch.setattr(mlp, "fused_router", True)
        monkeypatch.setenv("TL_MOE_FUSED_ROUTER", "1")
        before = ops.moe_route_dispatch_count
        assert torch.equal(mlp(x), want)
    assert ops.moe_route_dispatch_count == before


@pytest.mark.parametrize("T,k,E,H,ok", [
    (1, 2, 8, 4096, True), (4096, 8, 128, 2048, True), (3, 1, 1, 8, True),
    (4, 9, 16, 64, False), (4, 2, 129, 64, False), (4, 2, 8, 68, False)])
def test_plan_served_shapes(T, k, E, H, ok):
    assert ops.moe_plan_served(T, k, E, H) is ok


@pytest.mark.parametrize("H,E,k,ok", [
    (4096, 8, 2, True), (2048, 128, 8, True), (96, 3, 1, True),
    (80, 8, 2, False), (64, 129, 2, False), (64, 4, 5, False)])
def test_route_served_shapes(H, E, k, ok):
    assert ops.moe_route_served(H, E, k) is ok
