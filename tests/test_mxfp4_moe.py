"""CPU tier of fp4 MoE serving: the experts-only quantize mode, the routing
of MoEMLP to the grouped MXFP4 kernel by shape, row-blocked quantisation,
the expert-parallel build, the op's CPU contract, and proof that the
acceptance rule of tests/test_mxfp4_moe_gpu.py rejects plausibly wrong
grouped kernels."""

import copy

import pytest
import torch
import torch.nn as nn

import kernel_oracle as ko
import mxfp4_moe_oracle as mmo
from tensorlink_amd.models.dense import MoEMLP
from tensorlink_amd.models.quant import (Fp4Linear, dequantize_mxfp4,
                                         quantize_experts_fp4,
                                         quantize_mxfp4)
from tensorlink_amd.ops import reference as ref


def _runner(model, quantize):
    from tensorlink_amd.parallel.pipeline import PipelineRunner
    from tensorlink_amd.parallel.planner import plan_for_world
    return PipelineRunner(plan_for_world(model, 1), 0, 1, device="cpu",
                          quantize=quantize)


def test_quantize_fp4_converts_the_experts_only():
    from tensorlink_amd.parallel.pipeline import SamplingParams
    r = _runner("tiny-moe", "fp4")
    n_experts = 0
    for layer in r.stage.layers:
        assert isinstance(layer.mlp, MoEMLP)
        for e in layer.mlp.experts:
            assert isinstance(e.gate_up_proj, Fp4Linear)
            assert isinstance(e.down_proj, Fp4Linear)
            n_experts += 1
        assert type(layer.mlp.gate) is nn.Linear
        assert isinstance(layer.self_attn.qkv_proj, nn.Linear)
        assert isinstance(layer.self_attn.o_proj, nn.Linear)
    assert n_experts == 4 * 4
    assert sum(isinstance(m, Fp4Linear) for m in r.stage.modules()) \
        == 2 * n_experts
    torch.manual_seed(0)
    ids = torch.randint(0, 1024, (2, 8))
    out = r.generate(ids, SamplingParams(max_new_tokens=4))
    assert out.shape == (2, 4)
    assert int(out.min()) >= 0 and int(out.max()) < 1024


@pytest.mark.parametrize("model,kind", [("tiny-moe", "fp4"),
                                        ("tiny-qwen3-moe", None)])
def test_fused_kind_follows_the_kernel_shapes(model, kind):
    """tiny-moe: gate_up 768x256, down 256x384 -> grouped kernel.
    tiny-qwen3-moe: down K = 192 is no multiple of 128 -> the loop."""
    from tensorlink_amd.models.configs import get_config
    torch.manual_seed(0)
    mlp = MoEMLP(get_config(model))
    assert mlp._fused_kind() == "bf16"
    assert quantize_experts_fp4(mlp) == 2 * mlp.num_experts
    assert mlp._fused_kind() == kind
    if kind is None:
        assert mlp.experts[0].down_proj.in_features % 128 != 0


def test_fused_kind_needs_every_expert_bias_free_fp4():
    from tensorlink_amd.models.configs import get_config
    torch.manual_seed(0)
    mlp = MoEMLP(get_config("tiny-moe"))
    quantize_experts_fp4(mlp)
    mixed = copy.deepcopy(mlp)
    mixed.experts[2].down_proj = nn.Linear(384, 256, bias=False)
    assert mixed._fused_kind() is None
    biased = copy.deepcopy(mlp)
    biased.experts[3].gate_up_proj.bias = torch.zeros(768)
    assert biased._fused_kind() is None


def test_row_blocked_quantisation_is_identical():
    """N = 4096 + 64: one block seam inside the weight."""
    torch.manual_seed(1)
    lin = nn.Linear(64, 4096 + 64, bias=False)
    with torch.no_grad():
        # rows of very different scale on both sides of the seam
        lin.weight.mul_(torch.pow(2.0, torch.randint(-9, 9, (4160, 1))))
    q = Fp4Linear.from_linear(lin)
    p, e = quantize_mxfp4(lin.weight.detach())
    assert q.packed.shape == (4160, 32) and q.exponents.shape == (4160, 2)
    assert q.packed.is_contiguous() and q.exponents.is_contiguous()
    assert torch.equal(q.packed, p)
    assert torch.equal(q.exponents, e)


def test_ep_model_fp4_equals_dequantized_linears():
    from tensorlink_amd.parallel.ep import build_ep_model
    stage = build_ep_model("tiny-moe", 0, 1, device=torch.device("cpu"),
                           quantize="fp4")
    twin = copy.deepcopy(stage)
    n = 0
    for layer in twin.layers:
        for ex in layer.mlp.experts:
            for name in ("gate_up_proj", "down_proj"):
                q = getattr(ex, name)
                assert isinstance(q, Fp4Linear)
                lin = nn.Linear(q.in_features, q.out_features, bias=False)
                lin.weight.data = dequantize_mxfp4(q.packed, q.exponents)
                setattr(ex, name, lin)
                n += 1
    assert n == 4 * 4 * 2
    torch.manual_seed(3)
    ids = torch.randint(0, 1024, (2, 10))
    pos = torch.arange(10).unsqueeze(0).expand(2, -1).contiguous()
    with torch.no_grad():
        got = stage(ids, pos)
        want = twin(ids, pos)
    assert got.dtype == torch.float32
    assert torch.allclose(got, want)


# --------------------------------------------------------------------------
# the op's CPU contract and the rule
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mmo.SEGMENT_SETS))
@pytest.mark.parametrize("K", [256, 1024])
def test_reference_op_meets_the_rule(name, K):
    c = mmo.cpu_case(name, K=K)
    out = ref.mxfp4_moe_grouped(c["x"], c["tok"], c["seg"], c["packed"],
                                c["exps"])
    assert out.dtype == torch.bfloat16
    assert out.shape == (sum(c["segments"]), c["N"])
    got = ko.nme(out, c["ref"])
    print(f"CONF ref.mxfp4_moe_grouped {name} K{K}: nme={got:.3e} "
          f"E0={c['e0']:.3e}")
    assert got <= ko.tolerance(c["e0"])
    # tok_idx None: x holds the pair rows themselves
    rows = c["x"][c["tok"].long()]
    out2 = ref.mxfp4_moe_grouped(rows, None, c["seg"], c["packed"],
                                 c["exps"])
    assert torch.equal(out2, out)


def test_unreferenced_rows_would_show():
    c = mmo.cpu_case("P200", K=256)
    used = torch.zeros(mmo.T_ROWS, dtype=torch.bool)
    used[c["tok"].long()] = True
    assert bool((c["x"][~used] == mmo.UNREFERENCED).all())
    assert float(c["x"][used].abs().max()) < 10
    shifted = dict(c, tok=(c["tok"] + 1) % mmo.T_ROWS)
    out = ko.bf16_round(ko.moe_grouped(shifted["x"], shifted["tok"],
                                       c["seg"],
                                       mmo.exact_weights(c, torch.float32),
                                       dtype=torch.float32))
    assert ko.nme(out, c["ref"]) >= 2 * ko.tolerance(c["e0"])


@pytest.mark.parametrize("name", mmo.MUTANTS)
@pytest.mark.parametrize("K", [256, 1024])
def test_mutant_is_rejected(name, K):
    c = mmo.cpu_case("P200", K=K)
    err = ko.nme(mmo.mutant_output(name, c), c["ref"])
    tol = ko.tolerance(c["e0"])
    print(f"MUTANT {name} K{K}: nme {err:.3e} tol {tol:.3e} "
          f"ratio {err / tol:.1f}")
    assert err >= 2 * tol, (name, K, err, tol)
