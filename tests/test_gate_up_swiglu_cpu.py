"""ops.gate_up_swiglu away from the fused kernel's domain (CPU here): it is
swiglu_fused(linear(x, w)), and the dense MLP built on it computes what the
two-step formula computes."""

import torch

from tensorlink_amd import ops
from tensorlink_amd.models.configs import ModelConfig
from tensorlink_amd.models.dense import MLP


def test_gate_up_swiglu_falls_back_to_the_chain():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 32, generator=g)
    w = torch.randn(2 * 48, 32, generator=g) / 32 ** 0.5
    with torch.no_grad():
        before = ops.gemm_dispatch_count
        got = ops.gate_up_swiglu(x, w)
        assert ops.gemm_dispatch_count == before
        want = ops.swiglu_fused(ops.linear(x, w))
    assert got.shape == (3, 5, 48)
    assert torch.equal(got, want)
    gu = x @ w.t()
    ref = torch.nn.functional.silu(gu[..., :48]) * gu[..., 48:]
    torch.testing.assert_close(got, ref)


def test_mlp_inference_matches_training_formula():
    cfg = ModelConfig(name="mlp-tiny", vocab_size=64, hidden_size=32,
                      intermediate_size=48, num_hidden_layers=1,
                      num_attention_heads=2, num_key_value_heads=1,
                      max_position_embeddings=16)
    torch.manual_seed(1)
    mlp = MLP(cfg)
    x = torch.randn(2, 4, 32)
    with torch.no_grad():
        infer = mlp(x)
    train = mlp(x)          # grad enabled: split + ops.swiglu path
    assert train.requires_grad
    torch.testing.assert_close(infer, train.detach())
