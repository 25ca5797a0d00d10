"""Greedy head on CPU: ops.linear_argmax and StageModel.head_tokens /
forward(greedy=True) are the two-step form (logits, then argmax) wherever
the fused kernel (ops/csrc/head_argmax.hip) does not serve, and a CPU
tensor never reaches it."""

import pytest
import torch

from tensorlink_amd import ops
from tensorlink_amd.models.configs import ModelConfig
from tensorlink_amd.models.dense import build_full_model
from tensorlink_amd.models.loader import init_random_stage


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lead", [(5,), (3, 2)])
def test_linear_argmax_is_linear_then_argmax(lead, dtype):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(*lead, 64, generator=gen).to(dtype)
    w = torch.randn(512, 64, generator=gen).to(dtype)
    before = ops.head_argmax_dispatch_count
    got = ops.linear_argmax(x, w)
    assert ops.head_argmax_dispatch_count == before == 0
    assert got.dtype == torch.int64 and got.shape == lead
    assert torch.equal(got, ops.linear(x, w).argmax(-1))


def test_linear_argmax_takes_the_first_of_equal_maxima():
    x = torch.ones(2, 8)
    w = torch.zeros(16, 8)
    w[3] = 1.0
    w[11] = 1.0
    assert ops.linear_argmax(x, w).tolist() == [3, 3]


def _stage(tied: bool):
    cfg = ModelConfig(name="head-tiny", vocab_size=512, hidden_size=64,
                      intermediate_size=128, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=1,
                      max_position_embeddings=32, tie_word_embeddings=tied)
    m = build_full_model(cfg)
    init_random_stage(m, dtype=torch.float32, seed=2)
    assert hasattr(m, "lm_head") != tied
    return m.eval(), cfg


@pytest.mark.parametrize("tied", [False, True])
def test_stage_greedy_equals_argmax_of_logits(tied):
    m, cfg = _stage(tied)
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(0, cfg.vocab_size, (3, 7), generator=gen)
    pos = torch.arange(7, dtype=torch.int32).unsqueeze(0).expand(3, -1)
    logits = m(ids, pos)
    tok = m(ids, pos, greedy=True)
    assert logits.shape == (3, 7, cfg.vocab_size)
    assert tok.dtype == torch.int64 and tok.shape == (3, 7)
    assert torch.equal(tok, logits.argmax(-1))
    # the default is logits, and greedy without a head request is ignored
    assert torch.equal(m(ids, pos, greedy=False), logits)
    hidden = m(ids, pos, return_logits=False, greedy=True)
    assert hidden.shape == (3, 7, cfg.hidden_size)


@pytest.mark.parametrize("tied", [False, True])
def test_head_tokens_equals_argmax_of_head(tied):
    m, cfg = _stage(tied)
    gen = torch.Generator().manual_seed(4)
    h = torch.randn(3, 1, cfg.hidden_size, generator=gen)
    pending = torch.randn(3, 1, cfg.hidden_size, generator=gen)
    assert torch.equal(m.head_tokens(h), m.head(h).argmax(-1))
    assert torch.equal(m.head_tokens(h, pending),
                       m.head(h, pending).argmax(-1))
    assert ops.head_argmax_dispatch_count == 0


@pytest.mark.parametrize("arch", ["gpt2", "neox"])
def test_other_families_accept_greedy(arch):
    cfg = ModelConfig(name=f"head-{arch}", vocab_size=128, hidden_size=32,
                      intermediate_size=64, num_hidden_layers=1,
                      num_attention_heads=2, num_key_value_heads=2,
                      max_position_embeddings=16, architecture=arch,
                      tie_word_embeddings=arch == "gpt2")
    m = build_full_model(cfg)
    init_random_stage(m, dtype=torch.float32, seed=5)
    m.eval()
    ids = torch.randint(0, 128, (2, 5),
                        generator=torch.Generator().manual_seed(6))
    pos = torch.arange(5, dtype=torch.int32).unsqueeze(0).expand(2, -1)
    logits = m(ids, pos)
    assert torch.equal(m(ids, pos, greedy=True), logits.argmax(-1))
