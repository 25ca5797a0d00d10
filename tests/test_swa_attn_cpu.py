"""Sliding-window attention off the GPU: config, reference, model paths."""

import dataclasses

import pytest
import torch

from tensorlink_amd.models import build_full_model, get_config
from tensorlink_amd.models.configs import ModelConfig
from tensorlink_amd.models.loader import init_random_stage
from tensorlink_amd.ops import reference as ref


def test_hf_mapping():
    cfg = {"architectures": ["MistralForCausalLM"], "sliding_window": 4096}
    assert ModelConfig.from_hf_config(cfg).sliding_window == 4096
    cfg["sliding_window"] = None
    assert ModelConfig.from_hf_config(cfg).sliding_window == 0
    cfg = {"architectures": ["Qwen2ForCausalLM"], "sliding_window": 4096}
    assert ModelConfig.from_hf_config(cfg).sliding_window == 0
    cfg["use_sliding_window"] = True
    with pytest.raises(KeyError, match="use_sliding_window"):
        ModelConfig.from_hf_config(cfg)


def test_reference_band_mask():
    S, W, D = 9, 3, 4
    torch.manual_seed(0)
    q, k, v = (torch.randn(1, S, 1, D, dtype=torch.float64) for _ in range(3))
    want = torch.zeros_like(q)
    for p in range(S):
        js = [j for j in range(S) if p - W < j <= p]
        w = torch.stack([q[0, p, 0] @ k[0, j, 0] / D ** 0.5
                         for j in js]).softmax(0)
        want[0, p, 0] = sum(wj * v[0, j, 0] for wj, j in zip(w, js))
    got = ref.attention_prefill(q, k, v, window=W)
    torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-6)
    dec = ref.attention_decode(q[:, -1:], k, v, torch.tensor([S]), window=W)
    torch.testing.assert_close(dec[:, 0], want[:, -1], atol=1e-6, rtol=1e-6)


def test_windowed_model_cache_matches_full_forward():
    """Cached prefill (40) + 20 decode steps == the no-cache forward at
    test_decode_matches_full_forward's tolerance; chunked == one-shot."""
    B, P, N, TOL = 2, 40, 20, dict(atol=1e-4, rtol=1e-3)
    cfg = dataclasses.replace(get_config("tiny"), sliding_window=24)
    m, m0 = build_full_model(cfg), build_full_model(get_config("tiny"))
    init_random_stage(m, dtype=torch.float32, seed=0)
    init_random_stage(m0, dtype=torch.float32, seed=0)
    pos = lambda lo, hi: torch.arange(lo, hi).repeat(B, 1)
    torch.manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (B, P + N))
    full = m(ids, pos(0, P + N))
    cache = m.make_kv_cache(B, 64, "cpu")
    steps = [m(ids[:, :P], pos(0, P), kv_cache=cache)]
    for t in range(P, P + N):
        steps.append(m(ids[:, t:t + 1], pos(t, t + 1), kv_cache=cache))
    torch.testing.assert_close(torch.cat(steps, 1), full, **TOL)
    cache = m.make_kv_cache(B, 64, "cpu")
    parts = [m(ids[:, :17], pos(0, 17), kv_cache=cache),
             m(ids[:, 17:P], pos(17, P), kv_cache=cache)]
    torch.testing.assert_close(torch.cat(parts, 1), steps[0], **TOL)
    plain = m0(ids, pos(0, P + N))      # same weights, no window
    torch.testing.assert_close(plain[:, :24], full[:, :24], **TOL)
    assert not torch.allclose(plain[:, 24:], full[:, 24:], **TOL)
