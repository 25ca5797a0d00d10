"""CPU checks of the decoder's residual carry (StageModel.forward hands
each layer's closing residual add to the next norm): same fp32 results as
the layer-by-layer chain, and a headless stage still returns the fully
added stream."""

import os

import torch

from tensorlink_amd.models.configs import get_config
from tensorlink_amd.models.dense import StageModel
from tensorlink_amd.models.loader import init_random_stage


def _model(has_head=True):
    cfg = get_config("tiny")
    m = StageModel(cfg, 0, 3, True, has_head)
    init_random_stage(m, device="cpu", dtype=torch.float32, seed=5)
    with torch.no_grad():
        g = torch.Generator().manual_seed(6)
        for name, p in m.named_parameters():
            if "norm" in name:
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
    return m.eval()


def _inputs(cfg, B=2, S=6):
    ids = torch.randint(0, cfg.vocab_size, (B, S),
                        generator=torch.Generator().manual_seed(7))
    pos = torch.arange(S, dtype=torch.int32).expand(B, S).contiguous()
    return ids, pos


@torch.no_grad()
def _prefill_and_decode(m, ids, pos):
    B, S = ids.shape
    cache = m.make_kv_cache(B, S + 2, "cpu")
    a = m(ids, pos, kv_cache=cache)
    nxt = a[:, -1].argmax(-1, keepdim=True)
    b = m(nxt, torch.full((B, 1), S, dtype=torch.int32), kv_cache=cache)
    return a, b


def test_carry_forward_matches_layerwise_chain_cpu():
    m = _model()
    ids, pos = _inputs(m.config)
    with torch.no_grad():
        nocache = m(ids, pos)
    a, b = _prefill_and_decode(m, ids, pos)
    os.environ["TL_NO_DECODE_FUSION"] = "1"
    try:
        with torch.no_grad():
            nocache_ref = m(ids, pos)
        a_ref, b_ref = _prefill_and_decode(m, ids, pos)
    finally:
        os.environ.pop("TL_NO_DECODE_FUSION", None)
    assert torch.equal(nocache, nocache_ref)
    assert torch.equal(a, a_ref)
    assert torch.equal(b, b_ref)


@torch.no_grad()
def test_headless_stage_returns_added_stream_cpu():
    m = _model(has_head=False)
    ids, pos = _inputs(m.config)
    out = m(ids, pos)
    # layer by layer, each layer adding its own MLP output
    hidden = m.embed(ids)
    for i, layer in enumerate(m.layers):
        hidden = layer(hidden, pos, None, i, False)
    assert torch.equal(out, hidden)
    # and the carry itself really defers the last add
    res, pending = m.embed(ids), None
    for i, layer in enumerate(m.layers):
        res, pending = layer.forward_carry(res, pending, pos, None, i)
    assert pending is not None and not torch.equal(res, hidden)
    assert torch.equal(res + pending, hidden)
