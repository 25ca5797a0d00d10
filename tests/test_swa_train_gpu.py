"""Windowed training attention (position p sees key j iff p - W < j <= p):
ops.attention_train(window=W) through the WIN prefill kernel (with lse) and
the WIN instantiations of flash_bwd.hip, against a float64 masked softmax
with autograd. W <= 3 probes the band edge at the default scale; W >= 64
probes the 64-row tile ranges with scale 4/sqrt(D), which peaks every row on
a few keys so that a dropped or extra tile moves some gradient by O(1).
"""

import dataclasses
import functools
import math

import pytest
import torch

from tensorlink_amd import ops

pytestmark = pytest.mark.gpu

TOL_OUT, TOL_GRAD = 2e-2, 7e-2   # test_flash_attn_backward's, same kernels
B, HQ, HKV, G = 2, 4, 2, 2


@functools.lru_cache(maxsize=None)
def _inputs(D):
    """q, k, v, dout at S = 330 (CPU generator: the same values anywhere)."""
    gen = torch.Generator().manual_seed(D)
    return [torch.randn(B, 330, h, D, generator=gen).bfloat16().cuda()
            for h in (HQ, HKV, HKV, HQ)]


def _ref(q, k, v, dout, W, scale):
    """float64 out, dq, dk, dv; autograd sums k/v grads over the group."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    kf = k.transpose(1, 2).repeat_interleave(G, dim=1)
    vf = v.transpose(1, 2).repeat_interleave(G, dim=1)
    s = q.transpose(1, 2) @ kf.transpose(-1, -2) * scale
    p = torch.arange(q.shape[1], device=q.device).unsqueeze(1)
    j = torch.arange(q.shape[1], device=q.device).unsqueeze(0)
    s = s.masked_fill((j > p) | (j <= p - W), float("-inf"))
    out = (s.softmax(-1) @ vf).transpose(1, 2)
    out.backward(dout.double())
    return out.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S,W", [(200, 1), (200, 2), (200, 3), (330, 64),
                                 (330, 65), (330, 100), (330, 129),
                                 (100, 64)])
def test_band_and_tile_ranges(D, S, W):
    scale = (4.0 if W >= 64 else 1.0) / math.sqrt(D)
    q, k, v, dout = (t[:, :S].clone() for t in _inputs(D))
    for t in (q, k, v):
        t.requires_grad_(True)
    n0 = ops.attn_window_dispatch_count
    out = ops.attention_train(q, k, v, scale=scale, window=W)
    assert "FlashAttn" in type(out.grad_fn).__name__
    assert ops.attn_window_dispatch_count == n0 + 1
    out.backward(dout)
    want = _ref(q, k, v, dout, W, scale)
    torch.testing.assert_close(out.double(), want[0], atol=TOL_OUT,
                               rtol=TOL_OUT)
    for got, ref in zip((q.grad, k.grad, v.grad), want[1:]):
        torch.testing.assert_close(got.double(), ref, atol=TOL_GRAD,
                                   rtol=TOL_GRAD)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("W", [200, 5000])
def test_window_past_s_is_the_plain_kernel(D, W):
    """A window that hides nothing: the same bits as window = 0."""
    from tensorlink_amd import _C
    q, k, v, dout = (t[:, :200].contiguous() for t in _inputs(D))
    scale = 1.0 / math.sqrt(D)
    out, lse = _C.prefill_attn_lse(q, k, v, scale, True, 0)
    out_w, lse_w = _C.prefill_attn_lse(q, k, v, scale, True, W)
    assert torch.equal(out_w, out) and torch.equal(lse_w, lse)
    delta = (dout.float() * out.float()).sum(-1).permute(0, 2, 1).contiguous()
    plain = _C.attn_bwd(q, k, v, dout, lse, delta, scale, True, 0)
    win = _C.attn_bwd(q, k, v, dout, lse, delta, scale, True, W)
    for a, b in zip(win, plain):
        assert torch.equal(a, b)


def test_model_step_matches_sdpa_route(monkeypatch):
    """One loss + backward of a windowed tiny model at S = 160: the HIP
    route against the SDPA band-mask composition (TL_NO_SWA_TRAIN=1). The
    routes differ in arithmetic, so the kernels' gradient tolerance."""
    from tensorlink_amd.models import build_full_model, get_config
    from tensorlink_amd.models.loader import init_random_stage
    cfg = dataclasses.replace(get_config("tiny"), sliding_window=48)
    m = build_full_model(cfg)
    init_random_stage(m, device="cuda", dtype=torch.bfloat16)
    ids = torch.randint(0, cfg.vocab_size, (2, 160),
                        generator=torch.Generator().manual_seed(7)).cuda()
    pos = torch.arange(160, device="cuda").repeat(2, 1)

    def step():
        m.zero_grad(set_to_none=True)
        n0 = ops.attn_window_dispatch_count
        loss = ops.causal_lm_loss(m(ids, pos, training=True), ids)
        loss.backward()
        return (ops.attn_window_dispatch_count - n0, loss.detach(),
                [p.grad for p in m.parameters()])

    n_hip, loss_hip, grads_hip = step()
    monkeypatch.setenv("TL_NO_SWA_TRAIN", "1")
    n_sdpa, loss_sdpa, grads_sdpa = step()
    assert (n_hip, n_sdpa) == (cfg.num_hidden_layers, 0)
    torch.testing.assert_close(loss_hip, loss_sdpa, atol=TOL_GRAD,
                               rtol=TOL_GRAD)
    for a, b in zip(grads_hip, grads_sdpa):
        torch.testing.assert_close(a.float(), b.float(), atol=TOL_GRAD,
                                   rtol=TOL_GRAD)


@pytest.mark.parametrize("causal,W", [(False, 4), (True, -1)])
def test_argument_errors(causal, W):
    from tensorlink_amd import _C
    q, k, v, dout = (t[:, :64].contiguous() for t in _inputs(64))
    lse = torch.zeros(B, HQ, 64, device="cuda")
    with pytest.raises(RuntimeError, match="window"):
        _C.prefill_attn_lse(q, k, v, 0.125, causal, W)
    with pytest.raises(RuntimeError, match="window"):
        _C.attn_bwd(q, k, v, dout, lse, lse, 0.125, causal, W)
