"""ops.attention_prefill takes K/V as strided views (the permuted KV cache,
read in place on the GPU): on CPU the same call must equal the reference on
contiguous copies."""

import pytest
import torch

from tensorlink_amd import ops
from tensorlink_amd.ops import reference as ref


@pytest.mark.parametrize("extra", [0, 1, 70])
@pytest.mark.parametrize("B,Sq,Skv,q_off,Hq,Hkv,D", [
    (2, 50, 127, 77, 4, 2, 32),
    (1, 40, 40, 0, 6, 2, 16),
])
def test_prefill_on_cache_views_equals_contiguous(B, Sq, Skv, q_off, Hq, Hkv,
                                                  D, extra):
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, Sq, Hq, D, generator=g)
    kc = torch.full((B, Hkv, Skv + extra, D), float("nan"))
    vc = torch.full((B, Hkv, Skv + extra, D), float("nan"))
    kc[:, :, :Skv] = torch.randn(B, Hkv, Skv, D, generator=g)
    vc[:, :, :Skv] = torch.randn(B, Hkv, Skv, D, generator=g)
    kview = kc[:, :, :Skv].permute(0, 2, 1, 3)
    vview = vc[:, :, :Skv].permute(0, 2, 1, 3)
    out = ops.attention_prefill(q, kview, vview, causal=True, q_off=q_off)
    want = ref.attention_prefill(q, kview.contiguous(), vview.contiguous(),
                                 causal=True, q_off=q_off)
    assert torch.isfinite(out).all()
    assert torch.equal(out, want)
