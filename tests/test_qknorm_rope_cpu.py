"""CPU ops.rope_append_(q_norm=, k_norm=) == split / ref.rmsnorm / cat."""

import pytest
import torch

from tensorlink_amd import ops
from tensorlink_amd.ops import reference as ref

HQ, HKV, D, B, S, EPS = 3, 2, 16, 2, 3, 1e-5


@pytest.mark.parametrize("paged", [False, True])
def test_cpu_norm_keywords_equal_composition(paged):
    g = torch.Generator().manual_seed(3)
    W = (HQ + 2 * HKV) * D
    qkv = plain = torch.randn(B * S, W, generator=g)
    wq, wk = (1 + 0.5 * torch.randn(D, generator=g) for _ in range(2))
    pos = (torch.tensor([126, 5])[:, None] + torch.arange(S)).reshape(-1)
    inv = 1.0 / 10000.0 ** (torch.arange(0, D, 2).float() / D)
    shape = (2 * B, HKV, 128, D) if paged else (B, HKV, 160, D)
    table = torch.tensor([[3, 0], [1, 2]]) if paged else None
    k0 = torch.randn(*shape, generator=g).to(plain.dtype)
    v0 = torch.randn(*shape, generator=g).to(plain.dtype)

    q, k, v = plain.split([HQ * D, HKV * D, HKV * D], dim=-1)
    q = ref.rmsnorm(q.reshape(-1, HQ, D), wq.to(q.dtype), EPS)
    k = ref.rmsnorm(k.reshape(-1, HKV, D), wk.to(k.dtype), EPS)
    k_ref, v_ref = k0.clone(), v0.clone()
    q_ref = ops.rope_append_(torch.cat([q.flatten(1), k.flatten(1), v], -1),
                             k_ref, v_ref, pos, inv, S, HQ, HKV,
                             block_table=table)

    got = ops.rope_append_(qkv, k0, v0, pos, inv, S, HQ, HKV,
                           block_table=table, q_norm=wq.to(plain.dtype),
                           k_norm=wk.to(plain.dtype), eps=EPS)
    assert torch.equal(got, q_ref)
    assert torch.equal(k0, k_ref) and torch.equal(v0, v_ref)
