"""Carried-state prefill attention off the GPU: the fp32 reference of the
state semantics (ops/reference.py attention_prefill_carry), the op layer's
CPU dispatch, and the factored CP ring accumulation (parallel/cp.py
_ring_accumulate) against the partial/merge math it was factored from."""

import pytest
import torch

from tensorlink_amd import ops
from tensorlink_amd.ops import reference as ref
from tensorlink_amd.parallel import cp


def _qkv(B, Sq, Skv, Hq, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, generator=g)
    k = torch.randn(B, Skv, Hkv, D, generator=g)
    v = torch.randn(B, Skv, Hkv, D, generator=g)
    return q, k, v


def _bounds(lengths):
    out, c0 = [], 0
    for n in lengths:
        out.append((c0, c0 + n))
        c0 += n
    return out


def _carried(fn, q, k, v, chunks, causal, hist, scale):
    """fn over the key chunks [(c0, c1), ...] in the given order. With
    causal every chunk is masked against the global diagonal: key c0 + j is
    visible to row i when c0 + j <= hist + i, which is q_off = hist - c0
    (negative for a chunk that starts inside the query range)."""
    B, Sq, Hq, D = q.shape
    o_state = torch.full((B, Sq, Hq, D), float("nan"))
    ml_state = torch.full((B, Hq, Sq, 2), float("nan"))
    out = None
    for i, (c0, c1) in enumerate(chunks):
        out = fn(q, k[:, c0:c1], v[:, c0:c1], o_state, ml_state,
                 causal=causal, scale=scale, q_off=hist - c0,
                 first=i == 0, last=i == len(chunks) - 1)
        assert (out is None) == (i != len(chunks) - 1)
    return out


def _ref_fn(q, k, v, o_state, ml_state, **kw):
    return ref.attention_prefill_carry(q, k, v, o_state, ml_state, **kw)


ORDERS = {
    "ascending": lambda b: b,
    "ring": lambda b: [b[-1]] + b[-2::-1],     # last chunk, then descending
    "shuffled": lambda b: [b[i] for i in
                           torch.randperm(len(b), generator=torch.Generator()
                                          .manual_seed(5)).tolist()],
}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,Sq,Hq,Hkv,D,lengths", [
    (2, 37, 6, 2, 16, [13, 40, 1, 29, 37]),    # GQA 3, last chunk = queries
    (1, 50, 4, 4, 32, [7, 64, 30, 19]),        # chunks cut the query range
])
def test_reference_carry_equals_one_pass(B, Sq, Hq, Hkv, D, lengths, causal,
                                         order):
    Skv = sum(lengths)
    hist = Skv - Sq
    q, k, v = _qkv(B, Sq, Skv, Hq, Hkv, D, seed=61)
    scale = D ** -0.5
    chunks = ORDERS[order](_bounds(lengths))
    out = _carried(_ref_fn, q, k, v, chunks, causal, hist, scale)
    want = ref.attention_prefill(q, k, v, causal, scale, hist)
    torch.testing.assert_close(out, want, atol=1e-5, rtol=0)


def test_reference_carry_state_semantics():
    """A row that has seen no key holds (-1e30, 0) and a zero accumulator,
    `first` ignores what the buffers held, `last` leaves them alone and a
    row with no key at all comes out 0."""
    q, k, v = _qkv(1, 4, 3, 2, 2, 8, seed=62)
    o_state = torch.full((1, 4, 2, 8), float("nan"))
    ml_state = torch.full((1, 2, 4, 2), float("nan"))
    # q_off = -2: rows 0 and 1 see no key, row 2 key 0, row 3 keys 0..1
    assert ref.attention_prefill_carry(q, k[:, :2], v[:, :2], o_state,
                                       ml_state, causal=True, q_off=-2,
                                       first=True, last=False) is None
    assert torch.equal(ml_state[0, :, :2, 0], torch.full((2, 2), -1e30))
    assert torch.equal(ml_state[0, :, :2, 1], torch.zeros(2, 2))
    assert torch.equal(o_state[0, :2], torch.zeros(2, 2, 8))
    assert torch.isfinite(o_state).all() and torch.isfinite(ml_state).all()
    # unnormalised: o / l is the softmax output
    want = ref.attention_prefill(q[:, 2:], k[:, :2], v[:, :2], True, None, 0)
    l = ml_state[0, :, 2:, 1].transpose(0, 1).unsqueeze(-1)
    torch.testing.assert_close(o_state[:, 2:] / l, want, atol=1e-6, rtol=0)
    o_before, ml_before = o_state.clone(), ml_state.clone()
    # the last chunk (key 2) lies past every row's diagonal
    out = ref.attention_prefill_carry(q, k[:, 2:], v[:, 2:], o_state,
                                      ml_state, causal=True, q_off=-4,
                                      first=False, last=True)
    assert torch.equal(o_state, o_before) and torch.equal(ml_state, ml_before)
    assert torch.equal(out[:, :2], torch.zeros(1, 2, 2, 8))
    torch.testing.assert_close(out[:, 2:], want, atol=1e-6, rtol=0)


def test_ops_carry_dispatches_to_reference_on_cpu():
    q, k, v = _qkv(2, 20, 52, 4, 2, 64, seed=63)     # D the kernel supports
    scale = 0.11
    chunks = _bounds([32, 20])
    before = ops.attn_carry_dispatch_count

    carry = ops.AttnCarry.empty(q)
    assert carry.o.shape == (2, 20, 4, 64) and carry.o.dtype == torch.float32
    assert carry.ml.shape == (2, 4, 20, 2) and carry.ml.dtype == torch.float32

    def ops_fn(q, k, v, o_state, ml_state, **kw):
        return ops.attention_prefill_carry(q, k, v, carry, **kw)

    got = _carried(ops_fn, q, k, v, chunks, True, 32, scale)
    want = _carried(_ref_fn, q, k, v, chunks, True, 32, scale)
    assert torch.equal(got, want)
    assert ops.attn_carry_dispatch_count == before


@pytest.mark.parametrize("sc", [24, 7])
def test_ring_accumulate_equals_partial_merge_on_cpu(sc, monkeypatch):
    monkeypatch.delenv("TL_NO_CP_KERNEL", raising=False)
    world, Hq, Hkv, D = 4, 4, 2, 16
    q, k, v = _qkv(2, sc * world, sc * world, Hq, Hkv, D, seed=64)
    scale = D ** -0.5
    before = ops.attn_carry_dispatch_count
    for rank in range(world):
        qr = q[:, rank * sc:(rank + 1) * sc]
        steps = [((rank - r) % world,
                  k[:, ((rank - r) % world) * sc:((rank - r) % world + 1) * sc],
                  v[:, ((rank - r) % world) * sc:((rank - r) % world + 1) * sc])
                 for r in range(world)]
        acc = None
        for src, kc, vc in steps:
            if src <= rank:
                acc = cp._merge(acc, cp._partial_attn(qr, kc, vc, scale,
                                                      causal_diag=src == rank))
        o, m, l = acc
        want = o / l.permute(0, 2, 1).unsqueeze(-1).clamp(min=1e-30)
        seen = []

        def feed():
            for s in steps:
                seen.append(s[0])
                yield s

        got = cp._ring_accumulate(qr, scale, rank, feed())
        assert torch.equal(got, want)
        assert len(seen) == world           # the ring is always drained
        full = ref.attention_prefill(qr, k, v, True, scale, rank * sc)
        torch.testing.assert_close(got, full, atol=1e-5, rtol=0)
    assert ops.attn_carry_dispatch_count == before
