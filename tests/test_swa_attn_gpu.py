"""Sliding-window attention (position p sees key j iff p - W < j <= p): the
WIN prefill kernel and the windowed MFMA decode kernel against a float64
masked softmax. Small W (<= 17) probes the band edge: one key wrongly in or
out moves an output by ~|v| / W >> TOL. Larger W probes the 64-key tile skip.
"""

import functools
import math

import pytest
import torch

from tensorlink_amd import ops

pytestmark = pytest.mark.gpu

TOL = 2e-2          # what the project holds these two kernels to
B, HQ, HKV, G = 2, 4, 2, 2
LENS = [1, 15, 16, 17, 100, 129, 700, 2100]
PAGE, NPG = 128, 17                      # 17 pages >= 2100 keys per row


def _randn(gen, *shape):
    return torch.randn(*shape, device="cuda", generator=gen).bfloat16()


def _ref(q, k, v, q_off, W):
    """q [B,Sq,Hq,D], k/v [B,Skv,Hkv,D] -> float64 [B,Sq,Hq,D]."""
    qf = q.double().transpose(1, 2)
    kf = k.double().transpose(1, 2).repeat_interleave(G, dim=1)
    vf = v.double().transpose(1, 2).repeat_interleave(G, dim=1)
    s = qf @ kf.transpose(-1, -2) / math.sqrt(q.shape[-1])
    p = torch.arange(q.shape[1], device=q.device).unsqueeze(1) + q_off
    j = torch.arange(k.shape[1], device=q.device).unsqueeze(0)
    s = s.masked_fill((j > p) | (j <= p - W), float("-inf"))
    return (s.softmax(-1) @ vf).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def _prefill_inputs(D):
    gen = torch.Generator(device="cuda").manual_seed(D)
    return [_randn(gen, B, 407, h, D) for h in (HQ, HKV, HKV)]


def _prefill(D, Sq, q_off, W):
    q, k, v = _prefill_inputs(D)
    q, k, v = q[:, q_off:q_off + Sq], k[:, :q_off + Sq], v[:, :q_off + Sq]
    return q, k, v, ops.attention_prefill(q, k, v, q_off=q_off, window=W)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("Sq,q_off,W", [
    (200, 0, 2), (330, 0, 17), (330, 0, 64), (330, 0, 65), (330, 0, 100),
    (130, 190, 100), (77, 300, 17), (200, 0, 1), (77, 300, 1)])
def test_prefill_window(D, Sq, q_off, W):
    q, k, v, got = _prefill(D, Sq, q_off, W)
    torch.testing.assert_close(got.double(), _ref(q, k, v, q_off, W),
                               atol=TOL, rtol=TOL)
    if W == 1:      # the row's own key has weight exactly 1
        assert torch.equal(got, v[:, q_off:].repeat_interleave(G, dim=2))


@pytest.mark.parametrize("D", [64, 128])
def test_prefill_window_chunk_independent(D):
    """Chunked == one-shot, bit for bit; a window past Skv == none."""
    chunks = [_prefill(D, n, off, 100)[3]
              for n, off in ((77, 0), (130, 77), (123, 207))]
    assert torch.equal(torch.cat(chunks, dim=1), _prefill(D, 330, 0, 100)[3])
    assert torch.equal(_prefill(D, 330, 0, 1000)[3], _prefill(D, 330, 0, 0)[3])


@functools.lru_cache(maxsize=None)
def _decode_inputs(D):
    """q, caches [B,Hkv,Smax,D], the same as shuffled page pools + table,
    lens, and the float64 reference per window."""
    nb = len(LENS)
    gen = torch.Generator(device="cuda").manual_seed(100 + D)
    q = _randn(gen, nb, HQ, D)
    kc, vc = (_randn(gen, nb, HKV, NPG * PAGE, D) for _ in range(2))
    table = torch.randperm(nb * NPG, device="cuda", generator=gen).int()

    def pool(c):        # page pg of row b goes to pool slot table[b, pg]
        pages = c.view(nb, HKV, NPG, PAGE, D).transpose(1, 2).flatten(0, 1)
        return torch.empty_like(pages).index_copy_(0, table.long(), pages)

    def want(W):
        return torch.cat([
            _ref(q[b:b + 1, None], kc[b:b + 1, :, :L].transpose(1, 2),
                 vc[b:b + 1, :, :L].transpose(1, 2), L - 1, W)[:, 0]
            for b, L in enumerate(LENS)])

    lens = torch.tensor(LENS, device="cuda", dtype=torch.int32)
    return q, kc, vc, pool(kc), pool(vc), table.view(nb, NPG), lens, want


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("W", [1, 2, 16, 17, 128, 1000, 4096])
def test_decode_window(D, W):
    """Against the reference; bit-equal to the plain kernel on a cache of
    only each row's last min(W, L) keys (same splits, same relative tiles),
    to the paged run, and to no window where W >= L; W = 1 copies v."""
    q, kc, vc, kp, vp, table, lens, want = _decode_inputs(D)
    ks, vs = torch.zeros_like(kc), torch.zeros_like(vc)
    for b, L in enumerate(LENS):
        n = min(W, L)
        ks[b, :, :n], vs[b, :, :n] = kc[b, :, L - n:L], vc[b, :, L - n:L]
    full = [b for b, L in enumerate(LENS) if W >= L]
    for ns in (0, 4):
        got = ops.attention_decode(q, kc, vc, lens, n_split=ns, window=W)
        torch.testing.assert_close(got.double(), want(W), atol=TOL, rtol=TOL)
        assert torch.equal(got, ops.attention_decode(
            q, ks, vs, lens.clamp(max=W), n_split=ns))
        assert torch.equal(got, ops.attention_decode(
            q, kp, vp, lens, n_split=ns, block_table=table, window=W))
        plain = ops.attention_decode(q, kc, vc, lens, n_split=ns)
        assert torch.equal(got[full], plain[full])
        if W == 1:
            assert torch.equal(got, vs[:, :, 0].repeat_interleave(G, dim=1))


def test_wide_group_raises_and_dispatch_count():
    # G > 16 runs the v1 kernel, which has no window: an error, not a read
    q = torch.zeros(1, 34, 64, device="cuda", dtype=torch.bfloat16)
    kc = torch.zeros(1, 2, 128, 64, device="cuda", dtype=torch.bfloat16)
    lens = torch.tensor([5], device="cuda", dtype=torch.int32)
    n0 = ops.attn_window_dispatch_count
    ops.attention_decode(q, kc, kc, lens)
    with pytest.raises(RuntimeError, match="window"):
        ops.attention_decode(q, kc, kc, lens, window=4)
    _prefill(64, 77, 0, 17), _prefill(64, 77, 0, 0)
    ops.attention_decode(q[:, :4], kc, kc, lens, window=4)
    assert ops.attn_window_dispatch_count == n0 + 2
