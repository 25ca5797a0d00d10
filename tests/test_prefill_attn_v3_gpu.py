"""Prefill attention v3 (ops/csrc/prefill_attn_v3.hip) against the v2
kernel it replaces: v3 keeps every row's arithmetic, so out and lse must be
bit-identical (torch.equal) to the TL_NO_PREFILL_V3=1 path for every shape,
and K/V given as strided views of a [B,Hkv,Smax,D] cache must give what
contiguous copies give."""

import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def _ext():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


@contextlib.contextmanager
def _v2():
    """The switch is read per call: v2 inside, v3 outside."""
    old = os.environ.get("TL_NO_PREFILL_V3")
    os.environ["TL_NO_PREFILL_V3"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["TL_NO_PREFILL_V3"]
        else:
            os.environ["TL_NO_PREFILL_V3"] = old


def _qkv(B, Sq, Skv, Hq, Hkv, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, device=DEV, dtype=BF, generator=g)
    k = torch.randn(B, Skv, Hkv, D, device=DEV, dtype=BF, generator=g)
    v = torch.randn(B, Skv, Hkv, D, device=DEV, dtype=BF, generator=g)
    return q, k, v


def _both(q, k, v, causal=True, q_off=0):
    ops = _ext()
    assert "TL_NO_PREFILL_V3" not in os.environ
    o3 = ops.attention_prefill(q, k, v, causal=causal, q_off=q_off)
    with _v2():
        o2 = ops.attention_prefill(q, k, v, causal=causal, q_off=q_off)
    return o3, o2


def _both_lse(q, k, v, causal=True):
    from tensorlink_amd import _C as C
    scale = q.shape[-1] ** -0.5
    o3, l3 = C.prefill_attn_lse(q, k, v, scale, causal)
    with _v2():
        o2, l2 = C.prefill_attn_lse(q, k, v, scale, causal)
    return (o3, l3), (o2, l2)


#          B, Sq, Skv, q_off, Hq, Hkv, D
SHAPES = [
    (2, 128, 128, 0, 28, 4, 128),   # GQA 7
    (1, 500, 500, 0, 8, 8, 128),    # row tail, 4 blocks of 128
    (1, 1, 1, 0, 4, 4, 128),
    (1, 65, 65, 0, 14, 2, 128),     # one row into the second 64-row half
    (1, 129, 129, 0, 7, 1, 128),    # one row into the second block
    (2, 64, 64, 0, 4, 2, 64),       # D = 64
    (1, 33, 99, 66, 4, 4, 64),
    (1, 64, 192, 128, 8, 2, 128),   # chunked, aligned
    (2, 50, 127, 77, 4, 2, 128),    # chunked, ragged chunk and history
]


@pytest.mark.parametrize("B,Sq,Skv,q_off,Hq,Hkv,D", SHAPES)
def test_v3_equals_v2_bitwise(B, Sq, Skv, q_off, Hq, Hkv, D):
    q, k, v = _qkv(B, Sq, Skv, Hq, Hkv, D, seed=31)
    o3, o2 = _both(q, k, v, q_off=q_off)
    assert torch.equal(o3, o2)
    if q_off == 0 and Sq == Skv:   # the lse entry point has no q_off
        (o3, l3), (o2, l2) = _both_lse(q, k, v)
        assert torch.equal(o3, o2)
        assert torch.equal(l3, l2)


def test_v3_against_reference():
    from tensorlink_amd.ops import reference as ref
    q, k, v = _qkv(2, 200, 200, 28, 4, 128, seed=32)
    o3, o2 = _both(q, k, v)
    assert torch.equal(o3, o2)
    out_ref = ref.attention_prefill(q.float(), k.float(), v.float(),
                                    causal=True)
    torch.testing.assert_close(o3.float(), out_ref, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("Sq,Skv", [(130, 130), (70, 200)])
def test_v3_non_causal(Sq, Skv):
    q, k, v = _qkv(2, Sq, Skv, 8, 2, 128, seed=33)
    o3, o2 = _both(q, k, v, causal=False)
    assert torch.equal(o3, o2)
    if Sq != Skv:
        return
    (o3, l3), (o2, l2) = _both_lse(q, k, v, causal=False)
    assert torch.equal(o3, o2)
    assert torch.equal(l3, l2)


@pytest.mark.parametrize("extra", [0, 1, 70])
@pytest.mark.parametrize("B,Sq,Skv,q_off,Hq,Hkv,D", [
    (2, 50, 127, 77, 4, 2, 128),
    (2, 130, 130, 0, 14, 2, 128),
    (1, 33, 99, 66, 4, 4, 64),
])
def test_v3_reads_cache_views_in_place(B, Sq, Skv, q_off, Hq, Hkv, D, extra):
    """K/V as permuted views of a [B,Hkv,Smax,D] buffer whose rows past Skv
    are NaN: a key past Skv must contribute exactly zero (V zeroed, not
    only masked), and with Smax == Skv the last tile's rows past Skv lie
    outside the buffer, so the kernel's clamped row index is what keeps
    every address inside it."""
    ops = _ext()
    q, k, v = _qkv(B, Sq, Skv, Hq, Hkv, D, seed=34)
    Smax = Skv + extra
    kc = torch.full((B, Hkv, Smax, D), float("nan"), device=DEV, dtype=BF)
    vc = torch.full((B, Hkv, Smax, D), float("nan"), device=DEV, dtype=BF)
    kc[:, :, :Skv] = k.permute(0, 2, 1, 3)
    vc[:, :, :Skv] = v.permute(0, 2, 1, 3)
    kview = kc[:, :, :Skv].permute(0, 2, 1, 3)
    vview = vc[:, :, :Skv].permute(0, 2, 1, 3)
    assert extra == 0 or not kview.is_contiguous()
    o_view = ops.attention_prefill(q, kview, vview, q_off=q_off)
    o_copy, o2 = _both(q, k, v, q_off=q_off)
    assert torch.isfinite(o_view.float()).all()
    assert torch.equal(o_view, o_copy)
    assert torch.equal(o_view, o2)
    with _v2():   # the v2 route copies the views itself
        assert torch.equal(ops.attention_prefill(q, kview, vview,
                                                 q_off=q_off), o2)


def test_v3_rescale_every_tile_and_ties():
    # q x30: scores spread over +-300, so the running max moves at almost
    # every tile and alpha underflows to 0 on some
    q, k, v = _qkv(1, 320, 320, 8, 2, 128, seed=35)
    (o3, l3), (o2, l2) = _both_lse(q * 30, k, v)
    assert torch.equal(o3, o2)
    assert torch.equal(l3, l2)
    # constant K: every score of a row ties with the row max
    kc = torch.ones_like(k) * 0.5
    (o3, l3), (o2, l2) = _both_lse(q, kc, v)
    assert torch.equal(o3, o2)
    assert torch.equal(l3, l2)


def test_v3_deterministic():
    ops = _ext()
    q, k, v = _qkv(2, 300, 300, 14, 2, 128, seed=36)
    first = ops.attention_prefill(q, k, v)
    for _ in range(4):
        assert torch.equal(ops.attention_prefill(q, k, v), first)


def test_model_prefill_and_greedy_tokens_equal():
    from tensorlink_amd.parallel.planner import plan_for_world
    from tensorlink_amd.parallel.pipeline import PipelineRunner, SamplingParams
    plan = plan_for_world("tiny", 1, batch_size=2, seq_len=160)
    r = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    ids = torch.randint(0, 1024, (2, 150),
                        generator=torch.Generator().manual_seed(37))
    sp = SamplingParams(temperature=0.0, max_new_tokens=4)
    t3 = r.generate(ids, sp).cpu()
    with _v2():
        t2 = r.generate(ids, sp).cpu()
    assert t3.shape == (2, 4)
    assert torch.equal(t3, t2)


def test_attention_train_loss_and_grads_equal():
    ops = _ext()
    q0, k0, v0 = _qkv(2, 150, 150, 8, 2, 64, seed=38)
    w = torch.randn(q0.shape, device=DEV, dtype=BF,
                    generator=torch.Generator(device=DEV).manual_seed(39))

    def run():
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        loss = (ops.attention_train(q, k, v).float() * w.float()).sum()
        loss.backward()
        return loss.detach(), q.grad, k.grad, v.grad

    r3 = run()
    with _v2():
        r2 = run()
    for a, b in zip(r3, r2):
        assert torch.equal(a, b)
