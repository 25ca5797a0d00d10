"""Carried-state prefill attention (prefill_attn_v3.hip, CARRY variant)
against the one-call v3 kernel and the fp32 reference.

The contract: carried calls over key chunks in ascending order with every
chunk boundary on a multiple of 64 keys run the tile steps of one call over
the concatenated keys in the same order, so the result is bit-identical
(torch.equal) to _C.prefill_attn / _C.prefill_attn_lse. Any other order or
boundary is the same softmax merged in another order and is held to the
tolerance test_v3_against_reference uses for this kernel (2e-2)."""

import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
TOL = 2e-2


def _C():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    from tensorlink_amd import _C as C
    return C


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _qkv(B, Sq, Skv, Hq, Hkv, D, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, Sq, Hq, D, device=DEV, dtype=BF, generator=g)
    k = torch.randn(B, Skv, Hkv, D, device=DEV, dtype=BF, generator=g)
    v = torch.randn(B, Skv, Hkv, D, device=DEV, dtype=BF, generator=g)
    return q, k, v


def _state(q, fill=float("nan")):
    B, Sq, Hq, D = q.shape
    return (torch.full((B, Sq, Hq, D), fill, device=DEV),
            torch.full((B, Hq, Sq, 2), fill, device=DEV))


def _carry(q, steps, state=None, want_lse=False):
    """steps = [(k, v, causal, q_off), ...]; the first is `first`, the last
    is `last`. The state starts as NaN: `first` must not read it."""
    C = _C()
    o_state, ml_state = state if state is not None else _state(q)
    scale = q.shape[-1] ** -0.5
    res = None
    for i, (k, v, causal, q_off) in enumerate(steps):
        last = i == len(steps) - 1
        res = C.prefill_attn_carry(q, k, v, o_state, ml_state, scale, causal,
                                   q_off, i == 0, last, want_lse and last)
        assert (res is None) == (not last)
    return res


def _ascending(k, v, lengths, causal_last):
    steps, c0 = [], 0
    for i, n in enumerate(lengths):
        steps.append((k[:, c0:c0 + n], v[:, c0:c0 + n],
                      causal_last and i == len(lengths) - 1, 0))
        c0 += n
    return steps


#   B, Sq, Hq, Hkv, D, history chunks (+ a final chunk of Sq keys)
ALIGNED = [
    (1, 128, 8, 2, 128, [64, 64]),
    (2, 65, 14, 2, 128, [128]),       # ragged final chunk, second half row
    (1, 129, 4, 4, 64, [64, 192]),    # second block, D = 64
    (1, 1, 4, 4, 128, [64]),
]


@pytest.mark.parametrize("B,Sq,Hq,Hkv,D,hist", ALIGNED)
def test_aligned_ascending_is_bitwise_one_call(B, Sq, Hq, Hkv, D, hist):
    C = _C()
    H = sum(hist)
    q, k, v = _qkv(B, Sq, H + Sq, Hq, Hkv, D, seed=71)
    got = _carry(q, _ascending(k, v, hist + [Sq], causal_last=True))
    want = C.prefill_attn(q, k, v, D ** -0.5, True, H)
    assert got.dtype == BF and got.shape == q.shape
    assert torch.equal(got, want)


def test_aligned_ascending_non_causal_out_and_lse():
    C = _C()
    q, k, v = _qkv(2, 70, 200, 8, 2, 128, seed=72)
    got, lse = _carry(q, _ascending(k, v, [64, 128, 8], causal_last=False),
                      want_lse=True)
    assert torch.equal(got, C.prefill_attn(q, k, v, 128 ** -0.5, False, 0))
    want, want_lse = C.prefill_attn_lse(q, k, v, 128 ** -0.5, False)
    assert torch.equal(got, want)
    assert lse.shape == (2, 8, 70) and torch.equal(lse, want_lse)


def test_aligned_ascending_rescale_every_tile():
    # q x30: scores spread over +-300, so the running max moves at almost
    # every tile and alpha underflows to 0 on some, across chunk boundaries
    C = _C()
    hist = [64, 128, 64]
    q, k, v = _qkv(1, 192, 256 + 192, 8, 2, 128, seed=73)
    q = q * 30
    got = _carry(q, _ascending(k, v, hist + [192], causal_last=True))
    assert torch.equal(got, C.prefill_attn(q, k, v, 128 ** -0.5, True, 256))


def test_aligned_ascending_cache_views_with_nan_tail():
    """K/V chunks as permuted views of a [B,Hkv,Smax,D] buffer whose rows
    past Skv are NaN: the last chunk's ragged tile reads clamped rows and
    zeroes them, exactly as the one-call kernel does."""
    C = _C()
    B, Sq, Hq, Hkv, D, H = 2, 65, 14, 2, 128, 128
    Skv = H + Sq
    q, k, v = _qkv(B, Sq, Skv, Hq, Hkv, D, seed=74)
    kc = torch.full((B, Hkv, Skv + 70, D), float("nan"), device=DEV, dtype=BF)
    vc = torch.full((B, Hkv, Skv + 70, D), float("nan"), device=DEV, dtype=BF)
    kc[:, :, :Skv] = k.permute(0, 2, 1, 3)
    vc[:, :, :Skv] = v.permute(0, 2, 1, 3)
    kview = kc[:, :, :Skv].permute(0, 2, 1, 3)
    vview = vc[:, :, :Skv].permute(0, 2, 1, 3)
    assert not kview.is_contiguous()
    got = _carry(q, _ascending(kview, vview, [64, 64, Sq], causal_last=True))
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, C.prefill_attn(q, k, v, D ** -0.5, True, H))


@pytest.mark.parametrize("B,S,Hq,Hkv,D", [(2, 130, 14, 2, 128),
                                          (1, 33, 4, 4, 64)])
def test_first_and_last_is_the_plain_kernel(B, S, Hq, Hkv, D):
    C = _C()
    q, k, v = _qkv(B, S, S, Hq, Hkv, D, seed=75)
    got = _carry(q, [(k, v, True, 0)])
    assert torch.equal(got, C.prefill_attn(q, k, v, D ** -0.5, True, 0))
    got, lse = _carry(q, [(k, v, True, 0)], want_lse=True)
    want, want_lse = C.prefill_attn_lse(q, k, v, D ** -0.5, True)
    assert torch.equal(got, want)
    assert torch.equal(lse, want_lse)


def test_first_ignores_the_state():
    C = _C()
    q, k, v = _qkv(2, 150, 150, 8, 2, 128, seed=76)
    scale = 128 ** -0.5
    states = []
    for fill in (float("nan"), 0.0):
        o_state, ml_state = _state(q, fill)
        assert C.prefill_attn_carry(q, k, v, o_state, ml_state, scale, True,
                                    0, True, False) is None
        states.append((o_state, ml_state))
    (o_nan, ml_nan), (o_zero, ml_zero) = states
    assert torch.isfinite(o_nan).all() and torch.isfinite(ml_nan).all()
    assert torch.equal(o_nan, o_zero)
    assert torch.equal(ml_nan, ml_zero)
    # the state is the unnormalised accumulator: o / l is the output, up
    # to one bf16 rounding (2^-8 relative, 2^-7 at the bottom of a binade)
    l = ml_nan[..., 1].permute(0, 2, 1).unsqueeze(-1)
    want = C.prefill_attn(q, k, v, scale, True, 0)
    torch.testing.assert_close((o_nan / l).to(BF).float(), want.float(),
                               rtol=2.0 ** -7, atol=0)


def test_last_writes_no_state():
    C = _C()
    q, k, v = _qkv(1, 100, 228, 4, 2, 64, seed=77)
    scale = 64 ** -0.5
    o_state, ml_state = _state(q)
    C.prefill_attn_carry(q, k[:, :128], v[:, :128], o_state, ml_state, scale,
                         False, 0, True, False)
    o_before, ml_before = o_state.clone(), ml_state.clone()
    out = C.prefill_attn_carry(q, k[:, 128:], v[:, 128:], o_state, ml_state,
                               scale, True, 0, False, True)
    assert torch.equal(o_state, o_before)
    assert torch.equal(ml_state, ml_before)
    assert torch.equal(out, C.prefill_attn(q, k, v, scale, True, 128))


def _ring_steps(k, v, sc, rank):
    """The ring as rank sees it with local chunks: the diagonal chunk first
    (causal), then the earlier chunks in descending order."""
    return [(k[:, c * sc:(c + 1) * sc], v[:, c * sc:(c + 1) * sc],
             c == rank, 0) for c in range(rank, -1, -1)]


@pytest.mark.parametrize("sc,Hq,Hkv,D", [(50, 8, 2, 128), (100, 8, 2, 128),
                                         (50, 4, 4, 64)])
def test_ring_order_ragged_boundaries_against_reference(sc, Hq, Hkv, D):
    from tensorlink_amd.ops import reference as ref
    rank = 3
    q, k, v = _qkv(2, sc, 4 * sc, Hq, Hkv, D, seed=78)
    got = _carry(q, _ring_steps(k, v, sc, rank))
    want = ref.attention_prefill(q.float(), k.float(), v.float(),
                                 causal=True, q_off=rank * sc)
    print(f"ring order sc={sc} D={D}: max abs err "
          f"{(got.float() - want).abs().max().item():.3e}")
    torch.testing.assert_close(got.float(), want, atol=TOL, rtol=TOL)


def test_carried_sequence_is_deterministic_in_place():
    q, k, v = _qkv(2, 100, 400, 14, 2, 128, seed=79)
    steps = _ring_steps(k, v, 100, 3)
    state = _state(q)
    first = _carry(q, steps, state=state)
    first_state = (state[0].clone(), state[1].clone())
    for _ in range(4):
        assert torch.equal(_carry(q, steps, state=state), first)
        assert torch.equal(state[0], first_state[0])
        assert torch.equal(state[1], first_state[1])


def test_binding_checks_state_and_shapes():
    C = _C()
    q, k, v = _qkv(1, 64, 64, 4, 2, 64, seed=80)
    o_state, ml_state = _state(q)
    args = (0.125, True, 0, True, True)
    with pytest.raises(RuntimeError):       # state dtype
        C.prefill_attn_carry(q, k, v, o_state.to(BF), ml_state, *args)
    with pytest.raises(RuntimeError):       # ml_state layout [B,Sq,Hq,2]
        C.prefill_attn_carry(q, k, v, o_state, ml_state.permute(0, 2, 1, 3)
                             .contiguous(), *args)
    with pytest.raises(RuntimeError):       # non-contiguous state
        C.prefill_attn_carry(q, k, v, o_state.transpose(1, 2), ml_state,
                             *args)
    with pytest.raises(RuntimeError):       # causal needs q_off + Sq <= Skv
        C.prefill_attn_carry(q, k[:, :32], v[:, :32], o_state, ml_state,
                             *args)
    q32 = q[..., :32].contiguous()
    with pytest.raises(RuntimeError):       # head dim
        C.prefill_attn_carry(q32, k[..., :32].contiguous(),
                             v[..., :32].contiguous(), *_state(q32), *args)


@pytest.mark.parametrize("sc", [64, 40])
def test_cp_accumulation_runs_the_kernel_per_step(sc):
    """parallel/cp.py's factored ring accumulation for every rank of
    cp = 4, fed local chunks in ring order (no process group)."""
    from tensorlink_amd import ops
    from tensorlink_amd.ops import reference as ref
    from tensorlink_amd.parallel import cp
    assert "TL_NO_CP_KERNEL" not in os.environ
    world, Hq, Hkv, D = 4, 4, 2, 64
    q, k, v = _qkv(2, world * sc, world * sc, Hq, Hkv, D, seed=81)
    scale = D ** -0.5
    want = ref.attention_prefill(q.float(), k.float(), v.float(),
                                 causal=True, scale=scale)
    for rank in range(world):
        qr = q[:, rank * sc:(rank + 1) * sc].contiguous()
        steps = [((rank - r) % world,
                  k[:, ((rank - r) % world) * sc:((rank - r) % world + 1) * sc],
                  v[:, ((rank - r) % world) * sc:((rank - r) % world + 1) * sc])
                 for r in range(world)]
        want_r = want[:, rank * sc:(rank + 1) * sc]

        before = ops.attn_carry_dispatch_count
        got = cp._ring_accumulate(qr, scale, rank, iter(steps))
        assert ops.attn_carry_dispatch_count == before + rank + 1
        assert got.dtype == BF
        torch.testing.assert_close(got.float(), want_r, atol=TOL, rtol=TOL)

        with _env("TL_NO_CP_KERNEL", "1"):
            math_out = cp._ring_accumulate(qr, scale, rank, iter(steps))
        assert ops.attn_carry_dispatch_count == before + rank + 1
        torch.testing.assert_close(math_out.float(), want_r, atol=TOL,
                                   rtol=TOL)


def test_cp_runner_single_rank_on_gpu():
    """CPRunner on one GPU rank: every layer's attention is one carried
    kernel call, and the logits are no further from the fp32 CPU model than
    twice the torch-math route's own error (+1e-3): both are bf16 pipelines
    over the same GEMMs, the kernel adds only the bf16 rounding of P."""
    from tensorlink_amd import ops
    from tensorlink_amd.models.configs import get_config
    from tensorlink_amd.models.dense import build_full_model
    from tensorlink_amd.parallel.cp import CPRunner
    assert "TL_NO_CP_KERNEL" not in os.environ
    r = CPRunner("tiny", 0, 1, device=DEV)
    ids = torch.randint(0, 1024, (2, 96),
                        generator=torch.Generator().manual_seed(82))
    before = ops.attn_carry_dispatch_count
    logits = r.forward_logits(ids)
    assert ops.attn_carry_dispatch_count == before + len(r.stage.layers)
    assert logits.shape == (2, 96, 1024)
    assert torch.isfinite(logits.float()).all()
    with _env("TL_NO_CP_KERNEL", "1"):
        logits_math = r.forward_logits(ids)
    assert ops.attn_carry_dispatch_count == before + len(r.stage.layers)

    # the fp32 CPU model with the runner's (bf16-valued) weights
    m = build_full_model(get_config("tiny"))
    m.to(dtype=torch.float32)
    m.load_state_dict({n: t.detach().float().cpu()
                       for n, t in r.stage.state_dict().items()})
    m.eval()
    pos = torch.arange(96).unsqueeze(0).expand(2, -1).contiguous()
    with torch.no_grad():
        ref_logits = m(ids, pos)
    err_kernel = (logits.float().cpu() - ref_logits).abs().max().item()
    err_math = (logits_math.float().cpu() - ref_logits).abs().max().item()
    print(f"CPRunner tiny [2,96] max abs logit err vs fp32 CPU: "
          f"kernel {err_kernel:.3e}, torch math {err_math:.3e}")
    assert err_kernel <= 2 * err_math + 1e-3
