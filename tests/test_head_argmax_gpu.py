"""Fused greedy head (ops/csrc/head_argmax.hip): lm_head GEMM with the
argmax taken on the accumulators, no logits written.

The oracle is ``torch.argmax`` of the logits the family kernel writes
(``_C.skinny_gemm``, itself held against float64 by the conformance suite):
in the wide class the policy never splits K, every logit is one K chain, so
the fused kernel compares the very bf16 values the family stores and every
check is ``torch.equal`` on integers.

Shapes are the smallest that reach each path: N = 65536 has only full
256-column panels, 65664 a half-empty last panel (clamped W rows whose
duplicates must not win), 65600 a quarter-full one; K = 64 is one chunk,
96 a chunk plus the 32-wide tail, 192 prologue, steady state and drain of
the double buffer; M walks the streaming range, the 64/65 kernel boundary
of the fallback, the 256-row block boundary with its clamped ghost rows,
and two full row blocks."""

import os
from contextlib import contextmanager

import pytest
import torch

import kernel_oracle as ko
from tensorlink_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
MS = (1, 16, 64, 65, 255, 256, 257, 512)


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _C():
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops._require_ext()


@contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _family_tokens(x, w):
    return _C().skinny_gemm(x, w, None).argmax(-1)


# ---------------------------------------------------------------------------
# equals the family on random data (bf16 ties at the maximum included)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [192, 64, 96])
@pytest.mark.parametrize("N", [65536, 65664, 65600])
def test_head_argmax_equals_family(N, K):
    C = _C()
    assert C.gemm_n_split(N, K) == 1
    c = ko.gemm_case(max(MS), N, K, False, seed=11)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    tied_rows = 0
    for M in MS:
        xm = x[:M].contiguous()
        logits = C.skinny_gemm(xm, w, None)
        want = logits.argmax(-1)
        got = C.lm_head_argmax(xm, w)
        assert got.shape == (M,) and got.dtype == torch.int64
        assert int(got.max()) < N and int(got.min()) >= 0
        assert torch.equal(got, want), (M, (got != want).nonzero().tolist())
        top = logits.max(-1, keepdim=True).values
        tied_rows += int(((logits == top).sum(-1) > 1).sum())
    print(f"N{N} K{K}: rows with a tie at the maximum: {tied_rows}")


def test_head_argmax_keeps_leading_dims_and_rows_do_not_depend_on_m():
    C = _C()
    c = ko.gemm_case(257, 65664, 96, False, seed=12)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    big = C.lm_head_argmax(x, w)
    small = C.lm_head_argmax(x[:65].contiguous(), w)
    assert torch.equal(big[:65], small)
    x3 = x[:66].reshape(6, 11, 96).contiguous()
    tok3 = C.lm_head_argmax(x3, w)
    assert tok3.shape == (6, 11)
    assert torch.equal(tok3.reshape(-1), big[:66])


# ---------------------------------------------------------------------------
# constructed ties: every product and sum is an exact small integer, the
# same maximal W row sits at several columns, the lowest must win. Dropping
# the lowest copy in turn walks the reduction: the next lane of the column
# group, the lane's next nt register, the next wn wave (LDS), the next panel
# (combine kernel), and the last column of the half-empty last panel.
# ---------------------------------------------------------------------------
def test_head_argmax_constructed_ties():
    C = _C()
    M, N, K = 65, 65664, 96
    gen = torch.Generator().manual_seed(13)
    x = torch.randint(1, 4, (M, K), generator=gen).to(BF)
    w = torch.randint(-1, 2, (N, K), generator=gen).to(BF)
    c = 3 * 256 + 5
    copies = [c, c + 1, c + 16, c + 64, c + 256, N - 1]
    w[copies] = 2.0            # logit 2 * sum(x) > sum(x) >= any other
    x, w = x.to(DEV), w.to(DEV)
    for i, want in enumerate(copies):
        got = C.lm_head_argmax(x, w)
        assert torch.equal(got, _family_tokens(x, w)), i
        assert got.tolist() == [want] * M, (i, want)
        w[want] = 0.0
    # nothing stands out any more; still the family's answer
    assert torch.equal(C.lm_head_argmax(x, w), _family_tokens(x, w))
    # all logits equal (0): the first column, not a clamped duplicate
    z = torch.zeros_like(x)
    assert C.lm_head_argmax(z, w).tolist() == [0] * M
    # all logits equal and negative
    w.fill_(-1.0)
    assert C.lm_head_argmax(x, w).tolist() == [0] * M
    assert _family_tokens(x, w).tolist() == [0] * M


# ---------------------------------------------------------------------------
# NaN beats everything, the first NaN wins, either sign
# ---------------------------------------------------------------------------
def test_head_argmax_nan_wins_first_nan_first():
    C = _C()
    M, N, K = 65, 65536, 64
    c = ko.gemm_case(M, N, K, False, seed=14)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    j2, j1 = 40000, 777
    w[j2, 3] = float("nan")
    got = C.lm_head_argmax(x, w)
    assert got.tolist() == [j2] * M
    assert torch.equal(got, _family_tokens(x, w))
    # a second NaN column below it, with the sign bit set
    w[j1, 40] = -float("nan")
    assert bool(torch.isnan(w[j1, 40]))
    got = C.lm_head_argmax(x, w)
    assert got.tolist() == [j1] * M
    assert torch.equal(got, _family_tokens(x, w))
    # +inf loses to NaN
    w[5] = float("inf")
    x_pos = x.abs().contiguous()
    assert torch.equal(C.lm_head_argmax(x_pos, w), _family_tokens(x_pos, w))
    assert C.lm_head_argmax(x_pos, w).tolist() == [j1] * M


# ---------------------------------------------------------------------------
# op routing
# ---------------------------------------------------------------------------
def test_linear_argmax_routing():
    C = _C()
    N, K = 65536, 64
    assert "wide" not in ops._LIB_CLASSES, "default must be the family"
    assert ops._gemm_class(N, K) == "wide"
    m_in = max(ops.HEAD_ARGMAX_M_MIN, 65)
    c = ko.gemm_case(ops.GEMM_M_MAX + 1, N, K, False, seed=15)
    x, w = c["x"].to(DEV), c["w"].to(DEV)
    xin = x[:m_in].contiguous()
    assert ops._use_head_argmax(ops.HEAD_ARGMAX_M_MIN, N, K)
    assert ops._use_head_argmax(ops.GEMM_M_MAX, N, K)

    before = ops.head_argmax_dispatch_count
    got = ops.linear_argmax(xin, w)
    assert ops.head_argmax_dispatch_count == before + 1
    assert torch.equal(got, _family_tokens(xin, w))
    xlo = x[:ops.HEAD_ARGMAX_M_MIN].contiguous()
    assert torch.equal(ops.linear_argmax(xlo, w), _family_tokens(xlo, w))
    before += 1
    top = ops.linear_argmax(x[:ops.GEMM_M_MAX].contiguous(), w)
    assert ops.head_argmax_dispatch_count == before + 2
    assert torch.equal(top, _family_tokens(x[:ops.GEMM_M_MAX].contiguous(), w))
    # leading dimensions are kept
    x3 = x[:6 * 11].reshape(6, 11, K).contiguous()
    tok3 = ops.linear_argmax(x3, w)
    assert ops.head_argmax_dispatch_count == before + 3
    assert tok3.shape == (6, 11)
    assert torch.equal(tok3, ops.linear(x3, w).argmax(-1))

    # outside the domain: the two-step form, and the count does not move
    before = ops.head_argmax_dispatch_count
    outside = [(xin, w[:32768].contiguous()),          # not the wide class
               (x, w)]                                 # M = GEMM_M_MAX + 1
    if ops.HEAD_ARGMAX_M_MIN > 1:                      # unrouted small M
        m_lo = ops.HEAD_ARGMAX_M_MIN - 1
        outside.append((x[:m_lo].contiguous(), w))
        outside.append((x[:1].contiguous(), w))
    for xo, wo in outside:
        assert not ops._use_head_argmax(xo.shape[0], wo.shape[0], K)
        assert torch.equal(ops.linear_argmax(xo, wo),
                           ops.linear(xo, wo).argmax(-1))
    with _env(TL_NO_HEAD_FUSION="1"):
        assert not ops._use_head_argmax(m_in, N, K)
        assert torch.equal(ops.linear_argmax(xin, w), got)
    with torch.enable_grad():                          # library GEMM's bits
        assert torch.equal(ops.linear_argmax(xin, w),
                           ops.linear(xin, w).argmax(-1))
    assert torch.equal(ops.linear_argmax(xin.float(), w.float()),
                       ops.linear(xin.float(), w.float()).argmax(-1))
    assert ops.head_argmax_dispatch_count == before
    # the binding refuses what the op keeps away from it
    with pytest.raises(RuntimeError):
        C.lm_head_argmax(xin, w[:32768].contiguous())
    with pytest.raises(RuntimeError):
        C.lm_head_argmax(x, w)


# ---------------------------------------------------------------------------
# capture: no host sync, no allocation the graph cannot replay
# ---------------------------------------------------------------------------
def test_linear_argmax_captures_and_replays():
    N, K, M = 65664, 96, 66
    c = ko.gemm_case(2 * M, N, K, False, seed=16)
    xs, w = c["x"].to(DEV), c["w"].to(DEV)
    x = xs[:M].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.linear_argmax(x, w)
    torch.cuda.current_stream().wait_stream(s)
    before = ops.head_argmax_dispatch_count
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tok = ops.linear_argmax(x, w)
    assert ops.head_argmax_dispatch_count == before + 1
    graph.replay()
    assert torch.equal(tok, _family_tokens(x, w))
    x.copy_(xs[M:])
    graph.replay()
    fresh = ops.linear_argmax(xs[M:].contiguous(), w)
    assert torch.equal(tok, fresh)
    assert torch.equal(tok, _family_tokens(xs[M:].contiguous(), w))
    assert not torch.equal(fresh, _family_tokens(xs[:M].contiguous(), w))


# ---------------------------------------------------------------------------
# model level: vocab 65536 puts lm_head in the wide class
# ---------------------------------------------------------------------------
def test_generate_fused_head_equals_logits_argmax():
    from tensorlink_amd.models.configs import ModelConfig
    from tensorlink_amd.models.dense import TLLinear
    from tensorlink_amd.parallel.planner import plan_for_world
    from tensorlink_amd.parallel.pipeline import PipelineRunner, SamplingParams
    cfg = ModelConfig(name="head-tiny", vocab_size=65536, hidden_size=128,
                      intermediate_size=256, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=1,
                      max_position_embeddings=64)
    B, S, T = 66, 6, 8            # head M = 66 in prefill and in decode
    plan = plan_for_world(cfg, 1, batch_size=B, seq_len=S + T)
    ids = torch.randint(0, cfg.vocab_size, (B, S),
                        generator=torch.Generator().manual_seed(17))
    sp = SamplingParams(temperature=0.0, max_new_tokens=T)

    def count(fn):
        before = ops.head_argmax_dispatch_count
        out = fn().cpu()
        return out, ops.head_argmax_dispatch_count - before

    r = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    assert type(r.stage.lm_head) is TLLinear
    out_graph, n_graph = count(lambda: r.generate(ids, sp))
    assert r._decode_graph is not None, "graph was not captured"
    # prefill + warm-up step + captured step
    assert n_graph == 3
    r2 = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    with _env(TL_NO_HEAD_FUSION="1"):
        out_graph_unfused, n = count(lambda: r2.generate(ids, sp))
        assert r2._decode_graph is not None and n == 0
    r3 = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    with _env(TL_NO_GRAPH="1"):
        out_eager, n_eager = count(lambda: r3.generate(ids, sp))
        assert n_eager == T           # prefill + T - 1 decode steps
        with _env(TL_NO_HEAD_FUSION="1"):
            out_eager_unfused, n = count(lambda: r3.generate(ids, sp))
            assert n == 0
    assert out_graph.shape == (B, T)
    assert torch.equal(out_graph, out_graph_unfused)
    assert torch.equal(out_graph, out_eager)
    assert torch.equal(out_graph, out_eager_unfused)
    # a sampled call does not go near the fused head
    _, n = count(lambda: r3.generate(
        ids, SamplingParams(temperature=0.8, max_new_tokens=T, seed=1)))
    assert n == 0
