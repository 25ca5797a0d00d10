"""Decode-chain fusion (split-K partials handed to the next kernel, residual
adds carried into the next norm, in-kernel length offset): every fused path
must give bit-for-bit what the unfused op chain gives on the same inputs.
The unfused ops are the reference throughout; comparisons are torch.equal
on bf16 bits."""

import os
from contextlib import contextmanager

import pytest
import torch

from tensorlink_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _inference_mode():
    # the hand-written GEMM family only serves grad-free calls
    with torch.no_grad():
        yield


@contextmanager
def _unfused():
    os.environ["TL_NO_DECODE_FUSION"] = "1"
    try:
        yield
    finally:
        os.environ.pop("TL_NO_DECODE_FUSION", None)


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV, BF)


# ---------------------------------------------------------------------------
# 1. partials entry point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,bias,n_split", [(128, 512, False, 8),
                                              (256, 128, True, 2)])
def test_linear_partials_sum_equals_linear(N, K, bias, n_split):
    w = _randn(N, K, seed=1, scale=K ** -0.5)
    b = _randn(N, seed=2) if bias else None
    for M in (1, 3, 64, 65, 128, 129, 300):
        x = _randn(M, K, seed=10 + M)
        before = ops.gemm_dispatch_count
        p = ops.linear_partials(x, w, b)
        assert ops.gemm_dispatch_count == before + 1
        assert isinstance(p, ops.Partials), (M, type(p))
        # the policy's split count: a policy change must not hollow this out
        assert p.n_split == n_split
        assert p.data.dtype == torch.float32
        assert p.data.shape == (n_split, M, N)
        acc = torch.zeros(M, N, device=DEV, dtype=torch.float32)
        for s in range(n_split):
            acc = acc + p.data[s]
        if bias:
            assert p.bias is not None
            acc = acc + b.float()
        else:
            assert p.bias is None
        want = ops.linear(x, w, b)
        assert torch.equal(acc.to(BF), want), M
        assert torch.equal(p.materialize(), want), M


def test_linear_partials_unsplit_returns_linear():
    """n_split == 1 (wide N fills the chip): the bf16 output comes back,
    bias applied, exactly as from ops.linear."""
    w = _randn(16384 - 64, 64, seed=3, scale=0.1)
    b = _randn(16384 - 64, seed=4)
    x = _randn(5, 64, seed=5)
    out = ops.linear_partials(x, w, b)
    assert isinstance(out, torch.Tensor) and out.dtype == BF
    assert torch.equal(out, ops.linear(x, w, b))


# ---------------------------------------------------------------------------
# 2. rope_append from partials + bias
# ---------------------------------------------------------------------------
HQ, HKV, D = 2, 1, 64


def _rope_inputs(B, S):
    K = 128
    N = (HQ + 2 * HKV) * D
    x = _randn(B * S, K, seed=20 + S)
    w = _randn(N, K, seed=21, scale=K ** -0.5)
    b = _randn(N, seed=22)
    starts = torch.tensor([5, 0, 17][:B])
    pos = (starts[:, None] + torch.arange(S)[None, :]).reshape(-1)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    return x, w, b, pos.to(DEV, torch.int32), inv.to(DEV)


def _caches(B, paged, seed):
    if paged:
        shape = (2 * B, HKV, 128, D)
        # each row owns two pages, deliberately not in pool order
        table = torch.tensor([[2 * B - 1 - 2 * b, 2 * b] for b in range(B)],
                             device=DEV, dtype=torch.int32)
    else:
        shape = (B, HKV, 40, D)
        table = None
    return _randn(*shape, seed=seed), _randn(*shape, seed=seed + 1), table


@pytest.mark.parametrize("inv_dtype", [torch.float32, BF])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_rope_append_from_partials(S, paged, inv_dtype):
    B = 3
    x, w, b, pos, inv = _rope_inputs(B, S)
    inv = inv.to(inv_dtype)
    k0, v0, table = _caches(B, paged, seed=30)

    # reference: reduce kernel -> bf16 qkv -> rope_append, with the fp32
    # widening of a bf16 spectrum done by torch as the old chain did
    k_ref, v_ref = k0.clone(), v0.clone()
    q_ref = ops.rope_append_(ops.linear(x, w, b), k_ref, v_ref, pos,
                             inv.float(), S, HQ, HKV, block_table=table)

    p = ops.linear_partials(x, w, b)
    assert isinstance(p, ops.Partials) and p.n_split == 2
    k_f, v_f = k0.clone(), v0.clone()
    q_f = ops.rope_append_(p, k_f, v_f, pos, inv, S, HQ, HKV,
                           block_table=table)

    assert torch.equal(q_f, q_ref)
    assert torch.equal(k_f, k_ref) and torch.equal(v_f, v_ref)

    # which slots were written: exactly the B*S addressed ones
    touched = torch.zeros(k0.shape[:3], dtype=torch.bool, device=DEV)
    for t, pp in enumerate(pos.tolist()):
        bb = t // S
        if paged:
            touched[int(table[bb, pp // 128]), :, pp % 128] = True
        else:
            touched[bb, :, pp] = True
    assert int(touched.sum()) == B * S * HKV
    assert torch.equal(k_f[~touched], k0[~touched])
    assert torch.equal(v_f[~touched], v0[~touched])
    assert not torch.equal(k_f[touched], k0[touched])
    assert not torch.equal(v_f[touched], v0[touched])


# ---------------------------------------------------------------------------
# 3. residual add + norm, modes A / B, from partials and from bf16
# ---------------------------------------------------------------------------
_NORM_K = 512      # n_split == 8 at both widths below


def _norm_case(H, rows, grid=False):
    if grid:
        # everything on a 2^-3 grid, exact through the GEMM; the sums
        # x + res reach [32, 64) where bf16 steps by 2^-2, so odd eighths
        # are exact rounding ties
        g = torch.Generator().manual_seed(40)
        x = torch.randint(0, 2, (rows, _NORM_K), generator=g).to(DEV, BF)
        w = (torch.randint(-2, 3, (H, _NORM_K), generator=g) / 8).to(DEV, BF)
        res = (torch.randint(0, 512, (rows, H), generator=g) / 8).to(DEV, BF)
    else:
        x = _randn(rows, _NORM_K, seed=41 + rows)
        w = _randn(H, _NORM_K, seed=42, scale=_NORM_K ** -0.5)
        res = _randn(rows, H, seed=43 + rows)
    nw = (_randn(H, seed=44) * 0.1 + 1.0).to(BF)
    return x, w, res, nw


def _check_norm_modes(x, w, res, nw):
    eps = 1e-6
    lin = ops.linear(x, w)
    y_a, r_a = ops.rmsnorm_residual(lin, res, nw, eps)        # mode A ref
    r_b = lin + res                                           # mode B ref
    y_b = ops.rmsnorm(r_b, nw, eps)
    assert torch.equal(r_a, r_b)

    p = ops.linear_partials(x, w)
    assert isinstance(p, ops.Partials) and p.n_split == 8
    for src in (p, lin):
        ya, ra = ops.add_rmsnorm(src, res, nw, eps)
        assert torch.equal(ya, y_a) and torch.equal(ra, r_a)
        yb, rb = ops.add_rmsnorm(src, res, nw, eps, rounded=True)
        assert torch.equal(yb, y_b) and torch.equal(rb, r_b)
        assert torch.equal(ops.add_residual(src, res), r_b)
    return y_a, y_b


@pytest.mark.parametrize("H", [128, 3584])
def test_add_rmsnorm_modes(H):
    for rows in (1, 65, 300):
        _check_norm_modes(*_norm_case(H, rows))


def test_add_rmsnorm_modes_on_rounding_ties():
    x, w, res, nw = _norm_case(128, 65, grid=True)
    f = ops.linear(x, w).float() + res.float()
    ties = (f * 8).round() == f * 8
    ties &= (f >= 32) & ((f * 8).long() % 2 == 1)
    assert int(ties.sum()) > 100, "input does not exercise ties"
    y_a, y_b = _check_norm_modes(x, w, res, nw)
    # the two modes really differ here: a swap cannot pass
    assert not torch.equal(y_a, y_b)


# ---------------------------------------------------------------------------
# 4. decode attention length offset
# ---------------------------------------------------------------------------
def test_attention_decode_len_add():
    lens = torch.tensor([0, 1, 37, 1024, 1100], device=DEV,
                        dtype=torch.int32)
    B, Smax = lens.numel(), 1152
    q = _randn(B, 1, 4, D, seed=50)
    k = _randn(B, 2, Smax, D, seed=51)
    v = _randn(B, 2, Smax, D, seed=52)
    want = ops.attention_decode(q, k, v, lens + 1)
    got = ops.attention_decode(q, k, v, lens, len_add=1)
    assert torch.equal(got, want)
    # the offset matters (row 3 crosses the 1024 split threshold with it)
    assert not torch.equal(got[1:],
                           ops.attention_decode(q[1:], k[1:], v[1:],
                                                lens[1:]))


# ---------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------
def _tiny_cfg():
    from tensorlink_amd.models.configs import ModelConfig
    return ModelConfig(name="fusion-tiny", vocab_size=256, hidden_size=128,
                       intermediate_size=512, num_hidden_layers=2,
                       num_attention_heads=2, num_key_value_heads=1,
                       max_position_embeddings=64, qkv_bias=True)


def _tiny_model():
    from tensorlink_amd.models.dense import StageModel
    from tensorlink_amd.models.loader import init_random_stage
    m = StageModel(_tiny_cfg(), 0, 2, True, True)
    init_random_stage(m, device=DEV, dtype=BF, seed=3)
    # biases and norm weights that matter
    with torch.no_grad():
        for i, (name, p) in enumerate(m.named_parameters()):
            if name.endswith(".bias"):
                p.copy_(_randn(*p.shape, seed=60 + i, scale=0.5))
            elif "norm" in name:
                p.copy_((_randn(*p.shape, seed=60 + i) * 0.1 + 1).to(BF))
    return m.eval()


def _split(full):
    """The same weights as two stages (layer 0 + embedding | layer 1 +
    head)."""
    from tensorlink_amd.models.dense import StageModel
    cfg = full.config
    s0 = StageModel(cfg, 0, 1, True, False).to(DEV, BF).eval()
    s1 = StageModel(cfg, 1, 2, False, True).to(DEV, BF).eval()
    sd = full.state_dict()
    s0.load_state_dict({k: v for k, v in sd.items()
                        if k.startswith(("embed_tokens.", "layers.0."))})
    s1.load_state_dict({k.replace("layers.1.", "layers.0."): v
                        for k, v in sd.items()
                        if k.startswith(("layers.1.", "norm", "lm_head."))})
    return s0, s1


def _run(stages, ids, steps=4):
    """Prefill + greedy decode steps through a chain of stages; returns
    every step's logits."""
    B, S = ids.shape
    caches = [s.make_kv_cache(B, S + steps + 1, DEV) for s in stages]
    pos = torch.arange(S, device=DEV, dtype=torch.int32).expand(B, S)
    outs = []
    x, p = ids, pos.contiguous()
    for t in range(steps + 1):
        h = x
        for s, c in zip(stages, caches):
            h = s(h, p, kv_cache=c)
        logits = h[:, -1]
        outs.append(logits)
        x = logits.argmax(-1, keepdim=True)
        p = torch.full((B, 1), S + t, device=DEV, dtype=torch.int32)
    return torch.stack(outs)


def test_stage_model_fused_equals_unfused():
    from tensorlink_amd.models.dense import _project
    m = _tiny_model()
    # the fused route is really taken at these shapes
    probe = _randn(3, 1, 512, seed=70)
    assert isinstance(_project(m.layers[0].mlp.down_proj, probe),
                      ops.Partials)
    ids = torch.randint(0, 256, (3, 5), generator=torch.Generator()
                        .manual_seed(71)).to(DEV)
    fused = _run([m], ids)
    with _unfused():
        plain = _run([m], ids)
    assert torch.equal(fused, plain)

    # two stages: the stream handed over is the fully added one
    s0, s1 = _split(m)
    fused2 = _run([s0, s1], ids)
    assert torch.equal(fused2, plain)
    with _unfused():
        plain2 = _run([s0, s1], ids)
    assert torch.equal(plain2, plain)


def test_generate_graph_fused_equals_eager_unfused():
    from tensorlink_amd.parallel.planner import plan_for_world
    from tensorlink_amd.parallel.pipeline import PipelineRunner, SamplingParams
    plan = plan_for_world("tiny", 1)
    ids = torch.randint(0, 1024, (4, 16),
                        generator=torch.Generator().manual_seed(9))
    sp = SamplingParams(max_new_tokens=8)
    r = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    out_graph = r.generate(ids, sp).cpu()
    assert r._decode_graph is not None, "graph was not captured"
    r2 = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
    os.environ["TL_NO_GRAPH"] = "1"
    try:
        out_eager = r2.generate(ids, sp).cpu()
        with _unfused():
            out_plain = r2.generate(ids, sp).cpu()
    finally:
        os.environ.pop("TL_NO_GRAPH", None)
    assert torch.equal(out_graph, out_eager)
    assert torch.equal(out_graph, out_plain)
