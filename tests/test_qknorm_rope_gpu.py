"""qknorm_rope_append.hip against the chain it replaces (bit for bit),
against a plain fp64 reference, and through tiny-qwen3."""

import os

import pytest
import torch

from tensorlink_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
EPS = 1e-6
SHAPES = [(4, 2, 64), (5, 1, 128), (32, 8, 128), (40, 8, 64)]
# (B, S, first position per row), (paged, inv_freq dtype)
DECODE, PREFILL = (3, 1, [0, 77, 130]), (2, 5, [126, 126])
LAYOUTS = [(DECODE, False, torch.float32), (DECODE, True, BF),
           (PREFILL, True, torch.float32), (PREFILL, False, BF)]


def _case(Hq, Hkv, D, n_split, bias, B, S, starts, paged, seed=0):
    g = torch.Generator().manual_seed(seed + Hq * D + S)
    rn = lambda *s: torch.randn(*s, generator=g)
    NH, T = Hq + 2 * Hkv, B * S
    scale = (2.0 ** (torch.arange(NH) % 7 - 3)).repeat_interleave(D)
    if n_split:
        data = (rn(n_split, T, NH * D) * scale).to(DEV)
        qkv = ops.Partials(data, rn(NH * D).to(DEV, BF) if bias else None)
    else:
        qkv = (rn(T, NH * D) * scale).to(DEV, BF)
    wq, wk = ((1 + 0.5 * rn(D)).to(DEV, BF) for _ in range(2))
    pos = (torch.tensor(starts)[:, None] + torch.arange(S)).reshape(-1)
    inv = (1.0 / 10000.0 ** (torch.arange(0, D, 2).float() / D)).to(DEV)
    shape = (2 * B, Hkv, 128, D) if paged else (B, Hkv, 256, D)
    table = torch.tensor([[2 * B - 1 - 2 * b, 2 * b] for b in range(B)],
                         device=DEV, dtype=torch.int32) if paged else None
    return (qkv, wq, wk, pos.to(DEV, torch.int32), inv,
            rn(*shape).to(DEV, BF), rn(*shape).to(DEV, BF), table)


def _chain(qkv, wq, wk, pos, inv, k, v, table, S, Hq, Hkv):
    """Today's chain: reduce, ops.rmsnorm per head, cat, ops.rope_append_."""
    D = k.shape[-1]
    x = qkv.materialize() if isinstance(qkv, ops.Partials) else qkv
    q, kk, vv = x.split([Hq * D, Hkv * D, Hkv * D], dim=-1)
    q = ops.rmsnorm(q.reshape(-1, Hq, D).contiguous(), wq, EPS)
    kk = ops.rmsnorm(kk.reshape(-1, Hkv, D).contiguous(), wk, EPS)
    x = torch.cat([q.flatten(1), kk.flatten(1), vv], dim=-1)
    return ops.rope_append_(x, k, v, pos, inv, S, Hq, Hkv, block_table=table)


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
@pytest.mark.parametrize("n_split,bias", [(0, False), (2, False), (3, True)])
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_kernel_equals_chain(Hq, Hkv, D, n_split, bias, layout):
    (B, S, starts), paged, inv_dtype = layout
    qkv, wq, wk, pos, inv, k0, v0, table = _case(Hq, Hkv, D, n_split, bias,
                                                 B, S, starts, paged)
    inv = inv.to(inv_dtype)
    k_ref, v_ref = k0.clone(), v0.clone()   # random sentinels in every slot
    q_ref = _chain(qkv, wq, wk, pos, inv, k_ref, v_ref, table, S, Hq, Hkv)
    q = ops.rope_append_(qkv, k0, v0, pos, inv, S, Hq, Hkv, block_table=table,
                         q_norm=wq, k_norm=wk, eps=EPS)
    assert torch.equal(q, q_ref)
    assert torch.equal(k0, k_ref) and torch.equal(v0, v_ref)


def chain_and_kernel_error(Hq, Hkv, D):
    """max |x - fp64 ref| of chain and kernel; ref rounds as they do."""
    B, S, starts = DECODE
    qkv, wq, wk, pos, inv, k0, v0, _ = _case(Hq, Hkv, D, 0, False, B, S,
                                             starts, False, seed=1)
    x = qkv.double().view(B, -1, D)[:, :Hq + Hkv]
    w = torch.cat([wq.expand(Hq, D), wk.expand(Hkv, D)]).double()
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w
    y = y.to(BF).double()
    ang = pos.double()[:, None, None] * inv.double()
    y1, y2 = y[..., :D // 2], y[..., D // 2:]
    ref = torch.cat([y1 * ang.cos() - y2 * ang.sin(),
                     y2 * ang.cos() + y1 * ang.sin()], -1).to(BF)
    errs = []
    for norms in (None, dict(q_norm=wq, k_norm=wk, eps=EPS)):
        k, v = k0.clone(), v0.clone()
        q = (ops.rope_append_(qkv, k, v, pos, inv, S, Hq, Hkv, **norms)
             if norms else _chain(qkv, wq, wk, pos, inv, k, v, None, S, Hq,
                                  Hkv))
        got = torch.cat([q, k[torch.arange(B), :, pos.long()]], dim=1)
        errs.append(float((got.double() - ref.double()).abs().max()))
    return errs


# chain_err: today's chain on the same seeds (profiles/qknorm_rope_append.md)
@pytest.mark.parametrize("Hq,Hkv,D,chain_err", [(5, 1, 128, 2.0 ** -11),
                                                (4, 2, 64, 0.0)])
def test_kernel_against_fp64_reference(Hq, Hkv, D, chain_err):
    chain, kernel = chain_and_kernel_error(Hq, Hkv, D)
    print(f"chain {chain:.6g} kernel {kernel:.6g} bound {2 * chain_err:.6g}")
    assert kernel <= 2 * chain_err


def test_tiny_qwen3_routes_agree():
    from tensorlink_amd.parallel.planner import plan_for_world
    from tensorlink_amd.parallel.pipeline import PipelineRunner, SamplingParams
    r = PipelineRunner(plan_for_world("tiny-qwen3", 1), 0, 1, device=DEV,
                       dtype=BF)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, p in r.stage.named_parameters():
            if "norm" in name:      # norm weights that matter
                p.copy_(1 + 0.3 * torch.randn(p.shape, generator=g))
    ids = torch.randint(0, 1024, (3, 12), generator=g)
    sp = SamplingParams(max_new_tokens=9)    # prefill + 8 decode steps

    def run():
        n0 = ops.qknorm_rope_dispatch_count
        toks = r.generate(ids, sp)
        with torch.no_grad():               # the step after: its logits
            logits = r.stage(toks[:, -1:], torch.full((3, 1), 12 + 8,
                             device=DEV, dtype=torch.int32),
                             kv_cache=r.kv_cache)
        return toks.cpu(), logits.cpu(), ops.qknorm_rope_dispatch_count - n0

    graph_toks, graph_logits, n = run()
    assert r._decode_graph is not None, "graph was not captured"
    replay_toks, _, _ = run()               # second call replays the capture
    os.environ["TL_NO_GRAPH"] = "1"
    try:
        toks, logits, n_eager = run()
        os.environ["TL_NO_QKNORM_FUSION"] = "1"
        want_toks, want_logits, n_off = run()
    finally:
        os.environ.pop("TL_NO_GRAPH", None)
        os.environ.pop("TL_NO_QKNORM_FUSION", None)
    assert n > 0 and n_eager > 0 and n_off == 0
    for t in (toks, graph_toks, replay_toks):
        assert torch.equal(t, want_toks)
    assert torch.equal(logits, want_logits)
    assert torch.equal(graph_logits, want_logits)
