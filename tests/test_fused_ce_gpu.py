"""GPU tier of the fused cross-entropy suite (MI355X): head_ce.hip through
its bindings and through ops.linear_cross_entropy, on the inputs, metric
and tolerance of tests/fused_ce_oracle.py, which tests/test_fused_ce_cpu.py
shows to reject the wrong variants. ``CONF`` lines are visible with -s;
docs/TESTING.md records them."""

import pytest
import torch

import fused_ce_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16
SENTINEL = -1.5          # bf16 0xBFC0: no gradient of these cases has it


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


def _C():
    from tensorlink_amd import _C as C
    return C


def dev(c):
    return c["x"].to(DEV), c["w"].to(DEV), c["labels"].to(DEV)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def scale_of(labels, V, dloss=1.0):
    valid = (labels >= 0) & (labels < V)
    return torch.where(valid, dloss / valid.sum().clamp(min=1).float(), 0.0)


def check(name, out, V, K, M, worst):
    r = fo.ratio(name, out, V, K, M)
    _, e0 = fo.references(V, K, M)
    print(f"CONF head_ce {name} V{V} K{K} M{M}: E0={e0[name]:.3e} "
          f"nme/tol={r:.3f}")
    worst[name] = max(worst.get(name, 0.0), r)
    return r


# --------------------------------------------------------------------------
# exact check: layout, ghosts, clamping, K tail, label addressing
# --------------------------------------------------------------------------
@pytest.mark.parametrize("V", fo.VS)
@pytest.mark.parametrize("K", fo.KS)
def test_exact_one_hot(V, K):
    for M in fo.MS:
        c, lse, loss_row = fo.exact_case(V, K, M)
        got_lse, got_loss = _C().head_ce_stats(*dev(c))
        assert fo.exact_ok({"lse": got_lse, "loss_row": got_loss}, lse,
                           loss_row), (V, K, M)


# --------------------------------------------------------------------------
# the oracle rule
# --------------------------------------------------------------------------
@pytest.mark.parametrize("V", fo.VS)
@pytest.mark.parametrize("K", fo.KS)
def test_stats_and_gradient_against_oracle(V, K):
    worst, failed = {}, []
    for M in fo.MS:
        fo.check_mass(V, K, M)
        x, w, labels = dev(fo.ce_case(V, K, M))
        lse, loss_row = _C().head_ce_stats(x, w, labels)
        # g lands as a view inside a sentinel-filled buffer
        pad = 3 * V + 5
        buf = torch.full((pad + M * V + pad,), SENTINEL, dtype=BF16,
                         device=DEV)
        g = buf[pad:pad + M * V].view(M, V)
        out = _C().head_ce_grad(x, w, labels, lse, scale_of(labels, V),
                                out=g)
        assert out.data_ptr() == g.data_ptr()
        for name, t in (("lse", lse), ("loss_row", loss_row), ("g", g)):
            if check(name, t, V, K, M, worst) > 1.0:
                failed.append((name, M))
        edge = torch.cat([buf[:pad], buf[pad + M * V:]])
        assert (bits(edge) == bits(torch.tensor(SENTINEL, dtype=BF16))).all()
        ignored = ~((labels >= 0) & (labels < V))
        assert ignored.any()
        assert not bits(g[ignored]).any(), "ignored rows must be zero bits"
        assert not bits(loss_row[ignored]).any()
    print(f"CONF head_ce V{V} K{K} worst nme/tol: "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert not failed, failed


@pytest.mark.parametrize("V", fo.VS)
@pytest.mark.parametrize("K", fo.KS)
def test_backward_against_oracle(V, K):
    """dh and dW through ops.linear_cross_entropy(...).backward() at M =
    300: three chunks of 128 with a partial last one (dW summed in fp32
    over the chunks), then one chunk (dW straight from the GEMM)."""
    M = 300
    r64, _ = fo.references(V, K, M)
    worst, failed = {}, []
    for chunk in (128, 4096):
        x, w, labels = dev(fo.ce_case(V, K, M))
        x.requires_grad_()
        w.requires_grad_()
        loss = _ops().linear_cross_entropy(x, w, labels, chunk=chunk)
        loss.backward()
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert x.grad.dtype == BF16 and w.grad.dtype == BF16
        # the scalar: the mean of loss_row, whose rule is checked above;
        # its rows carry up to an fp32 ulp of |lse| ~ 100 (7.6e-6) each
        # and the mean is of order 5
        ref = float(r64["loss"])
        got = float(loss.detach())
        assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
        print(f"CONF head_ce backward chunk={chunk}:")
        for name, t in (("dh", x.grad), ("dW", w.grad)):
            if check(name, t, V, K, M, worst) > 1.0:
                failed.append((name, chunk))
    assert not failed, failed


# --------------------------------------------------------------------------
# bitwise
# --------------------------------------------------------------------------
@pytest.mark.parametrize("V,K", [(16, 32), (272, 160), (777, 96),
                                 (777, 256)])
def test_rows_do_not_depend_on_the_call(V, K):
    x, w, labels = dev(fo.ce_case(V, K, 300))
    C = _C()
    scale = scale_of(labels, V)
    lse, loss_row = C.head_ce_stats(x, w, labels)
    g = C.head_ce_grad(x, w, labels, lse, scale)

    def run(sl, **kw):
        l2, r2 = C.head_ce_stats(x[sl], w, labels[sl], **kw)
        g2 = C.head_ce_grad(x[sl], w, labels[sl], lse[sl], scale[sl], **kw)
        return l2, r2, g2

    # M = 1 (row 7), one full row block, one block plus a row
    for sl in (slice(7, 8), slice(0, 256), slice(0, 257)):
        for a, b in zip(run(sl), (lse[sl], loss_row[sl], g[sl])):
            assert same_bits(a, b), (V, K, sl)
    # a repeated call repeats; the launch split and the grid order change
    # no bit
    for kw in ({}, {"rows_per_launch": 256}, {"rows_fast": 0}):
        for a, b in zip(run(slice(0, 300), **kw), (lse, loss_row, g)):
            assert same_bits(a, b), (V, K, kw)


def test_linear_cross_entropy_repeats():
    ops = _ops()
    outs = []
    for _ in range(2):
        x, w, labels = dev(fo.ce_case(777, 160, 300))
        x.requires_grad_()
        w.requires_grad_()
        loss = ops.linear_cross_entropy(x, w, labels, chunk=128)
        loss.backward()
        outs.append((loss.detach(), x.grad, w.grad))
    for a, b in zip(*outs):
        assert same_bits(a, b)


def test_ignore_index_and_no_valid_row():
    ops = _ops()
    x, w, labels = dev(fo.ce_case(272, 96, 257))
    base = ops.linear_cross_entropy(x, w, labels)
    # another ignore_index: the same rows, marked differently
    other = torch.where(labels == -100, 5, labels)
    keep = labels != 5
    l5 = ops.linear_cross_entropy(x[keep], w, other[keep], ignore_index=5)
    l0 = ops.linear_cross_entropy(x[keep], w, labels[keep])
    assert same_bits(l5, l0) and torch.isfinite(base)
    # no valid row at all: loss 0, gradients 0
    x.requires_grad_()
    none = ops.linear_cross_entropy(x, w, torch.full_like(labels, -100))
    none.backward()
    assert float(none.detach()) == 0.0 and not bits(x.grad).any()


# --------------------------------------------------------------------------
# no host sync: the forward is graph-capturable
# --------------------------------------------------------------------------
def test_forward_under_graph_capture():
    ops = _ops()
    x, w, labels = dev(fo.ce_case(777, 160, 300))
    eager = ops.linear_cross_entropy(x, w, labels)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        ops.linear_cross_entropy(x, w, labels)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        captured = ops.linear_cross_entropy(x, w, labels)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, eager)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, eager)


# --------------------------------------------------------------------------
# routing
# --------------------------------------------------------------------------
def test_trainer_takes_the_fused_route(monkeypatch):
    from tensorlink_amd.parallel.pipeline import PipelineTrainer
    from tensorlink_amd.parallel.planner import plan_for_world
    ops = _ops()
    monkeypatch.delenv("TL_NO_FUSED_CE", raising=False)
    plan = plan_for_world("tiny-bigvocab", 1)
    t = PipelineTrainer(plan, 0, 1, device=DEV, seed=1, lr=1e-3)
    assert t._chunked_ce
    torch.manual_seed(3)
    ids = torch.randint(0, 38400, (2, 64))
    before = ops.fused_ce_dispatch_count
    losses = [t.train_step(ids, labels=ids) for _ in range(3)]
    assert ops.fused_ce_dispatch_count >= before + 3
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0]

    monkeypatch.setenv("TL_NO_FUSED_CE", "1")
    before = ops.fused_ce_dispatch_count
    loss = t.train_step(ids, labels=ids)
    assert ops.fused_ce_dispatch_count == before
    assert loss == loss


def test_dispatcher_equals_the_torch_route():
    """The two routes of ops.chunked_causal_lm_loss compute the same mean
    over the valid shifted positions. Both take exact products of the bf16
    operands into fp32, so each row's lse and label logit obey the lse rule
    on either route, 16 x 1e-7 of |lse|; the means may differ by twice
    that."""
    ops = _ops()
    from tensorlink_amd.ops import reference as ref
    torch.manual_seed(11)
    B, S, H, V = 3, 40, 64, 777
    h = (torch.randn(B, S, H) * 0.5).to(BF16).to(DEV)
    w = (torch.randn(V, H) * 0.2).to(BF16).to(DEV)
    labels = torch.randint(0, V, (B, S), device=DEV)
    labels[1, 7] = -100
    before = ops.fused_ce_dispatch_count
    fused = ops.chunked_causal_lm_loss(h, w, labels)
    assert ops.fused_ce_dispatch_count == before + 1
    torch_route = ref.chunked_causal_lm_loss(h, w, labels)
    assert abs(float(fused) - float(torch_route)) \
        <= 2 * 16e-7 * float(torch_route)
