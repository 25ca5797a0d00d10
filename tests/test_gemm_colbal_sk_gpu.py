"""Column-balanced split-K GEMM (ops/csrc/gemm_colbal_sk.hip) on MI355X.

The kernel writes the fp32 split-K partials [n_split, M, N] with the family's
K chain, so every comparison here is on bits (gemm_family_oracle.bits_equal /
torch.equal): against the parent kernel (``_C.skinny_gemm_partials`` under
TL_NO_COLBAL_SK=1, which is gemm_tiled_kernel), against columns of W for
one-hot rows, against itself at other M, other workgroup counts and on a
poisoned buffer. The one check with a bound is the conformance rule of
tests/test_gemm_family_gpu.py::test_split_k_meets_the_oracle_rule, with that
test's cases and that test's bound.

Shapes are those of gemm_family_oracle.SHAPES that hit every slice edge — a
tail-only last split (64, 160), an empty last split (64, 288), three empty
splits (128, 544), no tail (128, 512), the tail closing a full split
(1024, 1056), a four-way split with a tail (4096, 1376) — plus (448, 1024),
whose 28 tiles over 4 workgroups are the 7-tile one-pass range, and
(4608, 1376), whose 288 tiles over the default 64 workgroups are dealt 5 / 4
as qkv's are. Workgroups per split: 1 forces multi-pass sub-ranges, 3 uneven
ranges and, at N = 64, workgroups with no tiles; 0 is the default rule.
"""

import functools
import os
from contextlib import contextmanager

import pytest
import torch

import gemm_family_oracle as fo
import kernel_oracle as ko
from test_ops_conformance_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
# (N, K) -> n_split; the first six are rows of fo.SHAPES
EXTRA = {(448, 1024): 8, (4608, 1376): 4}
SHAPES = [(64, 160), (64, 288), (128, 544), (128, 512), (1024, 1056),
          (4096, 1376)] + sorted(EXTRA)
MS = (65, 128, 129, 255, 256, 257, 512)
M_MAX = max(MS)


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


def _C():
    return _ops()._require_ext()


def _n_split(N, K):
    want = EXTRA.get((N, K)) or fo.SHAPES[(N, K)]
    assert _C().gemm_n_split(N, K) == want == fo.n_split_for(N, K), \
        "the policy no longer splits this shape as the table says"
    return want


def _blocks(N, K):
    nbs = [1, 3, 0]
    if (N, K) == (448, 1024):
        nbs.append(4)             # 28 tiles / 4 = the 7-tile range, one pass
    return nbs


@contextmanager
def _parent():
    """The parent's kernels: gemm_tiled_kernel for every split shape."""
    old = os.environ.get("TL_NO_COLBAL_SK")
    os.environ["TL_NO_COLBAL_SK"] = "1"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("TL_NO_COLBAL_SK", None)
        else:
            os.environ["TL_NO_COLBAL_SK"] = old


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """kernel_oracle.gemm_case at the largest M, on the device; smaller M
    are row prefixes. Never modified."""
    c = ko.gemm_case(M_MAX, N, K, True)
    return {k: v.to(DEV) for k, v in c.items()}


def _parent_partials(x, w):
    C = _C()
    with _parent():
        assert not C.colbal_sk_routed(x.shape[0], w.shape[0], w.shape[1])
        return C.skinny_gemm_partials(x, w, None)


def _host_reduce(p, b):
    acc = torch.zeros_like(p[0])
    for s in range(p.shape[0]):
        acc = acc + p[s]
    if b is not None:
        acc = acc + b.float()
    return acc.to(BF)


# --------------------------------------------------------------------------
# partials against the parent kernel
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_partials_equal_the_parent_kernel(N, K):
    C = _C()
    n_split = _n_split(N, K)
    c = _case(N, K)
    slices = fo.k_slices(K, n_split)
    for M in MS:
        x = c["x"][:M].contiguous()
        want = _parent_partials(x, c["w"])
        assert want.shape == (n_split, M, N) and want.dtype == torch.float32
        for nb in _blocks(N, K):
            got = C.gemm_colbal_sk(x, c["w"], nb)
            assert fo.bits_equal(got, want), (M, nb)
            for s, (b, e) in enumerate(slices):
                if e <= b:
                    assert fo.bits_equal(got[s], torch.zeros_like(got[s])), \
                        f"M={M} nb={nb}: empty split {s} is not +0.0"


# --------------------------------------------------------------------------
# partials against the oracle
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_onehot_rows_return_columns_of_w(N, K):
    C = _C()
    n_split = _n_split(N, K)
    w = _case(N, K)["w"]
    slices = fo.k_slices(K, n_split)
    ks = fo.onehot_ks(K, slices)
    for M in MS:
        x = fo.onehot_rows(M, K, ks).to(DEV)
        want = torch.zeros(n_split, M, N, dtype=torch.float32, device=DEV)
        holder = torch.tensor([fo.split_of(ks[i % len(ks)], slices)
                               for i in range(M)], device=DEV)
        want[holder, torch.arange(M, device=DEV)] = \
            fo.onehot_expected(w, None, M, ks).float()
        for nb in _blocks(N, K):
            got = C.gemm_colbal_sk(x, w, nb)
            assert fo.bits_equal(got, want), \
                f"M={M} nb={nb}: a split's partial is not its slice of w"


@functools.lru_cache(maxsize=None)
def _reference(N, K, bias):
    """(ref64, emu) [M_MAX, N] as tests/test_gemm_family_gpu.py computes
    them: once per case, never modified."""
    c = _case(N, K)
    b = c["b"] if bias else None
    ref = ko.linear(c["x"], c["w"], b)
    emu = ko.bf16_round(ko.linear(c["x"], c["w"], b, dtype=torch.float32))
    return ref, emu


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
def test_reduced_partials_meet_the_oracle_rule(N, K, bias):
    """The cases and the rule of test_split_k_meets_the_oracle_rule —
    nme(out, ref64) <= MARGIN * E0, E0 from the bf16-rounded fp32 linear —
    on the new kernel's partials reduced in the contract's order. The
    contract model family_emulated is held to the same bound, so the two
    stand as close to float64 as the family test asks of the parent."""
    C = _C()
    n_split = _n_split(N, K)
    c = _case(N, K)
    b = c["b"] if bias else None
    ref, emu = _reference(N, K, bias)
    model = fo.family_emulated(c["x"], c["w"], b, fo.k_slices(K, n_split))
    for M in MS:
        x = c["x"][:M].contiguous()
        out = _host_reduce(C.gemm_colbal_sk(x, c["w"], 0), b)
        e0 = ko.nme(emu[:M], ref[:M])
        check(f"colbal_sk N{N} K{K} M{M} bias{int(bias)}", out, ref[:M], e0)
        check(f"family_emulated N{N} K{K} M{M} bias{int(bias)}", model[:M],
              ref[:M], e0)


# --------------------------------------------------------------------------
# routing and bias: the reduce applies the bias once
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_routed_gemm_equals_the_switch_with_and_without_bias(N, K):
    C = _C()
    _n_split(N, K)
    c = _case(N, K)
    for M in MS:
        x = c["x"][:M].contiguous()
        routed = C.colbal_sk_routed(M, N, K)
        for b in (None, c["b"]):
            out = C.skinny_gemm(x, c["w"], b)
            part = C.skinny_gemm_partials(x, c["w"], b)
            with _parent():
                want = C.skinny_gemm(x, c["w"], b)
                want_part = C.skinny_gemm_partials(x, c["w"], b)
            assert fo.bits_equal(out, want), (M, b is not None, routed)
            assert fo.bits_equal(part, want_part), (M, b is not None, routed)
            # bias once, in the reduce: the partials carry none
            assert fo.bits_equal(_host_reduce(C.gemm_colbal_sk(x, c["w"], 0),
                                              b), want), (M, b is not None)


def test_routing_domain_and_switch():
    C = _C()
    N, K = 4096, 1376
    assert C.gemm_n_split(N, K) > 1
    # never below the streaming threshold, above 512 rows, or unsplit shapes
    assert not C.colbal_sk_routed(64, N, K)
    assert not C.colbal_sk_routed(513, N, K)
    assert C.gemm_n_split(16384, 192) == 1
    assert not C.colbal_sk_routed(256, 16384, 192)
    with _parent():
        for M in MS:
            assert not C.colbal_sk_routed(M, N, K)


# --------------------------------------------------------------------------
# M independence, poisoning
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(128, 544), (4608, 1376)])
def test_rows_do_not_depend_on_m(N, K):
    C = _C()
    c = _case(N, K)
    full = C.gemm_colbal_sk(c["x"], c["w"], 0)
    assert full.shape[1] == 512
    for M in (65, 129, 257):
        part = C.gemm_colbal_sk(c["x"][:M].contiguous(), c["w"], 0)
        assert fo.bits_equal(part, full[:, :M].contiguous()), M


@pytest.mark.parametrize("N,K", [(64, 288), (448, 1024), (4608, 1376)])
def test_poisoned_buffer_is_fully_overwritten_and_not_overrun(N, K):
    C = _C()
    n_split = _n_split(N, K)
    c = _case(N, K)
    for M in (65, 257):
        x = c["x"][:M].contiguous()
        want = C.gemm_colbal_sk(x, c["w"], 0)
        for nb in _blocks(N, K):
            n = n_split * M * N
            # room for 256 more rows behind the last split: rows >= M of
            # its last row block would land there
            buf = torch.full((n + 256 * N,), float("nan"), device=DEV)
            got = C.gemm_colbal_sk(x, c["w"], nb, buf)
            assert got.data_ptr() == buf.data_ptr()
            assert fo.bits_equal(got, want), (M, nb)
            assert not torch.isnan(buf[:n]).any(), (M, nb)
            assert torch.isnan(buf[n:]).all(), \
                f"M={M} nb={nb}: rows past M were written"


# --------------------------------------------------------------------------
# model level
# --------------------------------------------------------------------------
@pytest.mark.parametrize("B", [65, 130])
def test_generate_equals_the_parent_kernels(B):
    from tensorlink_amd.parallel.planner import plan_for_world
    from tensorlink_amd.parallel.pipeline import PipelineRunner, SamplingParams
    ops = _ops()
    S, T = 4, 6
    plan = plan_for_world("tiny", 1, batch_size=B, seq_len=S + T)
    ids = torch.randint(0, 1024, (B, S),
                        generator=torch.Generator().manual_seed(9))
    sp = SamplingParams(max_new_tokens=T)

    def run(graph):
        r = PipelineRunner(plan, 0, 1, device=DEV, dtype=BF)
        if graph:
            out = r.generate(ids, sp).cpu()
            assert r._decode_graph is not None, "graph was not captured"
            return out
        os.environ["TL_NO_GRAPH"] = "1"
        try:
            return r.generate(ids, sp).cpu()
        finally:
            os.environ.pop("TL_NO_GRAPH", None)

    before = ops.gemm_dispatch_count
    out_graph = run(True)
    assert ops.gemm_dispatch_count > before
    before = ops.gemm_dispatch_count
    out_eager = run(False)
    assert ops.gemm_dispatch_count > before
    with _parent():
        want_graph = run(True)
        want_eager = run(False)
    assert out_graph.shape == (B, T)
    assert torch.equal(out_graph, want_graph)
    assert torch.equal(out_eager, want_eager)
    assert torch.equal(out_graph, out_eager)


# --------------------------------------------------------------------------
# the three real shapes, once each
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,K,n_split", [("qkv", 4608, 3584, 4),
                                              ("o", 3584, 3584, 8),
                                              ("down", 3584, 18944, 8)])
def test_real_shapes_equal_the_parent_and_repeat(name, N, K, n_split):
    C = _C()
    M = 256
    assert C.gemm_n_split(N, K) == n_split
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(M, K, generator=gen, device=DEV).to(BF)
    w = (torch.randn(N, K, generator=gen, device=DEV) / K ** 0.5).to(BF)
    want = _parent_partials(x, w)
    first = C.gemm_colbal_sk(x, w, 0)
    assert fo.bits_equal(first, want), name
    for _ in range(9):
        assert torch.equal(C.gemm_colbal_sk(x, w, 0), first), name
    # and through the routing, whichever kernel the band takes
    assert fo.bits_equal(C.skinny_gemm_partials(x, w, None), want), name
