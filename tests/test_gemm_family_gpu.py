"""GPU tier of the bf16 GEMM family's split-K tests (MI355X).

skinny_gemm.hip, gemm_tiled.hip and their shared splitk_reduce.hip, through
ops.linear and ops.linear_partials, at the shapes of
gemm_family_oracle.SHAPES: every one splits K under the default policy, with
the 32-wide K tail inside a split, at the end of the last split, with empty
trailing splits, and at every M template (streaming MT 1 / 2 / 4, tiled MT
8, tiled MT 16 with one and two row blocks). Three kinds of check:

* exact: one-hot rows must return columns of W bit for bit, and each split's
  partial must hold exactly its own slice of K;
* the conformance rule nme(out, ref64) <= MARGIN * E0 of
  tests/test_ops_conformance_gpu.py, E0 from the bf16-rounded fp32 linear;
* bitwise: a row is the same at every M, a call repeats, and the partials
  reduced on the host in the contract's order are ops.linear's bits.

The 256x256 kernel (N >= WIDE_N, M >= 65) splits no small K, so it has a
test of its own at the end, at n_split == 1: the same three kinds of check,
the bitwise one against the streaming kernel, which shares no loop with it.

tests/test_gemm_family_cpu.py shows that wrong kernels fail the first two.
Every call asserts that the hand-written family served it and that the
policy split K the way the table says, so neither a fallback nor a changed
split target can hollow these out.
"""

import functools

import pytest
import torch

import gemm_family_oracle as fo
import kernel_oracle as ko
from test_ops_conformance_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = sorted(fo.SHAPES)
M_MAX = max(fo.MS)


@pytest.fixture(autouse=True)
def _inference_mode():
    # the hand-written GEMM family only serves grad-free calls
    with torch.no_grad():
        yield


def _ops():
    from tensorlink_amd import ops
    assert ops.extension_loaded(), "HIP extension must be built on GPU boxes"
    return ops


def _ext():
    from tensorlink_amd import _C
    return _C


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """kernel_oracle.gemm_case at the largest M, on the device; smaller M
    are row prefixes, the bias-free case is the same x and w."""
    c = ko.gemm_case(M_MAX, N, K, True)
    return {k: v.to(DEV) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def _reference(N, K, bias):
    """(ref64, emu) [M_MAX, N]: computed once per case, never modified."""
    c = _case(N, K)
    b = c["b"] if bias else None
    ref = ko.linear(c["x"], c["w"], b)
    emu = ko.bf16_round(ko.linear(c["x"], c["w"], b, dtype=torch.float32))
    return ref, emu


def _family(fn_name, N, K, x, w, b=None, n_split=None):
    """ops.linear / ops.linear_partials with the two per-call asserts."""
    ops = _ops()
    if n_split is None:
        n_split = fo.SHAPES[(N, K)]
    assert _ext().gemm_n_split(N, K) == n_split, \
        "the policy no longer splits this shape as the table says"
    before = ops.gemm_dispatch_count
    out = getattr(ops, fn_name)(x, w, b)
    assert ops.gemm_dispatch_count == before + 1, "not the hand-written GEMM"
    return out


def _linear(N, K, x, w, b=None, n_split=None):
    out = _family("linear", N, K, x, w, b, n_split)
    assert out.dtype == torch.bfloat16 and out.shape == (x.shape[0], N)
    return out


def _partials(N, K, x, w, b=None):
    p = _family("linear_partials", N, K, x, w, b)
    assert isinstance(p, _ops().Partials), type(p)
    assert p.data.dtype == torch.float32
    assert p.data.shape == (fo.SHAPES[(N, K)], x.shape[0], N)
    assert (p.bias is None) == (b is None)
    return p


def _host_reduce(p, b):
    """The contract's reduce: ascending split order from 0, then bias,
    then one rounding."""
    acc = torch.zeros_like(p.data[0])
    for s in range(p.data.shape[0]):
        acc = acc + p.data[s]
    if b is not None:
        acc = acc + b.float()
    return acc.to(torch.bfloat16)


# --------------------------------------------------------------------------
# one-hot rows: no tolerance
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_onehot_rows_return_columns_of_w(N, K):
    c = _case(N, K)
    w, b = c["w"], c["b"]
    slices = fo.k_slices(K, fo.SHAPES[(N, K)])
    ks = fo.onehot_ks(K, slices)
    for M in fo.MS:
        x = fo.onehot_rows(M, K, ks).to(DEV)
        out = _linear(N, K, x, w)
        assert fo.bits_equal(out, fo.onehot_expected(w, None, M, ks)), \
            f"M={M}: linear(one-hot) is not w[:, k]"
        out_b = _linear(N, K, x, w, b)
        assert fo.bits_equal(out_b, fo.onehot_expected(w, b, M, ks)), \
            f"M={M}: linear(one-hot, bias) is not bf16(w[:, k] + b)"
        # partials: the split whose slice holds k has the value, every
        # other split 0.0
        want = torch.zeros(len(slices), M, N, dtype=torch.float32, device=DEV)
        holder = torch.tensor([fo.split_of(ks[i % len(ks)], slices)
                               for i in range(M)], device=DEV)
        want[holder, torch.arange(M, device=DEV)] = \
            fo.onehot_expected(w, None, M, ks).float()
        for bias in (None, b):
            p = _partials(N, K, x, w, bias)
            assert torch.equal(p.data, want), \
                f"M={M}: a split's partial holds more or less than its slice"
            assert fo.bits_equal(_host_reduce(p, bias),
                                 out if bias is None else out_b), M


@pytest.mark.parametrize("N,K", [s for s in SHAPES if s[1] <= 512])
def test_identity_returns_w_transposed(N, K):
    """Every k at once: the K x K identity as one tiled call, and in 64-row
    pieces through the streaming kernel."""
    c = _case(N, K)
    w, b = c["w"], c["b"]
    eye = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    assert K > fo.STREAM_M
    want = w.t().contiguous()
    want_b = (w.t().float() + b.float()).to(torch.bfloat16)
    assert fo.bits_equal(_linear(N, K, eye, w), want)
    assert fo.bits_equal(_linear(N, K, eye, w, b), want_b)
    for r0 in range(0, K, fo.STREAM_M):
        piece = eye[r0:r0 + fo.STREAM_M].contiguous()
        assert fo.bits_equal(_linear(N, K, piece, w),
                             want[r0:r0 + fo.STREAM_M]), r0
        assert fo.bits_equal(_linear(N, K, piece, w, b),
                             want_b[r0:r0 + fo.STREAM_M]), r0


# --------------------------------------------------------------------------
# the oracle rule
# --------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
def test_split_k_meets_the_oracle_rule(N, K, bias):
    c = _case(N, K)
    b = c["b"] if bias else None
    ref, emu = _reference(N, K, bias)
    for M in fo.MS:
        out = _linear(N, K, c["x"][:M].contiguous(), c["w"], b)
        check(f"gemm split N{N} K{K} M{M} bias{int(bias)}", out, ref[:M],
              ko.nme(emu[:M], ref[:M]))


# --------------------------------------------------------------------------
# bitwise
# --------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
def test_rows_are_the_same_at_every_m(N, K):
    """All ten shapes, so the tail shapes that split and their controls."""
    c = _case(N, K)
    full = _linear(N, K, c["x"], c["w"])
    assert fo.bits_equal(_linear(N, K, c["x"], c["w"]), full), \
        "a repeated call differs"
    for M in (64, 65, 150):
        part = _linear(N, K, c["x"][:M].contiguous(), c["w"])
        assert fo.bits_equal(part, full[:M]), f"M={M} differs from M={M_MAX}"
    one = _linear(N, K, c["x"][7:8].contiguous(), c["w"])
    assert fo.bits_equal(one[0], full[7]), f"M=1 differs from M={M_MAX}"


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
def test_partials_reduced_on_the_host_equal_linear(N, K, bias):
    c = _case(N, K)
    b = c["b"] if bias else None
    for M in fo.MS:
        x = c["x"][:M].contiguous()
        p = _partials(N, K, x, c["w"], b)
        want = _linear(N, K, x, c["w"], b)
        assert fo.bits_equal(_host_reduce(p, b), want), M
        assert fo.bits_equal(p.materialize(), want), M
        # a repeated call gives the same partials
        again = _partials(N, K, x, c["w"], b)
        assert fo.bits_equal(again.data, p.data), M


# --------------------------------------------------------------------------
# the slice contract, from the function the kernels call
# --------------------------------------------------------------------------
def test_k_slices_of_the_code_are_the_contract():
    """gemm_k_slice (gemm_policy.hpp) through its binding: host arithmetic
    only, no device memory."""
    C = _ext()
    for K in range(32, 16416 + 1, 32):
        for n_split in (1, 2, 4, 8, 16):
            got = [tuple(s) for s in C.gemm_k_slices(K, n_split)]
            assert got == fo.k_slices(K, n_split), (K, n_split)


# --------------------------------------------------------------------------
# the 256x256 kernel, against oracles that share no code with it
# --------------------------------------------------------------------------
# full panels with one chunk; a half-empty last panel with a K tail;
# prologue, steady state and drain with a quarter-full last panel
SQ_SHAPES = ((65536, 64), (65664, 96), (65600, 192))
# one row block with ghost rows, a full one, two
SQ_MS = (65, 256, 257)


@functools.lru_cache(maxsize=None)
def _sq_case(N, K):
    c = ko.gemm_case(max(SQ_MS), N, K, True)
    return {k: v.to(DEV) for k, v in c.items()}


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", SQ_SHAPES)
def test_sq256_kernel_against_streaming_fp64_and_onehot(N, K, bias):
    """gemm_tiled_sq_kernel, and with it the K loop the fused heads call:
    the head tests compare those against this kernel, so it is held here
    against the streaming kernel's rows (bitwise), float64 (the conformance
    rule) and columns of W (one-hot rows, exact)."""
    assert N >= fo.WIDE_N and min(SQ_MS) > fo.STREAM_M
    c = _sq_case(N, K)
    x, w = c["x"], c["w"]
    b = c["b"] if bias else None

    def lin(x_rows):
        """ops.linear: the 256x256 kernel above 64 rows, the streaming
        kernel up to 64."""
        return _linear(N, K, x_rows, w, b, n_split=1)

    def streamed(x_rows):
        return torch.cat([lin(x_rows[r0:r0 + fo.STREAM_M].contiguous())
                          for r0 in range(0, x_rows.shape[0], fo.STREAM_M)])

    want = streamed(x)
    ref = ko.linear(x, w, b)
    emu = ko.bf16_round(ko.linear(x, w, b, dtype=torch.float32))
    ks = fo.onehot_ks(K, fo.k_slices(K, 1))
    for M in SQ_MS:
        out = lin(x[:M].contiguous())
        assert torch.equal(out, want[:M]), \
            f"M={M}: rows differ from the streaming kernel's"
        check(f"gemm sq256 N{N} K{K} M{M} bias{int(bias)}", out, ref[:M],
              ko.nme(emu[:M], ref[:M]))
        hot = fo.onehot_rows(M, K, ks).to(DEV)
        assert fo.bits_equal(lin(hot), fo.onehot_expected(w, b, M, ks)), \
            f"M={M}: linear(one-hot) is not w[:, k]"
