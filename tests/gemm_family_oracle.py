"""Contract of the bf16 GEMM family's split-K range, as a CPU model
(docs/TESTING.md, "bf16 GEMM family, split-K range").

A plain module, torch only; nothing here comes from the code under test.
It states what skinny_gemm.hip, gemm_tiled.hip and splitk_reduce.hip must
compute when the policy splits K, builds the cases the CPU tier
(tests/test_gemm_family_cpu.py) and the GPU tier
(tests/test_gemm_family_gpu.py) share, and carries the deliberately wrong
variants ("mutants") the CPU tier shows the checks reject.

The contract
------------
* the split count is pure in (N, K): ``n_split_for``;
* split s covers ``k_slices(K, n_split)[s]``: contiguous ascending ranges
  that begin at multiples of 64 and whose union is exactly [0, K); a
  trailing split may be empty (end <= begin) and then contributes zeros;
* each split's partial is an fp32 sum of exact bf16 products; the partials
  are summed in ascending split order from 0, then bias, then ONE rounding
  to bf16: ``family_emulated``.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

BF16 = torch.bfloat16
F32 = torch.float32

STREAM_M = 64          # rows up to which the streaming kernel serves
WIDE_N = 65536

# (N, K) -> n_split at the default target. What each one exercises is in
# docs/TESTING.md; TAIL_DROPPED are the shapes whose last 32 k belonged to
# no split under the floor-division slice.
SHAPES = {
    (64, 160): 2,
    (64, 224): 2,
    (64, 288): 4,
    (64, 320): 4,
    (64, 352): 4,
    (128, 512): 8,
    (128, 544): 8,
    (1024, 1056): 8,
    (4096, 1376): 4,
    (128, 8224): 8,
}
TAIL_DROPPED = ((64, 160), (64, 288), (128, 544), (1024, 1056), (128, 8224))

# streaming MT 1 / 2 / 4, tiled MT 8, tiled MT 16 with one and two
# blockIdx.z blocks, and a partial last m-tile
MS = (1, 16, 17, 33, 64, 65, 128, 129, 257, 300)


def n_split_for(N: int, K: int, target: int = 256) -> int:
    """gemm_n_split_for of gemm_policy.hpp, transcribed."""
    n_split = 1
    if N >= WIDE_N:
        while (((N + 255) // 256) * n_split < target and n_split < 16
               and (K // 64) // (n_split * 2) >= 16):
            n_split <<= 1
        return n_split
    while ((N // 64) * n_split < target and n_split < 8
           and (K // 32) // (n_split * 2) >= 2):
        n_split <<= 1
    return n_split


def k_slices(K: int, n_split: int) -> List[Tuple[int, int]]:
    """The contract: whole 64-k chunks, the 32-wide tail counting as one,
    ceil-divided over the splits. (begin, end) per split; end <= begin is
    an empty split."""
    per = (((K + 63) // 64 + n_split - 1) // n_split) * 64
    return [(s * per, min(K, s * per + per)) for s in range(n_split)]


def k_slices_floor(K: int, n_split: int) -> List[Tuple[int, int]]:
    """The floor-division slice the kernels had: K // 64 does not count the
    32-wide tail, so when n_split divides K // 64 the tail is in no split."""
    per = ((K // 64 + n_split - 1) // n_split) * 64
    return [(s * per, min(K, s * per + per)) for s in range(n_split)]


def covered(slices: Sequence[Tuple[int, int]], K: int) -> bool:
    """True when the non-empty slices are contiguous from 0 to K and every
    empty one trails them."""
    at, seen_empty = 0, False
    for b, e in slices:
        if e <= b:
            seen_empty = True
            continue
        if seen_empty or b != at:
            return False
        at = e
    return at == K


def split_of(k: int, slices: Sequence[Tuple[int, int]]) -> int:
    for s, (b, e) in enumerate(slices):
        if b <= k < e:
            return s
    raise ValueError(f"k = {k} is in no slice of {list(slices)}")


def onehot_ks(K: int, slices: Sequence[Tuple[int, int]]) -> List[int]:
    """The k a split kernel can lose or misplace: each slice's first
    element, the two around its first kk boundary and its last element;
    the first chunk's edges; the tail's first and last element."""
    ks = {0, 63, 64, K - 32, K - 1}
    for b, e in slices:
        if e > b:
            ks.update(k for k in (b, b + 31, b + 32, e - 1) if b <= k < e)
    return sorted(k for k in ks if 0 <= k < K)


def onehot_rows(M: int, K: int, ks: Sequence[int]) -> torch.Tensor:
    """x [M, K] bf16: row i is 1.0 at ks[i % len(ks)], 0 elsewhere."""
    x = torch.zeros(M, K, dtype=BF16)
    idx = torch.tensor([ks[i % len(ks)] for i in range(M)])
    x[torch.arange(M), idx] = 1.0
    return x


def onehot_expected(w: torch.Tensor, b: Optional[torch.Tensor], M: int,
                    ks: Sequence[int]) -> torch.Tensor:
    """[M, N] bf16: w[:, k] of each row's k; with bias the one rounding of
    w + b."""
    idx = torch.tensor([ks[i % len(ks)] for i in range(M)], device=w.device)
    rows = w.t()[idx]
    if b is None:
        return rows.contiguous()
    return (rows.float() + b.float()).to(BF16)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same shape, dtype and bit pattern (so -0.0 != 0.0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.contiguous().view(as_int),
                       b.contiguous().to(a.device).view(as_int))


# --------------------------------------------------------------------------
# emulation and mutants
# --------------------------------------------------------------------------
MUTANTS = ("floor_slice", "skip_first_chunk", "drop_last_split",
           "bias_per_split", "wrong_tail_half")

# Shapes where a mutant IS the contract, so nothing can reject it there;
# the CPU tier asserts the equality instead. bias_per_split is also the
# contract wherever there is no bias.
MUTANT_NOOP = {
    # the floor slice already covers K: K % 64 == 0, or n_split does not
    # divide K // 64
    "floor_slice": ((64, 224), (64, 320), (64, 352), (128, 512),
                    (4096, 1376)),
    "skip_first_chunk": (),
    "drop_last_split": (),
    "bias_per_split": (),
    # no 32-wide tail
    "wrong_tail_half": ((64, 320), (128, 512)),
}


def mutant_is_noop(name: str, N: int, K: int, bias: bool) -> bool:
    if name == "bias_per_split" and not bias:
        return True
    return (N, K) in MUTANT_NOOP[name]


def partials_emulated(x: torch.Tensor, w: torch.Tensor,
                      slices: Sequence[Tuple[int, int]],
                      mutant: Optional[str] = None) -> torch.Tensor:
    """fp32 [n_split, M, N]: split s holds x[:, slice s] @ w[:, slice s]^T;
    an empty split holds zeros.

    Mutants: ``skip_first_chunk`` starts the last non-empty split 64 k
    late. ``wrong_tail_half`` multiplies, for the 32-wide tail, what the
    second half of its staged 64-k chunk holds: slots past K re-read the
    row's last 8 elements, so tail element j becomes element
    K - 8 + j % 8 of both operands."""
    M, K = x.shape
    N = w.shape[0]
    xf, wf = x.to(F32), w.to(F32)
    live = [s for s, (b, e) in enumerate(slices) if e > b]
    out = torch.zeros(len(slices), M, N, dtype=F32, device=x.device)
    for s in live:
        b, e = slices[s]
        if mutant == "skip_first_chunk" and s == live[-1]:
            b = min(b + 64, e)
        idx = torch.arange(b, e, device=x.device)
        if mutant == "wrong_tail_half" and K % 64 == 32:
            tail = idx >= K - 32
            idx = torch.where(tail, K - 8 + (idx - (K - 32)) % 8, idx)
        if idx.numel():
            out[s] = xf[:, idx] @ wf[:, idx].t()
    return out


def reduce_emulated(partials: torch.Tensor, b: Optional[torch.Tensor],
                    mutant: Optional[str] = None,
                    last_live: Optional[int] = None) -> torch.Tensor:
    """The one reduce: ascending split order from 0, then bias, then one
    rounding to bf16. Mutants: ``drop_last_split`` leaves split
    ``last_live`` out, ``bias_per_split`` adds the bias after every
    split."""
    acc = torch.zeros_like(partials[0])
    for s in range(partials.shape[0]):
        if mutant == "drop_last_split" and s == last_live:
            continue
        acc = acc + partials[s]
        if mutant == "bias_per_split" and b is not None:
            acc = acc + b.to(F32)
    if b is not None and mutant != "bias_per_split":
        acc = acc + b.to(F32)
    return acc.to(BF16)


def family_emulated(x: torch.Tensor, w: torch.Tensor,
                    b: Optional[torch.Tensor],
                    slices: Sequence[Tuple[int, int]],
                    mutant: Optional[str] = None) -> torch.Tensor:
    """bf16 [M, N] of the contract over ``slices`` (or of one mutant of
    it; ``floor_slice`` is the contract over k_slices_floor, so the caller
    passes those slices)."""
    live = [s for s, (lo, hi) in enumerate(slices) if hi > lo]
    return reduce_emulated(partials_emulated(x, w, slices, mutant), b, mutant,
                           live[-1] if live else None)


def mutant_output(name: str, x, w, b, K: int, n_split: int) -> torch.Tensor:
    slices = (k_slices_floor if name == "floor_slice" else k_slices)(
        K, n_split)
    return family_emulated(x, w, b, slices, name)
