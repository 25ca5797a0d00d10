"""CPU tier of the bf16 GEMM family's split-K tests.

Without a GPU this shows that

* the contract model in tests/gemm_family_oracle.py is sound: the slices
  partition K, the split counts are the policy's, the emulation of the
  contract meets the conformance rule and the exact one-hot check;
* the GPU tier (tests/test_gemm_family_gpu.py) "would fail if the kernel
  were subtly wrong": each mutant, run through that tier's inputs, metric
  and tolerance, misses the rule by 2x or more AND fails the one-hot
  check, at every shape where it differs from the contract. Shapes where a
  mutant is the contract are listed in the oracle module and asserted to
  be exactly that;
* the slice the kernels now use equals the floor-division one wherever
  that one covered K, so only the shapes it broke change bits.
"""

import functools

import pytest
import torch

import gemm_family_oracle as fo
import kernel_oracle as ko

SHAPES = sorted(fo.SHAPES)
SWEEP_KS = range(32, 16416 + 1, 32)
SWEEP_SPLITS = (1, 2, 4, 8, 16)


@functools.lru_cache(maxsize=None)
def _case(N, K, bias):
    """The GPU tier's inputs at the largest M, with the fp64 reference and
    the bf16-rounded fp32 linear E0 comes from. Smaller M are row
    prefixes."""
    c = ko.gemm_case(max(fo.MS), N, K, bias)
    ref = ko.linear(c["x"], c["w"], c["b"])
    emu = ko.bf16_round(ko.linear(c["x"], c["w"], c["b"],
                                  dtype=torch.float32))
    return dict(c, ref=ref, emu=emu)


def _onehot(N, K, bias, out_of):
    """(got, want) of the one-hot check at M = 300 for a function
    x -> bf16 output."""
    c = _case(N, K, bias)
    ks = fo.onehot_ks(K, fo.k_slices(K, fo.SHAPES[(N, K)]))
    M = max(fo.MS)
    return (out_of(fo.onehot_rows(M, K, ks)),
            fo.onehot_expected(c["w"], c["b"], M, ks))


# --------------------------------------------------------------------------
# the contract model
# --------------------------------------------------------------------------
def test_split_counts_are_the_policys():
    for (N, K), n_split in fo.SHAPES.items():
        assert fo.n_split_for(N, K) == n_split, (N, K)
    # the rest of the transcription: the wide class, the caps, the floor
    assert fo.n_split_for(65664, 128) == 1
    assert fo.n_split_for(65664, 96) == 1
    assert fo.n_split_for(151936, 3584) == 1
    assert fo.n_split_for(65536, 8192) == 1
    assert fo.n_split_for(65536, 8192, target=1024) == 4
    assert fo.n_split_for(16320, 4096) == 2
    assert fo.n_split_for(16384, 4096) == 1
    assert fo.n_split_for(64, 96) == 1
    assert fo.n_split_for(64, 128) == 2
    assert fo.n_split_for(3584, 18944) == 8


def test_k_slices_partition_k():
    for K in SWEEP_KS:
        for n_split in SWEEP_SPLITS:
            sl = fo.k_slices(K, n_split)
            assert len(sl) == n_split
            assert all(b % 64 == 0 for b, _ in sl), (K, n_split)
            assert fo.covered(sl, K), (K, n_split, sl)
            assert sum(max(0, e - b) for b, e in sl) == K


def test_k_slices_equal_the_floor_slice_wherever_it_covered_k():
    """The fix may change bits only at the shapes the floor slice broke:
    those with K % 64 == 32 and n_split dividing K // 64."""
    broken = 0
    for K in SWEEP_KS:
        for n_split in SWEEP_SPLITS:
            old = fo.k_slices_floor(K, n_split)
            was_broken = K % 64 == 32 and (K // 64) % n_split == 0
            assert fo.covered(old, K) == (not was_broken), (K, n_split)
            if was_broken:
                broken += 1
                assert n_split * (old[0][1] - old[0][0]) == K - 32
            else:
                assert fo.k_slices(K, n_split) == old, (K, n_split)
    assert broken > 0


def test_table_marks_the_dropped_tails():
    for (N, K), n_split in fo.SHAPES.items():
        dropped = not fo.covered(fo.k_slices_floor(K, n_split), K)
        assert dropped == ((N, K) in fo.TAIL_DROPPED), (N, K)
    # the table's empty trailing splits
    assert fo.k_slices(320, 4)[3] == (384, 320)
    assert fo.k_slices(352, 4)[2:] == [(256, 352), (384, 352)]
    assert fo.k_slices(160, 2) == [(0, 128), (128, 160)]


def test_onehot_ks_hit_every_slice_edge():
    for (N, K), n_split in fo.SHAPES.items():
        sl = fo.k_slices(K, n_split)
        ks = fo.onehot_ks(K, sl)
        assert ks == sorted(set(ks)) and 0 <= ks[0] and ks[-1] == K - 1
        assert {0, 63, 64, K - 32, K - 1} <= set(ks)
        for b, e in sl:
            if e > b:
                assert {b, e - 1} <= set(ks)
                assert fo.split_of(b, sl) == fo.split_of(e - 1, sl)
        # every row of the largest call sees a k, every k a row
        assert len(ks) <= max(fo.MS)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
def test_contract_emulation_meets_the_rule(N, K, bias):
    c = _case(N, K, bias)
    sl = fo.k_slices(K, fo.SHAPES[(N, K)])
    out = fo.family_emulated(c["x"], c["w"], c["b"], sl)
    for M in fo.MS:
        e0 = ko.nme(c["emu"][:M], c["ref"][:M])
        assert ko.nme(out[:M], c["ref"][:M]) <= ko.tolerance(e0), M
    got, want = _onehot(N, K, bias, lambda x: fo.family_emulated(
        x, c["w"], c["b"], sl))
    assert fo.bits_equal(got, want)


# --------------------------------------------------------------------------
# mutants
# --------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("name", fo.MUTANTS)
def test_mutant_is_rejected(name, N, K, bias):
    c = _case(N, K, bias)
    n_split = fo.SHAPES[(N, K)]
    run = lambda x: fo.mutant_output(name, x, c["w"], c["b"], K, n_split)
    out = run(c["x"])
    got, want = _onehot(N, K, bias, run)
    if fo.mutant_is_noop(name, N, K, bias):
        # listed as the contract itself at this shape: it must be
        true = fo.family_emulated(c["x"], c["w"], c["b"],
                                  fo.k_slices(K, n_split))
        assert fo.bits_equal(out, true), (name, N, K)
        assert fo.bits_equal(got, want), (name, N, K)
        return
    worst = None
    for M in fo.MS:
        tol = ko.tolerance(ko.nme(c["emu"][:M], c["ref"][:M]))
        err = ko.nme(out[:M], c["ref"][:M])
        if worst is None or err / tol < worst[0]:
            worst = (err / tol, M, err, tol)
    print(f"MUTANT {name} N{N} K{K} bias{int(bias)}: weakest at M={worst[1]} "
          f"nme {worst[2]:.3e} tol {worst[3]:.3e} ratio {worst[0]:.1f}")
    # misses the rule by >= 2x at every M AND fails the exact check
    assert worst[0] >= 2, (name, N, K, worst)
    assert not fo.bits_equal(got, want), (name, N, K)
