"""The column ranges of the column-balanced GEMMs, from the functions the
kernel walks (colbal_range / colbal_sub_range of ops/csrc/gemm_policy.hpp)
through their binding ``_C.colbal_ranges``: host arithmetic only, no device.

For T column tiles dealt to G workgroups at `slots` tiles per pass, the
ranges must be contiguous and ascending, cover every tile exactly once and
differ in size by at most one, and no sub-range may exceed the slot count.
The expected sizes are stated here independently: the first T % G workgroups
get ceil(T / G) tiles, the rest floor(T / G)."""

import pytest

from tensorlink_amd import ops

pytestmark = pytest.mark.skipif(
    not ops.extension_loaded(), reason="HIP extension is not built")

TS = (4, 28, 224, 288, 2368)
GS = (1, 3, 7, 32, 64, 300)


def _slot_counts():
    return list(ops._require_ext().colbal_sk_slot_counts())


def test_the_kernel_is_built_with_some_slot_counts():
    slots = _slot_counts()
    assert slots and all(s >= 1 for s in slots)
    # o_proj / down_proj: 224 tiles over 32 workgroups is 7 each, one pass
    assert max(slots) >= 7


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("T", TS)
def test_ranges_cover_every_tile_once_and_fit_the_slots(T, G):
    C = ops._require_ext()
    for slots in _slot_counts():
        ranges = C.colbal_ranges(T, G, slots)
        assert len(ranges) == G
        at = 0
        sizes = []
        for b, subs in enumerate(ranges):
            size = 0
            sub_sizes = []
            for start, count in subs:
                # contiguous and ascending, within and across workgroups
                assert start == at, (T, G, slots, b)
                assert 1 <= count <= slots, (T, G, slots, b)
                at += count
                size += count
                sub_sizes.append(count)
            # equalised passes, and no more of them than needed
            if sub_sizes:
                assert max(sub_sizes) - min(sub_sizes) <= 1
                assert len(sub_sizes) == -(-size // slots)
            sizes.append(size)
        assert at == T, "not every tile is covered exactly once"
        assert max(sizes) - min(sizes) <= 1
        want = [T // G + (1 if b < T % G else 0) for b in range(G)]
        assert sizes == want
