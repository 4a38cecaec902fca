"""CPU tests of the shared device-wide scan and radix sort (csrc/radix.hip) through the debug entries of the emulated library
(tests/hipemu): the groups of tests/prim_cases.py that fit a host, each in a child process -- every size up to three sort blocks + 1,
all four pass counts and both result buffers, the count on the device, zero_words_behind in its paths of the single-kernel regime and
for n == 0, scratch_zeroed, sort_keys63, the argument errors.  Every comparison is exact against numpy; every call runs on a poisoned
workspace between canaries.  Of the regimes that begin at 2 M / 8 M words the emulator takes three groups at 2-3 s each (below the
slowest tests over it): the sort's histogram / scan / scatter launches at their smallest (2 M + 1 pairs, one pass), and the scan in big
tiles and in its three-launch form, each form once.  The others -- first_hist_done, n_dev / zero_words_behind / patterns / four passes /
sort_keys63 across the sort's regime edge -- cost it 7-28 s each and run in tests/test_primitives_gpu.py only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import host_child  # noqa: E402
import prim_cases as PC  # noqa: E402


def _child(group, out):
    import ctypes as C
    lib = PC.bind(C.CDLL(os.environ["GOF_HIP_LIB"]))
    f = PC.GPU_GROUPS[group]
    np.savez(out, calls=f(lib, PC.HostMem()))


def test_constants_come_from_the_source():
    """the sizes of the cases follow the constants of radix.hip (what they are today is not asserted: a retuned constant moves them)"""
    assert PC.BLOCK == 4 * PC.QUARTER and PC.QUARTER % PC.STEP == 0 and PC.SCAN_SMALL <= PC.SCAN_BIG
    assert PC.SCAN_DIRECT_EDGE >= PC.SCAN_TILE_EDGE and PC.OS_EDGE % PC.BLOCK == 0
    assert {0, 1, PC.STEP + 1, PC.QUARTER - 1, PC.BLOCK, PC.SCAN_BIG + 1, 3 * PC.BLOCK + 1} <= set(PC.SMALL_SIZES)
    assert sorted({PC.passes_of(e) for e in PC.END_BITS}) == [1, 2, 3, 4]


def test_references_on_answers_that_are_obvious():
    x = np.array([1, 2, 0xFFFFFFFF, 5], np.uint32)
    assert PC.scan_ref(x, None, True)[0].tolist() == [1, 3, 2, 7]
    ex, tot = PC.scan_ref(x, None, False)
    assert ex.tolist() == [0, 1, 3, 2] and tot == 7
    assert PC.scan_ref(x, np.array([3, 3, 0], np.uint32), True)[0].tolist() == [5, 10, 11]
    k = np.array([0x2001, 0x0F00, 0x1001, 0x0001], np.uint32)
    assert PC.sort_order(k, 12).tolist() == [3, 1, 2, 0]              # whole digits: bits 12 and 13 count although end_bit = 12
    assert PC.sort_order(k, 8).tolist() == [1, 0, 2, 3]               # one digit: stable among the three keys that end in 01
    assert PC.first_histogram(np.array([1, 1, 2], np.uint32), 3)[[1, 2]].tolist() == [2, 1]
    for p in PC.KEY_PATTERNS:
        for e in PC.END_BITS:
            k = PC.sort_keys(p, 1000, e)
            assert k.dtype == np.uint32 and len(k) == 1000
            assert p == "high_bits" or not (k & ~np.uint32(PC.mask_of(e))).any()
    assert (PC.sort_keys("high_bits", 1000, 9) >> 16).any()
    assert all((PC.keys63(p, 100) >> np.uint64(63) == 0).all() for p in ("low", "high", "both", "bit62"))
    assert (PC.keys63("bit62", 100) >> np.uint64(62)).any()


@pytest.mark.parametrize("group", list(PC.HOST_GROUPS) + list(PC.HOST_EDGE_GROUPS))
def test_group_equals_numpy(group, tmp_path):
    r = host_child.run_child(__file__, group, tmp_path, timeout=1200)
    assert int(r["calls"]) > 0


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
