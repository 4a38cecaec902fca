"""CPU: the backward blend's entry merging (csrc/blend_backward.hip, GOF_BW_MERGE) run from source on the host emulator
(tests/hipemu, as tests/test_hipemu_parity.py) on the hand-built scenes of tests/backward_merge_scenes.py: every gradient of the
default build is bit-equal to the build without merging (-DGOF_BW_MERGE=0) and within the oracle bars, and the instrumented build
counts exactly the merged trips the scenes are built to have -- so the equality is not that of a path that never ran.  The emulator
aborts the process when the lanes of a wave meet at different cross-lane sites (the ballots of the merge decision)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import oracle_binding as ob  # noqa: E402
import backward_merge_scenes as M  # noqa: E402
import test_parity_gpu as TP  # noqa: E402
from gpu_common import bits  # noqa: E402

build_emu = pytest.importorskip("build_emu")
if not os.path.exists(build_emu.CXX):
    pytest.skip("no host clang++ (%s) to build the emulated library" % build_emu.CXX, allow_module_level=True)
import emu_binding as E  # noqa: E402
if os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu", "_build", "BUILD_FAILED_build_emu")):
    raise RuntimeError("__graft_entry__.build() recorded a failed build_emu run (tests/hipemu/_build/BUILD_FAILED_build_emu): these tests must not be skipped over it")

BLEND = ("means2D", "colors", "opacity", "view2gaussian")
K9 = ("means3D", "sh", "scales", "rotations")


def _nomerge():
    return E.load(extra_flags=("-DGOF_BW_MERGE=0",), tag="nomerge")


def _stats():
    return E.load(extra_flags=("-DGOF_STATS", "-DGOF_CULL_AUDIT"), tag="audit")       # (the build tests/test_hipemu_parity.py's cull audit uses)


def _backward(sc, dL, lib=None):
    e = E.EmuScene(sc, lib=lib)
    e.forward()
    return e, e.backward(dL)


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", M.NAMES)
def test_emulated_merged_backward_is_bit_equal_to_the_unmerged_one(name, size):
    sc = M.scene(name, *size)
    o = ob.OracleScene(sc)
    oc, orad = o.forward()
    dL = np.random.default_rng(1).normal(size=oc.shape).astype(np.float32)
    e, got = _backward(sc, dL)
    _, want = _backward(sc, dL, _nomerge())
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert (got["means2D"][:, 2] >= 0).all() and got["means2D"][:, 2].any()
    go = o.backward(dL)
    for k in BLEND:
        TP.assert_grad_close(got[k], go[k], k)
    iso = o.preprocess_backward(got["view2gaussian"], got["colors"])
    for k in K9:
        TP.assert_k9_close(got[k], iso[k], k)
    if name == "depth_branch":                # B (nearer: list position 0) is the median-depth contributor of some pixel: its depth gradient is taken in a merged trip
        HW = size[0] * size[1]
        assert (e.fetch("n_contrib")[HW:] == 1).any()


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(M.MERGED_TRIPS))
def test_emulated_merged_trips_are_counted_where_the_scenes_have_them(name, size):
    lib = _stats()
    sc = M.scene(name, *size)
    out = (C.c_ulonglong * 12)()
    e = E.EmuScene(sc, lib=lib)
    img, _ = e.forward()
    lib.gof_debug_bw_stats(out, 1)
    e.backward(np.ones_like(img))
    lib.gof_debug_bw_stats(out, 1)
    assert out[11] == M.MERGED_TRIPS[name] and out[5] == out[11], (name, list(out))


@pytest.mark.parametrize("seed", range(4))
def test_emulated_merged_backward_fuzz(seed):
    sc = M.fuzz_scene(seed)
    dL = np.random.default_rng(seed).normal(size=(9, sc["H"], sc["W"])).astype(np.float32)
    _, got = _backward(sc, dL)
    _, want = _backward(sc, dL, _nomerge())
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
