"""GPU: the backward blend's entry merging (csrc/blend_backward.hip, GOF_BW_MERGE) against the same sources built without it
(lib/libgof_hip_nomerge.so, built by __graft_entry__.build()): every gradient -- dL_dmeans3D, scales, rotations, opacities, shs,
means2D with its |.| z component, and the blend's own dL_dcolors / dL_dview2gaussian -- is BIT-IDENTICAL between the two libraries, and
within the oracle bars of tests/test_parity_gpu.py, on the hand-built scenes of tests/backward_merge_scenes.py (64x48 and 70x50) and
on 20 seeded small scenes.  The instrumented build (lib/libgof_hip_audit.so) counts the merged trips of the two merging scenes:
exactly the number they are built to have, so the equality is not that of a path that never ran."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_binding as ob
import backward_merge_scenes as M
import test_parity_gpu as TP
from gpu_common import PKG, bits, product_forward_raw, to_dev

pytestmark = pytest.mark.gpu

BLEND = ("means2D", "colors", "opacity", "view2gaussian")
K9 = ("means3D", "sh", "scales", "rotations")
_libs = {}


@contextlib.contextmanager
def _library(tag):
    """the calls inside the block go to lib/libgof_hip_<tag>.so (the binding looks its library up per call)"""
    from diff_gaussian_rasterization import _backend as B
    if tag not in _libs:
        path = os.path.join(PKG, "lib", "libgof_hip_%s.so" % tag)
        assert os.path.exists(path), "lib/libgof_hip_%s.so is missing: run __graft_entry__.build()" % tag
        keep = B.LIB_PATH
        try:
            B.LIB_PATH = path
            _libs[tag] = B._load()
        finally:
            B.LIB_PATH = keep
    keep = B.lib
    B.lib = _libs[tag]
    try:
        yield _libs[tag]
    finally:
        torch.cuda.synchronize()
        B.lib = keep


def _gradients(sd, dL):
    res = product_forward_raw(sd)
    torch.cuda.synchronize()
    return TP._product_backward(res, dL)


def _check(sc, seed):
    o = ob.OracleScene(sc)
    oc, orad = o.forward()
    dL = np.random.default_rng(seed).normal(size=oc.shape).astype(np.float32)
    sd = to_dev(sc)
    got = _gradients(sd, dL)
    with _library("nomerge"):
        want = _gradients(sd, dL)
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, int((bits(got[k]) != bits(want[k])).sum()))
    assert (got["means2D"][:, 2] >= 0).all()
    go = o.backward(dL)
    for k in BLEND:
        TP.assert_grad_close(got[k], go[k], k)
    iso = o.preprocess_backward(got["view2gaussian"], got["colors"])
    for k in K9:
        TP.assert_k9_close(got[k], iso[k], k)
    return got


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", M.NAMES)
def test_merged_backward_is_bit_identical_to_the_unmerged_one(name, size):
    got = _check(M.scene(name, *size), 1)
    assert got["means2D"][:, 2].any()


@pytest.mark.parametrize("seed", range(20))
def test_merged_backward_fuzz(seed):
    _check(M.fuzz_scene(seed), seed)


@pytest.mark.parametrize("size", M.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["pair", "chain3"])
def test_the_merging_scenes_take_their_merged_trips(name, size):
    sd = to_dev(M.scene(name, *size))
    out = (C.c_ulonglong * 12)()
    with _library("audit") as lib:
        res = product_forward_raw(sd)
        torch.cuda.synchronize()
        lib.gof_debug_bw_stats(out, 1)
        TP._product_backward(res, np.ones((9, size[1], size[0]), np.float32))
        lib.gof_debug_bw_stats(out, 1)
    assert out[11] == M.MERGED_TRIPS[name] and out[5] == out[11], (name, list(out))
