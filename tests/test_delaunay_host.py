"""CPU tests of the Delaunay tetrahedralization: the kernels of csrc/delaunay.hip through the host emulator
(tests/hipemu) behind delaunay.triangulate itself, each run in a child process so that an emulator abort fails one test, not the
session, held to the independent checker (tests/delaunay_check.py) and, in general position, to SciPy's Qhull; plus the tetranerf
shim's host path.

In the child the product module runs unchanged except for the test seams of tests/hipemu/host_child.py: GOF_HIP_LIB names the
emulated library, the device check / stream / device context are host stand-ins, and every arena is filled with 0xA5 (as
uninitialised as a device allocation) and followed by guard bytes that are checked after the run."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import host_child  # noqa: E402
from host_child import PKG  # noqa: E402
import delaunay_check as K  # noqa: E402

GOF_E_INVALID = -1


def case_points(name):
    """the inputs of the contract's cases (float32 [N,3])"""
    rng = np.random.default_rng(7)
    if name == "uniform_2k":
        return rng.random((2000, 3)).astype(np.float32)
    if name == "uniform_20k":
        return rng.random((20000, 3)).astype(np.float32)
    if name == "tetra_2k":
        import synthetic_scenes as S
        sc = S.scene_frustum(2000, seed=3)
        sc["rotations"] = np.tile(np.array([1, 0, 0, 0], np.float32), (2000, 1))      # unrotated boxes: near-cospherical corners
        return S.tetra_points(sc)
    if name.startswith("lattice"):
        g = np.arange(8, dtype=np.float32)
        L = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        if name == "lattice_perm":
            L = L[np.random.default_rng(11).permutation(len(L))]
        return np.ascontiguousarray(L)
    if name == "sphere":
        v = rng.normal(size=(4096, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return np.vstack([v.astype(np.float32), np.zeros((1, 3), np.float32)])
    if name == "dup":
        P = rng.random((500, 3)).astype(np.float32)
        Q = np.vstack([P, P])
        return np.ascontiguousarray(Q[rng.permutation(len(Q))])
    if name == "scales":
        return np.vstack([(rng.random((300, 3)) * 1e-6).astype(np.float32), (rng.random((300, 3)) * 2e6 - 1e6).astype(np.float32)])
    if name == "coplanar":
        P = rng.random((200, 3)).astype(np.float32)
        P[:, 2] = 0.5
        return P
    if name == "three":
        return rng.random((3, 3)).astype(np.float32)
    if name == "dup4":
        P = rng.random((1, 3)).astype(np.float32)
        return np.vstack([P, P, P, P, rng.random((2, 3)).astype(np.float32)])
    if name == "nan":
        P = rng.random((100, 3)).astype(np.float32)
        P[17, 1] = np.nan
        return P
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------
# the child: delaunay.triangulate over the emulated library
# ---------------------------------------------------------------------------------------------------------------------------
def _child(name, out, cap):
    import torch
    import delaunay
    check = host_child.install_seams(delaunay)
    res = {"T": np.zeros((0, 4), np.int32), "code": 0, "error": ""}
    try:
        res["T"] = delaunay.triangulate(torch.from_numpy(case_points(name)), capacity=cap or None).numpy()
    except RuntimeError as e:
        res["code"], res["error"] = getattr(e, "code", 0), str(e)
    assert check() > 0
    np.savez(out, stats=json.dumps(delaunay.last_stats()), **res)


def _emulate(name, tmp_path, order=None, cap=0):
    """-> (None or the (code, text) of the error triangulate raised, cells, last_stats())"""
    res = host_child.run_child(__file__, name, tmp_path, cap, order=order, timeout=1200)
    return (int(res["code"]), str(res["error"])) if str(res["error"]) else None, res["T"], json.loads(str(res["stats"]))


def _scipy_sets(P):
    from scipy.spatial import Delaunay
    return K.as_sets(Delaunay(P.astype(np.float64)).simplices)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform_2k", "uniform_20k"])
def test_uniform_matches_scipy(name, tmp_path):
    err, T, st = _emulate(name, tmp_path)
    assert err is None
    P = case_points(name)
    K.check(P, T)
    assert K.as_sets(T) == _scipy_sets(P)
    assert st["rounds"] > 0 and st["distinct_points"] == len(P)


@pytest.mark.parametrize("name", ["tetra_2k", "lattice", "sphere", "scales"])
def test_degenerate_inputs_are_valid(name, tmp_path):
    err, T, st = _emulate(name, tmp_path)
    assert err is None
    P = case_points(name)
    info = K.check(P, T, hull_sample=4000)
    if name == "lattice":
        assert st["exact_evaluations"] > 0, "the lattice must reach the exact predicates"
        assert len(T) >= 7 ** 3 * 5
    if name == "sphere":
        assert st["slow_insertions"] > 0, "the centre of a sphere needs a cavity beyond the fast path's slot"
        assert info["boundary_faces"] > 0


def test_duplicates_keep_the_lowest_index(tmp_path):
    err, T, _ = _emulate("dup", tmp_path)
    assert err is None
    P = case_points("dup")
    K.check(P, T)                       # (all distinct points used, by their lowest-index copy)
    rep = K.representatives(P)
    assert len(rep) == 500 and set(np.unique(T).tolist()) == set(rep.tolist())


@pytest.mark.parametrize("name", ["coplanar", "three", "dup4"])
def test_degenerate_dimension_gives_no_cells(name, tmp_path):
    err, T, _ = _emulate(name, tmp_path)
    assert err is None and T.shape == (0, 4)


def test_non_finite_input_is_invalid(tmp_path):
    err, T, _ = _emulate("nan", tmp_path)
    assert err is not None and err[0] == GOF_E_INVALID


def test_canonical_form(tmp_path):
    _, T, _ = _emulate("uniform_2k", tmp_path)
    T = T.astype(np.int64)
    assert (T[:, 0] < T[:, 1:].min(1)).all() and (T[:, 1] < T[:, 2:].min(1)).all()
    order = np.lexsort((T[:, 3], T[:, 2], T[:, 1], T[:, 0]))
    assert (order == np.arange(len(T))).all()


@pytest.mark.parametrize("order", ["reverse", "random:5"])
def test_bytes_do_not_depend_on_the_schedule(order, tmp_path):
    _, T0, _ = _emulate("lattice", tmp_path)
    _, T1, _ = _emulate("lattice", tmp_path, order=order)
    assert T0.tobytes() == T1.tobytes()


def test_permuted_input_gives_permuted_cells(tmp_path):
    _, T0, _ = _emulate("lattice", tmp_path)
    _, T1, _ = _emulate("lattice_perm", tmp_path)
    perm = np.random.default_rng(11).permutation(512)
    assert K.as_sets(perm[T1]) == K.as_sets(T0)


def test_tiny_capacity_retries_to_the_same_bytes(tmp_path):
    _, T0, s0 = _emulate("uniform_2k", tmp_path)
    _, T1, s1 = _emulate("uniform_2k", tmp_path, cap=64)
    assert s0["retries"] == 0 and s1["retries"] > 0
    assert T0.tobytes() == T1.tobytes()


def test_shim_host_tensor_keeps_scipy():
    import torch
    sys.path.insert(0, os.path.join(PKG, "shims"))
    try:
        from tetranerf.utils.extension import cpp
    finally:
        sys.path.remove(os.path.join(PKG, "shims"))
    from scipy.spatial import Delaunay
    P = case_points("uniform_2k")[:300]
    out = cpp.triangulate(torch.from_numpy(P))
    assert out.dtype == torch.int32 and out.device.type == "cpu"
    assert np.array_equal(out.numpy(), Delaunay(P.astype(np.float64)).simplices.astype(np.int32))


def test_checker_rejects_a_broken_triangulation():
    """the checker is the yardstick: a flipped cell and a non-Delaunay pair must fail it"""
    P = case_points("uniform_2k")[:200]
    from scipy.spatial import Delaunay
    S = Delaunay(P.astype(np.float64)).simplices.astype(np.int64)
    o, _ = K.orient(P, S[:, 0], S[:, 1], S[:, 2], S[:, 3])
    S[o < 0] = S[o < 0][:, [0, 1, 3, 2]]
    K.check(P, S)
    bad = S.copy()
    bad[0] = bad[0][[0, 1, 3, 2]]
    with pytest.raises(AssertionError, match="not positively oriented"):
        K.check(P, bad)
    # a 2-3 flip of an interior face: still a valid, positively oriented triangulation of the hull, but not Delaunay
    faces = {}
    for t, cell in enumerate(S.tolist()):
        for i in range(4):
            faces.setdefault(tuple(sorted(cell[:i] + cell[i + 1:])), []).append((t, cell[i]))
    for (a, b, c), pair in faces.items():
        if len(pair) != 2:
            continue
        (t0, d), (t1, e) = pair
        o = [K.orient(P, *[np.array([x]) for x in q])[0][0] for q in ((a, b, d, e), (b, c, d, e), (c, a, d, e))]
        if not (all(x > 0 for x in o) or all(x < 0 for x in o)):
            continue                     # the segment d-e does not cross the triangle's interior: no 2-3 flip
        new = np.array([[a, b, d, e], [b, c, d, e], [c, a, d, e]], np.int64)
        if o[0] < 0:
            new = new[:, [1, 0, 2, 3]]
        flipped = np.vstack([np.delete(S, [t0, t1], axis=0), new])
        with pytest.raises(AssertionError, match="not locally Delaunay"):
            K.check(P, flipped)
        break
    else:
        pytest.fail("no flippable interior face")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
