"""CPU tests of the Delaunay tetrahedralization: the kernels of csrc/delaunay.hip through the host emulator
(tests/hipemu), each run in a child process so that an emulator abort fails one test, not the session, held to the independent
checker (tests/delaunay_check.py) and, in general position, to SciPy's Qhull; plus the tetranerf shim's host path."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
for _p in (HERE, PKG, os.path.join(HERE, "hipemu")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import delaunay_check as K  # noqa: E402

GOF_E_INVALID, GOF_E_CAPACITY = -1, -5


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
# the emulated library, driven from a child process
# ---------------------------------------------------------------------------------------------------------------------------
def _emu_lib():
    import build_emu
    lib = C.CDLL(build_emu.build())
    lib.gof_last_error.restype = C.c_char_p
    lib.gof_delaunay_ws_bytes.restype = C.c_size_t
    lib.gof_delaunay_ws_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.gof_delaunay_build.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.c_void_p]
    lib.gof_delaunay_emit.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.gof_delaunay_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def emu_triangulate(lib, P, cap=None):
    """triangulate's host logic over numpy buffers -> (rc, cells, stats, retries)"""
    P = np.ascontiguousarray(P, np.float32)
    n = len(P)
    cap = cap or 7 * n + 64
    retries = 0
    while True:
        ws = np.full(lib.gof_delaunay_ws_bytes(n, cap) + 256, 0xA5, np.uint8)      # (as uninitialised as a device allocation)
        m = C.c_int64()
        rc = lib.gof_delaunay_build(n, P.ctypes.data if n else None, cap, ws.ctypes.data, ws.size, C.byref(m), None)
        if rc == GOF_E_CAPACITY and m.value > cap:
            cap, retries = m.value, retries + 1
            continue
        if rc:
            return rc, np.zeros((0, 4), np.int32), np.zeros(8, np.int64), retries
        break
    T = np.zeros((m.value, 4), np.int32)
    assert lib.gof_delaunay_emit(ws.ctypes.data, m.value, T.ctypes.data, None) == 0, lib.gof_last_error()
    st = np.zeros(8, np.int64)
    assert lib.gof_delaunay_stats(ws.ctypes.data, st.ctypes.data, None) == 0
    return rc, T, st, retries


def _child(name, out, cap):
    lib = _emu_lib()
    base = name.split("@")[0]
    rc, T, st, retries = emu_triangulate(lib, case_points(base), cap=cap)
    np.savez(out, rc=rc, T=T, stats=st, retries=retries)


def _emulate(name, tmp_path, order=None, cap=0):
    out = str(tmp_path / ("%s_%s_%d.npz" % (name, (order or "forward").replace(":", "_"), cap)))
    env = dict(os.environ)
    if order:
        env["HIPEMU_ORDER"] = order
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name, out, str(cap)], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, "emulated run of %s (order %s) failed (rc %d):\n%s\n%s" % (name, order, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = dict(np.load(out))
    return int(res["rc"]), res["T"], res["stats"], int(res["retries"])


def _needs_emulator():
    import build_emu
    if not os.path.exists(build_emu.CXX):
        pytest.skip("no host clang++ (%s) to build the emulated library" % build_emu.CXX)


def _scipy_sets(P):
    from scipy.spatial import Delaunay
    return K.as_sets(Delaunay(P.astype(np.float64)).simplices)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform_2k", "uniform_20k"])
def test_uniform_matches_scipy(name, tmp_path):
    _needs_emulator()
    rc, T, st, _ = _emulate(name, tmp_path)
    assert rc == 0
    P = case_points(name)
    K.check(P, T)
    assert K.as_sets(T) == _scipy_sets(P)
    assert st[0] > 0 and st[5] == len(P)


@pytest.mark.parametrize("name", ["tetra_2k", "lattice", "sphere", "scales"])
def test_degenerate_inputs_are_valid(name, tmp_path):
    _needs_emulator()
    rc, T, st, _ = _emulate(name, tmp_path)
    assert rc == 0
    P = case_points(name)
    info = K.check(P, T, hull_sample=4000)
    if name == "lattice":
        assert st[1] > 0, "the lattice must reach the exact predicates"
        assert len(T) >= 7 ** 3 * 5
    if name == "sphere":
        assert st[3] > 0, "the centre of a sphere needs a cavity beyond the fast path's slot"
        assert info["boundary_faces"] > 0


def test_duplicates_keep_the_lowest_index(tmp_path):
    _needs_emulator()
    rc, T, _, _ = _emulate("dup", tmp_path)
    assert rc == 0
    P = case_points("dup")
    K.check(P, T)                       # (all distinct points used, by their lowest-index copy)
    rep = K.representatives(P)
    assert len(rep) == 500 and set(np.unique(T).tolist()) == set(rep.tolist())


@pytest.mark.parametrize("name", ["coplanar", "three", "dup4"])
def test_degenerate_dimension_gives_no_cells(name, tmp_path):
    _needs_emulator()
    rc, T, _, _ = _emulate(name, tmp_path)
    assert rc == 0 and T.shape == (0, 4)


def test_non_finite_input_is_invalid(tmp_path):
    _needs_emulator()
    rc, T, _, _ = _emulate("nan", tmp_path)
    assert rc == GOF_E_INVALID


def test_canonical_form(tmp_path):
    _needs_emulator()
    rc, T, _, _ = _emulate("uniform_2k", tmp_path)
    T = T.astype(np.int64)
    assert (T[:, 0] < T[:, 1:].min(1)).all() and (T[:, 1] < T[:, 2:].min(1)).all()
    order = np.lexsort((T[:, 3], T[:, 2], T[:, 1], T[:, 0]))
    assert (order == np.arange(len(T))).all()


@pytest.mark.parametrize("order", ["reverse", "random:5"])
def test_bytes_do_not_depend_on_the_schedule(order, tmp_path):
    _needs_emulator()
    _, T0, _, _ = _emulate("lattice", tmp_path)
    _, T1, _, _ = _emulate("lattice", tmp_path, order=order)
    assert T0.tobytes() == T1.tobytes()


def test_permuted_input_gives_permuted_cells(tmp_path):
    _needs_emulator()
    _, T0, _, _ = _emulate("lattice", tmp_path)
    _, T1, _, _ = _emulate("lattice_perm", tmp_path)
    perm = np.random.default_rng(11).permutation(512)
    assert K.as_sets(perm[T1]) == K.as_sets(T0)


def test_tiny_capacity_retries_to_the_same_bytes(tmp_path):
    _needs_emulator()
    _, T0, _, r0 = _emulate("uniform_2k", tmp_path)
    _, T1, _, r1 = _emulate("uniform_2k", tmp_path, cap=64)
    assert r0 == 0 and r1 > 0
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
