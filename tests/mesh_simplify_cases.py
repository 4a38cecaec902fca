"""The case tables of the mesh simplification tests, shared by the CPU suite (test_mesh_simplify_host.py: the kernels
through the host emulator) and the GPU suite (test_mesh_simplify_gpu.py: the real library).  run(...) drives mesh_simplify's Python
layer and DeviceMesh.simplify and returns numpy arrays, want(...) is what tests/mesh_simplify_restatement.py says they must be; the tests
compare the two with equalities (same) and check the properties that do not need the restatement (properties).
A case is (V (NV,3) float64, F (NF,3) int32, N (NV,3) float32 or None, Col (NV,3) uint8 or None, h, origin or None).
Test infrastructure only."""
import numpy as np

import mesh_simplify_restatement as R
from mesh_components_cases import same, strip  # noqa: F401

_WANT = {}


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def _attrs(nv, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(nv, 3)).astype(np.float32), rng.integers(0, 256, (nv, 3)).astype(np.uint8)


def hand_cases():
    z3, zf = np.zeros((0, 3)), np.zeros((0, 3), np.int32)
    tri = np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.2], [0.1, 0.9, 0.3]])
    near = tri + np.array([0.01, 0.02, -0.03])
    cases = {
        "empty": (z3, zf, None, None, 0.5, None),
        "no_faces": (np.random.default_rng(1).uniform(0, 1, (5, 3)), zf, None, _attrs(5, 1)[1], 0.4, None),
        "one_triangle": (tri, [[0, 1, 2]], _attrs(3, 2)[0], _attrs(3, 2)[1], 0.25, None),
        "repeated_index": (np.vstack([tri, near]), [[0, 1, 2], [3, 3, 4], [5, 5, 5]], None, None, 0.25, (0.0, 0.0, 0.0)),
        # (face 1 lies on a line, its cross product is exactly zero in fp64: three distinct cells, so it is kept, and adds nothing to a quadric)
        "zero_area": ([[0.125, 0.125, 0.125], [0.875, 0.125, 0.375], [0.125, 0.875, 0.25], [0.5, 0.125, 0.25]], [[0, 1, 2], [0, 3, 1]], None, None, 0.25, (0.0, 0.0, 0.0)),
        "opposite": (np.vstack([tri, near]), [[0, 1, 2], [5, 4, 3], [0, 4, 2]], None, _attrs(6, 3)[1], 0.25, (0.0, 0.0, 0.0)),
        "on_a_boundary": (np.array([[0.5, 0.25, 0.0], [0.4999999999999999, 0.25, 0.0], [1.0, 0.75, 0.5], [0.0, 1.0, 1.0]]), [[0, 2, 3], [1, 2, 3]], None, None,
                          0.25, (0.0, 0.0, 0.0)),
        "one_cell": (np.random.default_rng(4).uniform(0, 1, (9, 3)), strip(7), _attrs(9, 4)[0], _attrs(9, 4)[1], 4.0, None),
    }
    return {k: (np.asarray(V, np.float64).reshape(-1, 3), np.asarray(F, np.int32).reshape(-1, 3), N, C, h, o) for k, (V, F, N, C, h, o) in cases.items()}


def icosphere(levels=5, noise=0.01, seed=11):
    """20 * 4^levels faces; vertices pushed along their normal by seeded noise"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    F = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
                  [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    for _ in range(levels):
        e = np.sort(np.stack([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], axis=1).reshape(-1, 2), axis=1)
        u, inv = np.unique(e, axis=0, return_inverse=True)
        mid = len(V) + inv.reshape(-1, 3)
        V = np.vstack([V, 0.5 * (V[u[:, 0]] + V[u[:, 1]])])
        a, b, c = F[:, 0], F[:, 1], F[:, 2]
        ab, bc, ca = mid[:, 0], mid[:, 1], mid[:, 2]
        F = np.vstack([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)])
    V = V / np.linalg.norm(V, axis=1, keepdims=True)
    V = V * (1.0 + noise * np.random.default_rng(seed).uniform(-1, 1, (len(V), 1)))
    N, C = _attrs(len(V), seed)
    return V, F.astype(np.int32), N, C, 0.11, None


def identity():
    """an icosphere with its coordinates on a grid of 1/64 and a cell of 1/128: below the smallest spacing of two different coordinates"""
    V, F, N, Col, _, _ = icosphere(2)
    V = np.round(V * 64) / 64
    assert len(np.unique(V, axis=0)) == len(V)
    return V, F, N, Col, 1.0 / 128, None


def torus(nu=96, nv=40):
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    V = np.stack([(1.0 + 0.35 * np.cos(v)) * np.cos(u), (1.0 + 0.35 * np.cos(v)) * np.sin(u), 0.35 * np.sin(v)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    F = np.vstack([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return V, F.astype(np.int32), None, _attrs(len(V), 12)[1], 0.17, None


FLAT_NORMAL = np.array([0.3, -0.2, 0.9327379053088815])          # unit


def flat_grid(n=70, seed=13):
    """a jittered n x n grid on the plane FLAT_NORMAL . p = 0.25"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    uv = np.stack([i, j], -1).reshape(-1, 2) / (n - 1.0) + rng.uniform(-0.3, 0.3, (n * n, 2)) / (n - 1.0)
    e1 = np.cross(FLAT_NORMAL, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(FLAT_NORMAL, e1)
    V = 0.25 * FLAT_NORMAL[None, :] + uv[:, :1] * e1[None, :] + uv[:, 1:] * e2[None, :]
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    F = np.vstack([np.stack([a, a + n, a + n + 1], -1), np.stack([a, a + n + 1, a + 1], -1)])
    return V, F.astype(np.int32), None, None, 0.09, None


def soup(nf=200000, nv=100000, seed=14):
    rng = np.random.default_rng(seed)
    V = rng.uniform(0, 1, (nv, 3))
    a = rng.integers(0, nv, nf)
    F = np.stack([a, (a + rng.integers(0, 40, nf)) % nv, rng.integers(0, nv, nf)], axis=-1)       # (some faces repeat an index)
    return V, F.astype(np.int32), None, rng.integers(0, 256, (nv, 3)).astype(np.uint8), 1.0 / 16, (0.0, 0.0, 0.0)


def fan(n, seed=15):
    """n faces around vertex 0, which shares its cell with the unreferenced vertex 1 only (a cluster of one vertex would skip the solve):
    that cluster (number 0) has exactly n corners, at sorted positions 0..n-1"""
    rng = np.random.default_rng(seed + n)
    a = np.arange(n + 1) * (2 * np.pi / (n + 1))
    rim = np.stack([np.cos(a), np.sin(a), rng.uniform(-0.05, 0.05, n + 1)], axis=-1)
    V = np.vstack([[[0.05, 0.07, 0.3], [0.06, 0.05, 0.31]], rim])
    i = np.arange(2, n + 2)
    F = np.stack([np.zeros(n, np.int64), i, i + 1], axis=-1)
    return V, F.astype(np.int32), None, None, 0.4, (-1.2, -1.2, -0.2)


def fan_sizes(tiling):
    s, b = tiling["sum_tile"], tiling["sum_block"]
    return (s - 1, s, s + 1), (b - 1, b, b + 1)


def cloud_strip(nv, seed=16):
    """nv random vertices of the unit cube joined by a strip: for the vertex counts at which the sort and the scan change their path"""
    V = np.random.default_rng(seed + nv).uniform(0, 1, (nv, 3))
    return V, strip(max(nv - 2, 0)), None, None, 0.125, None


def boundary_vertex_counts(tiling):
    b, t = tiling["sort_block"], tiling["scan_tile"]
    return tuple(sorted({b - 1, b, b + 1, t - 2, t - 1, t, t + 1}))


def refusals():
    """tag -> (case, the word the error names)"""
    V, F, _, _, h, _ = hand_cases()["one_triangle"]
    bad_f = F.copy()
    bad_f[0, 1] = 3
    neg_f = F.copy()
    neg_f[0, 2] = -1
    nan_v, inf_v = V.copy(), V.copy()
    nan_v[1, 2], inf_v[2, 0] = np.nan, np.inf
    return {"index_high": ((V, bad_f, None, None, h, None), "index"), "index_negative": ((V, neg_f, None, None, h, None), "index"),
            "nan_vertex": ((nan_v, F, None, None, h, (0.0, 0.0, 0.0)), "vertex is not finite"), "inf_vertex": ((inf_v, F, None, None, h, (0.0, 0.0, 0.0)), "vertex is not finite"),
            "nan_vertex_default_origin": ((nan_v, F, None, None, h, None), "vertex is not finite"), "inf_vertex_default_origin": ((inf_v, F, None, None, h, None), "vertex is not finite"),
            "inf_origin": ((V, F, None, None, h, (0.0, np.inf, 0.0)), "origin"), "nan_h": ((V, F, None, None, np.nan, None), "cell size"),
            "zero_h": ((V, F, None, None, 0.0, None), "cell size"), "negative_h": ((V, F, None, None, -1.0, None), "cell size"),
            "below_origin": ((V, F, None, None, h, (0.5, 0.0, 0.0)), "2^21"), "too_many_cells": ((V, F, None, None, 2.0 ** -23, (0.0, 0.0, 0.0)), "2^21")}


# ---- run and want --------------------------------------------------------------------------------------------------------------------
def _pad(Col):
    if Col is None:
        return None
    c = np.zeros((len(Col), 4), np.uint8)
    c[:, :3] = Col
    return c


def _np(t):
    return None if t is None else t.cpu().numpy()


def run(MS, M, up, case, dedupe=True, ply=None):
    """the module-level functions and DeviceMesh.simplify -> numpy arrays"""
    V, F, N, Col, h, origin = case
    vc, nc = MS.cluster(up(V), h, origin)
    out = MS.simplify(up(V), up(F), None if Col is None else up(_pad(Col)), cell=h, dedupe=dedupe, origin=origin)
    res = {"cluster_only": _np(vc), "cluster_only_count": np.array(nc), "count_only": np.array(MS.count_clusters(up(V), h, origin)),
           "counts": np.array([out["clusters"], out["used_mean_count"], out["dropped_degenerate"], out["dropped_duplicate"]])}
    for k in ("vertex_cluster", "cluster_vertices", "cluster_colors", "used_mean", "cluster_faces", "face_keep"):
        if out[k] is not None:
            res[k] = _np(out[k])
    if True:
        mesh = M.DeviceMesh(V, F, N, Col)
        st = mesh.simplify(cell=h, dedupe=dedupe, origin=origin)
        res.update({"v": mesh.vertices, "f": mesh.faces, "stats": np.array([st[k] for k in ("vertices_before", "faces_before", "vertices_after", "faces_after", "clusters",
                                                                                            "used_mean", "dropped_degenerate", "dropped_duplicate")])})
        if N is not None:
            res["n"] = mesh.vertex_normals
        if Col is not None:
            res["c"] = mesh.vertex_colors
        if ply:
            mesh.export(ply)
            res["ply"] = np.frombuffer(open(ply, "rb").read(), np.uint8)
    return res


def want(case, dedupe=True, ply=False, key=None):
    """what the restatement says run() returns (kept per key: the references are computed once per process)"""
    if key is not None and (key, dedupe, ply) in _WANT:
        return _WANT[(key, dedupe, ply)]
    V, F, N, Col, h, origin = case
    r = R.simplify(V, F, N, Col, h, dedupe, origin)
    res = {"cluster_only": r["vertex_cluster"], "cluster_only_count": np.array(r["clusters"]), "count_only": np.array(r["clusters"]),
           "counts": np.array([r["clusters"], int(r["used_mean"].sum()), r["dropped_degenerate"], r["dropped_duplicate"]])}
    for k in ("vertex_cluster", "cluster_vertices", "cluster_colors", "used_mean", "cluster_faces", "face_keep"):
        if r[k] is not None:
            res[k] = r[k]
    if True:
        res.update({"v": r["v"], "f": r["f"], "stats": np.array([len(V), len(F), len(r["v"]), len(r["f"])] + res["counts"].tolist())})
        if N is not None:
            res["n"] = r["n"]
        if Col is not None:
            res["c"] = r["c"]
        if ply:
            res["ply"] = np.frombuffer(R.ply_bytes(r["v"], r["f"], r["n"], r["c"]), np.uint8)
    if key is not None:
        _WANT[(key, dedupe, ply)] = res
    return res


def run_filled(MS, up, case, fill):
    """the C ABI itself over buffers (workspaces and outputs) filled with one byte value"""
    import ctypes as C
    L = MS.lib
    V, F, _, Col, h, origin = case
    V, F = np.ascontiguousarray(V, np.float64), np.ascontiguousarray(F, np.int32)
    nv, nf = len(V), len(F)
    o = (C.c_double * 3)(*[float(x) for x in (R.default_origin(V) if origin is None else origin)])

    def buf(nbytes):
        return up(np.full(max(int(nbytes), 1), fill, np.uint8))

    def down(t, n, dt):
        return t.cpu().numpy()[:n].copy().view(dt)
    v, f, col = up(V), up(F), None if Col is None else up(_pad(Col))
    nb = L.gof_mesh_cluster_ws_bytes(nv)
    ws, vc = buf(nb), buf(4 * nv)
    count = C.c_int64(-7)
    assert L.gof_mesh_cluster(nv, v.data_ptr(), o, h, vc.data_ptr(), C.byref(count), ws.data_ptr(), nb, MS._stream()) == 0, L.gof_last_error()
    nc = int(count.value)
    nb = L.gof_mesh_cluster_solve_ws_bytes(nv, nf, nc)
    ws, pos, oc, used = buf(nb), buf(24 * nc), buf(4 * nc), buf(nc)
    ucount = C.c_int64(-7)
    assert L.gof_mesh_cluster_solve(nv, nf, v.data_ptr(), f.data_ptr(), None if col is None else col.data_ptr(), vc.data_ptr(), nc, o, h, pos.data_ptr(),
                                    None if col is None else oc.data_ptr(), used.data_ptr(), C.byref(ucount), ws.data_ptr(), nb, MS._stream()) == 0, L.gof_last_error()
    nb = L.gof_mesh_cluster_faces_ws_bytes(nf)
    ws, cf, keep = buf(nb), buf(12 * nf), buf(nf)
    counts = (C.c_int64 * 2)(-7, -7)
    assert L.gof_mesh_cluster_faces(nv, nf, f.data_ptr(), vc.data_ptr(), nc, 1, cf.data_ptr(), keep.data_ptr(), counts, ws.data_ptr(), nb, MS._stream()) == 0, L.gof_last_error()
    res = {"vertex_cluster": down(vc, 4 * nv, np.int32), "cluster_vertices": down(pos, 24 * nc, np.float64).reshape(nc, 3), "used_mean": down(used, nc, np.uint8),
           "cluster_faces": down(cf, 12 * nf, np.int32).reshape(nf, 3), "face_keep": down(keep, nf, np.uint8),
           "counts": np.array([nc, ucount.value, counts[0], counts[1]])}
    if col is not None:
        res["cluster_colors"] = down(oc, 4 * nc, np.uint8).reshape(nc, 4)
    return res


def want_filled(case, key=None):
    w = want(case, key=key)
    return {k: w[k] for k in ("vertex_cluster", "cluster_vertices", "used_mean", "cluster_faces", "face_keep", "counts", "cluster_colors") if k in w}


# ---- properties that do not need the restatement's sums -----------------------------------------------------------------------------------
def properties(case, got, dedupe=True):
    """-> list of the properties that fail: structure of the output faces, every output vertex referenced, locality"""
    V, F, _, _, h, _ = case
    bad = []
    f, v = got["f"], got["v"]
    if len(f) and not (f.min() >= 0 and f.max() < len(v) and (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()):
        bad.append("three distinct in-range indices")
    if dedupe and len(np.unique(np.sort(f, axis=1), axis=0)) != len(f):
        bad.append("no unordered triple twice")
    if len(np.unique(f)) != len(v):
        bad.append("every output vertex referenced")
    # every input vertex and its cluster's vertex lie in one cell of side h: at most sqrt(3) h apart, up to the rounding of centre + y
    d = np.linalg.norm(np.asarray(V) - got["cluster_vertices"][got["vertex_cluster"]], axis=1) if len(V) else np.zeros(0)
    if not (d <= np.sqrt(3.0) * h * (1.0 + 2.0 ** -40)).all():
        bad.append("locality")
    return bad


def quadric_holds(case, got):
    """where used_mean is 0: objective(y) <= objective(m) + 2^-40 (|objective(m)| + t h^2), the objective Q(y) + lambda |y - m|^2 in numpy
    from the restatement's sums, y = the PRODUCT's position minus the cell centre"""
    V, F, _, Col, h, origin = case
    o = R.default_origin(V) if origin is None else np.asarray(origin, np.float64)
    S = R.sums(V, F, None, got["vertex_cluster"], int(got["counts"][0]), h, o)
    _, m, _, _ = R.solve(S, h)
    Q = S["quadric"]
    t = (Q[:, 0] + Q[:, 3]) + Q[:, 5]
    lam = t * R.REG
    y = got["cluster_vertices"] - S["centre"]
    free = got["used_mean"] == 0
    fy, fm = R.objective(Q, lam, m, y), R.objective(Q, lam, m, m)
    return bool((fy[free] <= fm[free] + 2.0 ** -40 * (np.abs(fm[free]) + t[free] * h * h)).all()), int(free.sum())
