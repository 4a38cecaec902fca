"""The case tables of the mesh connected-components tests, shared by the CPU suite (test_mesh_components_host.py:
the kernels through the host emulator) and the GPU suite (test_mesh_components_gpu.py: the real library).  run(MC, up, ...) drives
mesh_components' Python layer and returns numpy arrays, want(...) is what tests/mesh_components_restatement.py says they must be;
the tests compare the two with equalities.  Test infrastructure only."""
import numpy as np

import mesh_components_restatement as R

MODES = ("edge", "vertex")
STRIP_SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
def _points(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


def strip(n, first_vertex=0):
    """a triangle strip of n faces over n + 2 vertices"""
    i = np.arange(n, dtype=np.int64)[:, None]
    return (i + np.arange(3)[None, :] + first_vertex).astype(np.int32).reshape(n, 3)


def strip_vertices(n, seed=0):
    i = np.arange(n + 2)
    z = np.random.default_rng(seed).uniform(-0.1, 0.1, n + 2)
    return np.stack([0.5 * i, (i % 2).astype(np.float64), z], axis=-1)


def hand_cases():
    """name -> (vertices (NV,3) float64, faces (NF,3) int32)"""
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)
    cases = {
        "two_tetrahedra": (8, np.vstack([tet, tet + 4])),
        "shared_vertex": (5, [[0, 1, 2], [2, 3, 4]]),
        "three_on_an_edge": (8, [[0, 1, 2], [5, 6, 7], [1, 0, 3], [0, 1, 4]]),
        "duplicated_face": (6, [[0, 1, 2], [3, 4, 5], [0, 1, 2], [2, 1, 0]]),
        "face_aab": (8, [[0, 0, 1], [1, 2, 3], [4, 5, 6], [1, 0, 7]]),
        "face_aaa": (7, [[2, 2, 2], [0, 1, 3], [2, 2, 5], [4, 4, 4], [6, 4, 6]]),
        "unreferenced_vertices": (12, [[1, 2, 3], [3, 2, 5], [8, 9, 10]]),
        "no_faces": (3, np.zeros((0, 3), np.int32)),
        "nothing": (0, np.zeros((0, 3), np.int32)),
        "one_face": (3, [[2, 0, 1]]),
    }
    return {k: (_points(nv, 100 + i), np.asarray(f, np.int32).reshape(-1, 3)) for i, (k, (nv, f)) in enumerate(cases.items())}


def strip_sizes(tiling):
    """the fixed sizes plus the face counts whose 3 NF straddle the sort's block, whose NF + 1 straddle the scan's tile, and whose
    sorted positions straddle the tiles and the block of the area sums -- `tiling` read from the library (mesh_components.tiling())"""
    sizes = set(STRIP_SIZES)
    b = tiling["sort_block"]
    sizes |= {(b - 1) // 3, b // 3, b // 3 + 1, (2 * b) // 3, (2 * b) // 3 + 1}
    t = tiling["scan_tile"]
    sizes |= {t - 2, t - 1, t, t + 1}
    s = tiling["sum_tile"]
    sizes |= {s - 1, s, s + 1, 2 * s + 1}
    return tuple(sorted(n for n in sizes if n >= 1))


def block_strip_size(tiling):
    """one strip that reaches into a second block of the area sums, and a tile into it"""
    return tiling["sum_block"] + tiling["sum_tile"] + 1


def strip_case(n):
    return strip_vertices(n, n), strip(n)


def deep_chain(n=20000, seed=5):
    """one strip in a random face order over randomly relabelled vertices: the deepest trees the hooking can build"""
    rng = np.random.default_rng(seed)
    relabel = rng.permutation(n + 2)
    F = relabel[strip(n)][rng.permutation(n)].astype(np.int32)
    V = np.empty((n + 2, 3))
    V[relabel] = strip_vertices(n, seed)
    return V, F


def floaters(big=50000, small=3000, seed=6):
    """one component of `big` faces and `small` components of 1..7 faces, a few stray vertices, the faces shuffled"""
    rng = np.random.default_rng(seed)
    parts, verts, off = [strip(big)], [strip_vertices(big, seed)], big + 2
    for i in range(small):
        n = int(rng.integers(1, 8))
        parts.append(strip(n, off))
        verts.append(strip_vertices(n, seed + 1 + i) + rng.uniform(-50, 50, 3))
        off += n + 2 + (i % 97 == 0)                         # (a stray vertex now and then)
        if i % 97 == 0:
            verts.append(np.zeros((1, 3)))
    F = np.vstack(parts)
    return np.vstack(verts), F[rng.permutation(len(F))].astype(np.int32)


def soup(nf=200000, seed=7):
    """strips of heavy-tailed lengths, a part of them glued to another strip along an edge (both modes join them), a part at one vertex
    only (the vertex mode joins them), the faces shuffled"""
    rng = np.random.default_rng(seed)
    lengths, total = [], 0
    while total < nf:
        lengths.append(int(min(nf - total, 1 + rng.pareto(0.9) * 3)))
        total += lengths[-1]
    starts = np.concatenate([[0], np.cumsum(np.array(lengths) + 2)])
    F = np.vstack([strip(n, int(s)) for n, s in zip(lengths, starts[:-1])])
    nv = int(starts[-1])
    rep = np.arange(nv)
    k = len(lengths)
    for i in rng.choice(k, k // 3, replace=False):
        j = int(rng.integers(0, k))
        a, b = int(starts[i + 1]) - 2, int(starts[j])         # the last two vertices of strip i, the first two of strip j
        if i % 2:
            rep[b], rep[b + 1] = rep[a], rep[a + 1]
        else:
            rep[b] = rep[a]
    while not np.array_equal(rep[rep], rep):
        rep = rep[rep]
    F = rep[F][rng.permutation(len(F))].astype(np.int32)
    return rng.uniform(-1, 1, (nv, 3)), F


def nan_case():
    V, F = hand_cases()["two_tetrahedra"]
    V = V.copy()
    V[5, 1] = np.nan
    return V, F


def inf_case():
    V, F = hand_cases()["two_tetrahedra"]
    V = V.copy()
    V[2, 0] = np.inf
    return V, F


# ---- run and want --------------------------------------------------------------------------------------------------------------------
def run(MC, up, V, F, connectivity):
    c = MC.components(up(np.asarray(V, np.float64).reshape(-1, 3)), up(F), connectivity)
    comp2, count2 = MC.face_components(up(F), len(V), connectivity)
    return {"label": c.face_label.cpu().numpy(), "comp": c.face_comp.cpu().numpy(), "count": np.array(c.count), "faces": c.faces, "first": c.first_face,
            "area": c.area, "comp_again": comp2.cpu().numpy(), "count_again": count2.cpu().numpy()}


def want(V, F, connectivity):
    label = R.labels(F, connectivity)
    comp, C = R.numbering(label)
    cf, first, area = R.stats(V, F, comp, C)
    return {"label": label, "comp": comp, "count": np.array(C), "faces": cf, "first": first, "area": area, "comp_again": comp,
            "count_again": np.array(C, np.int64)}


def run_filled(MC, up, V, F, connectivity, fill):
    """the C ABI itself over buffers (workspaces and outputs) filled with one byte value"""
    import ctypes as C
    L = MC.lib
    V, F = np.ascontiguousarray(V, np.float64).reshape(-1, 3), np.ascontiguousarray(F, np.int32).reshape(-1, 3)
    nv, nf, mode = len(V), len(F), MC.CONNECTIVITY[connectivity]

    def buf(nbytes):
        return up(np.full(max(int(nbytes), 1), fill, np.uint8))
    v, f = up(V) if nv else buf(8), up(F) if nf else buf(8)
    nb = L.gof_mesh_components_ws_bytes(nv, nf, mode)
    ws, label, comp = buf(nb), buf(4 * nf), buf(4 * nf)
    count = C.c_int64(-7)
    rc = L.gof_mesh_components(nv, nf, f.data_ptr(), mode, label.data_ptr(), comp.data_ptr(), C.byref(count), ws.data_ptr(), nb, MC._stream())
    assert rc == 0, L.gof_last_error()
    nc = int(count.value)
    nb2 = L.gof_mesh_component_stats_ws_bytes(nf, nc)
    ws2, cf, first, area = buf(nb2), buf(8 * nc), buf(4 * nc), buf(8 * nc)
    rc = L.gof_mesh_component_stats(nv, nf, v.data_ptr(), f.data_ptr(), comp.data_ptr(), nc, cf.data_ptr(), first.data_ptr(), area.data_ptr(),
                                    ws2.data_ptr(), nb2, MC._stream())
    assert rc == 0, L.gof_last_error()
    down = lambda t, n, dt: t.cpu().numpy()[:n].copy().view(dt)        # noqa: E731
    return {"label": down(label, 4 * nf, np.int32), "comp": down(comp, 4 * nf, np.int32), "count": np.array(nc), "faces": down(cf, 8 * nc, np.int64),
            "first": down(first, 4 * nc, np.int32), "area": down(area, 8 * nc, np.float64)}


def area_bound_holds(V, F, got):
    """|area[c] - bincount| <= (n_c - 1) 2^-53 sum |a_f|: the fp64 bound of a sum of n_c terms in any order; NaN / Inf components are
    compared as such"""
    a = R.face_areas(V, F)
    comp, C = got["comp"], int(got["count"])
    with np.errstate(invalid="ignore"):
        ref = np.bincount(comp, weights=a, minlength=C)
        bound = (np.maximum(got["faces"], 1) - 1) * 2.0 ** -53 * np.bincount(comp, weights=np.abs(a), minlength=C)
        fin = np.isfinite(ref)
        ok = np.where(fin, np.abs(got["area"] - ref) <= bound, (np.isnan(ref) & np.isnan(got["area"])) | (ref == got["area"]))
    return bool(ok.all())


# ---- selection -----------------------------------------------------------------------------------------------------------------------
def keep_mesh(seed=9):
    """components of 40, 12, 12, 40, 3, 1 faces (ties in the face counts; the two of 40 have different areas, the two of 12 equal
    ones), stray vertices, normals and colours, the faces shuffled but the first faces in this order -> (V, F, N, Col)"""
    rng = np.random.default_rng(seed)
    sizes = (40, 12, 12, 40, 3, 1)
    parts, verts, off = [], [], 0
    for i, n in enumerate(sizes):
        parts.append(strip(n, off))
        v = strip_vertices(n, 0)
        v[:, 2] = 0.0
        verts.append(v * (2.0 if i == 3 else 1.0) + np.array([0.0, 4.0 * i, 0.0]))
        off += n + 2
        verts.append(np.full((2, 3), 9.0))                   # two stray vertices behind every component
        off += 2
    F = np.vstack(parts)
    firsts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rest = np.setdiff1d(np.arange(len(F)), firsts)
    F = np.vstack([F[firsts], F[rng.permutation(rest)]]).astype(np.int32)
    V = np.vstack(verts).astype(np.float32).astype(np.float64)
    return V, F, rng.normal(size=V.shape).astype(np.float32), rng.integers(0, 256, V.shape).astype(np.uint8)


CRITERIA = (("largest1", dict(largest=1)), ("largest2_tie", dict(largest=2)), ("largest3_tie", dict(largest=3)), ("largest0", dict(largest=0)),
            ("largest1_area", dict(largest=1, by="area")), ("largest3_area_tie", dict(largest=3, by="area")), ("min_faces", dict(min_faces=12)),
            ("ratio", dict(min_area_ratio=0.2)), ("ratio_and_largest", dict(min_area_ratio=0.05, largest=3, by="faces")),
            ("vertex_min_faces", dict(min_faces=2, connectivity="vertex")), ("all", dict(min_faces=0)))


def run_keep(M, path_of):
    """M = mesh_cull; -> arrays per criterion, and the exported file's bytes"""
    V, F, N, Col = keep_mesh()
    res = {}
    for name, kw in CRITERIA:
        mesh = M.DeviceMesh(V, F, N, Col)
        kept, dropped = mesh.keep_components(**kw)
        mesh.export(path_of(name))
        res.update({name + "_v": mesh.vertices, name + "_f": mesh.faces, name + "_n": mesh.vertex_normals, name + "_c": mesh.vertex_colors,
                    name + "_counts": np.array([kept, dropped]), name + "_ply": np.frombuffer(open(path_of(name), "rb").read(), np.uint8)})
    plain = M.DeviceMesh(V, F)
    plain.remove_unreferenced_vertices()
    res["unreferenced_v"], res["unreferenced_f"] = plain.vertices, plain.faces
    res["mesh_area"] = np.array(M.DeviceMesh(V, F).area)
    return res


def want_keep():
    V, F, N, Col = keep_mesh()
    res = {}
    for name, kw in CRITERIA:
        v, f, n, c, kept, dropped = R.keep_components(V, F, N, Col, **kw)
        res.update({name + "_v": v, name + "_f": f, name + "_n": n, name + "_c": c, name + "_counts": np.array([kept, dropped]),
                    name + "_ply": np.frombuffer(R.ply_bytes(v, f, n, c), np.uint8)})
    v, f, _, _ = R.keep_faces(np.ones(len(F), bool), V, F)
    res["unreferenced_v"], res["unreferenced_f"] = v, f
    comp, C = R.numbering(R.labels(F))
    res["mesh_area"] = np.array(R.total_area(R.stats(V, F, comp, C)[2]))
    return res


def same(got, want):
    """every array of `want` is in `got` with the same shape, type and bytes -> list of the names that differ.  A NaN equals a NaN
    whatever its sign and payload: 0 x Inf gives the default NaN, whose sign bit the host and the device choose differently."""
    bad = []
    for k, w in want.items():
        g = got.get(k)
        w = np.asarray(w)
        if g is None or g.shape != w.shape or g.dtype != w.dtype:
            bad.append(k)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)          # (0-d arrays become 1-d here, both of them)
        if w.dtype.kind == "f":
            nan = np.isnan(w)
            if not np.array_equal(nan, np.isnan(g)) or np.where(nan, 0, g).tobytes() != np.where(nan, 0, w).tobytes():
                bad.append(k)
        elif g.tobytes() != w.tobytes():
            bad.append(k)
    return bad
