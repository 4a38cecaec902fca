"""CPU tests of the mesh simplification: the kernels of csrc/mesh_simplify.hip through the host emulator (tests/hipemu)
behind mesh_simplify's own Python layer and DeviceMesh.simplify, each group of cases in a child process, held to
tests/mesh_simplify_restatement.py with equalities: vertex_cluster, the cluster count, positions bit for bit, colours, used_mean, kept
faces and exported bytes.  Independently of the restatement: identity below the vertex spacing, the structure of the output, locality,
the flat grid's plane, the quadric objective, determinism over runs and workspace contents, and the target search.

In the child the product modules run unchanged except for their test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context are host stand-ins, and EVERY buffer the modules allocate (workspaces and outputs) is filled with 0xA5 and
followed by guard bytes that are checked after the run."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import mesh_simplify_cases as K  # noqa: E402
import mesh_simplify_restatement as R  # noqa: E402
import mesh_components_restatement as RC  # noqa: E402

FILLS = ((0x00, 0), (0xA5, 0), (0xFF, 0), (0xA5, 1))          # (byte value of every workspace and output, which run with it)
MESHES = {"icosphere": K.icosphere, "torus": K.torus, "flat": K.flat_grid, "small_soup": lambda: K.soup(20000, 8000)}
GROUP_MESHES = dict(MESHES, identity=K.identity, soup=K.soup)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def tiling():
    import mesh_simplify
    return mesh_simplify.tiling()


def group_cases(kind, name):
    """-> [(tag, case)] of one child"""
    if kind == "hand":
        return list(K.hand_cases().items())
    if kind == "mesh":
        return [(name, GROUP_MESHES[name]())]
    if kind == "fans":
        small, large = K.fan_sizes(tiling())
        return [("fan%d" % n, K.fan(n)) for n in (small if name == "tile" else (large[int(name)],))]
    if kind == "counts":
        return [("cloud%d" % n, K.cloud_strip(n)) for n in K.boundary_vertex_counts(tiling())]
    raise KeyError(kind)


def _flatten(tag, res):
    return {"%s_%s" % (tag, k): v for k, v in res.items()}


def want_group(kind, name):
    out = {}
    for tag, case in group_cases(kind, name):
        out.update(_flatten(tag, K.want(case, ply=True, key=tag)))
        if kind == "hand":
            out.update(_flatten(tag + "_all", K.want(case, dedupe=False, key=tag)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the child: mesh_simplify over the emulated library
# ---------------------------------------------------------------------------------------------------------------------------
def _seams():
    import mesh_cull as M
    import mesh_components as MC
    import mesh_render as MR
    import mesh_simplify as MS
    return M, MS, host_child.install_seams(M, MC, MR, MS, buffers="all")


def _refusal(f):
    try:
        f()
        return np.array("")
    except (RuntimeError, ValueError) as e:
        return np.array(str(e))


def _child(case, out):
    M, MS, check = _seams()
    kind, name = case.split(":", 1)
    tmp = os.path.dirname(out)
    res = {}
    if kind in ("hand", "mesh", "fans", "counts"):
        for tag, c in group_cases(kind, name):
            res.update(_flatten(tag, K.run(MS, M, _up, c, ply=os.path.join(tmp, tag + ".ply"))))
            if kind == "hand":
                res.update(_flatten(tag + "_all", K.run(MS, M, _up, c, dedupe=False)))
    elif kind == "fills":
        c = K.soup(3000, 1500)
        for fill, again in FILLS:
            res.update(_flatten("%02x_%d" % (fill, again), K.run_filled(MS, _up, c, fill)))
    elif kind == "errors":
        import ctypes as C
        import torch
        for tag, (c, _) in K.refusals().items():
            V, F, _, _, h, origin = c
            res[tag] = _refusal(lambda: MS.simplify(_up(V), _up(F), cell=h, origin=origin))
            res[tag + "_mesh"] = _refusal(lambda: M.DeviceMesh(V, F).simplify(cell=h, origin=origin))
        # nothing written on a refused call: poisoned outputs stay poisoned
        L = MS.lib
        V, F, _, _, h, _ = K.hand_cases()["one_triangle"]
        o = (C.c_double * 3)(0.0, 0.0, 0.0)
        vc_good, nc = MS.cluster(_up(V), h, (0.0, 0.0, 0.0))
        bad_v, bad_f, bad_vc = V.copy(), F.copy(), vc_good.clone()
        bad_v[2, 1], bad_f[0, 0], bad_vc[1] = np.nan, 3, nc

        def poisoned(n, dt):
            return torch.full((n,), 0x5C, dtype=dt)
        nb = 1 << 16
        for tag, v, hh in (("cluster_nan", bad_v, h), ("cluster_range", V, 2.0 ** -23), ("cluster_h", V, 0.0)):
            ws, vc, n = poisoned(nb, torch.uint8), poisoned(3, torch.int32), C.c_int64(-7)
            rc = L.gof_mesh_cluster(3, _up(v).data_ptr(), o, hh, vc.data_ptr(), C.byref(n), ws.data_ptr(), nb, None)
            res[tag] = np.array("%d %s" % (rc, L.gof_last_error().decode()))
            res[tag + "_untouched"] = np.array(bool((vc == 0x5C).all() and n.value == 0))
        for tag, v, f, vc in (("solve_index", V, bad_f, vc_good), ("solve_nan", bad_v, F, vc_good), ("solve_cluster", V, F, bad_vc)):
            ws, pos, used, n = poisoned(nb, torch.uint8), poisoned(3 * nc, torch.int64), poisoned(nc, torch.uint8), C.c_int64(-7)
            rc = L.gof_mesh_cluster_solve(3, 1, _up(v).data_ptr(), _up(f).data_ptr(), None, vc.data_ptr(), nc, o, h, pos.data_ptr(), None, used.data_ptr(), C.byref(n),
                                          ws.data_ptr(), nb, None)
            res[tag] = np.array("%d %s" % (rc, L.gof_last_error().decode()))
            res[tag + "_untouched"] = np.array(bool((pos == 0x5C).all() and (used == 0x5C).all() and n.value == 0))
        for tag, f, vc in (("faces_index", bad_f, vc_good), ("faces_cluster", F, bad_vc)):
            ws, cf, keep = poisoned(nb, torch.uint8), poisoned(3, torch.int32), poisoned(1, torch.uint8)
            counts = (C.c_int64 * 2)(-7, -7)
            rc = L.gof_mesh_cluster_faces(3, 1, _up(f).data_ptr(), vc.data_ptr(), nc, 1, cf.data_ptr(), keep.data_ptr(), counts, ws.data_ptr(), nb, None)
            res[tag] = np.array("%d %s" % (rc, L.gof_last_error().decode()))
            res[tag + "_untouched"] = np.array(bool((cf == 0x5C).all() and (keep == 0x5C).all() and counts[0] == 0 and counts[1] == 0))
    elif kind == "target":
        V, F, N, Col, _, _ = K.torus()
        for target in (1, 50, 700, len(V), 10 * len(V)):
            mesh = M.DeviceMesh(V, F, N, Col)
            st = mesh.simplify(target_vertices=target)
            again = M.DeviceMesh(V, F, N, Col)
            st2 = again.simplify(cell=st["cell"])
            res["t%d" % target] = np.array([st["clusters"], st2["clusters"], len(st["probes"]), st["vertices_after"], st2["vertices_after"]])
            res["t%d_cell" % target] = np.array([st["cell"]] + [p for p, _ in st["probes"]])
            res["t%d_probed" % target] = np.array([n for _, n in st["probes"]])
            res["t%d_same" % target] = np.array(bool(np.array_equal(mesh.vertices, again.vertices) and np.array_equal(mesh.faces, again.faces)))
        o = (V.min(axis=0) - 0.013).tolist()                     # a caller's origin: the probes count with it
        mesh = M.DeviceMesh(V, F, N, Col)
        st = mesh.simplify(target_vertices=300, origin=o)
        res["origin"] = np.array([st["clusters"]] + [n for _, n in st["probes"]])
        res["origin_cell"] = np.array([st["cell"]] + [p for p, _ in st["probes"]])
        res["origin_outside"] = _refusal(lambda: M.DeviceMesh(V, F).simplify(target_vertices=300, origin=(V.min(axis=0) + 0.5).tolist()))
        mesh = M.DeviceMesh(V, F, N, Col)
        st = mesh.simplify(grid=16)
        res["grid"] = np.array([st["cell"], float(st["clusters"])])
        res["one_of"] = _refusal(lambda: mesh.simplify(cell=0.1, grid=4))
        res["none_of"] = _refusal(lambda: mesh.simplify())
    elif kind == "cli":
        import tsdf_fusion
        V, F, N, Col, h, _ = K.icosphere(3)
        files = {"coloured": (N, Col), "plain": (None, None)}
        for tag, (n, c) in files.items():
            M.DeviceMesh(V, F, n, c).export(os.path.join(tmp, tag + ".ply"))
        tsdf_fusion.write_ply(os.path.join(tmp, "tsdf.ply"), V, F, Col / 255.0, N)
        for tag in list(files) + ["tsdf"]:
            assert MS.main([os.path.join(tmp, tag + ".ply"), os.path.join(tmp, tag + "_out.ply"), "--cell", "0.3", "--stats", os.path.join(tmp, tag + ".json")]) == 0
            res[tag + "_ply"] = np.frombuffer(open(os.path.join(tmp, tag + "_out.ply"), "rb").read(), np.uint8)
            res[tag + "_stats"] = np.array(open(os.path.join(tmp, tag + ".json")).read())
        assert MS.main([os.path.join(tmp, "coloured.ply"), os.path.join(tmp, "all_out.ply"), "--grid", "6", "--no-dedupe"]) == 0
        res["all_ply"] = np.frombuffer(open(os.path.join(tmp, "all_out.ply"), "rb").read(), np.uint8)
        # the simplified file is a mesh the other tools read
        import mesh_components as MC
        import mesh_render as MR
        back = M.load(os.path.join(tmp, "coloured_out.ply"))
        res["back_components"] = np.array(len(back.components()))
        res["back_normals"] = MR.vertex_normals(back).cpu().numpy()
        res["stats"] = np.array(json.dumps(MS.last_stats()))
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **{k: v for k, v in res.items() if v is not None})


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=1800)
    assert int(res["buffers"]) > 0
    return res


def _check_group(kind, name, tmp_path):
    want = want_group(kind, name)
    got = _emulate("%s:%s" % (kind, name), tmp_path)
    assert K.same(got, want) == []
    for tag, case in group_cases(kind, name):
        g = {k[len(tag) + 1:]: v for k, v in got.items() if k.startswith(tag + "_") and not k.startswith(tag + "_all_")}
        assert K.properties(case, g) == [], tag
        assert K.quadric_holds(case, g)[0], tag
    return got


# ---------------------------------------------------------------------------------------------------------------------------
def test_hand_built_cases(tmp_path):
    got = _check_group("hand", "all", tmp_path)
    # the cases bite
    assert got["empty_counts"].tolist() == [0, 0, 0, 0] and got["empty_v"].shape == (0, 3) and got["no_faces_v"].shape == (0, 3) and int(got["no_faces_counts"][0]) > 1
    assert got["one_triangle_f"].tolist() == [[0, 1, 2]] and got["one_triangle_counts"].tolist() == [3, 3, 0, 0]
    assert got["repeated_index_face_keep"].tolist() == [1, 0, 0] and got["zero_area_face_keep"].tolist() == [1, 1]
    assert got["opposite_face_keep"].tolist() == [1, 0, 0] and got["opposite_all_face_keep"].tolist() == [1, 1, 1] and got["opposite_f"].tolist() == [[0, 1, 2]]
    assert got["opposite_counts"].tolist()[2:] == [0, 2] and got["opposite_all_cluster_faces"].tolist()[1] == [2, 1, 0]       # the second face keeps its orientation
    assert got["on_a_boundary_vertex_cluster"].tolist() == [0, 1, 2, 3] and got["on_a_boundary_f"].tolist() == [[0, 2, 3], [1, 2, 3]]
    V, F = K.hand_cases()["zero_area"][:2]
    assert not R.corner_quadrics(V, F, np.zeros((6, 3)))[3:].any() and R.corner_quadrics(V, F, np.zeros((6, 3)))[:3, 0].all()
    assert got["one_cell_counts"].tolist() == [1, 0, 7, 0] and got["one_cell_f"].shape == (0, 3) and got["one_cell_cluster_vertices"].shape == (1, 3)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_meshes(name, tmp_path):
    got = _check_group("mesh", name, tmp_path)
    case = MESHES[name]()
    assert 8 < int(got[name + "_counts"][0]) < len(case[0]) // 2 and 0 < len(got[name + "_f"]) < len(case[1])
    if name == "icosphere":
        assert len(case[1]) == 20480 and K.quadric_holds(case, {k[len(name) + 1:]: v for k, v in got.items()})[1] > 50
        assert 0 < int(got[name + "_counts"][1]) < int(got[name + "_counts"][0]) and int(got[name + "_counts"][3]) > 0          # both roads of the solve, duplicates
    if name == "flat":
        # every output vertex on the plane within 2^-40 x extent (extent: the largest side of the bounding box)
        extent = np.ptp(case[0], axis=0).max()
        assert (np.abs(got["flat_v"] @ K.FLAT_NORMAL - 0.25) <= 2.0 ** -40 * extent).all()


def test_fans_at_the_tile_boundaries(tmp_path):
    t = tiling()
    got = _check_group("fans", "tile", tmp_path)
    for n in K.fan_sizes(t)[0]:
        assert int(got["fan%d_used_mean" % n][0]) == 0
        assert np.count_nonzero(got["fan%d_vertex_cluster" % n][K.fan(n)[1].reshape(-1)] == 0) == n and n in (t["sum_tile"] - 1, t["sum_tile"], t["sum_tile"] + 1)


@pytest.mark.parametrize("which", range(3))
def test_fans_at_the_block_boundaries(which, tmp_path):
    n = K.fan_sizes(tiling())[1][which]
    got = _check_group("fans", str(which), tmp_path)
    assert int(got["fan%d_used_mean" % n][0]) == 0
    assert np.count_nonzero(got["fan%d_vertex_cluster" % n][K.fan(n)[1].reshape(-1)] == 0) == n == tiling()["sum_block"] - 1 + which


def test_vertex_counts_at_the_sort_and_scan_boundaries(tmp_path):
    t = tiling()
    counts = K.boundary_vertex_counts(t)
    assert t["sort_block"] in counts and t["scan_tile"] - 1 in counts
    _check_group("counts", "all", tmp_path)


def test_identity_below_the_vertex_spacing(tmp_path):
    """a cell below the smallest coordinate spacing: vertices (bit for bit: a cell of one vertex keeps it), faces, colours and order
    come back equal"""
    got = _check_group("mesh", "identity", tmp_path)
    V, F, N, Col, _, _ = K.identity()
    assert np.array_equal(got["identity_vertex_cluster"], np.arange(len(V))) and np.array_equal(got["identity_f"], F) and np.array_equal(got["identity_c"], Col)
    assert got["identity_v"].tobytes() == V.tobytes() and got["identity_cluster_vertices"].tobytes() == V.tobytes()
    assert got["identity_counts"].tolist() == [len(V), len(V), 0, 0]


def test_the_soup_of_200000_faces(tmp_path):
    got = _check_group("mesh", "soup", tmp_path)
    assert len(K.soup()[1]) == 200000 and int(got["soup_counts"][0]) == 4096 and int(got["soup_counts"][2]) > 100 and int(got["soup_counts"][3]) > 0


def test_runs_and_workspace_contents_do_not_matter(tmp_path):
    got = host_child.run_child(__file__, "fills:all", tmp_path, timeout=1800)          # (the C ABI over buffers of the case's own)
    want = K.want_filled(K.soup(3000, 1500))
    for fill, again in FILLS:
        p = "%02x_%d_" % (fill, again)
        assert K.same({k[len(p):]: v for k, v in got.items() if k.startswith(p)}, want) == [], p


def test_bad_input_is_refused_with_nothing_written(tmp_path):
    res = _emulate("errors:all", tmp_path)
    for tag, (_, word) in K.refusals().items():
        assert word in str(res[tag]), (tag, str(res[tag]))
        assert word in str(res[tag + "_mesh"]), tag
    for tag, text in (("cluster_nan", "not finite"), ("cluster_range", "2^21"), ("cluster_h", "cell size"), ("solve_index", "outside [0, 3)"), ("solve_nan", "not finite"),
                      ("solve_cluster", "cluster number"), ("faces_index", "outside [0, 3)"), ("faces_cluster", "cluster number")):
        assert str(res[tag]).startswith("-") and text in str(res[tag]), (tag, str(res[tag]))
        assert bool(res[tag + "_untouched"]), tag


def test_target_search_and_grid(tmp_path):
    res = _emulate("target:all", tmp_path)
    V = K.torus()[0]
    extent = np.ptp(V, axis=0).max()
    for target in (1, 50, 700, len(V), 10 * len(V)):
        clusters, again, probes, va, va2 = res["t%d" % target].tolist()
        cells, probed = res["t%d_cell" % target], res["t%d_probed" % target]
        assert clusters <= target and again == clusters and va == va2 and bool(res["t%d_same" % target]) and 1 <= probes <= 24
        assert cells[1] == 2.0 * extent and probed[0] == 1 and (cells[1:] >= extent * 2.0 ** -20).all()
        assert cells[0] == cells[1:][probed <= target].min()                                  # the smallest probed h that meets the target
        assert [R.cluster(V, h)[1] for h in cells[1:4]] == probed[:3].tolist()
    o = V.min(axis=0) - 0.013
    assert res["origin"][0] <= 300 and res["origin"][0] == R.cluster(V, res["origin_cell"][0], o)[1] and "2^21" in str(res["origin_outside"])
    assert [R.cluster(V, h, o)[1] for h in res["origin_cell"][1:]] == res["origin"][1:].tolist()
    assert res["t700"][0] > 350                                                                # the search comes close, not just below
    assert res["grid"][0] == extent / 16 and res["grid"][1] == R.cluster(V, extent / 16)[1]
    assert "exactly one" in str(res["one_of"]) and "exactly one" in str(res["none_of"])


def test_command_line_round_trips_and_writes_the_stats(tmp_path):
    res = _emulate("cli:all", tmp_path)
    V, F, N, Col, _, _ = K.icosphere(3)
    V32 = V.astype(np.float32).astype(np.float64)                                             # what the file holds
    tsdf_colours = np.round(np.clip(Col / 255.0, 0.0, 1.0) * 255.0).astype(np.uint8)
    for tag, (n, c) in {"coloured": (N, Col), "plain": (None, None), "tsdf": (N, tsdf_colours)}.items():
        r = R.simplify(V32, F, n, c, 0.3)
        assert res[tag + "_ply"].tobytes() == R.ply_bytes(r["v"], r["f"], r["n"], r["c"]), tag
        st = json.loads(str(res[tag + "_stats"]))
        assert st["vertices_before"] == len(V) and st["faces_after"] == len(r["f"]) and st["cell"] == 0.3 and st["clusters"] == r["clusters"]
        assert st["used_mean"] == int(r["used_mean"].sum()) and st["dropped_degenerate"] == r["dropped_degenerate"] and st["dropped_duplicate"] == r["dropped_duplicate"]
    h = np.ptp(V32, axis=0).max() / 6.0
    r = R.simplify(V32, F, N, Col, h, dedupe=False)
    assert res["all_ply"].tobytes() == R.ply_bytes(r["v"], r["f"], r["n"], r["c"]) and r["dropped_duplicate"] == 0
    r = R.simplify(V32, F, N, Col, 0.3)
    assert int(res["back_components"]) == RC.numbering(RC.labels(r["f"]))[1] and res["back_normals"].shape == (len(r["v"]), 3)
    assert json.loads(str(res["stats"]))["mesh"]["dedupe"] is False


# ---- without the emulator ----------------------------------------------------------------------------------------------------
def test_the_restatement_sums_in_the_written_order():
    """the vectorised runs of the restatement against the scalar loop of the components' restatement, over two blocks"""
    rng = np.random.default_rng(3)
    keys = np.sort(np.concatenate([np.zeros(300, np.int64), rng.integers(1, 40, 2000), np.full(70000, 40), np.full(5, 42)]))
    a = rng.uniform(-1, 1, len(keys)) * 10.0 ** rng.integers(-8, 8, len(keys))
    got = R.segment_sums(a[:, None], keys, 44)[:, 0]
    start = np.searchsorted(keys, np.arange(45))
    want = [RC.segment_sum(a.tolist(), int(start[c]), int(start[c + 1])) if start[c + 1] > start[c] else 0.0 for c in range(44)]
    assert got.tolist() == want and got[41] == 0.0 and got[43] == 0.0
    assert got[40] != np.sum(a[keys == 40]) or got[40] != float(np.cumsum(a[keys == 40])[-1])       # the order matters at this size


def test_host_tensors_are_refused():
    import torch
    import mesh_simplify as MS
    with pytest.raises(RuntimeError, match="ROCm device"):
        MS.cluster(torch.zeros((3, 3), dtype=torch.float64), 0.5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        MS.simplify(torch.zeros((3, 3), dtype=torch.float64), torch.zeros((1, 3), dtype=torch.int32), cell=0.5)


def test_size_queries_and_argument_checks():
    import ctypes as C
    import mesh_simplify as MS
    import mesh_cull
    L = MS.lib
    assert L.gof_mesh_simplify_abi_version() == 5 and L.gof_mesh_render_abi_version() == 4 and L.gof_mesh_abi_version() == 2 and L.gof_abi_version() == 12
    assert 0 < L.gof_mesh_cluster_ws_bytes(0) < L.gof_mesh_cluster_ws_bytes(1000)
    assert 0 < L.gof_mesh_cluster_solve_ws_bytes(0, 0, 0) < L.gof_mesh_cluster_solve_ws_bytes(1000, 2000, 10) < L.gof_mesh_cluster_solve_ws_bytes(1000, 2000, 1000)
    # no 80 bytes per corner: 3 * 10^7 faces stay below 64 bytes per face besides the clusters' own sums
    assert L.gof_mesh_cluster_solve_ws_bytes(15_000_000, 30_000_000, 0) < 64 * 30_000_000
    assert 0 < L.gof_mesh_cluster_faces_ws_bytes(0) < L.gof_mesh_cluster_faces_ws_bytes(1000)
    o, n = (C.c_double * 3)(0.0, 0.0, 0.0), C.c_int64(5)
    assert L.gof_mesh_cluster(-1, None, o, 1.0, None, C.byref(n), None, 0, None) < 0 and n.value == 0
    assert L.gof_mesh_cluster(3, None, o, 1.0, None, None, None, 0, None) < 0
    assert L.gof_mesh_cluster(3, None, None, 1.0, None, C.byref(n), None, 0, None) < 0
    assert L.gof_mesh_cluster_solve(3, (2 ** 31 + 2) // 3, None, None, None, None, 1, o, 1.0, None, None, None, None, None, 0, None) < 0 and b"2^31" in L.gof_last_error()
    assert L.gof_mesh_cluster_faces(3, (2 ** 31 + 2) // 3, None, None, 1, 1, None, None, None, None, 0, None) < 0 and b"2^31" in L.gof_last_error()
    assert L.gof_mesh_cluster_faces(3, 1, None, None, 4, 1, None, None, None, None, 0, None) < 0
    t = MS.tiling()
    assert set(t) == {"sort_block", "scan_tile", "sum_tile", "sum_block"} and t["sum_tile"] == R.SUM_TILE and t["sum_block"] == R.SUM_BLOCK
    assert hasattr(mesh_cull.DeviceMesh, "simplify")


def test_spec_parsing():
    import mesh_simplify as MS
    assert MS.parse_spec("grid:1024") == {"grid": 1024.0} and MS.parse_spec("target_vertices:2000000") == {"target_vertices": 2000000}
    assert MS.parse_spec(" cell:0.01 , dedupe:0 ") == {"cell": 0.01, "dedupe": False} and MS.parse_spec("target-vertices:5") == {"target_vertices": 5}
    for bad in ("grid", "grid:x", "cells:3", "grid:4,grid:5", "grid:4,cell:0.1", "dedupe:1", "cell:0", "cell:nan", "grid:0.5", "target_vertices:0", "grid:4,dedupe:2",
                "grid:4,,", ""):
        with pytest.raises(ValueError, match="GOF_MESH_SIMPLIFY"):
            MS.parse_spec(bad)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
