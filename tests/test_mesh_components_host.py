"""CPU tests of the mesh connected components: the kernels of csrc/mesh_components.hip through the host emulator
(tests/hipemu) behind mesh_components' own Python layer and DeviceMesh's methods, each group of cases in a child process, held to
tests/mesh_components_restatement.py with equalities: labels, component numbers, counts, first faces, areas bit for bit, kept meshes
and exported bytes.  Independently of the restatement's union-find the labels are held to SciPy's connected components.

In the child the product modules run unchanged except for their test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context are host stand-ins, and EVERY buffer mesh_components and mesh_cull allocate (workspaces and outputs) is filled
with 0xA5 and followed by guard bytes that are checked after the run."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import mesh_components_cases as K  # noqa: E402
import mesh_components_restatement as R  # noqa: E402

STRIP_GROUPS = 4
FILLS = ((0x00, 0), (0xA5, 0), (0xFF, 0), (0xA5, 1))          # (byte value of every workspace and output, which run with it)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def tiling():
    import mesh_components
    return mesh_components.tiling()


def group_cases(kind, name):
    """-> [(tag, V, F)] of one child"""
    if kind == "hand":
        cases = [(k, V, F) for k, (V, F) in K.hand_cases().items()]
        return cases + [("nan",) + K.nan_case(), ("inf",) + K.inf_case()]
    if kind == "strips":
        sizes = K.strip_sizes(tiling())
        return [("strip%d" % n,) + K.strip_case(n) for n in sizes[int(name)::STRIP_GROUPS]]
    if kind == "deep":
        return [("deep",) + K.deep_chain()]
    if kind == "floaters":
        return [("floaters",) + K.floaters()]
    if kind == "block":
        return [("block",) + K.strip_case(K.block_strip_size(tiling()))]
    raise KeyError(kind)


def want_group(kind, name, modes=K.MODES):
    return {"%s_%s_%s" % (tag, mode, k): v for tag, V, F in group_cases(kind, name) for mode in modes for k, v in K.want(V, F, mode).items()}


def _modes(kind):
    return ("edge",) if kind == "block" else K.MODES          # (the block case is about the area sums: one mode)


# ---------------------------------------------------------------------------------------------------------------------------
# the child: mesh_components over the emulated library
# ---------------------------------------------------------------------------------------------------------------------------
def _child(case, out):
    import mesh_cull as M
    import mesh_components as MC
    check = host_child.install_seams(M, MC, buffers="all")
    kind, name = case.split(":", 1)
    tmp = os.path.dirname(out)
    res = {}
    if kind in ("hand", "strips", "deep", "floaters", "block"):
        for tag, V, F in group_cases(kind, name):
            for mode in _modes(kind):
                res.update({"%s_%s_%s" % (tag, mode, k): v for k, v in K.run(MC, _up, V, F, mode).items()})
    elif kind == "fills":
        V, F = K.floaters(2000, 300)
        for mode in K.MODES:
            for fill, again in FILLS:
                res.update({"%s_%02x_%d_%s" % (mode, fill, again, k): v for k, v in K.run_filled(MC, _up, V, F, mode, fill).items()})
    elif kind == "keep":
        res = K.run_keep(M, lambda name: os.path.join(tmp, name + ".ply"))
    elif kind == "errors":
        import ctypes as C
        import torch
        V, F = K.strip_case(300)
        for tag, bad in (("high", len(V)), ("negative", -1)):
            f = F.copy()
            f[123, 2] = bad
            for mode in K.MODES:
                try:
                    MC.face_components(_up(f), len(V), mode)
                    res[tag + mode] = np.array("")
                except RuntimeError as e:
                    res[tag + mode] = np.array(str(e))
        # nothing written on a refused call: poisoned outputs stay poisoned (bad index; 3 NF >= 2^31)
        f = F.copy()
        f[7, 0] = len(V)
        L = MC.lib
        for tag, nf, mode in (("index_edge", len(f), 0), ("index_vertex", len(f), 1), ("toomany", (2 ** 31 + 2) // 3, 0), ("mode", len(f), 2)):
            nb = 1 << 20 if tag == "toomany" else max(L.gof_mesh_components_ws_bytes(len(V), len(f), mode), 1 << 16)
            ws, label, comp = torch.full((nb,), 0x5C, dtype=torch.uint8), torch.full((len(f),), 0x5C5C5C5C, dtype=torch.int32), torch.full((len(f),), 0x5C5C5C5C, dtype=torch.int32)
            count = C.c_int64(-7)
            rc = L.gof_mesh_components(len(V), nf, _up(f).data_ptr(), mode, label.data_ptr(), comp.data_ptr(), C.byref(count), ws.data_ptr(), nb, None)
            res[tag] = np.array("%d %s" % (rc, L.gof_last_error().decode()))
            res[tag + "_untouched"] = np.array(bool((label == 0x5C5C5C5C).all() and (comp == 0x5C5C5C5C).all() and count.value == 0))
        comp, cnt = MC.face_components(_up(F), len(V))
        for tag, fc, ff in (("stats_comp", comp + 1, F), ("stats_index", comp, f)):
            cf, first, area = (torch.full((int(cnt),), 0x5C, dtype=dt) for dt in (torch.int64, torch.int32, torch.int64))
            nb = L.gof_mesh_component_stats_ws_bytes(len(F), int(cnt))
            ws = torch.empty(nb, dtype=torch.uint8)
            rc = L.gof_mesh_component_stats(len(V), len(F), _up(V).data_ptr(), _up(ff).data_ptr(), fc.contiguous().data_ptr(), int(cnt), cf.data_ptr(), first.data_ptr(),
                                            area.data_ptr(), ws.data_ptr(), nb, None)
            res[tag] = np.array("%d %s" % (rc, L.gof_last_error().decode()))
            res[tag + "_untouched"] = np.array(bool((cf == 0x5C).all() and (first == 0x5C).all() and (area == 0x5C).all()))
    elif kind == "cli":
        import tsdf_fusion
        V, F, N, Col = K.keep_mesh()
        files = {"coloured": (N, Col), "colours_only": (None, Col), "plain": (None, None)}
        for tag, (n, c) in files.items():
            M.DeviceMesh(V, F, n, c).export(os.path.join(tmp, tag + ".ply"))
        tsdf_fusion.write_ply(os.path.join(tmp, "tsdf.ply"), V, F, Col / 255.0, N)
        for tag in list(files) + ["tsdf"]:
            rc = MC.main([os.path.join(tmp, tag + ".ply"), os.path.join(tmp, tag + "_out.ply"), "--largest", "2", "--by", "area", "--table",
                          os.path.join(tmp, tag + ".json")])
            assert rc == 0
            res[tag + "_ply"] = np.frombuffer(open(os.path.join(tmp, tag + "_out.ply"), "rb").read(), np.uint8)
            res[tag + "_table"] = np.array(open(os.path.join(tmp, tag + ".json")).read())
        MC.main([os.path.join(tmp, "coloured.ply"), os.path.join(tmp, "vertex_out.ply"), "--min-faces", "2", "--connectivity", "vertex"])
        res["vertex_ply"] = np.frombuffer(open(os.path.join(tmp, "vertex_out.ply"), "rb").read(), np.uint8)
        res["stats"] = np.array(json.dumps(MC.last_stats()))
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=1800)
    assert int(res["buffers"]) > 0
    return res


def _check_group(kind, name, tmp_path):
    want = want_group(kind, name, _modes(kind))
    got = _emulate("%s:%s" % (kind, name), tmp_path)
    assert K.same(got, want) == []
    for tag, V, F in group_cases(kind, name):
        for mode in _modes(kind):
            p = "%s_%s_" % (tag, mode)
            g = {k: got[p + k] for k in ("label", "comp", "count", "faces", "area")}
            assert np.array_equal(g["label"], R.scipy_labels(F, mode)), p                     # the labels by another road
            assert K.area_bound_holds(V, F, g), p
    return got


# ---------------------------------------------------------------------------------------------------------------------------
def test_hand_built_cases(tmp_path):
    got = _check_group("hand", "all", tmp_path)
    # the cases bite
    assert int(got["shared_vertex_edge_count"]) == 2 and int(got["shared_vertex_vertex_count"]) == 1
    assert got["three_on_an_edge_edge_comp"].tolist() == [0, 1, 0, 0] and got["duplicated_face_edge_comp"].tolist() == [0, 1, 0, 0]
    assert got["face_aab_edge_comp"].tolist() == [0, 1, 2, 0] and got["face_aab_vertex_comp"].tolist() == [0, 0, 1, 0]
    assert got["face_aaa_edge_comp"].tolist() == [0, 1, 0, 2, 3] and got["face_aaa_vertex_comp"].tolist() == [0, 1, 0, 2, 2]
    assert int(got["two_tetrahedra_edge_count"]) == 2 and got["two_tetrahedra_edge_faces"].tolist() == [4, 4]
    assert int(got["no_faces_edge_count"]) == 0 and int(got["nothing_vertex_count"]) == 0 and got["one_face_edge_first"].tolist() == [0]
    # a NaN (an infinite) vertex: the labels of the clean mesh, that component's area NaN (NaN or Inf), the other's a number
    for mode in K.MODES:
        assert np.array_equal(got["nan_%s_label" % mode], got["two_tetrahedra_%s_label" % mode])
        assert np.isnan(got["nan_%s_area" % mode][1]) and np.isfinite(got["nan_%s_area" % mode][0])
        assert not np.isfinite(got["inf_%s_area" % mode][0]) and np.isfinite(got["inf_%s_area" % mode][1])


@pytest.mark.parametrize("group", range(STRIP_GROUPS))
def test_strips_at_every_boundary(group, tmp_path):
    t = tiling()
    sizes = K.strip_sizes(t)
    assert set(K.STRIP_SIZES) <= set(sizes) and any(3 * n < t["sort_block"] <= 3 * (n + 1) for n in sizes) and t["scan_tile"] - 1 in sizes
    got = _check_group("strips", str(group), tmp_path)
    for n in sizes[group::STRIP_GROUPS]:
        assert int(got["strip%d_edge_count" % n]) == 1 and got["strip%d_vertex_faces" % n].tolist() == [n]


def test_deep_chain(tmp_path):
    got = _check_group("deep", "all", tmp_path)
    assert int(got["deep_edge_count"]) == 1 and not got["deep_edge_label"].any()


def test_floaters(tmp_path):
    got = _check_group("floaters", "all", tmp_path)
    assert int(got["floaters_edge_count"]) == 3001 and got["floaters_edge_faces"].max() == 50000 and got["floaters_edge_faces"].min() == 1


def test_a_component_across_two_blocks_of_the_area_sums(tmp_path):
    got = _check_group("block", "all", tmp_path)
    assert got["block_edge_faces"].tolist() == [K.block_strip_size(tiling())]


def test_runs_and_workspace_contents_do_not_matter(tmp_path):
    V, F = K.floaters(2000, 300)
    got = host_child.run_child(__file__, "fills:all", tmp_path, timeout=1800)          # (the C ABI over buffers of the case's own)
    for mode in K.MODES:
        want = {k: v for k, v in K.want(V, F, mode).items() if not k.endswith("_again")}
        for fill, again in FILLS:
            p = "%s_%02x_%d_" % (mode, fill, again)
            assert K.same({k[len(p):]: v for k, v in got.items() if k.startswith(p)}, want) == [], p


def test_keep_components_equals_boolean_indexing(tmp_path):
    want = K.want_keep()
    # the table bites: ties in the face counts and in the areas, strays, every criterion keeps something different
    assert want["largest1_counts"].tolist() == [1, 5] and want["largest2_tie_counts"].tolist() == [2, 4] and len(want["largest1_f"]) == 40
    assert len(want["largest3_tie_f"]) == 92 and len(want["largest3_area_tie_f"]) == 92 and len(want["largest0_v"]) == 0
    assert not np.array_equal(want["largest1_v"], want["largest1_area_v"]) and want["ratio_counts"].tolist() == [1, 5]
    assert want["vertex_min_faces_counts"].tolist() == [5, 1] and len(want["unreferenced_v"]) == len(K.keep_mesh()[0]) - 12
    got = _emulate("keep:all", tmp_path)
    assert K.same(got, want) == []


def test_bad_input_is_refused_with_nothing_written(tmp_path):
    res = _emulate("errors:all", tmp_path)
    for mode in K.MODES:
        assert "outside [0, 302)" in str(res["high" + mode]) and "outside [0, 302)" in str(res["negative" + mode])
    for tag, text in (("index_edge", "outside [0, 302)"), ("index_vertex", "outside [0, 302)"), ("toomany", "2^31"), ("mode", "mode"),
                      ("stats_comp", "component number"), ("stats_index", "outside [0, 302)")):
        assert str(res[tag]).startswith("-") and text in str(res[tag]), (tag, str(res[tag]))
        assert bool(res[tag + "_untouched"]), tag


def test_command_line_round_trips_and_writes_the_table(tmp_path):
    res = _emulate("cli:all", tmp_path)
    V, F, N, Col = K.keep_mesh()
    for tag, (n, c) in {"coloured": (N, Col), "colours_only": (None, Col), "plain": (None, None), "tsdf": (N, Col)}.items():
        v, f, n2, c2, kept, dropped = R.keep_components(V, F, n, c, largest=2, by="area")
        assert res[tag + "_ply"].tobytes() == R.ply_bytes(v, f, n2, c2), tag
        table = json.loads(str(res[tag + "_table"]))
        comp, C = R.numbering(R.labels(F))
        cf, first, area = R.stats(V, F, comp, C)
        assert table["components"] == 6 and table["faces"] == cf.tolist() and table["area"] == area.tolist() and table["first_face"] == first.tolist()
        assert table["kept"] == R.select(cf, area, largest=2, by="area").tolist() and table["connectivity"] == "edge"
    v, f, n2, c2, _, _ = R.keep_components(V, F, N, Col, min_faces=2, connectivity="vertex")
    assert res["vertex_ply"].tobytes() == R.ply_bytes(v, f, n2, c2)
    st = json.loads(str(res["stats"]))
    assert st["components"]["connectivity"] == "vertex" and st["keep"]["kept"] == 5 and st["stats"]["components"] == 6 and st["components"]["workspace_bytes"] > 0


# ---- without the emulator ----------------------------------------------------------------------------------------------------
def test_restatement_and_scipy_agree_on_the_soup():
    V, F = K.soup(20000)
    for mode in K.MODES:
        label = R.labels(F, mode)
        assert np.array_equal(label, R.scipy_labels(F, mode))
        comp, C = R.numbering(label)
        assert 10 < C < len(F) and np.array_equal(np.unique(comp), np.arange(C))
    assert R.numbering(R.labels(F, "vertex"))[1] < R.numbering(R.labels(F, "edge"))[1]


def test_host_tensors_are_refused():
    import torch
    import mesh_components as MC
    with pytest.raises(RuntimeError, match="ROCm device"):
        MC.face_components(torch.zeros((1, 3), dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        MC.component_stats(torch.zeros((3, 3), dtype=torch.float64), torch.zeros((1, 3), dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="connectivity"):
        MC.face_components(torch.zeros((1, 3), dtype=torch.int32), 3, connectivity="face")


def test_size_queries_and_argument_checks():
    import ctypes as C
    import mesh_components as MC
    import mesh_cull
    L = MC.lib
    assert L.gof_mesh_abi_version() == 2 and L.gof_abi_version() == 12
    assert 0 < L.gof_mesh_components_ws_bytes(0, 0, 0) and L.gof_mesh_components_ws_bytes(1000, 2000, 1) < L.gof_mesh_components_ws_bytes(1000, 2000, 0)
    assert L.gof_mesh_components_ws_bytes(10_000_000, 20_000_000, 0) < 128 * 20_000_000
    assert 0 < L.gof_mesh_component_stats_ws_bytes(0, 0) < L.gof_mesh_component_stats_ws_bytes(20000, 10)
    n = C.c_int64(5)
    assert L.gof_mesh_components(3, (2 ** 31 + 2) // 3, None, 0, None, None, C.byref(n), None, 0, None) < 0 and b"2^31" in L.gof_last_error() and n.value == 0
    assert L.gof_mesh_components(3, 1, None, 0, None, None, None, None, 0, None) < 0
    assert L.gof_mesh_components(-1, 1, None, 0, None, None, C.byref(n), None, 0, None) < 0
    assert L.gof_mesh_component_stats(3, (2 ** 31 + 2) // 3, None, None, None, 1, None, None, None, None, 0, None) < 0
    assert L.gof_mesh_mark_referenced(-1, 0, None, None, None, None) < 0 and L.gof_mesh_component_mask(-1, None, 0, None, None, None) < 0
    assert set(MC.tiling()) == {"sort_block", "scan_tile", "sum_tile", "sum_block"} and MC.tiling()["sum_tile"] == R.SUM_TILE and MC.tiling()["sum_block"] == R.SUM_BLOCK
    assert not hasattr(mesh_cull.DeviceMesh, "split") and "split" in MC.__doc__
    for name in ("components", "area", "remove_unreferenced_vertices", "keep_components"):
        assert hasattr(mesh_cull.DeviceMesh, name)


def test_selection_on_the_host():
    import mesh_components as MC
    cf = np.array([5, 9, 9, 2, 9], np.int64)
    area = np.array([4.0, np.nan, 1.0, 4.0, np.inf])
    for kw in (dict(largest=1), dict(largest=2), dict(largest=4), dict(largest=9), dict(largest=0), dict(largest=1, by="area"), dict(largest=3, by="area"),
               dict(largest=4, by="area"), dict(largest=5, by="area"), dict(min_faces=9), dict(min_area_ratio=0.0), dict(min_area_ratio=0.5),
               dict(largest=2, min_faces=6, by="area")):
        assert np.array_equal(MC.select(cf, area, **kw), R.select(cf, area, **kw)), kw
    assert MC.select(cf, area, largest=2).tolist() == [False, True, True, False, False]
    assert MC.select(cf, area, largest=4, by="area").tolist() == [True, False, True, True, True]            # the NaN area comes last
    assert MC.select(cf, [1.0, 2.0, 3.0, 4.0, 10.0], min_area_ratio=0.2).tolist() == [False, False, False, False, True]      # 4 > 4 is false
    assert MC.select([], [], largest=1).shape == (0,) and MC.total_area([]) == 0.0
    with pytest.raises(ValueError):
        MC.select(cf, area, largest=1, by="volume")


def test_spec_parsing():
    import mesh_components as MC
    assert MC.parse_spec("largest:1") == {"largest": 1}
    assert MC.parse_spec("min_area_ratio:0.2,connectivity:vertex") == {"min_area_ratio": 0.2, "connectivity": "vertex"}
    assert MC.parse_spec(" largest:2 , by:area, min-faces:10 ") == {"largest": 2, "by": "area", "min_faces": 10}
    for bad in ("largest", "largest:one", "biggest:1", "largest:1,largest:2", "connectivity:vertex", "by:volume,largest:1", "largest:-1",
                "min_area_ratio:nan", "largest:1,,", "connectivity:face,largest:1", ""):
        with pytest.raises(ValueError, match="GOF_MESH_COMPONENTS"):
            MC.parse_spec(bad)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
