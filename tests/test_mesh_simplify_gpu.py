"""GPU tests of the mesh simplification: the case tables of tests/mesh_simplify_cases.py through the real library, plus
the 200 000-face soup with colours -- all held to tests/mesh_simplify_restatement.py with equalities (vertex_cluster, the cluster count,
positions bit for bit, colours, used_mean, kept faces, exported bytes), and to the properties that need no restatement: structure,
locality, the flat grid's plane, the quadric objective, identity, determinism over runs and workspace contents, the target search."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mesh_simplify_cases as K  # noqa: E402
import mesh_simplify_restatement as R  # noqa: E402
import test_mesh_simplify_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(tag, case, tmp_path, dedupe=True):
    import mesh_cull as M
    import mesh_simplify as MS
    got = K.run(MS, M, dev, case, dedupe=dedupe, ply=str(tmp_path / (tag + ".ply")))
    assert K.same(got, K.want(case, dedupe=dedupe, ply=True, key=tag)) == [], tag
    assert K.properties(case, got, dedupe) == [], tag
    assert K.quadric_holds(case, got)[0], tag
    return got


def test_hand_built_cases(tmp_path):
    got = {tag: check(tag, case, tmp_path) for tag, case in K.hand_cases().items()}
    assert got["empty"]["counts"].tolist() == [0, 0, 0, 0] and got["one_triangle"]["f"].tolist() == [[0, 1, 2]] and got["zero_area"]["face_keep"].tolist() == [1, 1]
    assert got["opposite"]["face_keep"].tolist() == [1, 0, 0] and got["on_a_boundary"]["vertex_cluster"].tolist() == [0, 1, 2, 3] and got["one_cell"]["f"].shape == (0, 3)
    assert check("opposite_all", K.hand_cases()["opposite"], tmp_path, dedupe=False)["face_keep"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("name", sorted(set(H.GROUP_MESHES) - {"soup"}))      # (the soup: test_soup_twice)
def test_meshes(name, tmp_path):
    case = H.GROUP_MESHES[name]()
    got = check(name, case, tmp_path)
    if name == "flat":
        assert (np.abs(got["v"] @ K.FLAT_NORMAL - 0.25) <= 2.0 ** -40 * np.ptp(case[0], axis=0).max()).all()
    if name == "identity":
        assert np.array_equal(got["vertex_cluster"], np.arange(len(case[0]))) and np.array_equal(got["f"], case[1]) and np.array_equal(got["c"], case[3])
        assert got["v"].tobytes() == case[0].tobytes()                                # bit for bit: a cell of one vertex keeps it


def test_fans_at_the_tile_and_block_boundaries(tmp_path):
    small, large = K.fan_sizes(H.tiling())
    for n in small + large:
        got = check("fan%d" % n, K.fan(n), tmp_path)
        assert np.count_nonzero(got["vertex_cluster"][K.fan(n)[1].reshape(-1)] == 0) == n and int(got["used_mean"][0]) == 0


def test_vertex_counts_at_the_sort_and_scan_boundaries(tmp_path):
    for n in K.boundary_vertex_counts(H.tiling()):
        check("cloud%d" % n, K.cloud_strip(n), tmp_path)


def test_soup_twice(tmp_path):
    case = K.soup()
    got = check("soup", case, tmp_path)
    assert int(got["counts"][0]) == 4096 and len(case[1]) == 200000
    import mesh_cull as M
    import mesh_simplify as MS
    assert K.same(K.run(MS, M, dev, case, ply=str(tmp_path / "again.ply")), got) == []            # two runs: identical bytes


def test_runs_and_workspace_contents_do_not_matter():
    import mesh_simplify as MS
    case = K.soup(30000, 12000)
    want = K.want_filled(case)
    for fill, _ in H.FILLS:
        assert K.same(K.run_filled(MS, dev, case, fill), want) == [], fill


def test_target_search_reproduces_through_cell():
    import mesh_cull as M
    V, F, N, Col, _, _ = K.icosphere()
    for target in (100, 2000):
        mesh = M.DeviceMesh(V, F, N, Col)
        st = mesh.simplify(target_vertices=target)
        again = M.DeviceMesh(V, F, N, Col)
        st2 = again.simplify(cell=st["cell"])
        assert target // 2 < st["clusters"] <= target and st2["clusters"] == st["clusters"] and len(st["probes"]) <= 24
        assert st["clusters"] == R.cluster(V, st["cell"])[1] and np.array_equal(mesh.vertices, again.vertices) and np.array_equal(mesh.faces, again.faces)
        assert mesh._v.is_cuda and mesh._f.dtype == torch.int32 and mesh._n is not None


def test_bad_input_is_refused():
    import mesh_cull as M
    for tag, (case, word) in K.refusals().items():
        V, F, _, _, h, origin = case
        with pytest.raises((RuntimeError, ValueError), match=word.replace("^", r"\^")):
            M.DeviceMesh(V, F).simplify(cell=h, origin=origin)
