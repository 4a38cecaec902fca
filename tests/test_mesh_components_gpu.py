"""GPU tests of the mesh connected components: the case tables of tests/mesh_components_cases.py through the real
library, plus the 200 000-face soup in both modes -- all held to tests/mesh_components_restatement.py and, for the labels, to SciPy's
connected components, with equalities."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mesh_components_cases as K  # noqa: E402
import mesh_components_restatement as R  # noqa: E402
import test_mesh_components_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(tag, V, F, modes=K.MODES):
    import mesh_components as MC
    out = {}
    for mode in modes:
        got, want = K.run(MC, dev, V, F, mode), K.want(V, F, mode)
        assert K.same(got, want) == [], (tag, mode)
        assert np.array_equal(got["label"], R.scipy_labels(F, mode)), (tag, mode)
        assert K.area_bound_holds(V, F, got), (tag, mode)
        out[mode] = got
    return out


def test_hand_built_cases():
    got = {tag: check(tag, V, F) for tag, V, F in H.group_cases("hand", "all")}
    assert int(got["shared_vertex"]["edge"]["count"]) == 2 and int(got["shared_vertex"]["vertex"]["count"]) == 1
    assert got["three_on_an_edge"]["edge"]["comp"].tolist() == [0, 1, 0, 0] and got["face_aaa"]["vertex"]["comp"].tolist() == [0, 1, 0, 2, 2]
    assert int(got["nothing"]["edge"]["count"]) == 0 and int(got["no_faces"]["vertex"]["count"]) == 0
    for mode in K.MODES:
        assert np.array_equal(got["nan"][mode]["label"], got["two_tetrahedra"][mode]["label"])
        assert np.isnan(got["nan"][mode]["area"][1]) and np.isfinite(got["nan"][mode]["area"][0]) and not np.isfinite(got["inf"][mode]["area"][0])


@pytest.mark.parametrize("group", range(H.STRIP_GROUPS))
def test_strips_at_every_boundary(group):
    for tag, V, F in H.group_cases("strips", str(group)):
        got = check(tag, V, F)
        assert int(got["edge"]["count"]) == 1 and got["vertex"]["faces"].tolist() == [len(F)]


def test_deep_chain():
    got = check("deep", *K.deep_chain())
    assert int(got["edge"]["count"]) == 1 and not got["vertex"]["label"].any()


def test_floaters():
    got = check("floaters", *K.floaters())
    assert int(got["edge"]["count"]) == 3001 and got["edge"]["faces"].max() == 50000


def test_a_component_across_two_blocks_of_the_area_sums():
    V, F = K.strip_case(K.block_strip_size(H.tiling()))
    assert check("block", V, F, ("edge",))["edge"]["faces"].tolist() == [len(F)]


@pytest.fixture(scope="module")
def soup():
    V, F = K.soup()
    return V, F, {mode: K.want(V, F, mode) for mode in K.MODES}


@pytest.mark.parametrize("mode", K.MODES)
def test_soup(soup, mode):
    import mesh_components as MC
    V, F, want = soup
    assert len(F) == 200000 and 100 < int(want[mode]["count"]) < 150000 and want[mode]["faces"].max() > H.tiling()["sum_tile"]
    got = K.run(MC, dev, V, F, mode)
    assert K.same(got, want[mode]) == []
    assert np.array_equal(got["label"], R.scipy_labels(F, mode)) and K.area_bound_holds(V, F, got)
    again = K.run(MC, dev, V, F, mode)                                # two runs: identical bytes
    assert K.same(again, got) == []


def test_runs_and_workspace_contents_do_not_matter():
    import mesh_components as MC
    V, F = K.floaters(20000, 3000)
    for mode in K.MODES:
        want = {k: v for k, v in K.want(V, F, mode).items() if not k.endswith("_again")}
        for fill, _ in H.FILLS:
            assert K.same(K.run_filled(MC, dev, V, F, mode, fill), want) == [], (mode, fill)


def test_keep_components_equals_boolean_indexing(tmp_path):
    import mesh_cull as M
    assert K.same(K.run_keep(M, lambda name: str(tmp_path / (name + ".ply"))), K.want_keep()) == []


def test_keep_the_largest_of_the_floaters(tmp_path):
    """the use the unit is for: the floaters go, the object stays, in order, and the exported bytes are the restatement's"""
    import mesh_cull as M
    import mesh_components as MC
    V, F = K.floaters()
    V = V.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(3)
    N, Col = rng.normal(size=V.shape).astype(np.float32), rng.integers(0, 256, V.shape).astype(np.uint8)
    mesh = M.DeviceMesh(V, F, N, Col)
    assert mesh.keep_components(largest=1) == (1, 3000)
    v, f, n, c, _, _ = R.keep_components(V, F, N, Col, largest=1)
    assert len(f) == 50000 and len(v) == 50002
    path = str(tmp_path / "clean.ply")
    mesh.export(path)
    assert open(path, "rb").read() == R.ply_bytes(v, f, n, c)
    st = MC.last_stats()
    assert st["keep"]["kept_faces"] == 50000 and st["components"]["components"] == 3001 and mesh._v.is_cuda and mesh._f.dtype == torch.int32


def test_bad_indices_are_refused_with_nothing_written():
    import mesh_components as MC
    V, F = K.strip_case(300)
    F = F.copy()
    F[123, 2] = len(V)
    for mode in K.MODES:
        with pytest.raises(RuntimeError, match=r"outside \[0, 302\)"):
            MC.face_components(dev(F), len(V), mode)
    import ctypes as C
    label = torch.full((len(F),), 0x5C5C5C5C, dtype=torch.int32, device="cuda")
    comp = label.clone()
    nb = MC.lib.gof_mesh_components_ws_bytes(len(V), len(F), 0)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    n = C.c_int64(-7)
    assert MC.lib.gof_mesh_components(len(V), len(F), dev(F).data_ptr(), 0, label.data_ptr(), comp.data_ptr(), C.byref(n), ws.data_ptr(), nb, None) < 0
    torch.cuda.synchronize()
    assert bool((label == 0x5C5C5C5C).all()) and bool((comp == 0x5C5C5C5C).all()) and n.value == 0
    assert MC.lib.gof_mesh_components(len(V), (2 ** 31 + 2) // 3, dev(F).data_ptr(), 0, label.data_ptr(), comp.data_ptr(), C.byref(n), ws.data_ptr(), nb, None) < 0
    torch.cuda.synchronize()
    assert bool((label == 0x5C5C5C5C).all()) and bool((comp == 0x5C5C5C5C).all())
