"""CPU tests of the mesh culling: the kernels of csrc/mesh_cull.hip through the host emulator (tests/hipemu) behind
mesh_cull's own Python layer, each group of cases in a child process (an emulator abort fails one test, not the session), held to
tests/mesh_cull_restatement.py with equalities: packed masks, keep masks, compacted rows / faces / attribute bytes.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context are replaced by host stand-ins, and EVERY buffer mesh_cull allocates (workspaces and outputs) is filled with
0xA5 and followed by guard bytes that are checked after the run -- the pad bits of a packed mask and every workspace word the kernels
read must have been written by them."""
import ast
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
from host_child import PKG  # noqa: E402
import mesh_cull_cases as K  # noqa: E402
import mesh_cull_restatement as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ref_dtu_cull_golden.npz")
REF_SCRIPT = "/root/reference/evaluate_dtu_mesh.py"


def golden():
    return dict(np.load(GOLDEN))


# ---------------------------------------------------------------------------------------------------------------------------
# the child: mesh_cull over the emulated library
# ---------------------------------------------------------------------------------------------------------------------------
def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _cameras(g):
    import types
    import torch
    return [types.SimpleNamespace(world_view_transform=torch.from_numpy(g["world_view_transform"][i].copy()), gt_alpha_mask=torch.from_numpy(g["masks"][i].copy()),
                                  focal_x=float(g["focal"][i, 0]), focal_y=float(g["focal"][i, 1]), image_width=int(g["W"]), image_height=int(g["H"]),
                                  image_name="view%d" % i) for i in range(len(g["masks"]))]


def _child(case, out):
    import mesh_cull as M
    check = host_child.install_seams(M, buffers="all")
    kind, name = case.split(":", 1)
    if kind == "dilate":
        res = K.run_dilate(M, _up, tuple(int(v) for v in name.split("x")))
    elif kind == "cull":
        res = K.run_cull(M, _up, name, golden())
    elif kind == "compact":
        res = K.run_compact(M, _up, int(name))
    elif kind == "errors":
        res = {}
        keep, faces, _, _, _ = K.compact_case(1025, "half")
        for tag, bad in (("high", 1025), ("negative", -1)):
            f = faces.copy()
            f[100, 1] = bad
            try:
                M.compact_mesh(_up(keep), _up(f))
                res[tag] = np.array("")
            except RuntimeError as e:
                res[tag] = np.array(str(e))
        # a view record whose mask does not lie inside the mask buffer: refused, nothing outside is read
        import ctypes as C
        import torch
        rec = np.zeros(1, M._VIEW_DTYPE)
        rec[0] = (np.arange(12.0), 161, 120, 5, 3)
        v, masks, keep8, ws = _up(np.zeros((70, 3), np.float32)), torch.zeros(3 * 120, dtype=torch.int64), torch.zeros(70, dtype=torch.uint8), torch.zeros(4096, dtype=torch.uint8)
        rc = M.lib.gof_mesh_cull(70, v.data_ptr(), 1, _up(rec.view(np.uint8)).data_ptr(), masks.data_ptr(), 3 * 120, keep8.data_ptr(), ws.data_ptr(), 4096, None)
        res["record"] = np.array("%d %s" % (rc, M.lib.gof_last_error().decode()))
        assert isinstance(C.sizeof(M.GofCullView), int)
    elif kind == "mesh":
        # cull_mesh over a DeviceMesh and over a foreign mesh object, export -> load, update_vertices / update_faces
        g = golden()
        tmp = os.path.dirname(out)
        rng = np.random.default_rng(4)
        V, F = g["vertices"].astype(np.float64), g["faces"]
        N, C3 = rng.normal(size=V.shape).astype(np.float32), rng.integers(0, 256, V.shape).astype(np.uint8)
        mesh = M.cull_mesh(_cameras(g), M.DeviceMesh(V, F, N, C3))
        mesh.export(os.path.join(tmp, "culled.ply"))
        back = M.load(os.path.join(tmp, "culled.ply"))
        res = {"v": mesh.vertices, "f": mesh.faces, "n": mesh.vertex_normals, "c": mesh.vertex_colors,
               "bv": back.vertices, "bf": back.faces, "bn": back.vertex_normals, "bc": back.vertex_colors}
        mesh.vertices = mesh.vertices * 1.5                      # the script's alignment lines: host numpy, then the setter uploads
        mesh.vertices = mesh.vertices @ np.eye(3).T + 1.0
        res["aligned"] = mesh.vertices

        class Foreign:
            def __init__(self):
                self.vertices, self.faces = V.copy(), F.astype(np.int64)

            def update_vertices(self, mask):
                self.vertex_mask = np.asarray(mask).copy()

            def update_faces(self, mask):
                self.face_mask = np.asarray(mask).copy()
        fm = M.cull_mesh(_cameras(g), Foreign())
        res["foreign_vertex_mask"], res["foreign_face_mask"] = fm.vertex_mask, fm.face_mask
        plain = M.DeviceMesh(V, F)                                # trimesh's two-step protocol on the device
        plain.update_vertices(fm.vertex_mask)
        res["two_step_faces_all"] = plain.faces
        plain.update_faces(fm.face_mask)
        res["two_step_v"], res["two_step_f"] = plain.vertices, plain.faces
        cams = _cameras(g)
        cams[3].gt_alpha_mask = None
        try:
            M.cull_mesh(cams, M.DeviceMesh(V, F))
            res["no_mask"] = np.array("")
        except ValueError as e:
            res["no_mask"] = np.array(str(e))
        # a file written by tsdf_fusion.write_ply
        import tsdf_fusion
        tsdf_fusion.write_ply(os.path.join(tmp, "tsdf.ply"), V[:500], F[:0].reshape(0, 3).tolist() + [[0, 1, 2], [3, 4, 499]], C3[:500] / 255.0, N[:500])
        t = M.load(os.path.join(tmp, "tsdf.ply"))
        res["tv"], res["tf"], res["tn"], res["tc"] = t.vertices, t.faces, t.vertex_normals, t.vertex_colors
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=1800)
    assert int(res["buffers"]) > 0
    return res


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
def test_dilation_is_bit_equal(size, tmp_path):
    want = K.want_dilate(size)
    W, H = size
    assert len(want) == len(K.RADII) * (9 + sum(x < W for x in (63, 64, 127, 128)))
    if size == (161, 120):                                     # the cases bite: a tiny value is a set pixel, the disk is no square
        tiny = dict(K.dilate_masks(W, H))["tiny"]
        assert 0 < (tiny != 0).sum() and np.abs(tiny[tiny != 0]).max() < 1 / 256 and R.dilate(tiny, 6).sum() > 50 * (tiny != 0).sum()
        assert R.disk(6).sum() == 113 and R.disk(31).sum() < 63 * 63
    got = _emulate("dilate:%dx%d" % size, tmp_path)
    assert K.same(got, want) == []


@pytest.mark.parametrize("name", ["golden", "edges", "counts"])
def test_culling_is_bit_equal(name, tmp_path):
    want = K.want_cull(name, golden())
    if name == "edges":
        V, views = K.edge_scene()
        px, py = R.project(V, views[0][0], 129, 65)
        u = (px + 1.0) / 2.0 * 128
        assert (px == -1.0).sum() > 50 and (px == 1.0).sum() > 50 and (py == 1.0).sum() > 50          # on the bounds, exactly
        tie = (u - np.floor(u)) == 0.5
        assert (tie & (np.floor(u) % 2 == 0)).sum() > 1000 and (tie & (np.floor(u) % 2 == 1)).sum() > 1000
        assert np.isnan(V).any(axis=1).sum() >= 4 and want["keep3"][np.isnan(V).any(axis=1)].all()    # NaN vertices are kept
        assert want["keep2"].all()                                # z + 1e-6 == 0 in view C: nothing is valid, everything kept
        pxb, _ = R.project(V, views[1][0], 129, 65)
        assert ((V[:, 2] < 0) & (pxb > -1) & (pxb < 1)).any()     # behind the camera and still projected into the image
        assert 0 < want["keep0"].sum() < len(V) and not np.array_equal(want["keep0"], want["keep1"])
    if name == "counts":
        assert want["keep0"].all() and 0 < want["keep2"].sum() < want["keep1"].sum() < 3000
    got = _emulate("cull:" + name, tmp_path)
    assert K.same(got, want) == []


@pytest.mark.parametrize("nv", K.COMPACT_NV)
def test_compaction_is_bit_equal(nv, tmp_path):
    want = K.want_compact(nv)
    if nv > 1000:
        assert 0 < len(want["half_attrs_faces"]) < 2 * nv and len(want["all_plain_faces"]) == 2 * nv and len(want["none_plain_rows"]) == 0
    got = _emulate("compact:%d" % nv, tmp_path)
    assert K.same(got, want) == []


def test_bad_indices_and_records_are_refused(tmp_path):
    res = _emulate("errors:all", tmp_path)
    assert "outside [0, 1025)" in str(res["high"]) and "outside [0, 1025)" in str(res["negative"])
    assert str(res["record"]).startswith("-") and "view record" in str(res["record"])


def test_golden_the_reference_agrees_with_the_contract():
    """The restatement (fp64, the matrix itself) against the mask the reference's own cull_mesh produced (fp32 GEMMs, inverse of the
    inverse): they may differ only at vertices whose fp64 pixel coordinate lies, in some view, within 1e-3 px of a rounding tie or of
    a validity bound; the vertices at which they differ are left out and must be at most 0.1 % of all vertices.  (Not: "at most 0.1 %
    of the vertices lie that close to a tie" -- that is a property of the scene, not of the code: a vertex inside an image is within
    1e-3 px of a tie with probability 2e-3 per axis and view, ~3 % over the 16 coordinates of this scene.)"""
    g = golden()
    views = K.golden_views(g)
    dil = [(m, W, H, R.dilate(mask, 6)) for m, W, H, mask in views]
    keep = R.cull(g["vertices"], dil)
    near = R.near_decision(g["vertices"], dil, 1e-3)
    diff = keep != g["vertex_mask"]
    print("golden: %d of %d vertices differ from the reference, %d lie within 1e-3 px of a tie or bound" % (diff.sum(), len(keep), near.sum()))
    assert (diff & ~near).sum() == 0, "%d vertices away from every tie and bound differ from the reference" % (diff & ~near).sum()
    assert diff.sum() <= 0.001 * len(keep), "%d of %d vertices differ" % (diff.sum(), len(keep))
    assert 0.05 * len(keep) < keep.sum() < 0.5 * len(keep)
    if not diff.any():
        assert np.array_equal(R.compact(keep, g["faces"])["face_keep"], g["face_mask"])


def test_cull_mesh_device_mesh_foreign_mesh_and_ply(tmp_path):
    res = _emulate("mesh:all", tmp_path)
    g = golden()
    keep = K.want_cull("golden", g)["keep0"]
    V, F = g["vertices"].astype(np.float64), g["faces"]
    rng = np.random.default_rng(4)
    N, C3 = rng.normal(size=V.shape).astype(np.float32), rng.integers(0, 256, V.shape).astype(np.uint8)
    want = R.compact(keep, F, attrs=(V, N, C3))
    assert K.same(res, {"v": want["attrs"][0], "f": want["faces"], "n": want["attrs"][1], "c": want["attrs"][2]}) == []
    # export -> load: float32 coordinates widen exactly (the fixture's vertices are float32 values)
    assert K.same(res, {"bv": want["attrs"][0], "bf": want["faces"], "bn": want["attrs"][1], "bc": want["attrs"][2]}) == []
    assert open(str(tmp_path / "culled.ply"), "rb").read() == R.ply_bytes(want["attrs"][0], want["faces"], want["attrs"][1], want["attrs"][2])
    assert K.same(res, {"aligned": (want["attrs"][0] * 1.5) @ np.eye(3).T + 1.0}) == []
    assert K.same(res, {"foreign_vertex_mask": keep, "foreign_face_mask": want["face_keep"], "two_step_faces_all": R.compact(keep, F)["faces_all"],
                        "two_step_v": want["attrs"][0], "two_step_f": want["faces"]}) == []
    assert "camera 3" in str(res["no_mask"]) and "gt_alpha_mask" in str(res["no_mask"])
    assert K.same(res, {"tv": V[:500], "tf": np.array([[0, 1, 2], [3, 4, 499]], np.int32), "tn": N[:500],
                        "tc": np.round(np.clip(C3[:500] / 255.0, 0, 1) * 255.0).astype(np.uint8)}) == []


def test_read_ply_still_returns_what_it_did(tmp_path):
    import mesh_eval
    p = str(tmp_path / "m.ply")
    V = np.random.default_rng(0).normal(size=(50, 3)).astype(np.float32).astype(np.float64)
    F = np.random.default_rng(1).integers(0, 50, (20, 3)).astype(np.int32)
    open(p, "wb").write(R.ply_bytes(V, F, normals=V, colors=np.zeros((50, 3), np.uint8)))
    v, t = mesh_eval.read_ply(p)
    assert v.dtype == np.float64 and t.dtype == np.int32 and np.array_equal(v, V) and np.array_equal(t, F)
    el = mesh_eval.read_ply_elements(p)
    assert set(el) == {"vertex", "face"} and "nx" in el["vertex"].dtype.names and "red" in el["vertex"].dtype.names


def test_decompose_projection_matrix_recovers_the_centres():
    import mesh_cull
    rng = np.random.default_rng(8)
    for i in range(64):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Rm = q * np.sign(np.linalg.det(q))
        Km = np.array([[2800.0 + 50 * rng.random(), 0.3 * rng.normal(), 800 + 10 * rng.normal()], [0, 2790.0 + 50 * rng.random(), 600 + 10 * rng.normal()], [0, 0, 1.0]])
        C = rng.normal(size=3) * 500
        P = Km @ np.hstack([Rm, -(Rm @ C)[:, None]]) * (1.0 if i % 2 else 3.7)       # (defined up to scale)
        K2, R2, C2 = mesh_cull.decompose_projection_matrix(P)
        assert np.abs(C2 - C).max() <= 1e-9 * np.abs(C).max()
        assert (np.diag(K2) > 0).all() and abs(K2[2, 2] - 1) < 1e-12 and np.abs(np.tril(K2, -1)).max() < 1e-9
        assert np.abs(R2 @ R2.T - np.eye(3)).max() < 1e-9 and np.abs(K2 - Km).max() < 1e-6 * 2800 and np.abs(R2 - Rm).max() < 1e-9


def test_load_dtu_camera_reads_the_calibration_files(tmp_path):
    import mesh_cull
    rng = np.random.default_rng(9)
    cal = tmp_path / "Calibration" / "cal18"
    cal.mkdir(parents=True)
    centres = []
    for i in range(1, 65):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Rm = q * np.sign(np.linalg.det(q))
        C = rng.normal(size=3) * 300
        P = np.array([[2890.0, 0, 820], [0, 2880.0, 610], [0, 0, 1]]) @ np.hstack([Rm, -(Rm @ C)[:, None]])
        np.savetxt(str(cal / ("pos_%03d.txt" % i)), P)
        centres.append(C)
    poses = mesh_cull.load_dtu_camera(str(tmp_path))
    assert len(poses) == 64 and all(p.shape == (3, 4) and p.dtype == np.float32 for p in poses)
    got = np.array([p[:, 3] for p in poses])
    assert np.abs(got - np.array(centres)).max() <= 2e-3            # the files are read as float32 (the script's loadtxt): ~1e-7 x 2890 x 300 / 2890


def test_host_tensors_are_refused():
    import torch
    import mesh_cull
    with pytest.raises(RuntimeError, match="ROCm device"):
        mesh_cull.dilate_mask(torch.zeros((4, 4)), 6)
    with pytest.raises(RuntimeError, match="ROCm device"):
        mesh_cull.cull_vertices(torch.zeros((4, 3)), [])
    with pytest.raises(RuntimeError, match="ROCm device"):
        mesh_cull.compact_mesh(torch.zeros(4, dtype=torch.bool), torch.zeros((1, 3), dtype=torch.int32))


def test_size_queries_and_argument_checks():
    import ctypes as C
    import mesh_cull
    L = mesh_cull.lib
    assert [L.gof_mesh_mask_row_words(w) for w in (1, 64, 65, 1600)] == [1, 1, 2, 25]
    assert 0 < L.gof_mesh_compact_ws_bytes(0, 0) < L.gof_mesh_compact_ws_bytes(100000, 0) < L.gof_mesh_compact_ws_bytes(100000, 200000)
    assert L.gof_mesh_compact_ws_bytes(5_000_000, 10_000_000) < 16 * 15_000_000
    assert L.gof_mesh_cull_ws_bytes(10) > 0
    assert L.gof_mesh_dilate(16, 16, None, 0, 32, None, None) < 0 and b"radius" in L.gof_last_error()
    assert L.gof_mesh_dilate(0, 16, None, 0, 6, None, None) < 0
    n = (C.c_int64 * 2)()
    assert L.gof_mesh_compact(2 ** 31, None, 0, None, 1, None, None, None, None, 0, n, None) < 0
    assert L.gof_mesh_cull(-1, None, 0, None, None, 0, None, None, 0, None) < 0
    assert C.sizeof(mesh_cull.GofCullView) == 120


def test_launcher_rebinds_the_culling(tmp_path, monkeypatch):
    """A synthetic evaluate_dtu_mesh.py that imports the three packages and defines the two functions: under the launcher's rebinding
    cull_mesh is mesh_cull's, load_dtu_camera is mesh_cull's where cv2 is missing, `trimesh` is a namespace whose load is mesh_cull.load
    where trimesh is missing; GOF_DTU_CULL_TORCH=1 applies none of them; no other script is touched."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher_cull", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    import mesh_cull
    calls = []
    monkeypatch.setattr(mesh_cull, "cull_mesh", lambda cameras, mesh: calls.append(("cull", cameras, mesh)) or "culled")
    monkeypatch.setattr(mesh_cull, "load_dtu_camera", lambda DTU: calls.append(("cams", DTU)) or "poses")
    monkeypatch.setattr(mesh_cull, "load", lambda path: calls.append(("load", path)) or "mesh")
    script = tmp_path / "evaluate_dtu_mesh.py"
    result = tmp_path / "result.txt"
    script.write_text(
        "import cv2\n"
        "import trimesh\n"
        "from skimage.morphology import binary_dilation, disk\n"
        "def load_dtu_camera(DTU):\n"
        "    return 'script poses'\n"
        "def cull_mesh(cameras, mesh):\n"
        "    return 'script culled'\n"
        "if __name__ == '__main__':\n"
        "    out = [load_dtu_camera('/dtu'), trimesh.load('/m.ply'), cull_mesh('cams', 'm')]\n"
        "    open(%r, 'w').write(repr(out))\n" % str(result))
    missing = [m for m in ("cv2", "trimesh", "skimage") if importlib.util.find_spec(m) is None]
    path_before = list(sys.path)
    try:
        monkeypatch.delenv("GOF_DTU_CULL_TORCH", raising=False)
        rebind = L.dtu_cull_rebinding(str(script))
        assert "cull_mesh" in rebind and ("load_dtu_camera" in rebind) == ("cv2" in missing) and ("trimesh" in rebind) == ("trimesh" in missing)
        L.add_dtu_shims(str(script))
        L.run_script(str(script), rebind)
        got = ast.literal_eval(result.read_text())
        assert got[2] == "culled" and ("cull", "cams", "m") in calls
        assert got[0] == ("poses" if "cv2" in missing else "script poses")
        if "trimesh" in missing:
            assert got[1] == "mesh" and ("load", "/m.ply") in calls
        # the stand-ins were appended for this script only, behind everything else, and only for what is missing
        shim_dirs = [p for p in sys.path if p not in path_before]
        assert all(os.path.basename(os.path.dirname(p)) == "shims_dtu" and os.path.basename(p) in missing for p in shim_dirs) and len(shim_dirs) == len(missing)
        if shim_dirs:
            assert sys.path[-len(shim_dirs):] == shim_dirs
        if "skimage" in missing:
            import skimage.morphology
            with pytest.raises(RuntimeError, match="not installed"):
                skimage.morphology.binary_dilation(np.zeros((3, 3)), None)
        if "trimesh" in missing:
            import trimesh
            assert len(trimesh.creation.box().vertices) == 8
            with pytest.raises(RuntimeError, match="not installed"):
                trimesh.Trimesh()
        n = len(calls)
        monkeypatch.setenv("GOF_DTU_CULL_TORCH", "1")
        assert L.dtu_cull_rebinding(str(script)) == {}
        monkeypatch.delenv("GOF_DTU_CULL_TORCH")
        assert L.dtu_cull_rebinding(str(tmp_path / "train.py")) == {}
        sys_path = list(sys.path)
        L.add_dtu_shims(str(tmp_path / "train.py"))
        assert sys.path == sys_path and len(calls) == n
        assert set(L.dtu_eval_rebinding(str(script))) == {"os"}                  # the evaluation's rebinding is what it was
    finally:
        sys.path[:] = path_before
        for m in [k for k in sys.modules if k.split(".")[0] in missing]:
            del sys.modules[m]


def test_reference_script_defines_the_rebound_names():
    if not os.path.exists(REF_SCRIPT):
        pytest.skip("the reference checkout is not present")
    tree = ast.parse(open(REF_SCRIPT).read())
    funcs = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    imports = {a.asname or a.name for n in tree.body if isinstance(n, ast.Import) for a in n.names}
    assert {"cull_mesh", "load_dtu_camera"} <= funcs and "trimesh" in imports


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
