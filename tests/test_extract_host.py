"""CPU tests of the mesh extraction's own steps: the kernels of csrc/extract.hip through the host emulator
(tests/hipemu) behind mesh_extraction's own Python layer, each group of cases in a child process (an emulator abort fails one test, not
the session), held to tests/extract_restatement.py with equalities; and the restatement held to the reference through the committed
golden (tests/golden/ref_extract_golden.npz, written by tests/golden/make_golden_extract.py).

In the child the product modules run unchanged except for their test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context are replaced by host stand-ins, and EVERY buffer mesh_extraction and mesh_cull allocate (workspaces and
outputs) is filled with 0xA5 and followed by guard bytes that are checked after the run."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import extract_cases as K  # noqa: E402
import extract_restatement as R  # noqa: E402
import mesh_cull_restatement as MR  # noqa: E402
from mesh_cull_cases import same  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ref_extract_golden.npz")
f32 = np.float32


def golden():
    return dict(np.load(GOLDEN))


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _child(case, out):
    import ctypes as C
    import torch
    import mesh_cull as MC
    import mesh_extraction as ME
    check = host_child.install_seams(ME, MC, buffers="all")
    kind, name = case.split(":", 1)
    if kind == "tetra":
        res = K.run_tetra(ME, _up, int(name))
    elif kind == "bisect":
        res = K.run_bisect(ME, _up, int(name))
        res.update({"filter_" + k: v for k, v in K.run_filter(ME, _up, int(name)).items()})
    elif kind == "mesh":
        res = K.run_mesh(ME, MC, _up, int(name), os.path.dirname(out))
    elif kind == "errors":
        L = ME.lib
        res = {}
        xyz, sc, rot = (_up(a) for a in R.gaussians(10))
        ws = torch.zeros(8192, dtype=torch.uint8)
        n = C.c_int64(-7)
        rc = L.gof_tetra_points_count(10, xyz.data_ptr(), sc.data_ptr(), rot.data_ptr(), 3, None, 161, 120, 0.02, 1e6, ws.data_ptr(), 8192, C.byref(n), None)
        res["null_views"] = np.array("%d %d %s" % (rc, n.value, L.gof_last_error().decode()))
        rc = L.gof_tetra_points_count(10, xyz.data_ptr(), sc.data_ptr(), rot.data_ptr(), 0, None, 161, 120, 0.02, 1e6, ws.data_ptr(), 8192, C.byref(n), None)
        res["zero_views"] = np.array("%d %d" % (rc, n.value))
        pts, scales = torch.full((90, 3), 7.0), torch.full((90,), 7.0)
        rc = L.gof_tetra_points_emit(10, xyz.data_ptr(), sc.data_ptr(), rot.data_ptr(), ws.data_ptr(), 8192, 5, pts.data_ptr(), scales.data_ptr(), None)
        res["wrong_count"] = np.array("%d %s %d" % (rc, L.gof_last_error().decode(), int((pts == 7.0).all())))
        rc = L.gof_tetra_points_count(10, xyz.data_ptr(), sc.data_ptr(), rot.data_ptr(), 0, None, 161, 120, 0.02, 1e6, ws.data_ptr(), 100, C.byref(n), None)
        res["small_ws"] = np.array("%d" % rc)
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=1800)
    assert int(res["buffers"]) > 0
    return res


# ---- the kernels against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", K.TETRA_P)
def test_tetra_points_are_bit_equal(P, tmp_path):
    want = K.want_tetra(P)
    assert len(want["v0_points"]) == 0 and len(want["none_points"]) == 0 and len(want["all_points"]) == 9 * P       # the cases bite
    if P >= 113:
        assert 0 < len(want["v8_band_points"]) < len(want["v1_points"]) < len(want["v8_points"]) < 9 * P
        assert not np.array_equal(want["sizes_points"], want["sizes_swapped_points"]) and len(want["sizes_points"]) > len(want["sizes_swapped_points"])
        assert len(want["nan_points"]) < len(want["v8_points"]) and np.isfinite(want["nan_points"]).all()
    # z0: the centre with Z = 0 is not seen although near < 0 <= far, its neighbours in the plane z = 0 likewise
    cases = {c[0]: c for c in K.tetra_cases(P)}
    _, xyz, sc, rot, cams, near, far = cases["z0"]
    rec, W, H = R.frustum_records(cams)
    pts, _ = R.candidates(xyz, sc, rot)
    u, v, Z = R.project(pts, rec[0], W, H)
    assert Z[8 * P] == 0.0 and not R.seen(pts, rec, W, H, near, far)[8 * P]
    got = _emulate("tetra:%d" % P, tmp_path)
    assert same(got, want) == []


@pytest.mark.parametrize("E", K.EDGES)
def test_bisection_and_edge_filter_are_bit_equal(E, tmp_path):
    want = K.want_bisect(E)
    want.update({"filter_" + k: v for k, v in K.want_filter(E).items()})
    if E >= 63:
        e, sdf, sc, rounds = K.bisect_case(E)
        assert (rounds[0][0] == 0.5).sum() > 10 and np.isnan(rounds[0][0]).sum() > 5 and np.signbit(sdf[:, 0, 0][sdf[:, 0, 0] == 0]).any()
        fe, fs = K.filter_case(E)
        d = np.sqrt(((fe[:, 0].astype(np.float64) - fe[:, 1]) ** 2).sum(-1))
        exact = d == (fs[:, 0] + fs[:, 1]).astype(np.float64)
        assert exact.sum() >= 10 and want["filter_keep"][exact].all() and 0 < want["filter_keep"].sum() < E
        assert not want["filter_keep"][1] and not want["filter_keep"][2] and not want["filter_keep"][3]
    got = _emulate("bisect:%d" % E, tmp_path)
    assert same(got, want) == []


def test_mesh_of_the_last_round_and_its_ply(tmp_path):
    want = K.want_mesh(1025)
    assert len(want["plain_v"]) == 1025 and 0 < len(want["full_v"]) < 1025 and 0 < len(want["full_f"]) < 2050
    assert b"property uchar red" in want["full_ply"].tobytes() and b"alpha" not in want["full_ply"].tobytes()[:400]
    got = _emulate("mesh:1025", tmp_path)
    assert same(got, want) == []


def test_bad_arguments_are_refused(tmp_path):
    res = host_child.run_child(__file__, "errors:all", tmp_path, timeout=600)       # (raw calls into the library: no guarded buffer is handed out)
    assert str(res["null_views"]).startswith("-1 0 ") and "views is NULL" in str(res["null_views"])
    assert str(res["zero_views"]) == "0 0"
    assert str(res["wrong_count"]).startswith("-1 ") and "count" in str(res["wrong_count"]) and str(res["wrong_count"]).endswith(" 1")
    assert str(res["small_ws"]) == "-2"


def test_size_queries_and_argument_checks():
    import ctypes as C
    import mesh_extraction as ME
    L = ME.lib
    for P in (113, 114, 600, 70001, 5_000_000):
        assert 4 * 9 * P < L.gof_tetra_points_ws_bytes(P) <= 8 * 9 * P                  # at most 8 B per candidate: no buffer grows with views x points
    assert L.gof_tetra_points_ws_bytes(1) <= 8 * 9 + 4096                               # 9 candidates: the fixed alignment pads outweigh them
    n = C.c_int64()
    assert L.gof_tetra_points_count(-1, None, None, None, 0, None, 1, 1, 0.02, 1e6, None, 0, C.byref(n), None) < 0
    assert L.gof_tetra_points_count(2 ** 31 // 9 + 1, None, None, None, 0, None, 1, 1, 0.02, 1e6, None, 0, C.byref(n), None) < 0
    assert L.gof_tetra_points_count(1, None, None, None, -1, None, 1, 1, 0.02, 1e6, None, 0, C.byref(n), None) < 0 and b"views" in L.gof_last_error()
    assert L.gof_tetra_points_emit(-1, None, None, None, None, 0, 0, None, None, None) < 0
    assert L.gof_tetra_points_emit(1, None, None, None, None, 0, -1, None, None, None) < 0
    assert L.gof_bisect_step(-1, None, None, None, None, None, 0, None, None) < 0 and L.gof_bisect_step(0, None, None, None, None, None, 0, None, None) == 0
    assert L.gof_bisect_step(4, None, None, None, None, None, 3, None, None) < 0 and b"mode" in L.gof_last_error()
    assert L.gof_bisect_step(4, None, None, None, None, None, 1, None, None) < 0
    assert L.gof_edge_filter(-1, None, None, None, None) < 0 and L.gof_edge_filter(0, None, None, None, None) == 0 and L.gof_edge_filter(3, None, None, None, None) < 0
    assert C.sizeof(ME.GofFrustumView) == 112


def test_host_tensors_are_refused():
    import torch
    import mesh_extraction as ME
    rec, W, H = ME.frustum_records(R.ring_cameras(2))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ME.tetra_points(torch.zeros((4, 3)), torch.ones((4, 3)), torch.ones((4, 4)), rec, W, H)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ME.bisect_step(torch.zeros((4, 3)), torch.zeros((4, 3)), None, None, None, ME.BISECT_FIRST)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ME.edge_filter(torch.zeros((4, 2, 3)), torch.zeros((4, 2)))
    import mesh_cull
    with pytest.raises(RuntimeError, match="ROCm device"):
        mesh_cull.DeviceMesh.from_device(torch.zeros((4, 3)), torch.zeros((1, 3), dtype=torch.int32))


# ---- the restatement against the reference (the golden) -------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_tetra_points_the_reference_agrees_with_the_contract(tag):
    """Every candidate that is no near-tie has the reference's decision (a near-tie: in some view u or v within 1e-3 px of a bound or Z
    within 1e-6 relative of near / far; at most 0.5 % of the candidates may be one -- a condition on the scene, not a measurement);
    kept coordinates within 16 * 2^-24 * (|xyz_k| + s_0 + s_1 + s_2) of the reference's (about 8 roundings of magnitude <= 1 go into an
    entry of R, three products and three additions follow, and torch's bmm fixes neither their order nor contraction); scales equal."""
    g = golden()
    xyz, sc, rot = g["tp_xyz"], g["tp_scaling"], g["tp_rotation"]
    P = len(xyz)
    assert (P, tuple(a.tobytes() for a in (xyz, sc, rot))) == (600, tuple(a.tobytes() for a in R.gaussians(600)))
    rec, W, H = R.frustum_records(R.ring_cameras(8))
    near, far = (float(v) for v in g["tp_%s_near_far" % tag])
    pts, scales = R.candidates(xyz, sc, rot)
    keep = R.seen(pts, rec, W, H, near, far)
    ref = np.unpackbits(g["tp_%s_mask" % tag])[:9 * P].astype(bool)
    tie = R.near_tie(pts, rec, W, H, near, far)
    diff = keep != ref
    print("golden %s: %d of %d candidates kept (reference %d), %d differ, %d near-ties" % (tag, keep.sum(), len(keep), ref.sum(), diff.sum(), tie.sum()))
    assert tie.sum() <= 0.005 * len(keep)
    assert (diff & ~tie).sum() == 0
    assert 0.05 * len(keep) < keep.sum() < 0.95 * len(keep)
    both = keep & ref
    ref_pts = np.zeros_like(pts)
    ref_scales = np.zeros_like(scales)
    ref_pts[ref], ref_scales[ref] = g["tp_%s_points" % tag], g["tp_%s_scales" % tag]
    g_of = np.concatenate([np.repeat(np.arange(P), 8), np.arange(P)])
    bound = 16 * 2.0 ** -24 * (np.abs(xyz[g_of].astype(np.float64)) + (3.0 * sc[g_of].astype(np.float64)).sum(-1, keepdims=True))
    err = np.abs(pts.astype(np.float64) - ref_pts)
    print("golden %s: largest coordinate error / bound = %.3f" % (tag, (err[both] / bound[both]).max()))
    assert (err[both] <= bound[both]).all()
    assert np.array_equal(scales[both], ref_scales[both])


def _golden_mesh_inputs(g):
    pts, sc, ids = g["bs_points"], g["bs_scales"], g["bs_edge_ids"].astype(np.int64)
    sdf = (f32(1) - R.field_final_alpha(pts)) - f32(0.5)
    return pts[ids], sdf[ids][:, :, None], sc[ids][:, :, None], g["bs_faces"].astype(np.int32)


def test_golden_bisection_mesh_the_reference_agrees_with_the_contract(tmp_path):
    """End points bit-equal (the torch lines are elementwise), the filter's mask equal except where |d - s| <= 4 ulp of s (at most 0.5 %
    of the edges), faces and colours equal; PLY export -> load round trip."""
    g = golden()
    e, sdf, sc, faces = _golden_mesh_inputs(g)
    E, F = len(e), len(faces)
    m = R.bisect_and_mesh(e, sdf, sc, faces, R.field_final_alpha, R.field_color, True, True)
    assert m["end_vertices"].tobytes() == g["bs_vertices"].tobytes()
    ref_mask = np.unpackbits(g["bs_vertex_mask"])[:E].astype(bool)
    tie = R.edge_filter_near_tie(e, sc)
    diff = m["mask"] != ref_mask
    print("golden mesh: %d edges, %d kept, %d differ from the reference, %d near-ties" % (E, m["mask"].sum(), diff.sum(), tie.sum()))
    assert tie.sum() <= 0.005 * E and (diff & ~tie).sum() == 0 and 0.1 * E < ref_mask.sum() < 0.9 * E
    assert np.array_equal(R.colors_u8(R.field_color(m["end_vertices"])), g["bs_colors"])
    # one compaction with drop_faces is the reference's update_vertices + update_faces: on the reference's own mask, and the
    # restatement's mesh on its own mask (the two masks may differ at near-ties only, so faces that touch none must agree)
    ref_face_mask = np.unpackbits(g["bs_face_mask"])[:F].astype(bool)
    c = MR.compact(ref_mask, faces, attrs=(g["bs_vertices"], g["bs_colors"]))
    assert np.array_equal(c["face_keep"], ref_face_mask) and 0 < ref_face_mask.sum() < F
    mine = MR.compact(m["mask"], faces)
    away = ~tie[faces].any(axis=1)
    assert np.array_equal(mine["face_keep"][away], ref_face_mask[away])
    assert np.array_equal(m["vertices"], g["bs_vertices"][m["mask"]]) and np.array_equal(m["colors"], g["bs_colors"][m["mask"]]) and np.array_equal(m["faces"], mine["faces"])
    # the PLY the product writes for this mesh, read back by the product's loader (host arrays in, host arrays out)
    import mesh_eval
    path = str(tmp_path / "golden_mesh.ply")
    open(path, "wb").write(MR.ply_bytes(m["vertices"], m["faces"], colors=m["colors"]))
    el = mesh_eval.read_ply_elements(path)
    v = np.stack([el["vertex"][k] for k in "xyz"], -1)
    assert v.tobytes() == m["vertices"].tobytes() and np.array_equal(el["face"]["_i"].reshape(-1, 3), m["faces"])
    assert np.array_equal(np.stack([el["vertex"][k] for k in ("red", "green", "blue")], -1), m["colors"])


def test_golden_is_small():
    assert os.path.getsize(GOLDEN) < 300 * 1024


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
