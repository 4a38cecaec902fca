"""GPU tests of the mesh extraction's own steps: the case tables of tests/extract_cases.py through the real library,
one larger shape that crosses many scan tiles, the golden comparisons of tests/test_extract_host.py on the device, and the drop-in
marching_tetrahedra_with_binary_search with an analytic field against the reference's recorded mesh -- all held to
tests/extract_restatement.py with equalities.  No reference code runs here."""
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import extract_cases as K  # noqa: E402
import extract_restatement as R  # noqa: E402
import mesh_cull_restatement as MR  # noqa: E402
import test_extract_host as H  # noqa: E402
from mesh_cull_cases import same  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("P", K.TETRA_P)
def test_tetra_points_are_bit_equal(P):
    import mesh_extraction as ME
    assert same(K.run_tetra(ME, _up, P), K.want_tetra(P)) == []


def test_tetra_points_across_many_scan_tiles():
    import mesh_extraction as ME
    P = 70001
    xyz, sc, rot = R.gaussians(P)
    rec, W, H = R.frustum_records(R.ring_cameras(8))
    want_p, want_s = R.tetra_points(xyz, sc, rot, rec, W, H, 2.0, 3.5)
    pts, scales = ME.tetra_points(_up(xyz), _up(sc), _up(rot), rec, W, H, 2.0, 3.5)
    assert 0.05 * 9 * P < len(want_p) < 0.5 * 9 * P
    assert same({"p": pts.cpu().numpy(), "s": scales.cpu().numpy()}, {"p": want_p, "s": want_s}) == []
    assert ME.last_stats()["tetra_points"]["workspace_bytes"] <= 8 * 9 * P


@pytest.mark.parametrize("E", K.EDGES + (70001,))
def test_bisection_and_edge_filter_are_bit_equal(E):
    import mesh_extraction as ME
    want = K.want_bisect(E)
    want.update({"filter_" + k: v for k, v in K.want_filter(E).items()})
    got = K.run_bisect(ME, _up, E)
    got.update({"filter_" + k: v for k, v in K.run_filter(ME, _up, E).items()})
    assert same(got, want) == []


def test_mesh_of_the_last_round_and_its_ply(tmp_path):
    import mesh_cull as MC
    import mesh_extraction as ME
    assert same(K.run_mesh(ME, MC, _up, 1025, str(tmp_path)), K.want_mesh(1025)) == []


@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_tetra_points_on_the_device(tag):
    """the device's points against the reference's: equal to the restatement, which tests/test_extract_host.py holds to the golden --
    and directly: the same decisions away from near-ties, coordinates within the derived bound, equal scales"""
    import mesh_extraction as ME
    g = H.golden()
    xyz, sc, rot = g["tp_xyz"], g["tp_scaling"], g["tp_rotation"]
    P = len(xyz)
    cams = R.ring_cameras(8)
    near, far = (float(v) for v in g["tp_%s_near_far" % tag])
    model = types.SimpleNamespace(get_xyz=_up(xyz), get_scaling_with_3D_filter=_up(sc), _rotation=_up(rot))
    pts, scales = ME.get_tetra_points(model, cams, near, far)
    pts, scales = pts.cpu().numpy(), scales.cpu().numpy()
    rec, W, H_ = R.frustum_records(cams)
    want_p, want_s = R.tetra_points(xyz, sc, rot, rec, W, H_, near, far)
    assert same({"p": pts, "s": scales}, {"p": want_p, "s": want_s[:, None]}) == []
    cand, _ = R.candidates(xyz, sc, rot)
    keep = R.seen(cand, rec, W, H_, near, far)
    ref = np.unpackbits(g["tp_%s_mask" % tag])[:9 * P].astype(bool)
    tie = R.near_tie(cand, rec, W, H_, near, far)
    assert tie.sum() <= 0.005 * len(keep) and ((keep != ref) & ~tie).sum() == 0
    both = keep & ref                                                  # the candidates both keep: rows both[keep] of the device's, both[ref] of the reference's
    g_of = np.concatenate([np.repeat(np.arange(P), 8), np.arange(P)])[both]
    bound = 16 * 2.0 ** -24 * (np.abs(xyz[g_of].astype(np.float64)) + (3.0 * sc[g_of].astype(np.float64)).sum(-1, keepdims=True))
    assert both.sum() > 0.05 * len(keep)
    assert (np.abs(pts[both[keep]].astype(np.float64) - g["tp_%s_points" % tag][both[ref]]) <= bound).all()
    assert np.array_equal(scales.reshape(-1)[both[keep]], g["tp_%s_scales" % tag][both[ref]])


def test_drop_in_extraction_reproduces_the_references_mesh(tmp_path, capsys):
    """marching_tetrahedra_with_binary_search with the analytic field for evaluate_alpha, the golden's points and cells (cells.pt, as
    a second run of the script finds them): the 8 rounds, the filter, the colours and the exported PLY against what the reference's own
    function handed to trimesh"""
    import torch
    import mesh_cull as MC
    import mesh_extraction as ME
    g = H.golden()
    E, F = len(g["bs_vertices"]), len(g["bs_faces"])
    ref_mask = np.unpackbits(g["bs_vertex_mask"])[:E].astype(bool)
    e, sdf, sc, faces = H._golden_mesh_inputs(g)
    assert np.array_equal(R.edge_filter(e, sc), ref_mask)             # (no near-tie on this fixture: tests/test_extract_host.py)
    gaussians = types.SimpleNamespace(get_tetra_points=lambda views, near, far: (_up(g["bs_points"]), _up(g["bs_scales"])[:, None]))

    def evaluate_alpha(points, views, gaussians, pipeline, background, kernel_size, return_color=False):
        alpha = 1 - R.field_final_alpha(points)
        return (alpha, R.field_color(points)) if return_color else alpha
    model = str(tmp_path / "model")
    fusion = os.path.join(model, "test", "ours_7", "fusion")
    os.makedirs(fusion)
    torch.save(torch.from_numpy(g["bs_cells"].astype(np.int32)), os.path.join(fusion, "cells.pt"))
    for filter_mesh, texture_mesh in ((False, False), (True, True)):
        mesh = ME.marching_tetrahedra_with_binary_search(model, "test", 7, [], gaussians, None, None, 0.0, filter_mesh, texture_mesh, 0.02, 1e6,
                                                         evaluate_alpha=evaluate_alpha)
        out = capsys.readouterr().out
        assert "load existing cells" in out and [ln for ln in out.splitlines() if ln.startswith("binary search")] == ["binary search in step %d" % s for s in range(8)]
        assert isinstance(mesh, MC.DeviceMesh) and mesh._v.is_cuda
        back = MC.load(os.path.join(fusion, "mesh_binary_search_7.ply"))
        if filter_mesh:
            c = MR.compact(ref_mask, faces, attrs=(g["bs_vertices"], g["bs_colors"]))
            assert np.array_equal(c["face_keep"], np.unpackbits(g["bs_face_mask"])[:F].astype(bool))
            want_v, want_f, want_c = c["attrs"][0], c["faces"], c["attrs"][1]
        else:
            want_v, want_f, want_c = g["bs_vertices"], faces, None
        assert back.vertices.astype(f32).tobytes() == want_v.tobytes() and np.array_equal(back.faces, want_f)
        assert (back.vertex_colors is None) == (want_c is None) and (want_c is None or np.array_equal(back.vertex_colors, want_c))
        assert open(os.path.join(fusion, "mesh_binary_search_7.ply"), "rb").read() == MR.ply_bytes(want_v, want_f, colors=want_c)


def test_host_tensors_are_still_refused_next_to_a_device():
    import torch
    import mesh_extraction as ME
    with pytest.raises(RuntimeError, match="ROCm device"):
        ME.edge_filter(torch.zeros((4, 2, 3)), torch.zeros((4, 2)))
