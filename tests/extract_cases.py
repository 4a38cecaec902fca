"""The case tables of the mesh extraction tests, shared by the CPU suite (test_extract_host.py: the kernels through the
host emulator) and the GPU suite (test_extract_gpu.py: the real library).  run_*(ME, up, ...) drives mesh_extraction's Python layer and
returns numpy arrays, want_*(...) is what tests/extract_restatement.py says they must be -- the tests compare the two with equalities
(mesh_cull_cases.same).  Test infrastructure only."""
import types

import numpy as np

import extract_restatement as R
import mesh_cull_restatement as MR

f32 = np.float32
TETRA_P = (1, 113, 114, 600)                 # 9 * 113 = 1017 and 9 * 114 = 1026 straddle the scan's 1024-word tile
EDGES = (1, 63, 64, 65, 1025)


def identity_camera(W=161, H=120):
    """X, Y, Z = x, y, z: a point with z = 0 has Z = 0 exactly"""
    return types.SimpleNamespace(world_view_transform=np.eye(4, dtype=f32), focal_x=100.0, focal_y=90.0, image_width=W, image_height=H)


def tetra_cases(P):
    """-> [(name, xyz, scaling, rotation, cameras, near, far)]"""
    xyz, sc, rot = R.gaussians(P)
    ring = R.ring_cameras(8)
    cases = [("v8", xyz, sc, rot, ring, 0.02, 1e6), ("v8_band", xyz, sc, rot, ring, 2.0, 3.5), ("v1", xyz, sc, rot, ring[3:4], 0.02, 1e6),
             ("v0", xyz, sc, rot, [], 0.02, 1e6), ("none", xyz, sc, rot, ring, 100.0, 200.0)]
    small = R.gaussians(P, seed=22, extent=0.3)
    cases.append(("all", small[0], small[1], small[2], ring, 0.02, 1e6))
    bad_xyz, bad_rot = xyz.copy(), rot.copy()
    bad_xyz[0, 1] = np.nan                                           # a NaN position: none of its 9 candidates is seen
    if P > 2:
        bad_rot[1] = 0.0                                             # a zero quaternion: NaN corners, the centre is still a candidate
        bad_xyz[2] = (np.inf, 0.0, 0.0)
    cases.append(("nan", bad_xyz, sc, bad_rot, ring, 0.02, 1e6))
    z0 = xyz.copy()
    z0[0] = (0.0, 0.0, 0.0)                                          # its centre has Z = 0 in the identity view; near < 0 lets Z = 0 reach the division
    if P > 1:
        z0[1] = (0.25, -0.125, 0.0)
    cases.append(("z0", z0, sc, rot, [identity_camera()], -1.0, 10.0))
    mixed = R.ring_cameras(8, sizes=((161, 120), (64, 48)))
    cases.append(("sizes", xyz, sc, rot, mixed, 0.02, 1e6))          # view 0's W, H for all views (gaussian_model.py:32)
    cases.append(("sizes_swapped", xyz, sc, rot, mixed[1:] + mixed[:1], 0.02, 1e6))
    return cases


def run_tetra(ME, up, P):
    res = {}
    for name, xyz, sc, rot, cams, near, far in tetra_cases(P):
        rec, W, H = ME.frustum_records(cams)
        pts, scales = ME.tetra_points(up(xyz), up(sc), up(rot), rec, W, H, near, far)
        res[name + "_points"], res[name + "_scales"] = pts.cpu().numpy(), scales.cpu().numpy()
        st = ME.last_stats()["tetra_points"]
        # 8 B per candidate; only below P = 113 do the fixed alignment pads outweigh 9 P candidates
        assert st["workspace_bytes"] <= 8 * 9 * P + (0 if P >= 113 else 4096) and st["kept"] == len(res[name + "_points"])
    # the drop-in for the method, over a model object
    name, xyz, sc, rot, cams, near, far = tetra_cases(P)[1]
    model = types.SimpleNamespace(get_xyz=up(xyz), get_scaling_with_3D_filter=up(sc), _rotation=up(rot))
    pts, scales = ME.get_tetra_points(model, cams, near, far)
    assert tuple(scales.shape) == (pts.shape[0], 1)
    res["method_points"], res["method_scales"] = pts.cpu().numpy(), scales.cpu().numpy().reshape(-1)
    return res


def want_tetra(P):
    res = {}
    for name, xyz, sc, rot, cams, near, far in tetra_cases(P):
        rec, W, H = R.frustum_records(cams)
        res[name + "_points"], res[name + "_scales"] = R.tetra_points(xyz, sc, rot, rec, W, H, near, far)
    res["method_points"], res["method_scales"] = res["v8_band_points"], res["v8_band_scales"]
    return res


# ---- the bisection ---------------------------------------------------------------------------------------------------------------------
def bisect_case(E):
    """-> (end_points, end_sdf, end_scales, [(value, mode)]): three rounds on the analytic field's values are made by the runner; the
    special rounds here: mid_sdf = +0 (value 0.5 either way), NaN, and left_sdf = -0, +0, NaN against every sign of mid_sdf.
    (mid_sdf = -0 cannot be produced: alpha - 0.5 is +0 wherever it is zero, in round-to-nearest.)"""
    e, sdf, sc, _ = R.edges(E)
    rng = np.random.default_rng(E)
    sdf = sdf.copy()
    special = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf], f32)
    sdf[::3, 0, 0] = special[np.arange(len(sdf[::3])) % 5]
    v1 = rng.uniform(0, 1, E).astype(f32)
    v1[::2] = 0.5
    v1[1::4] = np.nan
    v2 = rng.uniform(0, 1, E).astype(f32)
    v2[::5] = 0.5
    return e, sdf, sc, [(v1, R.FINAL_ALPHA), (v2, R.ALPHA)]


def run_bisect(ME, up, E):
    e, sdf, sc, rounds = bisect_case(E)
    l, r = up(e[:, 0].copy()), up(e[:, 1].copy())
    ls, rs = up(sdf[:, 0, 0].copy()), up(sdf[:, 1, 0].copy())
    res = {}
    pts = ME.bisect_step(l, r, None, None, None, ME.BISECT_FIRST)
    res["first"] = pts.cpu().numpy().copy()
    for k in range(3):
        pts = ME.bisect_step(l, r, ls, rs, up(R.field_final_alpha(pts.cpu().numpy())), ME.BISECT_FINAL_ALPHA, mid_out=pts)
    for value, mode in rounds:
        pts = ME.bisect_step(l, r, ls, rs, up(value), mode)
    for k, t in (("mid", pts), ("l", l), ("r", r), ("ls", ls), ("rs", rs)):
        res[k] = t.cpu().numpy()
    return res


def want_bisect(E):
    e, sdf, sc, rounds = bisect_case(E)
    l, r, ls, rs = e[:, 0].copy(), e[:, 1].copy(), sdf[:, 0, 0].copy(), sdf[:, 1, 0].copy()
    res = {}
    pts = R.bisect_step(l, r, None, None, None, R.FIRST)
    res["first"] = pts.copy()
    for k in range(3):
        pts = R.bisect_step(l, r, ls, rs, R.field_final_alpha(pts), R.FINAL_ALPHA)
    for value, mode in rounds:
        pts = R.bisect_step(l, r, ls, rs, value, mode)
    res.update(mid=pts, l=l, r=r, ls=ls, rs=rs)
    return res


# ---- the edge filter -------------------------------------------------------------------------------------------------------------------
def filter_case(E):
    """random edges, and from the front: edges of length exactly 5 * 2^k with scales 2 * 2^k + 3 * 2^k (d = s: kept), with the sum a few ulp
    below (dropped), a NaN end point and a NaN scale"""
    e, _, sc, _ = R.edges(E)
    e, sc = e.copy(), sc.reshape(E, 2).copy()
    for i in range(0, min(E, 40), 4):
        k = f32(2.0 ** (i // 4 - 5))
        for j in range(i, min(E, i + 4)):
            e[j, 0], e[j, 1] = (0, 0, 0), (f32(3) * k, f32(4) * k, 0)
            sc[j] = (f32(2) * k, f32(3) * k)
        if i + 1 < E:
            sc[i + 1, 1] = sc[i + 1, 1] * f32(1 - 2.0 ** -20)
        if i + 2 < E:
            e[i + 2, 0, 2] = np.nan
        if i + 3 < E:
            sc[i + 3, 0] = np.nan
    return e, sc


def run_filter(ME, up, E):
    e, sc = filter_case(E)
    return {"keep": ME.edge_filter(up(e), up(sc)).cpu().numpy()}


def want_filter(E):
    e, sc = filter_case(E)
    return {"keep": R.edge_filter(e, sc)}


# ---- bisection + mesh + export ---------------------------------------------------------------------------------------------------------
def run_mesh(ME, MC, up, E, tmp):
    """bisect_and_build_mesh on synthetic edges and the analytic field, with and without filter / texture; export -> bytes -> load"""
    import os
    import torch
    e, sdf, sc, faces = R.edges(E)
    res = {}

    def query(pts, return_color):
        p = pts.cpu().numpy()
        color = up(R.field_color(p)).to(pts.device) if return_color else None
        return up(R.field_final_alpha(p)).to(pts.device), ME.BISECT_FINAL_ALPHA, color
    for tag, flt, tex in (("plain", False, False), ("full", True, True), ("filter", True, False)):
        mesh = ME.bisect_and_build_mesh(up(e.copy()), up(sdf.copy()), up(sc.copy()), up(faces), query, flt, tex)
        path = os.path.join(tmp, "mesh_%s.ply" % tag)
        mesh.export(path)
        res[tag + "_ply"] = np.frombuffer(open(path, "rb").read(), np.uint8)
        back = MC.load(path, device=mesh.device)
        res[tag + "_v"], res[tag + "_f"] = back.vertices, back.faces
        if tex:
            res[tag + "_c"] = back.vertex_colors
    assert isinstance(mesh._v, torch.Tensor)
    res["colors_edge"] = ME.vertex_colors_u8(up(color_edge_values())).cpu().numpy()
    return res


def color_edge_values():
    return np.array([[0.0, 1.0, 0.5], [1.004, -0.01, 2.0], [np.nan, np.inf, -np.inf], [1e30, -1e30, 255.999 / 255], [-3.5, 300.25, 1e15]], f32)


def want_mesh(E):
    e, sdf, sc, faces = R.edges(E)
    res = {}
    for tag, flt, tex in (("plain", False, False), ("full", True, True), ("filter", True, False)):
        m = R.bisect_and_mesh(e, sdf, sc, faces, R.field_final_alpha, R.field_color, flt, tex)
        res[tag + "_ply"] = np.frombuffer(MR.ply_bytes(m["vertices"], m["faces"], colors=m["colors"]), np.uint8)
        res[tag + "_v"], res[tag + "_f"] = m["vertices"].astype(np.float64), m["faces"]
        if tex:
            res[tag + "_c"] = m["colors"]
    res["colors_edge"] = R.colors_u8(color_edge_values())
    return res
