"""The mesh extraction on the device: the view loop with its reduction, the tetra points, the bisection and the mesh.

``evaluate_alpha`` is the reference's ``evaluage_alpha`` (extract_mesh.py:17-34): the opacity field at `points` is the minimum over
all training views of ``alpha_integrated``, optionally with the colour of the view that attains it.  The reference materialises
``ones`` / ``zeros`` outputs per view and combines them with ``torch.min`` / ``torch.where`` (four passes over N points per view);
here the point pass of ``integrate`` min-combines into the running buffers in its final store (``integrate_min_into`` ->
``gof_integrate_points_min``), with the Gaussian side of every view served from the per-view cache.  Same values, bit for bit
(``tests/test_mesh_extraction_gpu.py``).

``get_tetra_points`` is ``GaussianModel.get_tetra_points`` (scene/gaussian_model.py:433-463 with ``get_frustum_mask``, :31-72) and
``marching_tetrahedra_with_binary_search`` the script's function of that name (extract_mesh.py:36-120), both drop-ins over
``gof_tetra_points_*`` / ``gof_bisect_step`` / ``gof_edge_filter`` of libgof_hip.so (csrc/extract.hip, include/gof_extract_hip.h); the
contract is DESIGN.md §3.11: no views x points tensor, one launch per bisection round, the mesh a ``mesh_cull.DeviceMesh`` that never
visits the host before its export -- and no trimesh.  Host tensors are refused; there is no fallback.  Stated deviations (DESIGN.md
§7): the frustum decisions are made in fp64 instead of fp32 GEMMs, the corner arithmetic has a fixed order, the PLY carries ``red
green blue`` without ``alpha``.  ``launch/run_reference_script.py`` binds all three in place of the reference's own.
"""
import ctypes as C
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
from diff_gaussian_rasterization import integrate_min_into
import gof_native as gn

__all__ = ["evaluate_alpha", "get_tetra_points", "tetra_points", "bisect_step", "edge_filter", "marching_tetrahedra_with_binary_search",
           "GofFrustumView", "last_stats"]

lib = B.lib
_vp, _sz, _i64, _i32, _f64 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_double
_P64 = C.POINTER(C.c_int64)


class GofFrustumView(C.Structure):
    """Mirror of ``GofFrustumView`` in include/gof_extract_hip.h."""
    _fields_ = [("m", C.c_double * 12), ("fx", C.c_double), ("fy", C.c_double)]


_VIEW_DTYPE = np.dtype([("m", "<f8", (12,)), ("fx", "<f8"), ("fy", "<f8")])
assert _VIEW_DTYPE.itemsize == C.sizeof(GofFrustumView) == 112

gn.bind(lib, {"gof_tetra_points_ws_bytes": [_i64]}, {
        "gof_tetra_points_count": [_i64, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f64, _f64, _vp, _sz, _P64, _vp],
        "gof_tetra_points_emit": [_i64, _vp, _vp, _vp, _vp, _sz, _i64, _vp, _vp, _vp],
        "gof_bisect_step": [_i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
        "gof_edge_filter": [_i64, _vp, _vp, _vp, _vp]})

BISECT_FINAL_ALPHA, BISECT_FIRST, BISECT_ALPHA = 0, 1, 2
_last = {}

# the device seams, by the names the host tests replace (tests/test_extract_host.py); one definition each: gof_native
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr


def last_stats():
    """Statistics of the last tetra_points call: candidates, kept points, views, workspace bytes."""
    return {k: dict(v) for k, v in _last.items()}


def _tensor(t, who, what, dtypes, cols=None):
    return gn.rows(t, who, what, dtypes, cols, limit=2 ** 31, shape_first=False, on_device=_on_device)


def _reduce_views(points, views, gaussians, pipeline, background, kernel_size, return_color=False, integrate=None, progress=True):
    """-> (final_alpha, final_color or None): the minimum over the views of alpha_integrated (the transmittance), as the loop leaves it"""
    if integrate is None:
        from gaussian_renderer import integrate
    pts = points.detach().to(device="cuda", dtype=torch.float32).contiguous()
    final_alpha = torch.ones((pts.shape[0],), dtype=torch.float32, device=pts.device)                  # extract_mesh.py:18
    final_color = torch.ones((pts.shape[0], 3), dtype=torch.float32, device=pts.device) if return_color else None   # :20
    it = views
    if progress:
        try:
            from tqdm import tqdm
            it = tqdm(views, desc="Rendering progress")                                                   # :23
        except ImportError:
            pass
    with integrate_min_into(final_alpha, final_color):
        for view in it:
            integrate(pts, view, gaussians, pipeline, background, kernel_size=kernel_size)                # :24-29, reduction fused
    return final_alpha, final_color


@torch.no_grad()
def evaluate_alpha(points, views, gaussians, pipeline, background, kernel_size, return_color=False, integrate=None, progress=True):
    final_alpha, final_color = _reduce_views(points, views, gaussians, pipeline, background, kernel_size, return_color, integrate, progress)
    alpha = 1 - final_alpha                                                                               # :31
    if return_color:
        return alpha, final_color
    return alpha


# ---- the tetra points (scene/gaussian_model.py:31-72, 433-463) ------------------------------------------------------------------------
def frustum_records(views):
    """-> (records: numpy array of GofFrustumView, W, H): rows 0..2 of world_view_transform.T and focal_x, focal_y, the fp32 values
    widened to fp64; W, H are view 0's for all views (gaussian_model.py:32)"""
    rec = np.zeros(len(views), _VIEW_DTYPE)
    for i, cam in enumerate(views):
        wvt = cam.world_view_transform
        if isinstance(wvt, torch.Tensor):
            wvt = wvt.detach().cpu().numpy()
        w2c = np.asarray(wvt, np.float32).reshape(4, 4).T.astype(np.float64)
        rec[i] = (w2c[:3].reshape(12), float(np.float32(cam.focal_x)), float(np.float32(cam.focal_y)))
    W, H = (int(views[0].image_width), int(views[0].image_height)) if len(views) else (0, 0)
    return rec, W, H


def tetra_points(xyz, scaling, rotation, records, W, H, near=0.02, far=1e6):
    """xyz (P,3), scaling (P,3) (activated, with the 3D filter), rotation (P,4) (raw) float32 on a ROCm device; records: frustum_records'
    array -> (points (K,3), scales (K,)) there: the candidates some view sees, in candidate order (a count call, then an emit call
    into tensors of exactly K rows)."""
    x = _tensor(xyz, "tetra_points", "xyz", (torch.float32,), 3)
    s = _tensor(scaling, "tetra_points", "scaling", (torch.float32,), 3)
    q = _tensor(rotation, "tetra_points", "rotation", (torch.float32,), 4)
    P = int(x.size(0))
    if s.size(0) != P or q.size(0) != P or s.device != x.device or q.device != x.device:
        raise RuntimeError("tetra_points: xyz, scaling and rotation must have one row per Gaussian, on one device")
    if 9 * P + 1 >= 2 ** 31:
        raise RuntimeError("tetra_points: at most %d Gaussians" % ((2 ** 31 - 2) // 9))
    rec = np.ascontiguousarray(records, _VIEW_DTYPE).reshape(-1)
    n = len(rec)
    with _device_of(x):
        dev_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(x.device) if n else None
        nb = lib.gof_tetra_points_ws_bytes(P)
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        cnt = C.c_int64()
        B._check(lib.gof_tetra_points_count(P, _ptr(x), _ptr(s), _ptr(q), n, _ptr(dev_rec), int(W), int(H), float(near), float(far),
                                            ws.data_ptr(), nb, C.byref(cnt), _stream()))
        K = int(cnt.value)
        points = torch.empty((K, 3), dtype=torch.float32, device=x.device)
        scales = torch.empty((K,), dtype=torch.float32, device=x.device)
        B._check(lib.gof_tetra_points_emit(P, _ptr(x), _ptr(s), _ptr(q), ws.data_ptr(), nb, K, _ptr(points), _ptr(scales), _stream()))
    _last["tetra_points"] = {"gaussians": P, "candidates": 9 * P, "kept": K, "views": n, "workspace_bytes": int(nb)}
    return points, scales


@torch.no_grad()
def get_tetra_points(self, views, near=0.02, far=1e6):
    """GaussianModel.get_tetra_points, a drop-in -> (points (K,3), scales (K,1))"""
    rec, W, H = frustum_records(views)
    points, scales = tetra_points(self.get_xyz.detach(), self.get_scaling_with_3D_filter.detach(), self._rotation.detach(), rec, W, H, near, far)
    return points, scales[:, None]


# ---- the bisection (extract_mesh.py:73-102) and the filter (:85-86, 115) ----------------------------------------------------------------
def bisect_step(left_pts, right_pts, left_sdf, right_sdf, value, mode, mid_out=None):
    """One round in place, one launch.  left_pts, right_pts (E,3), left_sdf, right_sdf (E,), value (E,) float32 contiguous on a ROCm
    device; mode BISECT_FINAL_ALPHA: value is the transmittance the view reduction left, BISECT_ALPHA: value is 1 - that,
    BISECT_FIRST: only the midpoints (the sdf tensors and value may be None) -> mid_out (E,3): the next query points."""
    l = _tensor(left_pts, "bisect_step", "left_pts", (torch.float32,), 3)
    E = int(l.size(0))
    tensors = [(right_pts, "right_pts", (E, 3))]
    if mode != BISECT_FIRST:
        tensors += [(left_sdf, "left_sdf", (E,)), (right_sdf, "right_sdf", (E,)), (value, "value", (E,))]
    for t, what, shape in tensors + [(left_pts, "left_pts", (E, 3))] + ([(mid_out, "mid_out", (E, 3))] if mid_out is not None else []):
        _tensor(t, "bisect_step", what, (torch.float32,))
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != l.device:
            raise RuntimeError("bisect_step: %s must be a contiguous tensor of shape %s on left_pts' device (the step is in place)" % (what, shape))
    with _device_of(l):
        if mid_out is None:
            mid_out = torch.empty((E, 3), dtype=torch.float32, device=l.device)
        first = mode == BISECT_FIRST
        B._check(lib.gof_bisect_step(E, _ptr(left_pts), _ptr(right_pts), None if first else _ptr(left_sdf), None if first else _ptr(right_sdf),
                                     None if first else _ptr(value), int(mode), _ptr(mid_out), _stream()))
    return mid_out


def edge_filter(end_points, end_scales):
    """end_points (E,2,3), end_scales (E,2) or (E,2,1) float32 on a ROCm device -> keep (E,) bool there: |left - right| <= the scales' sum"""
    p = _tensor(end_points, "edge_filter", "end_points", (torch.float32,))
    s = _tensor(end_scales, "edge_filter", "end_scales", (torch.float32,))
    E = int(p.size(0))
    if tuple(p.shape) != (E, 2, 3) or s.numel() != 2 * E or s.device != p.device:
        raise RuntimeError("edge_filter: end_points must be (E, 2, 3) and end_scales (E, 2), on one device")
    with _device_of(p):
        keep = torch.empty(E, dtype=torch.uint8, device=p.device)
        B._check(lib.gof_edge_filter(E, _ptr(p), _ptr(s), _ptr(keep), _stream()))
    return keep.bool()


def vertex_colors_u8(color):
    """extract_mesh.py:108 on the device: (color * 255) truncated toward zero; outside [0, 256) the low 8 bits of the truncated
    integer (two's complement), and 0 for NaN and for |value| >= 2^62"""
    c = color * 255
    c = torch.where(c.abs() < 2.0 ** 62, c, torch.zeros_like(c))
    return (c.to(torch.int64) & 255).to(torch.uint8)


def bisect_and_build_mesh(end_points, end_sdf, end_scales, faces, query, filter_mesh=False, texture_mesh=False, n_binary_steps=8,
                          on_step=None):
    """extract_mesh.py:73-118 after marching tetrahedra, on the device: end_points (E,2,3), end_sdf (E,2,1), end_scales (E,2,1), faces
    (F,3); query(points, return_color, final) -> (value, mode[, color]): the field at the points as BISECT_FINAL_ALPHA or
    BISECT_ALPHA values -> a mesh_cull.DeviceMesh of the 8th round's midpoints."""
    import mesh_cull
    E = int(end_points.shape[0])
    keep = edge_filter(end_points, end_scales) if filter_mesh else None              # :85-86 (before the end points move)
    left_pts, right_pts = end_points[:, 0, :].contiguous(), end_points[:, 1, :].contiguous()
    left_sdf, right_sdf = end_sdf[:, 0, :].reshape(E).contiguous(), end_sdf[:, 1, :].reshape(E).contiguous()
    points = bisect_step(left_pts, right_pts, None, None, None, BISECT_FIRST)        # :91 of round 0
    for step in range(n_binary_steps):
        if on_step is not None:
            on_step(step)
        value, mode = query(points, False)[:2]
        points = bisect_step(left_pts, right_pts, left_sdf, right_sdf, value.reshape(E).contiguous(), mode, mid_out=points)     # :91-102
    colors = vertex_colors_u8(query(points, True)[2]) if texture_mesh else None      # :106-108
    mesh = mesh_cull.DeviceMesh.from_device(points, faces, colors=colors)
    if filter_mesh:
        mesh.compact(keep)                                    # :114-118: update_vertices, then update_faces
    return mesh


@torch.no_grad()
def marching_tetrahedra_with_binary_search(model_path, name, iteration, views, gaussians, pipeline, background, kernel_size, filter_mesh,
                                           texture_mesh, near, far, evaluate_alpha=None):
    """extract_mesh.py:36-120, a drop-in: the same cells.pt, prints, rounds and output path; the mesh is written once, after round 7.
    evaluate_alpha: the script's `evaluage_alpha` or whatever stands for it (returns alpha [, color]); None = this module's view
    loop, whose transmittance goes into the bisection as it is."""
    from tetmesh import marching_tetrahedra
    render_path = os.path.join(model_path, name, "ours_{}".format(iteration), "fusion")
    os.makedirs(render_path, exist_ok=True)
    points, points_scale = gaussians.get_tetra_points(views, near, far)              # :43 (the launcher binds the method to get_tetra_points above)
    if os.path.exists(os.path.join(render_path, "cells.pt")):
        print("load existing cells")
        cells = torch.load(os.path.join(render_path, "cells.pt"))
    else:
        print("create cells and save")
        try:
            from tetranerf.utils.extension import cpp                                # :13 (the launcher's stand-in where tetranerf is not installed)
            cells = cpp.triangulate(points)
        except ImportError:
            import delaunay                                                          # what that stand-in calls for device tensors
            cells = delaunay.triangulate(points.detach().float())
        torch.save(cells, os.path.join(render_path, "cells.pt"))

    def query(pts, return_color):
        if evaluate_alpha is None:
            fa, color = _reduce_views(pts, views, gaussians, pipeline, background, kernel_size, return_color)
            return fa, BISECT_FINAL_ALPHA, color
        if return_color:
            alpha, color = evaluate_alpha(pts, views, gaussians, pipeline, background, kernel_size, return_color=True)
            return alpha, BISECT_ALPHA, color
        return evaluate_alpha(pts, views, gaussians, pipeline, background, kernel_size), BISECT_ALPHA, None

    value, mode, _ = query(points, False)
    alpha = (1 - value) if mode == BISECT_FINAL_ALPHA else value
    vertices = points.cuda()[None]
    tets = cells.cuda().long()
    print(vertices.shape, tets.shape, alpha.shape)
    sdf = (alpha - 0.5)[None]
    torch.cuda.empty_cache()
    verts_list, scale_list, faces_list, _ = marching_tetrahedra(vertices, tets, sdf, points_scale[None])
    torch.cuda.empty_cache()
    end_points, end_sdf = verts_list[0]
    mesh = bisect_and_build_mesh(end_points, end_sdf, scale_list[0], faces_list[0], query, filter_mesh, texture_mesh,
                                 on_step=lambda step: print("binary search in step {}".format(step)))
    mesh.export(os.path.join(render_path, "mesh_binary_search_7.ply"))
    return mesh
