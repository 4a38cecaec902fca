"""Pictures of a mesh on the GPU: what the reference's mesh_viewer.py asks of Open3D (compute_vertex_normals, then an OpenGL
window), without a display.

    n = vertex_normals(mesh); fn = face_normals(mesh)      # area-weighted, fp64 sums in a fixed order
    img = render(mesh, c2w_list, H, W, fx, fy, cx, cy, mode="shaded")          # (N,3,H,W) float32 on the device
    python -m mesh_render MESH.ply (--cameras cameras.json | --turntable N) --mode shaded --out DIR

The kernels are ``gof_mesh_*`` of libgof_hip.so (csrc/mesh_render.hip, include/gof_mesh_hip.h (g)); the contract is DESIGN.md §3.20:
tensors on a ROCm device in and out, every image a pure function of the mesh and the cameras, bit-equal to a numpy restatement.
Built over mesh_cull's DeviceMesh and view records.  There is no host fallback.
"""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn
import mesh_cull
from mesh_cull import DeviceMesh, raster_views

__all__ = ["vertex_normals", "face_normals", "render", "cameras_from_json", "turntable", "GofShadeParams", "MODES", "main"]

lib = B.lib
_vp, _sz, _i64, _i32 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32
_P64 = C.POINTER(C.c_int64)


class GofShadeParams(C.Structure):
    """Mirror of ``GofShadeParams`` in include/gof_mesh_hip.h."""
    _fields_ = [("mode", C.c_int32), ("flags", C.c_int32), ("base", C.c_double * 3), ("background", C.c_double * 3), ("ambient", C.c_double)]


assert C.sizeof(GofShadeParams) == 64
MODES = {"normal_world": 0, "normal_camera": 1, "color": 2, "shaded": 3}
FLAT, VERTEX_BASE = 1, 2

lib.gof_mesh_render_abi_version.restype = C.c_int
lib.gof_mesh_render_abi_version.argtypes = []
gn.bind(lib, {"gof_mesh_vertex_normals_ws_bytes": [_i64, _i64], "gof_mesh_face_normals_ws_bytes": [], "gof_mesh_render_faces_ws_bytes": [_i64, _i32, _i64],
              "gof_mesh_shade_ws_bytes": []}, {
        "gof_mesh_vertex_normals": [_i64, _vp, _i64, _vp, _vp, _vp, _sz, _vp],
        "gof_mesh_face_normals": [_i64, _vp, _i64, _vp, _vp, _vp, _sz, _vp],
        "gof_mesh_render_faces": [_i64, _vp, _i64, _vp, _i32, _vp, _i64, _vp, _vp, _P64, _vp, _sz, _vp],
        "gof_mesh_shade": [_i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i64, _vp, C.POINTER(GofShadeParams), _vp, _vp, _vp, _sz, _vp]})

# the device seams, by the names the host tests replace per module (tests/test_mesh_render_host.py)
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "mesh_render")
_last = {}


def last_stats():
    return {k: dict(v) for k, v in _last.items()}


def _normals(mesh, who, entry, per_face):
    v, f = mesh_cull._mesh_arrays(mesh, who)
    nv, nf = int(v.size(0)), int(f.size(0))
    with _device_of(v):
        nb = lib.gof_mesh_face_normals_ws_bytes() if per_face else lib.gof_mesh_vertex_normals_ws_bytes(nv, nf)
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        out = torch.empty((nf if per_face else nv, 3), dtype=torch.float32, device=v.device)
        B._check(entry(nv, _ptr(v), nf, _ptr(f), _ptr(out), ws.data_ptr(), nb, _stream()))
    _last[who] = {"vertices": nv, "faces": nf, "workspace_bytes": int(nb)}
    return out


def vertex_normals(mesh):
    """Open3D's compute_vertex_normals for a DeviceMesh (or any object with .vertices / .faces): per vertex the sum of the
    unnormalised face crosses of its incident corners, in ascending (face, corner) order, normalised -> (NV,3) float32 on the device;
    (0,0,1) for a vertex without a face or with a sum that is zero or not finite."""
    return _normals(mesh, "vertex_normals", lib.gof_mesh_vertex_normals, False)


def face_normals(mesh):
    """-> (NF,3) float32 on the device: cross(v1 - v0, v2 - v0) normalised; (0,0,1) for a degenerate face"""
    return _normals(mesh, "face_normals", lib.gof_mesh_face_normals, True)


def render(mesh, c2w_list, H, W, fx, fy, cx, cy, mode="shaded", flat=False, base=(0.8, 0.8, 0.8), ambient=0.25, background=(1, 1, 1), znear=0.01,
           zfar=1e3, convention="opencv", batch=0, aux=False):
    """Pictures of the mesh from every camera -> (N,3,H,W) float32 on the device; with aux=True also {"depth" (N,H,W) float32, "face"
    (N,H,W) int32 (-1: nothing seen), "bary" (N,3,H,W) float32}.  mode: 'normal_world', 'normal_camera', 'color' (the vertex colours),
    'shaded' (a two-sided headlight over `base`: an RGB triple, or 'vertex' for the vertex colours).  flat: the face's normal instead
    of the interpolated vertex normals.  batch: views rendered per call (0: all at once); the face buffer costs 8 bytes of workspace
    per pixel of a batch.  Vertex normals are computed once where the mesh has none and the mode needs them."""
    if mode not in MODES:
        raise ValueError("render: mode must be one of %s, got %r" % (", ".join(sorted(MODES)), mode))
    v, f = mesh_cull._mesh_arrays(mesh, "render")
    rec = raster_views(c2w_list, H, W, fx, fy, cx, cy, znear, zfar, convention)
    H, W, n, nv, nf = max(int(H), 0), max(int(W), 0), len(rec), int(v.size(0)), int(f.size(0))
    stride = H * W
    vertex_base = isinstance(base, str)
    if vertex_base and base != "vertex":
        raise ValueError("render: base must be an RGB triple or 'vertex', got %r" % (base,))
    colors = getattr(mesh, "_c", None)
    normals = getattr(mesh, "_n", None)
    if MODES[mode] != MODES["color"] and not flat and normals is None:
        normals = vertex_normals(mesh)
        if isinstance(mesh, DeviceMesh):
            mesh._n = normals
    P = GofShadeParams()
    P.mode, P.flags = MODES[mode], (FLAT if flat else 0) | (VERTEX_BASE if vertex_base else 0)
    P.base[:] = [0.0, 0.0, 0.0] if vertex_base else [float(x) for x in base]
    P.background[:] = [float(x) for x in background]
    P.ambient = float(ambient)
    b = n if int(batch) <= 0 else int(batch)
    with _device_of(v):
        image = torch.empty((n, 3, H, W), dtype=torch.float32, device=v.device)
        depth = torch.empty((n, H, W), dtype=torch.float32, device=v.device)
        face = torch.empty((n, H, W), dtype=torch.int32, device=v.device)
        bary = torch.empty((n, 3, H, W), dtype=torch.float32, device=v.device) if aux else None
        nb = max(lib.gof_mesh_render_faces_ws_bytes(nf, min(b, n), stride), lib.gof_mesh_shade_ws_bytes())
        if n and lib.gof_mesh_render_faces_ws_bytes(nf, min(b, n), stride) == 0:
            raise RuntimeError("render: bad batch (%d) or image size (%d x %d)" % (int(batch), W, H))
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        records = mesh_cull._records(rec, v.device)
        for v0 in range(0, n, max(b, 1)):
            k = min(b, n - v0)
            r = records[v0 * rec.dtype.itemsize:]
            B._check(lib.gof_mesh_render_faces(nv, _ptr(v), nf, _ptr(f), k, r.data_ptr(), stride, _ptr(depth[v0:]), _ptr(face[v0:]), None,
                                               ws.data_ptr(), nb, _stream()))
            B._check(lib.gof_mesh_shade(nv, _ptr(v), nf, _ptr(f), _ptr(normals) if normals is not None else None,
                                        _ptr(colors) if colors is not None else None, k, r.data_ptr(), stride, _ptr(face[v0:]), C.byref(P),
                                        _ptr(image[v0:]), _ptr(bary[v0:]) if aux else None, ws.data_ptr(), nb, _stream()))
    _last["render"] = {"vertices": nv, "faces": nf, "views": n, "batch": b, "workspace_bytes": int(nb)}
    if aux:
        return image, {"depth": depth, "face": face, "bary": bary}
    return image


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------
def cameras_from_json(path):
    """train.py's cameras.json (utils/camera_utils.py camera_to_JSON: the camera-to-world rotation and position in the OpenCV
    convention, fx, fy, width, height) -> [dict(c2w (4,4) float64, H, W, fx, fy, cx = width / 2, cy = height / 2, name)]"""
    with open(path, encoding="UTF-8") as fh:
        cams = json.load(fh)
    out = []
    for c in cams:
        m = np.eye(4)
        m[:3, :3] = np.asarray(c["rotation"], np.float64).reshape(3, 3)
        m[:3, 3] = np.asarray(c["position"], np.float64).reshape(3)
        W, H = int(c["width"]), int(c["height"])
        out.append(dict(c2w=m, H=H, W=W, fx=float(c["fx"]), fy=float(c["fy"]), cx=W / 2.0, cy=H / 2.0, name=str(c.get("img_name", c.get("id", len(out))))))
    return out


def turntable(mesh, n, H, W, fov_deg=50, up=(0.0, 0.0, 1.0), elevation_deg=20.0):
    """n OpenCV camera-to-world poses on a circle around the centre of the vertex bounding box, at 1.5 x its half diagonal, raised by
    20 degrees and looking at the centre -> dict(c2w [n x (4,4)], H, W, fx = fy from the horizontal field of view, cx, cy, convention)"""
    v, _ = mesh_cull._mesh_arrays(mesh, "turntable", need_faces=False)
    pts = v.detach().cpu().numpy().astype(np.float64)
    pts = pts[np.isfinite(pts).all(axis=1)]
    lo, hi = (pts.min(axis=0), pts.max(axis=0)) if len(pts) else (np.zeros(3), np.zeros(3))
    centre, radius = (lo + hi) / 2.0, 1.5 * float(np.linalg.norm(hi - lo)) / 2.0
    radius = radius if radius > 0 else 1.0
    upv = np.asarray(up, np.float64) / np.linalg.norm(up)
    ref = np.eye(3)[int(np.argmin(np.abs(upv)))]
    e0 = np.cross(upv, ref)
    e0 /= np.linalg.norm(e0)
    e1 = np.cross(upv, e0)
    el = math.radians(elevation_deg)
    poses = []
    for k in range(int(n)):
        a = 2.0 * math.pi * k / max(int(n), 1)
        eye = centre + radius * (math.cos(el) * (math.cos(a) * e0 + math.sin(a) * e1) + math.sin(el) * upv)
        fwd = (centre - eye) / np.linalg.norm(centre - eye)                 # OpenCV: +z forward, +x right, +y down
        right = np.cross(fwd, upv)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, eye
        poses.append(m)
    f = (W / 2.0) / math.tan(math.radians(fov_deg) / 2.0)
    return dict(c2w=poses, H=int(H), W=int(W), fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, convention="opencv", radius=radius, centre=centre)


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    """python -m mesh_render MESH.ply (--cameras cameras.json | --turntable N) --mode M --out DIR [--size WxH] [--scale s]"""
    import argparse
    import image_writer
    ap = argparse.ArgumentParser(prog="mesh_render")
    ap.add_argument("mesh")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--cameras", type=str, help="train.py's cameras.json")
    g.add_argument("--turntable", type=int, help="that many views on a circle around the mesh")
    ap.add_argument("--mode", choices=sorted(MODES), default="shaded")
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--vertex-base", action="store_true", help="shaded: the vertex colours as the base colour")
    ap.add_argument("--out", type=str, required=True)
    ap.add_argument("--size", type=str, default="800x600", help="WxH of the turntable views")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the image size and the intrinsics")
    a = ap.parse_args(argv)
    mesh = mesh_cull.load(a.mesh)
    s = float(a.scale)
    if a.turntable is not None:
        W, H = (int(x) for x in a.size.lower().split("x"))
        t = turntable(mesh, a.turntable, int(round(H * s)), int(round(W * s)))
        groups = [(t["c2w"], t["H"], t["W"], t["fx"], t["fy"], t["cx"], t["cy"])]
        zfar = 4.0 * t["radius"] + 1.0
    else:
        cams = cameras_from_json(a.cameras)
        groups = [([c["c2w"]], int(round(c["H"] * s)), int(round(c["W"] * s)), c["fx"] * s, c["fy"] * s, int(round(c["W"] * s)) / 2.0, int(round(c["H"] * s)) / 2.0)
                  for c in cams]
        zfar = 1e3
    os.makedirs(a.out, exist_ok=True)
    k = 0
    for c2w, H, W, fx, fy, cx, cy in groups:
        img = render(mesh, c2w, H, W, fx, fy, cx, cy, mode=a.mode, flat=a.flat, base="vertex" if a.vertex_base else (0.8, 0.8, 0.8), zfar=zfar, batch=8)
        for i in range(int(img.size(0))):
            image_writer.save_image(img[i], os.path.join(a.out, "%05d.png" % k))
            k += 1
    image_writer.flush()
    print("mesh_render: wrote %d images to %s" % (k, a.out))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main(sys.argv[1:]))
