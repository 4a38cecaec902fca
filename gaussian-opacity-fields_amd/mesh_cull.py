"""Mesh culling of the DTU evaluation on the GPU: the reference's evaluate_dtu_mesh.py:59-131 without trimesh, scikit-image and cv2.

    packed = dilate_mask(mask, r)                          # :114-115  binary_dilation(mask / 256., disk(6)), bit-packed
    keep = cull_vertices(vertices, views)                  # :105-126  every vertex against every view's dilated mask
    out = compact_mesh(keep, faces, attrs)                 # :127-130  update_vertices / update_faces
    mesh = load(path); mesh = cull_mesh(cameras, mesh); mesh.export(path)       # trimesh.load, the script's cull_mesh, .export
    poses = load_dtu_camera(DTU)                           # :59-75    cv2.decomposeProjectionMatrix

The kernels are ``gof_mesh_*`` of libgof_hip.so (csrc/mesh_cull.hip, include/gof_mesh_hip.h); the contract is DESIGN.md §3.10: tensors
on a ROCm device in and out, results bit-equal to numpy's.  There is no host fallback: host tensors are refused.  Two stated
deviations: the keep / drop decisions are made in fp64 instead of fp32 GEMMs, and the world-to-camera matrix itself
is used instead of the script's fp32 inverse of its inverse.
"""
import ctypes as C
import functools
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn
import mesh_eval

__all__ = ["dilate_mask", "cull_vertices", "compact_mesh", "last_stats", "view_matrix", "DeviceMesh", "load", "cull_mesh",
           "load_dtu_camera", "decompose_projection_matrix", "GofCullView"]

lib = B.lib
_vp, _sz, _i64, _i32 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32
_P64 = C.POINTER(C.c_int64)


class GofCullView(C.Structure):
    """Mirror of ``GofCullView`` in include/gof_mesh_hip.h."""
    _fields_ = [("m", C.c_double * 12), ("W", C.c_int32), ("H", C.c_int32), ("mask_offset", C.c_int64), ("row_words", C.c_int64)]


_VIEW_DTYPE = np.dtype([("m", "<f8", (12,)), ("W", "<i4"), ("H", "<i4"), ("mask_offset", "<i8"), ("row_words", "<i8")])
assert _VIEW_DTYPE.itemsize == C.sizeof(GofCullView) == 120

lib.gof_mesh_mask_row_words.restype = _i64
lib.gof_mesh_mask_row_words.argtypes = [_i32]
gn.bind(lib, {"gof_mesh_cull_ws_bytes": [_i64], "gof_mesh_compact_ws_bytes": [_i64, _i64], "gof_densify_ws_bytes": [_i64]}, {
        "gof_mesh_dilate": [_i32, _i32, _vp, _i32, _i32, _vp, _vp],
        "gof_mesh_cull": [_i64, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _sz, _vp],
        "gof_mesh_compact": [_i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _P64, _vp],
        "gof_compact_rows": [_i64, _vp, _vp, _vp, _vp, _sz, _P64, _vp],
        "gof_rows_gather": [_i64, _i32, _vp, _vp, _vp, _vp, _vp]})

MAX_RADIUS = 31
_last = {}


def last_stats():
    """Statistics of the last dilate_mask / cull_vertices / compact_mesh calls (one sub-dictionary each): sizes, counts, workspace bytes."""
    return {k: dict(v) for k, v in _last.items()}


# the device seams, by the names the host tests replace per module (tests/test_mesh_cull_host.py); one definition each: gof_native
# (tsdf_fusion and delaunay bind them the same way)
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "mesh_cull")


def _tensor(t, who, what, dtypes, cols=None):
    """gn.rows with this module's limit (gof_mesh_* take at most 2^31 - 2 rows) and its order of complaints"""
    return gn.rows(t, who, what, dtypes, cols, limit=2 ** 31 - 1, shape_first=False, on_device=_on_device)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
def mask_row_words(W):
    return (int(W) + 63) // 64


def dilate_mask(mask, r=6, out=None):
    """evaluate_dtu_mesh.py:114-115: mask (H,W) float32 or uint8 on a ROCm device; a pixel is set iff mask / 256. != 0 ->
    (H, ceil(W/64)) int64 there: bit x % 64 of word x // 64 of row y = the disk dilation of radius r at (y, x); pad bits zero.
    `out`: a contiguous int64 tensor of that many words to write into."""
    m = _tensor(mask, "dilate_mask", "mask", (torch.float32, torch.uint8))
    if m.dim() != 2 or m.numel() == 0:
        raise RuntimeError("dilate_mask: mask must have dimensions (H, W), both at least 1")
    r = int(r)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError("dilate_mask: the radius must lie in [0, %d], got %d" % (MAX_RADIUS, r))
    H, W = int(m.size(0)), int(m.size(1))
    nw = mask_row_words(W)
    with _device_of(m):
        if out is None:
            out = torch.empty((H, nw), dtype=torch.int64, device=m.device)
        elif out.dtype != torch.int64 or out.numel() != H * nw or not out.is_contiguous() or out.device != m.device:
            raise RuntimeError("dilate_mask: out must be a contiguous int64 tensor of %d words on the mask's device" % (H * nw))
        B._check(lib.gof_mesh_dilate(W, H, m.data_ptr(), 1 if m.dtype == torch.uint8 else 0, r, out.data_ptr(), _stream()))
    _last["dilate"] = {"width": W, "height": H, "radius": r, "row_words": nw}
    return out.view(H, nw)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
def view_matrix(focal_x, focal_y, W, H, world_view_transform):
    """m (3,4) float64 = rows 0..2 of K W2C: K = the script's intrinsic (:94-98: focal_x, focal_y, W / 2., H / 2. stored in a float32
    matrix), W2C = world_view_transform.T in float32.  K has two entries per row: the product is written out, no BLAS."""
    wvt = world_view_transform
    if isinstance(wvt, torch.Tensor):
        wvt = wvt.detach().cpu().numpy()
    w2c = np.asarray(wvt, np.float32).reshape(4, 4).T.astype(np.float64)
    fx, fy, cx, cy = (float(np.float32(v)) for v in (focal_x, focal_y, W / 2.0, H / 2.0))
    return np.stack([fx * w2c[0] + cx * w2c[2], fy * w2c[1] + cy * w2c[2], w2c[2]])


def cull_vertices(vertices, views):
    """evaluate_dtu_mesh.py:105-126 in one launch: vertices (NV,3) float32 on a ROCm device; views: a sequence of (m, W, H, packed)
    with m (3,4) float64 (view_matrix) and packed = dilate_mask's result for that view -> keep (NV,) bool there: no view drops it."""
    v = _tensor(vertices, "cull_vertices", "vertices", (torch.float32,), 3)
    nv, n = int(v.size(0)), len(views)
    rec = np.zeros(n, _VIEW_DTYPE)
    packed, off = [], 0
    for i, (m, W, H, p) in enumerate(views):
        p = _tensor(p, "cull_vertices", "a packed mask", (torch.int64,))
        if p.device != v.device:
            raise RuntimeError("cull_vertices: vertices and masks are on different devices")
        W, H = int(W), int(H)
        if W < 1 or H < 1 or p.numel() != H * mask_row_words(W):
            raise RuntimeError("cull_vertices: view %d: a mask of %d words for an image of %d x %d" % (i, p.numel(), W, H))
        rec[i] = (np.asarray(m, np.float64).reshape(12), W, H, off, mask_row_words(W))
        packed.append(p.reshape(-1))
        off += p.numel()
    with _device_of(v):
        if n == 0:
            masks = None
        elif n == 1 or all(packed[i].data_ptr() == packed[0].data_ptr() + 8 * int(rec["mask_offset"][i]) for i in range(n)):
            masks = packed[0]                 # (cull_mesh dilates into one buffer: nothing to copy)
        else:
            masks = torch.cat(packed)
        records = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(v.device) if n else None
        nb = lib.gof_mesh_cull_ws_bytes(nv)
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        keep = torch.empty(nv, dtype=torch.uint8, device=v.device)
        B._check(lib.gof_mesh_cull(nv, _ptr(v), n, _ptr(records), _ptr(masks), off, _ptr(keep), ws.data_ptr(), nb, _stream()))
    _last["cull"] = {"vertices": nv, "views": n, "mask_words": int(off), "workspace_bytes": int(nb)}
    return keep.bool()


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def _gather(rows, t):
    """t[rows] for a 2-D tensor whose rows are whole 4-byte words, through gof_rows_gather (the bytes travel as float32 words)"""
    n = int(rows.numel())
    src = t.contiguous()
    if n == 0:
        return torch.empty((0, int(src.size(1))), dtype=src.dtype, device=src.device)
    words = src.view(torch.float32) if src.dtype != torch.float32 else src
    per = int(words.size(1))
    out = torch.empty((n, per), dtype=torch.float32, device=t.device)
    if n:
        B._check(lib.gof_rows_gather(n, per, rows.data_ptr(), words.data_ptr(), None, out.data_ptr(), _stream()))
    return out.view(t.dtype) if t.dtype != torch.float32 else out


def compact_mesh(keep, faces, attrs=(), drop_faces=True):
    """evaluate_dtu_mesh.py:127-130: keep (NV,) bool / uint8, faces (NF,3) int32, attrs: 2-D tensors of NV rows (whole 4-byte words per
    row), all on one ROCm device -> dict(rows (K,) int32: the kept vertices in order; attrs: their rows; face_keep (NF,) bool: all
    three vertices kept; faces (M,3) int32: drop_faces: the kept faces renumbered, else every face with removed vertices -> 0)."""
    k = _tensor(keep, "compact_mesh", "keep", (torch.bool, torch.uint8))
    k = k.view(torch.uint8) if k.dtype == torch.bool else k
    f = _tensor(faces, "compact_mesh", "faces", (torch.int32,), 3)
    if k.dim() != 1 or f.device != k.device:
        raise RuntimeError("compact_mesh: keep must be (NV,) and on the faces' device")
    nv, nf = int(k.numel()), int(f.size(0))
    for a in attrs:
        if a.dim() != 2 or a.size(0) != nv or a.device != k.device or (a.size(1) * a.element_size()) % 4:
            raise RuntimeError("compact_mesh: an attribute must be (NV, C) with whole 4-byte words per row, on keep's device")
    with _device_of(k):
        nb = lib.gof_mesh_compact_ws_bytes(nv, nf)
        ws = torch.empty(nb, dtype=torch.uint8, device=k.device)
        rows = torch.empty(nv, dtype=torch.int32, device=k.device)
        out_faces = torch.empty((nf, 3), dtype=torch.int32, device=k.device)
        face_keep = torch.empty(nf, dtype=torch.uint8, device=k.device)
        counts = (C.c_int64 * 2)()
        B._check(lib.gof_mesh_compact(nv, _ptr(k), nf, _ptr(f), 1 if drop_faces else 0, _ptr(rows), _ptr(out_faces), _ptr(face_keep),
                                      ws.data_ptr(), nb, counts, _stream()))
        rows = rows[:counts[0]]
        out = {"rows": rows, "faces": out_faces[:counts[1]], "face_keep": face_keep.bool(), "attrs": [_gather(rows, a) for a in attrs]}
    _last["compact"] = {"vertices": nv, "faces": nf, "kept_vertices": int(counts[0]), "kept_faces": int(counts[1]), "workspace_bytes": int(nb)}
    return out


def _compact_rows(keep_u8):
    """(N,) uint8 -> the indices of its non-zero entries, in order (gof_compact_rows)"""
    n = int(keep_u8.numel())
    nb = lib.gof_densify_ws_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=keep_u8.device)
    out = torch.empty(n, dtype=torch.int32, device=keep_u8.device)
    cnt = C.c_int64()
    B._check(lib.gof_compact_rows(n, _ptr(keep_u8), None, _ptr(out), ws.data_ptr(), nb, C.byref(cnt), _stream()))
    return out[:cnt.value]


# ---- the mesh object -----------------------------------------------------------------------------------------------------------------
class DeviceMesh:
    """What evaluate_dtu_mesh.py asks of a trimesh.Trimesh, with the arrays on the device: vertices fp64 (N,3), faces int32 (M,3),
    optional normals float32 (N,3) and colours uint8 (N,4: red green blue + a pad byte, one 4-byte word per vertex)."""

    def __init__(self, vertices, faces, normals=None, colors=None, device=None):
        self.device = torch.device(device) if device is not None else _device()
        v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
        n = len(v)
        c = None
        if colors is not None:
            c = np.zeros((n, 4), np.uint8)
            c[:, :3] = np.asarray(colors, np.uint8).reshape(n, -1)[:, :3]
        self._set_tensors(self._up(v), self._up(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)),
                          None if normals is None else self._up(np.ascontiguousarray(normals, np.float32).reshape(n, 3)),
                          None if c is None else self._up(c))

    def _set_tensors(self, v, f, n, c):
        """the one place the fields are set: fp64 (N,3), int32 (M,3), float32 (N,3) or None, uint8 (N,4) or None, on self.device"""
        self._v, self._f, self._n, self._c = v, f, n, c

    @classmethod
    def from_device(cls, vertices, faces, normals=None, colors=None):
        """A mesh over tensors that are on a ROCm device already, with no host round trip: vertices (N,3) float32 or float64, faces
        (M,3) int32 or int64, optional normals (N,3) float32 and colours (N,3) or (N,4) uint8 (red green blue first)."""
        v = _tensor(vertices, "DeviceMesh.from_device", "vertices", (torch.float32, torch.float64), 3)
        f = _tensor(faces, "DeviceMesh.from_device", "faces", (torch.int32, torch.int64), 3)
        n = int(v.size(0))
        nrm = col = None
        if normals is not None:
            nrm = _tensor(normals, "DeviceMesh.from_device", "normals", (torch.float32,), 3)
        if colors is not None:
            c = _tensor(colors, "DeviceMesh.from_device", "colors", (torch.uint8,))
            if c.dim() != 2 or c.size(1) not in (3, 4):
                raise RuntimeError("DeviceMesh.from_device: colors must have dimensions (N, 3) or (N, 4)")
            col = torch.cat([c[:, :3], torch.zeros((int(c.size(0)), 1), dtype=torch.uint8, device=c.device)], dim=1).contiguous()
        for a, rows in ((f, None), (nrm, n), (col, n)):
            if a is not None and (a.device != v.device or (rows is not None and a.size(0) != rows)):
                raise RuntimeError("DeviceMesh.from_device: every tensor must be on the vertices' device, attributes with one row per vertex")
        mesh = cls.__new__(cls)                               # (no host arrays to upload: __init__'s other half, the same setter)
        mesh.device = v.device
        mesh._set_tensors(v.to(torch.float64), f.to(torch.int32), nrm, col)
        return mesh

    def _up(self, a):
        return torch.from_numpy(a).to(self.device)

    def _mask(self, mask, n, who):
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask, bool)))
        if m.dtype not in (torch.bool, torch.uint8) or m.dim() != 1 or m.numel() != n:
            raise ValueError("%s: the mask must be boolean with %d entries" % (who, n))
        m = m.to(self.device).contiguous()
        return m.view(torch.uint8) if m.dtype == torch.bool else m

    # trimesh's getters return host arrays: the script's `mesh.vertices * s` and `@ r.T + t` run in numpy, bit for bit as with trimesh
    @property
    def vertices(self):
        return self._v.cpu().numpy()

    @vertices.setter
    def vertices(self, value):
        a = np.ascontiguousarray(value, np.float64)
        if a.shape != tuple(self._v.shape):
            raise ValueError("DeviceMesh.vertices: expected %s, got %s" % (tuple(self._v.shape), a.shape))
        self._v = self._up(a)

    @property
    def faces(self):
        return self._f.cpu().numpy()

    @property
    def vertex_normals(self):
        return None if self._n is None else self._n.cpu().numpy()

    @property
    def vertex_colors(self):
        return None if self._c is None else self._c.cpu().numpy()[:, :3]

    def _attrs(self):
        return [a for a in (self._v, self._n, self._c) if a is not None]

    def _set_attrs(self, new):
        it = iter(new)
        self._v = next(it)
        if self._n is not None:
            self._n = next(it)
        if self._c is not None:
            self._c = next(it)

    def _apply(self, keep_u8, drop_faces):
        out = compact_mesh(keep_u8, self._f, self._attrs(), drop_faces=drop_faces)
        self._set_attrs(out["attrs"])
        self._f = out["faces"].contiguous()

    def compact(self, keep):
        """keep the vertices with keep[i] (bool or uint8, (N,)) and the faces between them, renumbered: update_vertices(keep) followed
        by update_faces(keep[faces].all(1)) in one compaction"""
        self._apply(self._mask(keep, int(self._v.size(0)), "compact"), True)

    def update_vertices(self, mask):
        """trimesh's: keep vertices[mask] and renumber the faces (the index of a removed vertex becomes 0: update_faces removes those)"""
        self._apply(self._mask(mask, int(self._v.size(0)), "update_vertices"), False)

    def update_faces(self, mask):
        """trimesh's: keep faces[mask]"""
        m = self._mask(mask, int(self._f.size(0)), "update_faces")
        with _device_of(m):
            self._f = _gather(_compact_rows(m), self._f)

    # ---- connected components (mesh_components.py).  There is no split(): a list of 10^5 mesh objects is what these
    # methods replace -- select with keep_components, or index with components().face_comp
    def components(self, connectivity="edge"):
        """-> mesh_components.Components: face_comp (M,) int32 on the device (components numbered in the order of their first face) and
        the host arrays faces, area, first_face per component.  connectivity 'edge': faces sharing a pair of vertex indices hang
        together; 'vertex': faces sharing a vertex index."""
        import mesh_components
        return mesh_components.components(self._v, self._f, connectivity)

    @property
    def area(self):
        """the sum of the faces' areas: per component in the written order, the components added in ascending number"""
        import mesh_components
        return mesh_components.total_area(self.components().area)

    def remove_unreferenced_vertices(self):
        """trimesh's: drop the vertices no face refers to and renumber the faces; everything kept stays in its order"""
        import mesh_components
        self._apply(mesh_components.referenced_vertices(self._f, int(self._v.size(0))), True)

    def keep_components(self, largest=None, by="faces", min_faces=None, min_area_ratio=None, connectivity="edge"):
        """In place: keep the faces of the selected components and the vertices they still refer to (normals and colours follow),
        everything in its original order -> (components kept, components dropped).  largest=k with by='faces'|'area' (ties: the
        component whose first face comes first; a NaN area orders below every number), min_faces=n, min_area_ratio=r (area > r x
        the total area: eval_tnt/cull_mesh.py:197); criteria given together are ANDed.  The component table goes to the host once and
        is decided there; masks, marking and compaction run on the device."""
        import mesh_components
        comps = self.components(connectivity)
        keep = mesh_components.select(comps.faces, comps.area, largest, by, min_faces, min_area_ratio)
        if int(self._f.size(0)):
            self.update_faces(mesh_components.component_mask(comps.face_comp, keep))
        self.remove_unreferenced_vertices()
        kept = int(keep.sum())
        mesh_components._last["keep"] = {"components": len(keep), "kept": kept, "kept_faces": int(self._f.size(0)), "kept_vertices": int(self._v.size(0)),
                                         "kept_mask": keep.tolist(), "comp_faces": comps.faces.tolist(), "comp_first": comps.first_face.tolist(),
                                         "comp_area": comps.area.tolist()}
        return kept, len(keep) - kept

    # ---- simplification (mesh_simplify.py)
    def simplify(self, cell=None, grid=None, target_vertices=None, dedupe=True, origin=None):
        """In place: uniform vertex clustering with a quadric-error representative -> the statistics.  Exactly one of cell (the cell
        size h), grid (h = the largest extent of the bounding box / grid) and target_vertices (the smallest probed h with at most that
        many clusters: at most 24 count-only probes).  The grid's origin is the smallest coordinate per axis unless `origin` names one.  Every vertex of a cell
        becomes one vertex (the regularised quadric minimiser, or the cell's mean; a cell of one vertex keeps it bit for bit), colours their integer mean; a face with two
        corners in one cell goes, with dedupe also all but the first face of an unordered triple of cells; kept faces keep their order
        and orientation; cells no kept face refers to go; normals, if the mesh had them, are computed anew."""
        import mesh_simplify
        nv, nf = int(self._v.size(0)), int(self._f.size(0))
        h, probes = mesh_simplify.choose_cell(self._v, cell, grid, target_vertices, origin)
        out = mesh_simplify.simplify(self._v, self._f, self._c, cell=h, dedupe=dedupe, origin=origin)
        had_normals = self._n is not None
        self._v, self._c, self._n = out["cluster_vertices"], out["cluster_colors"], None
        with _device_of(self._v):
            self._f = _gather(_compact_rows(out["face_keep"]), out["cluster_faces"]) if nf else out["cluster_faces"]
        self.remove_unreferenced_vertices()
        if had_normals:
            self.compute_vertex_normals()
        stats = {"vertices_before": nv, "faces_before": nf, "vertices_after": int(self._v.size(0)), "faces_after": int(self._f.size(0)),
                 "clusters": out["clusters"], "used_mean": out["used_mean_count"], "dropped_degenerate": out["dropped_degenerate"],
                 "dropped_duplicate": out["dropped_duplicate"], "cell": h, "origin": out["origin"], "dedupe": bool(dedupe),
                 "probes": [[p, n] for p, n in probes]}
        mesh_simplify._last["mesh"] = stats
        return dict(stats)

    def cull_by_visibility(self, c2w_list, H, W, fx, fy, cx, cy, zfar=20.0, eps=0.005, min_views=20, znear=0.01, convention="opengl", batch=0):
        """eval_tnt/cull_mesh.py:220-249 in place: a depth image of this mesh per camera, the views that see each vertex in front of it,
        then update_faces(every vertex seen by at least min_views) and remove_unreferenced_vertices -> the per-vertex counts (before
        the compaction), on the device"""
        count, keep = visibility(self, c2w_list, H, W, fx, fy, cx, cy, znear=znear, zfar=zfar, eps=eps, min_views=min_views,
                                 convention=convention, batch=batch)
        out = compact_mesh(keep, self._f)
        self.update_faces(out["face_keep"])
        self.remove_unreferenced_vertices()
        return count

    def compute_vertex_normals(self):
        """Open3D's name (mesh_viewer.py:48): area-weighted vertex normals (mesh_render.vertex_normals) into the
        normals that export() writes -> self"""
        import mesh_render
        self._n = mesh_render.vertex_normals(self)
        return self

    def export(self, path):
        """binary little-endian PLY: float x y z [nx ny nz] [uchar red green blue], `list uchar int` faces"""
        v = self._v.cpu().numpy()
        fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
        head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(v)
        if self._n is not None:
            fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
            head += "property float nx\nproperty float ny\nproperty float nz\n"
        if self._c is not None:
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
            head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        f = self._f.cpu().numpy()
        head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f)
        rec = np.zeros(len(v), fields)
        n = None if self._n is None else self._n.cpu().numpy()
        c = None if self._c is None else self._c.cpu().numpy()
        for i, k in enumerate("xyz"):
            rec[k] = v[:, i].astype(np.float32)
            if n is not None:
                rec["n" + k] = n[:, i]
        if c is not None:
            for i, k in enumerate(("red", "green", "blue")):
                rec[k] = c[:, i]
        fr = np.zeros(len(f), [("n", "u1"), ("i", "<i4", (3,))])
        fr["n"], fr["i"] = 3, f
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii"))
            fh.write(rec.tobytes())
            fh.write(fr.tobytes())


def load(path, device=None):
    """trimesh.load for the PLY files of this pipeline (tsdf_fusion.write_ply: float x y z nx ny nz, uchar red green blue, triangle
    faces; ASCII and double coordinates as mesh_eval.read_ply reads them) -> DeviceMesh"""
    el = mesh_eval.read_ply_elements(path)
    rec = el["vertex"]
    names = rec.dtype.names
    v = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1).astype(np.float64)
    normals = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=-1).astype(np.float32) if all(k in names for k in ("nx", "ny", "nz")) else None
    colors = np.stack([rec["red"], rec["green"], rec["blue"]], axis=-1).astype(np.uint8) if all(k in names for k in ("red", "green", "blue")) else None
    faces = np.zeros((0, 3), np.int32)
    if "face" in el and "_i" in (el["face"].dtype.names or ()):
        faces = el["face"]["_i"].astype(np.int32).reshape(-1, 3)
    return DeviceMesh(v, faces, normals, colors, device=device)


# ---- the script's functions ----------------------------------------------------------------------------------------------------------
def cull_mesh(cameras, mesh, radius=6):
    """evaluate_dtu_mesh.py:77-139, a drop-in: every camera's gt_alpha_mask dilated on the device into one buffer, one culling launch
    over all views, the mesh compacted.  A DeviceMesh stays on the device; any other mesh object (a trimesh.Trimesh) gets the two
    masks through its own update_vertices / update_faces."""
    dev = mesh.device if isinstance(mesh, DeviceMesh) else _device()
    sizes = []
    for i, cam in enumerate(cameras):
        if getattr(cam, "gt_alpha_mask", None) is None:
            raise ValueError("cull_mesh: camera %d (%s) has no gt_alpha_mask: the culling needs every view's object mask "
                             "(DTU scenes carry it in the alpha channel of their images)" % (i, getattr(cam, "image_name", "?")))
        sizes.append((int(cam.image_width), int(cam.image_height)))
    words = [H * mask_row_words(W) for W, H in sizes]
    with torch.no_grad():
        buf = torch.empty(int(sum(words)), dtype=torch.int64, device=dev)
        views, off = [], 0
        for cam, (W, H), n in zip(cameras, sizes, words):
            m = torch.as_tensor(cam.gt_alpha_mask)[0].detach().to(dev)
            if m.dtype not in (torch.float32, torch.uint8):
                m = m.float()
            if tuple(m.shape) != (H, W):
                raise ValueError("cull_mesh: a mask of %s for an image of %d x %d" % (tuple(m.shape), W, H))
            p = dilate_mask(m.contiguous(), radius, out=buf[off:off + n])
            views.append((view_matrix(cam.focal_x, cam.focal_y, W, H, cam.world_view_transform), W, H, p))
            off += n
        if isinstance(mesh, DeviceMesh):
            keep = cull_vertices(mesh._v.float(), views)
            mesh.compact(keep)
            return mesh
        v32 = torch.from_numpy(np.ascontiguousarray(np.asarray(mesh.vertices), np.float32).reshape(-1, 3)).to(dev)
        f32 = torch.from_numpy(np.ascontiguousarray(np.asarray(mesh.faces), np.int32).reshape(-1, 3)).to(dev)
        keep = cull_vertices(v32, views)
        out = compact_mesh(keep, f32)
    mesh.update_vertices(keep.cpu().numpy())
    mesh.update_faces(out["face_keep"].cpu().numpy())
    return mesh


def decompose_projection_matrix(P):
    """P (3,4) = K [R | -R C] -> (K (3,3) upper triangular with a positive diagonal, K[2,2] = 1; R (3,3); C (3,)) in fp64: the RQ
    decomposition of P[:, :3] through numpy's QR, and the camera centre C = -P[:, :3]^-1 P[:, 3].  The centre is the contract (it is
    all evaluate_dtu_mesh.py reads); R's sign convention follows from the positive diagonal and is not pinned to OpenCV's."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    M = P[:, :3]
    J = np.eye(3)[::-1]
    q, r = np.linalg.qr((J @ M).T)
    K = J @ r.T @ J
    R = J @ q.T
    s = np.sign(np.diag(K))
    s[s == 0] = 1.0
    K, R = K * s[None, :], R * s[:, None]
    centre = -np.linalg.solve(M, P[:, 3])
    return K / K[2, 2], R, centre


def load_dtu_camera(DTU):
    """evaluate_dtu_mesh.py:59-75 without cv2: the 64 calibration matrices -> [pose (3,4) float32: R^T | centre]"""
    poses = []
    for i in range(1, 64 + 1):
        projection = np.loadtxt(os.path.join(DTU, "Calibration/cal18/pos_%03d.txt" % i), dtype=np.float32)
        _, R, centre = decompose_projection_matrix(projection)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3] = R.transpose()
        pose[:3, 3] = centre
        poses.append(pose[:3])
    return poses


# ---- eval_tnt/cull_mesh.py: depth rasteriser and visibility cull (csrc/mesh_raster.hip) -----------------------------
class GofRasterView(C.Structure):
    """Mirror of ``GofRasterView`` in include/gof_mesh_hip.h."""
    _fields_ = [("w2c", C.c_double * 12), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("znear", C.c_double), ("zfar", C.c_double), ("W", C.c_int32), ("H", C.c_int32)]


_RASTER_DTYPE = np.dtype([("w2c", "<f8", (12,)), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("znear", "<f8"), ("zfar", "<f8"),
                          ("W", "<i4"), ("H", "<i4")])
assert _RASTER_DTYPE.itemsize == C.sizeof(GofRasterView) == 152

_f64 = C.c_double
lib.gof_mesh_raster_abi_version.restype = C.c_int
lib.gof_mesh_raster_abi_version.argtypes = []
lib.gof_mesh_raster_tiling.restype = None
lib.gof_mesh_raster_tiling.argtypes = [_P64]
gn.bind(lib, {"gof_mesh_render_depth_ws_bytes": [_i64], "gof_mesh_visibility_ws_bytes": [_i64, _i64, _i32]}, {
        "gof_mesh_render_depth": [_i64, _vp, _i64, _vp, _i32, _vp, _i64, _vp, _P64, _vp, _sz, _vp],
        "gof_mesh_visible_count": [_i64, _vp, _i32, _vp, _i64, _vp, _f64, _vp, _vp, _sz, _vp],
        "gof_mesh_visibility": [_i64, _vp, _i64, _vp, _i32, _vp, _i64, _i32, _f64, _i32, _vp, _vp, _P64, _vp, _sz, _vp]})

_STAT_NAMES = ("triangles", "listed", "refused_by_full_list", "atomics", "pixels")
__all__ += ["GofRasterView", "raster_tiling", "raster_views", "render_depth", "visible_count", "visibility", "TntMesher", "get_traj", "main"]


def raster_tiling():
    """The sizes at which the rasteriser changes its path (gof_mesh_raster_tiling)."""
    out = (C.c_int64 * 8)()
    lib.gof_mesh_raster_tiling(out)
    return dict(zip(("inline_max", "tile_w", "tile_h", "guard", "max_side", "batch", "list_min", "stripes"), (int(v) for v in out)))


def raster_views(c2w_list, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, convention="opengl"):
    """The view records of a camera list: c2w (4,4) or (3,4), tensors or arrays; convention 'opengl' (the camera looks down -z, +y is
    up: what eval_tnt/cull_mesh.py hands to pyrender) or 'opencv' (+z forward, +y down).  World-to-camera is the fp64 inverse of the
    OpenCV camera-to-world, formed here on the host."""
    if convention not in ("opengl", "opencv"):
        raise ValueError("raster_views: convention must be 'opengl' or 'opencv', got %r" % (convention,))
    rec = np.zeros(len(c2w_list), _RASTER_DTYPE)
    for i, c2w in enumerate(c2w_list):
        if isinstance(c2w, torch.Tensor):
            c2w = c2w.detach().cpu().numpy()
        m = np.eye(4)
        a = np.asarray(c2w, np.float64)
        if a.shape not in ((4, 4), (3, 4)):
            raise ValueError("raster_views: camera %d: expected a (4,4) or (3,4) camera-to-world matrix, got %s" % (i, a.shape))
        m[:a.shape[0]] = a
        if convention == "opengl":
            m[:3, 1:3] *= -1.0
        rec[i] = (np.linalg.inv(m)[:3].reshape(12), float(fx), float(fy), float(cx), float(cy), float(znear), float(zfar), int(W), int(H))
    return rec


def _mesh_arrays(mesh, who, need_faces=True):
    """-> (vertices (NV,3) float32, faces (NF,3) int32 or None) on the device, of a DeviceMesh, a vertex tensor, or any object with
    .vertices / .faces host arrays (a trimesh.Trimesh)"""
    if isinstance(mesh, DeviceMesh):
        return mesh._v.float().contiguous(), mesh._f
    if isinstance(mesh, torch.Tensor):
        if need_faces:
            raise RuntimeError("%s: needs a mesh, got a tensor" % who)
        return _tensor(mesh, who, "vertices", (torch.float32, torch.float64), 3).float().contiguous(), None
    dev = _device()
    v = torch.from_numpy(np.ascontiguousarray(np.asarray(mesh.vertices), np.float32).reshape(-1, 3)).to(dev)
    f = torch.from_numpy(np.ascontiguousarray(np.asarray(mesh.faces), np.int32).reshape(-1, 3)).to(dev)
    return v, f


def _records(rec, dev):
    return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev) if len(rec) else None


def _stats(out, on):
    return dict(zip(_STAT_NAMES, (int(v) for v in out))) if on else {}


def render_depth(mesh, c2w_list, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, convention="opengl", stats=False):
    """eval_tnt/cull_mesh.py:17-66 (extract_depth_from_mesh) without pyrender: the depth of the mesh IT IS GIVEN from every camera ->
    (N,H,W) float32 on the device, 0 where nothing is seen; both face orientations are drawn (SKIP_CULL_FACES)."""
    v, f = _mesh_arrays(mesh, "render_depth")
    rec = raster_views(c2w_list, H, W, fx, fy, cx, cy, znear, zfar, convention)
    H, W, n, nv, nf = int(H), int(W), len(rec), int(v.size(0)), int(f.size(0))
    with _device_of(v):
        nb = lib.gof_mesh_render_depth_ws_bytes(nf)
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        depth = torch.empty((n, max(H, 0), max(W, 0)), dtype=torch.float32, device=v.device)
        st = (C.c_int64 * 8)()
        records = _records(rec, v.device)
        B._check(lib.gof_mesh_render_depth(nv, _ptr(v), nf, _ptr(f), n, _ptr(records), max(H, 0) * max(W, 0), _ptr(depth),
                                           st if stats else None, ws.data_ptr(), nb, _stream()))
    _last["render_depth"] = dict({"vertices": nv, "faces": nf, "views": n, "workspace_bytes": int(nb)}, **_stats(st, stats))
    return depth


def visible_count(mesh_or_vertices, c2w_list, H, W, fx, fy, cx, cy, depth=None, znear=0.01, zfar=20.0, eps=0.005, convention="opengl", batch=0):
    """Mesher.point_masks (:117-175) in fp64: per vertex the number of views that see it in front of the depth image -> (NV,) int32 on
    the device.  depth (N,H,W) float32 given: the vertices (a tensor or a mesh) against those images; depth None: the images are
    rendered from the mesh itself, a batch of views at a time (visibility)."""
    if depth is None:
        return visibility(mesh_or_vertices, c2w_list, H, W, fx, fy, cx, cy, znear=znear, zfar=zfar, eps=eps, min_views=0, convention=convention, batch=batch)[0]
    v, _ = _mesh_arrays(mesh_or_vertices, "visible_count", need_faces=False)
    rec = raster_views(c2w_list, H, W, fx, fy, cx, cy, znear, zfar, convention)
    d = _tensor(depth, "visible_count", "depth", (torch.float32,))
    if tuple(d.shape) != (len(rec), int(H), int(W)) or d.device != v.device:
        raise RuntimeError("visible_count: depth must be (%d, %d, %d) on the vertices' device" % (len(rec), int(H), int(W)))
    nv = int(v.size(0))
    with _device_of(v):
        nb = lib.gof_mesh_render_depth_ws_bytes(0)
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        count = torch.zeros(nv, dtype=torch.int32, device=v.device)
        records = _records(rec, v.device)
        B._check(lib.gof_mesh_visible_count(nv, _ptr(v), len(rec), _ptr(records), int(H) * int(W), _ptr(d), float(eps), _ptr(count),
                                            ws.data_ptr(), nb, _stream()))
    _last["visible_count"] = {"vertices": nv, "views": len(rec), "workspace_bytes": int(nb)}
    return count


def visibility(mesh, c2w_list, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, eps=0.005, min_views=20, convention="opengl", batch=0, stats=False):
    """Render and count, `batch` views at a time (0: the library's default): the depth images of all views never exist at once ->
    (count (NV,) int32, keep (NV,) bool = count >= min_views) on the device."""
    v, f = _mesh_arrays(mesh, "visibility")
    rec = raster_views(c2w_list, H, W, fx, fy, cx, cy, znear, zfar, convention)
    nv, nf, stride = int(v.size(0)), int(f.size(0)), max(int(H), 0) * max(int(W), 0)
    with _device_of(v):
        nb = lib.gof_mesh_visibility_ws_bytes(nf, stride, int(batch))
        if nb == 0:
            raise RuntimeError("visibility: bad batch (%d) or image size (%d x %d)" % (int(batch), int(W), int(H)))
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        count = torch.empty(nv, dtype=torch.int32, device=v.device)
        keep = torch.empty(nv, dtype=torch.uint8, device=v.device)
        st = (C.c_int64 * 8)()
        records = _records(rec, v.device)
        B._check(lib.gof_mesh_visibility(nv, _ptr(v), nf, _ptr(f), len(rec), _ptr(records), stride, int(batch), float(eps), int(min_views),
                                         _ptr(count), _ptr(keep), st if stats else None, ws.data_ptr(), nb, _stream()))
    _last["visibility"] = dict({"vertices": nv, "faces": nf, "views": len(rec), "batch": int(batch) or raster_tiling()["batch"], "workspace_bytes": int(nb)},
                               **_stats(st, stats))
    return count, keep.bool()


class TntMesher:
    """eval_tnt/cull_mesh.py's Mesher: the same constructor and __call__(mesh_path, c2w_list), writing <mesh>_cull.ply.  The mesh is the
    file it is given (the script's extract_depth_from_mesh renders a file of its author's instead, :28), its vertices are never merged
    by position (no merge_vertices / process=True).  components=<DeviceMesh.keep_components keyword arguments> adds the step the script
    leaves commented out (:256).  forecast_radius is 0 as in the script; anything else needs Open3D's oriented bounding box."""

    def __init__(self, H, W, fx, fy, cx, cy, far, points_batch_size=5e5, components=None):
        self.points_batch_size = int(points_batch_size)
        self.scale = 1.0
        self.forecast_radius = 0
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = H, W, fx, fy, cx, cy
        self.far = far
        self.eps = 0.005
        self.min_views = 20
        self.remove_small_geometry_threshold = 0.2
        self.get_largest_components = True
        self.components = components
        self.verbose = True

    def cull_mesh(self, mesh, estimate_c2w_list):
        """:204-289 -> (cull_mesh, forecast_mesh): the mesh is culled in place and is both"""
        if abs(self.forecast_radius) > 0:
            raise NotImplementedError("TntMesher: forecast_radius != 0 needs Open3D's oriented bounding box (eval_tnt/cull_mesh.py:261-283)")
        mesh.cull_by_visibility(estimate_c2w_list, self.H, self.W, self.fx, self.fy, self.cx, self.cy, zfar=20.0, eps=self.eps, min_views=self.min_views)
        if self.components is not None:
            mesh.keep_components(**self.components)
        return mesh, mesh

    def __call__(self, mesh_path, estimate_c2w_list):
        if abs(self.forecast_radius) > 0:
            raise NotImplementedError("TntMesher: forecast_radius != 0 needs Open3D's oriented bounding box (eval_tnt/cull_mesh.py:261-283)")
        mesh = load(mesh_path)
        out = mesh_path.replace(".ply", "_cull.ply")
        culled, _ = self.cull_mesh(mesh, estimate_c2w_list)
        culled.export(out)
        if self.verbose:
            print("\nINFO: Save mesh at {}!\n".format(out))
        return out


def _orient_up_and_center(poses):
    """nerfstudio's auto_orient_and_center_poses(method='up', center_poses=True) as eval_tnt/help_func.py:33-88 applies it, in numpy
    float32: the mean up vector (column 1) is rotated onto +z and the mean camera position moved to the origin -> (N,3,4)"""
    poses = np.asarray(poses, np.float32)
    mean_t = poses[:, :3, 3].mean(axis=0, dtype=np.float32)
    up = poses[:, :3, 1].mean(axis=0, dtype=np.float32)
    a = up / np.linalg.norm(up)
    a = a / np.linalg.norm(a)
    b = np.array([0, 0, 1], np.float32)
    v = np.cross(a, b).astype(np.float32)
    c = np.float32(np.dot(a, b))
    if c < -1 + 1e-8:
        raise ValueError("get_traj: the cameras' mean up vector points along -z exactly: the reference perturbs it at random here")
    s = np.float32(np.linalg.norm(v))
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float32)
    rot = (np.eye(3, dtype=np.float32) + k + k @ k * np.float32((1 - c) / (s ** 2 + 1e-8))).astype(np.float32)
    transform = np.concatenate([rot, rot @ -mean_t[:, None]], axis=-1).astype(np.float32)
    return transform @ poses


def get_traj(traj_path):
    """eval_tnt/cull_mesh.py:321-363 through numpy: a .npy of camera-to-world matrices, or a transforms .json (instant-ngp / sdfstudio),
    oriented, centred and scaled as the script does -> a list of (4,4) float32 tensors"""
    traj = []
    if traj_path.endswith(".npy"):
        traj = [m for m in np.load(traj_path)]
    elif traj_path.endswith(".json"):
        import json
        with open(traj_path, encoding="UTF-8") as fh:
            meta = json.load(fh)
        by_index = {int(frame["file_path"][13:18]) - 1: np.array(frame["transform_matrix"]) for frame in meta["frames"]}
        poses = np.array([by_index[i] for i in range(len(by_index))]).astype(np.float32)
        poses = _orient_up_and_center(poses)
        poses[:, :3, 3] *= np.float32(1.0 / float(np.max(np.abs(poses[:, :3, 3]))))
        traj = [m for m in poses]
    out = []
    for m in traj:
        c2w = torch.from_numpy(np.ascontiguousarray(m)).float()
        if tuple(c2w.shape) == (3, 4):
            c2w = torch.cat([c2w, torch.tensor([[0, 0, 0, 1]]).float()], dim=0)
        out.append(c2w)
    return out


# the script's Tanks-and-Temples intrinsics (eval_tnt/cull_mesh.py:387-392)
TNT_INTRINSICS = {"height": 1080, "width": 1920, "fx": 1163.8678928442187, "fy": 1172.793101201448, "cx": 962.3120628412543, "cy": 542.0667209577691}


def main(argv=None):
    """python -m mesh_cull tnt --traj-path T --ply-path P: the script's __main__ (:366-399)"""
    import argparse
    ap = argparse.ArgumentParser(prog="mesh_cull")
    sub = ap.add_subparsers(dest="command", required=True)
    t = sub.add_parser("tnt", help="eval_tnt/cull_mesh.py: keep what at least --min-views cameras see, write <ply>_cull.ply")
    t.add_argument("--traj-path", type=str, required=True)
    t.add_argument("--ply-path", type=str, required=True)
    for k, val in TNT_INTRINSICS.items():
        t.add_argument("--" + k, type=type(val), default=val)
    t.add_argument("--min-views", type=int, default=20)
    t.add_argument("--components", type=str, default=None, help="a mesh_components spec, e.g. largest:1")
    a = ap.parse_args(argv)
    comp = None
    if a.components:
        import mesh_components
        comp = mesh_components.parse_spec(a.components)
    mesher = TntMesher(a.height, a.width, a.fx, a.fy, a.cx, a.cy, 20.0, points_batch_size=5e5, components=comp)
    mesher.min_views = a.min_views
    mesher(a.ply_path, get_traj(a.traj_path))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main(sys.argv[1:]))
