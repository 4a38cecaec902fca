"""Connected components of a triangle mesh on the GPU: which faces hang together, how large each piece is, and the removal of the
small disconnected pieces a level set leaves around the object -- what the reference intends with trimesh's split() at
evaluate_dtu_mesh.py:132-138 ("Taking the biggest connected component") and eval_tnt/cull_mesh.py:186-201 (get_connected_mesh).

    face_comp, C = face_components(faces, num_vertices)         # component number of every face, in the order of their first face
    comps = mesh.components()                                   # + host arrays: faces, area, first_face per component
    kept, dropped = mesh.keep_components(largest=1)             # in place: faces, vertices, normals and colours compacted, in order
    python -m mesh_components IN.ply OUT.ply --min-area-ratio 0.2 --table components.json

The kernels are ``gof_mesh_component*`` of libgof_hip.so (csrc/mesh_components.hip, include/gof_mesh_hip.h (d)); the contract is
DESIGN.md §3.18: tensors on a ROCm device in and out, labels and counts equal to a sequential union-find's, areas bit-equal to the
written summation order.  There is no host fallback: host tensors are refused.  ``split()`` is deliberately not offered: a Python list
of 10^5 mesh objects is the thing this module replaces -- select with keep_components, or index with face_comp.  One stated deviation
(DESIGN.md §7): an edge joins every face that lies on it, where trimesh's face_adjacency pairs faces over edges shared by exactly two.
"""
import ctypes as C
import functools
import json
import sys

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["face_components", "component_stats", "component_mask", "referenced_vertices", "components", "select", "total_area",
           "Components", "parse_spec", "clean_file", "last_stats", "main", "CONNECTIVITY"]

lib = B.lib
_vp, _sz, _i64, _i32 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32
_P64 = C.POINTER(C.c_int64)
lib.gof_mesh_abi_version.restype = C.c_int
lib.gof_mesh_abi_version.argtypes = []
gn.bind(lib, {"gof_mesh_components_ws_bytes": [_i64, _i64, _i32], "gof_mesh_component_stats_ws_bytes": [_i64, _i64]}, {
        "gof_mesh_components": [_i64, _i64, _vp, _i32, _vp, _vp, _P64, _vp, _sz, _vp],
        "gof_mesh_component_stats": [_i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp],
        "gof_mesh_component_mask": [_i64, _vp, _i64, _vp, _vp, _vp],
        "gof_mesh_mark_referenced": [_i64, _i64, _vp, _vp, _vp, _vp]})

CONNECTIVITY = {"edge": 0, "vertex": 1}
MAX_FACES = (2 ** 31 - 1) // 3          # 3 * faces < 2^31
_last = {}


def tiling():
    """The sizes at which the unit changes its path (for tests): items per block of the radix sort, items per tile of the scan,
    sorted positions per tile and per block of the area sums."""
    out = (C.c_int64 * 4)()
    lib.gof_mesh_components_tiling.restype = None
    lib.gof_mesh_components_tiling.argtypes = [_P64]
    lib.gof_mesh_components_tiling(out)
    return {"sort_block": int(out[0]), "scan_tile": int(out[1]), "sum_tile": int(out[2]), "sum_block": int(out[3])}


def last_stats():
    """Statistics of the last face_components / component_stats / keep_components calls (one sub-dictionary each)."""
    return {k: dict(v) for k, v in _last.items()}


# the device seams, by the names the host tests replace per module (tests/test_mesh_components_host.py), as in mesh_cull
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "mesh_components")


def _tensor(t, who, what, dtypes, cols=None):
    return gn.rows(t, who, what, dtypes, cols, limit=2 ** 31 - 1, shape_first=False, on_device=_on_device)


def _mode(connectivity):
    if connectivity not in CONNECTIVITY:
        raise ValueError("connectivity must be 'edge' or 'vertex', got %r" % (connectivity,))
    return CONNECTIVITY[connectivity]


def _faces(faces, who):
    f = _tensor(faces, who, "faces", (torch.int32,), 3)
    if int(f.size(0)) > MAX_FACES:
        raise RuntimeError("%s: at most %d faces (3 * faces must be below 2^31)" % (who, MAX_FACES))
    return f


def _label(faces, num_vertices, connectivity):
    """-> (face_label, face_comp, C): int32 device tensors and a Python int"""
    mode = _mode(connectivity)
    f = _faces(faces, "face_components")
    nv, nf = int(num_vertices), int(f.size(0))
    with _device_of(f):
        nb = lib.gof_mesh_components_ws_bytes(nv, nf, mode)
        ws = torch.empty(nb, dtype=torch.uint8, device=f.device)
        label = torch.empty(nf, dtype=torch.int32, device=f.device)
        comp = torch.empty(nf, dtype=torch.int32, device=f.device)
        count = C.c_int64()
        B._check(lib.gof_mesh_components(nv, nf, _ptr(f), mode, _ptr(label), _ptr(comp), C.byref(count), ws.data_ptr(), nb, _stream()))
    _last["components"] = {"vertices": nv, "faces": nf, "connectivity": connectivity, "components": int(count.value), "workspace_bytes": int(nb)}
    return label, comp, int(count.value)


def face_components(faces, num_vertices, connectivity="edge"):
    """faces (NF,3) int32 on a ROCm device, indices in [0, num_vertices) -> (face_comp (NF,) int32, C (0-d int64)) there: the
    component number of every face, components numbered 0..C-1 in the order of their first face.  'edge': faces that share an unordered
    pair of vertex indices hang together; 'vertex': faces that share a vertex index."""
    _, comp, count = _label(faces, num_vertices, connectivity)
    return comp, torch.tensor(count, dtype=torch.int64, device=comp.device)


def component_stats(vertices, faces, face_comp, num_components):
    """vertices (NV,3) float64, faces (NF,3) int32, face_comp (NF,) int32 on one ROCm device -> host arrays (faces (C,) int64,
    first_face (C,) int32, area (C,) float64): per component its number of faces, its smallest face index and the sum of its faces'
    areas in the order DESIGN.md §3.18 writes down (the same bits on every run)."""
    v = _tensor(vertices, "component_stats", "vertices", (torch.float64,), 3)
    f = _faces(faces, "component_stats")
    fc = _tensor(face_comp, "component_stats", "face_comp", (torch.int32,))
    nv, nf, nc = int(v.size(0)), int(f.size(0)), int(num_components)
    if fc.dim() != 1 or fc.numel() != nf or fc.device != f.device or v.device != f.device:
        raise RuntimeError("component_stats: face_comp must be (NF,), and everything on one device")
    with _device_of(f):
        nb = lib.gof_mesh_component_stats_ws_bytes(nf, nc)
        ws = torch.empty(nb, dtype=torch.uint8, device=f.device)
        cf = torch.empty(nc, dtype=torch.int64, device=f.device)
        first = torch.empty(nc, dtype=torch.int32, device=f.device)
        area = torch.empty(nc, dtype=torch.float64, device=f.device)
        B._check(lib.gof_mesh_component_stats(nv, nf, _ptr(v), _ptr(f), _ptr(fc), nc, _ptr(cf), _ptr(first), _ptr(area), ws.data_ptr(), nb, _stream()))
        out = cf.cpu().numpy(), first.cpu().numpy(), area.cpu().numpy()
    _last["stats"] = {"vertices": nv, "faces": nf, "components": nc, "workspace_bytes": int(nb)}
    return out


def component_mask(face_comp, comp_keep):
    """face_comp (NF,) int32 on a ROCm device, comp_keep: C booleans on the host -> (NF,) uint8 there: comp_keep[face_comp]"""
    fc = _tensor(face_comp, "component_mask", "face_comp", (torch.int32,))
    k = np.ascontiguousarray(np.asarray(comp_keep, bool).reshape(-1)).view(np.uint8)
    nf, nc = int(fc.numel()), len(k)
    with _device_of(fc):
        table = torch.from_numpy(k.copy()).to(fc.device)
        out = torch.empty(nf, dtype=torch.uint8, device=fc.device)
        B._check(lib.gof_mesh_component_mask(nf, _ptr(fc), nc, _ptr(table), _ptr(out), _stream()))
    return out


def referenced_vertices(faces, num_vertices, face_keep=None):
    """faces (NF,3) int32 on a ROCm device [, face_keep (NF,) uint8 there] -> (NV,) uint8: the vertex is an index of some (kept) face"""
    f = _faces(faces, "referenced_vertices")
    nv, nf = int(num_vertices), int(f.size(0))
    with _device_of(f):
        out = torch.empty(nv, dtype=torch.uint8, device=f.device)
        B._check(lib.gof_mesh_mark_referenced(nv, nf, _ptr(f), None if face_keep is None else _ptr(face_keep), _ptr(out), _stream()))
    return out


class Components:
    """What DeviceMesh.components returns: face_comp and face_label (NF,) int32 on the device, count = C, and per component the host
    arrays faces (int64), area (float64), first_face (int32); connectivity as asked for."""

    def __init__(self, face_label, face_comp, count, faces, first_face, area, connectivity):
        self.face_label, self.face_comp, self.count = face_label, face_comp, count
        self.faces, self.first_face, self.area, self.connectivity = faces, first_face, area, connectivity

    def __len__(self):
        return self.count


def components(vertices, faces, connectivity="edge"):
    """vertices (NV,3) float64, faces (NF,3) int32 on a ROCm device -> Components"""
    v = _tensor(vertices, "components", "vertices", (torch.float64,), 3)
    label, comp, count = _label(faces, int(v.size(0)), connectivity)
    cf, first, area = component_stats(v, faces, comp, count)
    return Components(label, comp, count, cf, first, area, connectivity)


def total_area(area):
    """the components' areas added in ascending component number, from the first (0.0 without a component)"""
    total = 0.0
    for i, a in enumerate(np.asarray(area, np.float64).tolist()):
        total = a if i == 0 else total + a
    return total


def select(comp_faces, comp_area, largest=None, by="faces", min_faces=None, min_area_ratio=None):
    """The decision of keep_components, on the host over the component table -> (C,) bool.  largest=k with by='faces'|'area': the k
    largest (ties: the smaller component number; a NaN area orders below every number); min_faces=n: at least n faces;
    min_area_ratio=r: area > r * total_area (eval_tnt/cull_mesh.py:197).  Criteria given together are ANDed."""
    cf, area = np.asarray(comp_faces, np.int64), np.asarray(comp_area, np.float64)
    n = len(cf)
    keep = np.ones(n, bool)
    if by not in ("faces", "area"):
        raise ValueError("by must be 'faces' or 'area', got %r" % (by,))
    if largest is not None:
        k = int(largest)
        if k < 0:
            raise ValueError("largest must be at least 0, got %d" % k)
        nan = np.isnan(area) if by == "area" else np.zeros(n, bool)
        size = np.where(nan, 0.0, area) if by == "area" else cf
        order = np.lexsort((np.arange(n), -size, nan))               # not NaN first, then descending size, then ascending number
        m = np.zeros(n, bool)
        m[order[:k]] = True
        keep &= m
    if min_faces is not None:
        keep &= cf >= int(min_faces)
    if min_area_ratio is not None:
        with np.errstate(invalid="ignore"):
            keep &= area > float(min_area_ratio) * total_area(area)
    return keep


# ---- the spec of the launcher's GOF_MESH_COMPONENTS and the command line ---------------------------------------------------------------
_SPEC = {"largest": int, "by": str, "min_faces": int, "min_area_ratio": float, "connectivity": str}


def parse_spec(spec):
    """'largest:1' / 'min_area_ratio:0.2,connectivity:vertex' -> the keyword arguments of keep_components; ValueError for anything else"""
    out = {}
    for part in str(spec).split(","):
        key, sep, value = part.strip().partition(":")
        key = key.strip().replace("-", "_")
        if not sep or key not in _SPEC or key in out:
            raise ValueError("GOF_MESH_COMPONENTS: %r is not one of %s as key:value (given once)" % (part, ", ".join(sorted(_SPEC))))
        try:
            out[key] = _SPEC[key](value.strip())
        except ValueError:
            raise ValueError("GOF_MESH_COMPONENTS: %r is no %s" % (value, _SPEC[key].__name__)) from None
    if out.get("by", "faces") not in ("faces", "area") or out.get("connectivity", "edge") not in CONNECTIVITY:
        raise ValueError("GOF_MESH_COMPONENTS: by is faces or area, connectivity is edge or vertex")
    if out.get("largest", 0) < 0 or out.get("min_faces", 0) < 0 or not out.get("min_area_ratio", 0.0) >= 0.0:
        raise ValueError("GOF_MESH_COMPONENTS: largest, min_faces and min_area_ratio must not be negative")
    if not any(k in out for k in ("largest", "min_faces", "min_area_ratio")):
        raise ValueError("GOF_MESH_COMPONENTS: give at least one of largest, min_faces, min_area_ratio")
    return out


def clean_file(src, dst, table=None, **criteria):
    """mesh_cull.load(src), keep_components(**criteria), export(dst) [, the component table as JSON] -> (kept, dropped)"""
    import mesh_cull
    mesh = mesh_cull.load(src)
    kept, dropped = mesh.keep_components(**criteria)
    mesh.export(dst)
    if table:
        st = _last["keep"]
        with open(table, "w") as fh:
            json.dump({"connectivity": criteria.get("connectivity", "edge"), "components": kept + dropped, "kept": st["kept_mask"],
                       "faces": st["comp_faces"], "first_face": st["comp_first"], "area": st["comp_area"]}, fh)
    return kept, dropped


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m mesh_components", description="Keep the selected connected components of a PLY mesh.")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--largest", type=int, default=None)
    ap.add_argument("--by", choices=("faces", "area"), default="faces")
    ap.add_argument("--min-faces", type=int, default=None)
    ap.add_argument("--min-area-ratio", type=float, default=None)
    ap.add_argument("--connectivity", choices=tuple(CONNECTIVITY), default="edge")
    ap.add_argument("--table", default=None, help="write the per-component counts and areas to this JSON file")
    a = ap.parse_args(argv)
    kept, dropped = clean_file(a.input, a.output, table=a.table, largest=a.largest, by=a.by, min_faces=a.min_faces,
                               min_area_ratio=a.min_area_ratio, connectivity=a.connectivity)
    print("mesh_components: kept %d of %d components" % (kept, kept + dropped))
    return 0


if __name__ == "__main__":
    sys.exit(main())
