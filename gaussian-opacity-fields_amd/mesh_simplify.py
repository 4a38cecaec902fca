"""Mesh simplification on the GPU: uniform vertex clustering with a quadric-error representative (Lindstrom's scheme) -- what every user
of fusion/mesh_binary_search_7.ply (about nine points per Gaussian, tens of millions of faces) does first in MeshLab or another tool.

    vertex_cluster, NC = cluster(vertices, cell)                    # the cell of every vertex, cells numbered by their smallest vertex
    out = simplify(vertices, faces, colors, cell=0.01)              # dict: vertices, faces, colors, vertex_cluster, used_mean, ...
    stats = mesh.simplify(grid=1024)                                # DeviceMesh, in place; or cell=h, or target_vertices=n
    python -m mesh_simplify IN.ply OUT.ply --target-vertices 2000000 --stats stats.json

The kernels are ``gof_mesh_cluster*`` of libgof_hip.so (csrc/mesh_simplify.hip, include/gof_mesh_hip.h (h)); the contract is DESIGN.md
§3.21: tensors on a ROCm device in and out, every output equal to the written arithmetic bit for bit, on every run.  There is no host
fallback: host tensors are refused.  Out of scope: flipped faces are neither detected nor repaired, nothing preserves
boundaries or features beyond what the quadric gives, the result may be non-manifold, and there is no edge collapse.
"""
import ctypes as C
import functools
import json
import math
import sys

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["cluster", "count_clusters", "simplify", "choose_cell", "tiling", "last_stats", "parse_spec", "simplify_file", "main"]

lib = B.lib
_vp, _sz, _i64, _i32, _f64 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_double
_P64, _PF64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
lib.gof_mesh_simplify_abi_version.restype = C.c_int
lib.gof_mesh_simplify_abi_version.argtypes = []
lib.gof_mesh_simplify_tiling.restype = None
lib.gof_mesh_simplify_tiling.argtypes = [_P64]
gn.bind(lib, {"gof_mesh_cluster_ws_bytes": [_i64], "gof_mesh_cluster_solve_ws_bytes": [_i64, _i64, _i64], "gof_mesh_cluster_faces_ws_bytes": [_i64]}, {
        "gof_mesh_cluster": [_i64, _vp, _PF64, _f64, _vp, _P64, _vp, _sz, _vp],
        "gof_mesh_cluster_solve": [_i64, _i64, _vp, _vp, _vp, _vp, _i64, _PF64, _f64, _vp, _vp, _vp, _P64, _vp, _sz, _vp],
        "gof_mesh_cluster_faces": [_i64, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _P64, _vp, _sz, _vp]})

MAX_FACES = (2 ** 31 - 1) // 3          # 3 * faces < 2^31
MAX_PROBES = 24
_last = {}

# the device seams, by the names the host tests replace per module (tests/test_mesh_simplify_host.py), as in mesh_components
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "mesh_simplify")


def tiling():
    """The sizes at which the unit changes its path (for tests): items per block of the radix sort, items per tile of the scan,
    sorted positions per tile and per block of the sums."""
    out = (C.c_int64 * 4)()
    lib.gof_mesh_simplify_tiling(out)
    return {"sort_block": int(out[0]), "scan_tile": int(out[1]), "sum_tile": int(out[2]), "sum_block": int(out[3])}


def last_stats():
    """Statistics of the last cluster / simplify / DeviceMesh.simplify calls (one sub-dictionary each)."""
    return {k: dict(v) for k, v in _last.items()}


def _tensor(t, who, what, dtypes, cols=None):
    return gn.rows(t, who, what, dtypes, cols, limit=2 ** 31 - 1, shape_first=False, on_device=_on_device)


def _grid(v, cell, origin, who):
    """-> (origin as 3 C doubles, h); origin None: the smallest coordinate per axis (zeros without a vertex)"""
    h = float(cell)
    if not (h > 0.0 and math.isfinite(h)):
        raise ValueError("%s: the cell size must be finite and above 0, got %r" % (who, cell))
    if origin is None:
        origin = torch.amin(v, dim=0).cpu().tolist() if int(v.size(0)) else (0.0, 0.0, 0.0)
        if not all(math.isfinite(x) for x in origin):           # (the smallest coordinate of a mesh with a NaN or an infinity)
            raise RuntimeError("%s: a vertex is not finite" % who)
    o = [float(x) for x in np.asarray(origin, np.float64).reshape(3)]
    return (C.c_double * 3)(*o), h


def _cluster(v, o, h, count_only):
    nv = int(v.size(0))
    with _device_of(v):
        nb = lib.gof_mesh_cluster_ws_bytes(nv)
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        vc = None if count_only else torch.empty(nv, dtype=torch.int32, device=v.device)
        count = C.c_int64()
        B._check(lib.gof_mesh_cluster(nv, _ptr(v), o, h, _ptr(vc), C.byref(count), ws.data_ptr(), nb, _stream()))
    _last["cluster"] = {"vertices": nv, "clusters": int(count.value), "cell": h, "origin": list(o), "workspace_bytes": int(nb)}
    return vc, int(count.value)


def cluster(vertices, cell, origin=None):
    """vertices (NV,3) float64 on a ROCm device -> (vertex_cluster (NV,) int32 there, NC): the cell floor((x - origin) / cell) of every
    vertex, the occupied cells numbered 0..NC-1 in the order of their smallest vertex index.  origin: 3 numbers, default the smallest
    coordinate per axis.  Refused: a vertex that is not finite, a cell coordinate outside [0, 2^21)."""
    v = _tensor(vertices, "cluster", "vertices", (torch.float64,), 3)
    o, h = _grid(v, cell, origin, "cluster")
    return _cluster(v, o, h, False)


def count_clusters(vertices, cell, origin=None):
    """the NC of cluster() without the numbering (the probe of the target search)"""
    v = _tensor(vertices, "count_clusters", "vertices", (torch.float64,), 3)
    o, h = _grid(v, cell, origin, "count_clusters")
    return _cluster(v, o, h, True)[1]


def simplify(vertices, faces, colors=None, cell=None, dedupe=True, origin=None):
    """vertices (NV,3) float64, faces (NF,3) int32 [, colors (NV,4) uint8] on one ROCm device, cell = h -> a dictionary of device tensors
    and numbers: vertex_cluster (NV,) int32 and clusters = NC; per cluster cluster_vertices (NC,3) float64, cluster_colors (NC,4) uint8
    or None, used_mean (NC,) uint8; per input face cluster_faces (NF,3) int32 (the indices through vertex_cluster) and face_keep (NF,)
    uint8 (0: two corners in one cluster, or with dedupe the same unordered triple as a kept face with a smaller index);
    used_mean_count, dropped_degenerate, dropped_duplicate.  Compacting to the kept faces and the clusters they refer to is
    DeviceMesh.simplify's part (the marking and compaction kernels the other mesh operations use)."""
    if cell is None:
        raise ValueError("simplify: cell is required")
    v = _tensor(vertices, "simplify", "vertices", (torch.float64,), 3)
    f = _tensor(faces, "simplify", "faces", (torch.int32,), 3)
    nv, nf = int(v.size(0)), int(f.size(0))
    if nf > MAX_FACES:
        raise RuntimeError("simplify: at most %d faces (3 * faces must be below 2^31)" % MAX_FACES)
    col = None
    if colors is not None:
        col = _tensor(colors, "simplify", "colors", (torch.uint8,), 4)
        if int(col.size(0)) != nv or col.device != v.device:
            raise RuntimeError("simplify: colors must be (NV, 4) on the vertices' device")
    if f.device != v.device:
        raise RuntimeError("simplify: vertices and faces are on different devices")
    o, h = _grid(v, cell, origin, "simplify")
    vc, nc = _cluster(v, o, h, False)
    with _device_of(v):
        nb = lib.gof_mesh_cluster_solve_ws_bytes(nv, nf, nc)
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        pos = torch.empty((nc, 3), dtype=torch.float64, device=v.device)
        out_col = None if col is None else torch.empty((nc, 4), dtype=torch.uint8, device=v.device)
        used = torch.empty(nc, dtype=torch.uint8, device=v.device)
        used_count = C.c_int64()
        B._check(lib.gof_mesh_cluster_solve(nv, nf, _ptr(v), _ptr(f), _ptr(col), _ptr(vc), nc, o, h, _ptr(pos), _ptr(out_col), _ptr(used),
                                            C.byref(used_count), ws.data_ptr(), nb, _stream()))
        nb2 = lib.gof_mesh_cluster_faces_ws_bytes(nf)
        ws2 = torch.empty(nb2, dtype=torch.uint8, device=v.device)
        cf = torch.empty((nf, 3), dtype=torch.int32, device=v.device)
        keep = torch.empty(nf, dtype=torch.uint8, device=v.device)
        counts = (C.c_int64 * 2)()
        B._check(lib.gof_mesh_cluster_faces(nv, nf, _ptr(f), _ptr(vc), nc, 1 if dedupe else 0, _ptr(cf), _ptr(keep), counts, ws2.data_ptr(), nb2, _stream()))
    _last["simplify"] = {"vertices": nv, "faces": nf, "clusters": nc, "cell": h, "origin": list(o), "dedupe": bool(dedupe), "used_mean": int(used_count.value),
                         "dropped_degenerate": int(counts[0]), "dropped_duplicate": int(counts[1]),
                         "workspace_bytes": int(max(nb, nb2, _last["cluster"]["workspace_bytes"]))}
    return {"vertex_cluster": vc, "clusters": nc, "cluster_vertices": pos, "cluster_colors": out_col, "used_mean": used, "cluster_faces": cf, "face_keep": keep,
            "used_mean_count": int(used_count.value), "dropped_degenerate": int(counts[0]), "dropped_duplicate": int(counts[1]), "cell": h, "origin": list(o)}


def choose_cell(vertices, cell=None, grid=None, target_vertices=None, origin=None):
    """Exactly one of cell / grid / target_vertices -> (h, probes); origin: the grid's origin the probes count with (None: the smallest
    coordinate per axis, with which the first probe is one cluster; a probe that the given origin puts outside the grid is refused).  With E the largest extent of the bounding box (h = 1 where E is 0 or
    there is no vertex: one cell): grid: h = E / grid.  target_vertices: the smallest probed h whose cluster count (origin = the
    smallest coordinate per axis) is at most the target: the first probe is 2 E (one cluster), then at most 23 steps of a bisection of
    log h between log(E 2^-20) and log(2 E), each step probing exp of the midpoint.  probes: the (h, clusters) pairs in order."""
    given = [k for k, x in (("cell", cell), ("grid", grid), ("target_vertices", target_vertices)) if x is not None]
    if len(given) != 1:
        raise ValueError("simplify: give exactly one of cell, grid and target_vertices (got %s)" % (", ".join(given) or "none"))
    if cell is not None:
        h = float(cell)
        if not (h > 0.0 and math.isfinite(h)):
            raise ValueError("simplify: the cell size must be finite and above 0, got %r" % (cell,))
        return h, []
    v = _tensor(vertices, "simplify", "vertices", (torch.float64,), 3)
    extent = float((torch.amax(v, dim=0) - torch.amin(v, dim=0)).max().cpu()) if int(v.size(0)) else 0.0
    if not math.isfinite(extent):
        raise RuntimeError("simplify: a vertex is not finite")
    if grid is not None:
        if not (float(grid) >= 1.0 and math.isfinite(float(grid))):
            raise ValueError("simplify: grid must be at least 1, got %r" % (grid,))
        return (extent / float(grid) if extent > 0.0 else 1.0), []
    target = int(target_vertices)
    if target < 1:
        raise ValueError("simplify: target_vertices must be at least 1, got %r" % (target_vertices,))
    if not extent > 0.0:
        return 1.0, []
    best = 2.0 * extent                                          # (kept if no probe meets the target, which only a given origin can cause)
    probes = [(best, count_clusters(v, best, origin))]
    lo, hi = math.log(extent) - 20.0 * math.log(2.0), math.log(best)
    for _ in range(MAX_PROBES - 1):
        mid = 0.5 * (lo + hi)
        h = math.exp(mid)
        if not lo < mid < hi:
            break
        n = count_clusters(v, h, origin)
        probes.append((h, n))
        if n <= target:
            hi, best = mid, h
        else:
            lo = mid
    return best, probes


# ---- the spec of the launcher's GOF_MESH_SIMPLIFY and the command line -------------------------------------------------------------------
_SPEC = {"cell": float, "grid": float, "target_vertices": int, "dedupe": int}


def parse_spec(spec):
    """'grid:1024' / 'target_vertices:2000000' / 'cell:0.01,dedupe:0' -> the keyword arguments of DeviceMesh.simplify; ValueError for
    anything else"""
    out = {}
    for part in str(spec).split(","):
        key, sep, value = part.strip().partition(":")
        key = key.strip().replace("-", "_")
        if not sep or key not in _SPEC or key in out:
            raise ValueError("GOF_MESH_SIMPLIFY: %r is not one of %s as key:value (given once)" % (part, ", ".join(sorted(_SPEC))))
        try:
            out[key] = _SPEC[key](value.strip())
        except ValueError:
            raise ValueError("GOF_MESH_SIMPLIFY: %r is no %s" % (value, _SPEC[key].__name__)) from None
    if sum(k in out for k in ("cell", "grid", "target_vertices")) != 1:
        raise ValueError("GOF_MESH_SIMPLIFY: give exactly one of cell, grid, target_vertices")
    if "cell" in out and not (out["cell"] > 0.0 and math.isfinite(out["cell"])):
        raise ValueError("GOF_MESH_SIMPLIFY: cell must be finite and above 0")
    if "grid" in out and not (out["grid"] >= 1.0 and math.isfinite(out["grid"])):
        raise ValueError("GOF_MESH_SIMPLIFY: grid must be at least 1")
    if "target_vertices" in out and out["target_vertices"] < 1:
        raise ValueError("GOF_MESH_SIMPLIFY: target_vertices must be at least 1")
    if "dedupe" in out:
        if out["dedupe"] not in (0, 1):
            raise ValueError("GOF_MESH_SIMPLIFY: dedupe is 0 or 1")
        out["dedupe"] = bool(out["dedupe"])
    return out


def simplify_file(src, dst, stats=None, **how):
    """mesh_cull.load(src), DeviceMesh.simplify(**how), export(dst) [, the statistics as JSON] -> the statistics"""
    import mesh_cull
    mesh = mesh_cull.load(src)
    st = mesh.simplify(**how)
    mesh.export(dst)
    if stats:
        with open(stats, "w") as fh:
            json.dump(st, fh)
    return st


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m mesh_simplify", description="Simplify a PLY mesh by quadric vertex clustering.")
    ap.add_argument("input")
    ap.add_argument("output")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--cell", type=float, default=None, help="the cell size")
    how.add_argument("--grid", type=float, default=None, help="cells along the largest extent of the bounding box")
    how.add_argument("--target-vertices", type=int, default=None, help="the largest number of clusters to accept")
    ap.add_argument("--no-dedupe", action="store_true", help="keep faces that collapse to the same triple of clusters")
    ap.add_argument("--stats", default=None, help="write the statistics to this JSON file")
    a = ap.parse_args(argv)
    st = simplify_file(a.input, a.output, stats=a.stats, cell=a.cell, grid=a.grid, target_vertices=a.target_vertices, dedupe=not a.no_dedupe)
    print("mesh_simplify: %d -> %d vertices, %d -> %d faces (cell %.9g)" % (st["vertices_before"], st["vertices_after"], st["faces_before"],
                                                                          st["faces_after"], st["cell"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
