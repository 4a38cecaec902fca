"""Delaunay tetrahedralization on the GPU: the reference's ``tetranerf.utils.extension.cpp.triangulate`` (CGAL's
Delaunay_triangulation_3, extract_mesh.py:51) without CGAL.

    tets = triangulate(points)        # (N,3) float32 on a ROCm device -> (M,4) int32 on that device

The kernels are ``gof_delaunay_*`` of libgof_hip.so (csrc/delaunay.hip, include/gof_delaunay_hip.h); the contract is DESIGN.md §3.7:
exact predicates, ties broken by a symbolic perturbation, duplicates as one vertex (the lowest index), positively oriented cells in
a canonical sorted order.  There is no host fallback: host tensors are refused.
"""
import ctypes as C

import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["triangulate", "last_stats"]

GOF_E_CAPACITY = -5
_STAT_NAMES = ("rounds", "exact_evaluations", "peak_cells", "slow_insertions", "located_by_scan", "distinct_points", "capacity", "live_cells")

lib = B.lib
gn.bind(lib, {"gof_delaunay_ws_bytes": [C.c_int64, C.c_int64]}, {
    "gof_delaunay_build": [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.c_void_p],
    "gof_delaunay_emit": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "gof_delaunay_stats": [C.c_void_p, C.c_void_p, C.c_void_p]})

# The initial arena: cells per point, learnt from the last call of at least 1024 points (its live cells, finite and infinite --
# the arena holds both -- per point, with 10 % headroom), clamped to [6.5, 8] so that one unusual input neither starves nor inflates
# the next calls; a call that needs more grows its own arena (GOF_E_CAPACITY) without changing this.
_CPP_MIN, _CPP_MAX = 6.5, 8.0
_cells_per_point = 7.0
_last = {}

# the device seams, by the names the host tests replace per module (tests/test_delaunay_host.py); one definition each: gof_native
_stream, _device_of, _on_device = gn.stream, gn.device_of, gn.on_device


def last_stats():
    """Statistics of the last triangulate call: rounds, exact predicate evaluations, peak arena cells and bytes, ..., and how often it
    started over with a larger arena ("retries")"""
    return dict(_last)


def triangulate(points: torch.Tensor, capacity: int = None) -> torch.Tensor:
    """Finite cells of the Delaunay tetrahedralization of `points` -> (M,4) int32 on points.device.

    capacity: the initial cell arena (default: learnt, about 7 N + 64); the call doubles it and starts over while it is too small."""
    global _cells_per_point
    if points.dim() != 2 or points.size(1) != 3:
        raise RuntimeError("triangulate: points must have dimensions (num_points, 3)")
    if not _on_device(points):
        raise RuntimeError("triangulate (gfx950 backend) needs the points on a ROCm device, got %s" % points.device)
    if points.dtype != torch.float32:
        raise RuntimeError("triangulate: expected a float32 tensor, got %s" % points.dtype)
    pts = points.contiguous()
    n = int(pts.size(0))
    if n >= 2 ** 31:
        raise RuntimeError("triangulate: at most 2^31 - 1 points")
    cap = int(capacity) if capacity else int(_cells_per_point * n) + 64
    cap = max(16, min(cap, 2 ** 30 - 1))
    retries = 0
    with _device_of(pts):
        while True:
            nb = lib.gof_delaunay_ws_bytes(n, cap)
            ws = torch.empty(nb, dtype=torch.uint8, device=pts.device)
            m = C.c_int64()
            rc = lib.gof_delaunay_build(n, pts.data_ptr(), cap, ws.data_ptr(), nb, C.byref(m), _stream())
            if rc == GOF_E_CAPACITY and m.value > cap:
                del ws
                cap, retries = int(m.value), retries + 1
                continue
            B._check(rc)
            break
        out = torch.empty((m.value, 4), dtype=torch.int32, device=pts.device)
        B._check(lib.gof_delaunay_emit(ws.data_ptr(), m.value, out.data_ptr() if m.value else None, _stream()))
        st = (C.c_int64 * 8)()
        B._check(lib.gof_delaunay_stats(ws.data_ptr(), st, _stream()))
    _last.clear()
    _last.update(zip(_STAT_NAMES, list(st)))
    _last["workspace_bytes"] = int(nb)
    _last["cells"] = int(m.value)
    _last["retries"] = retries
    if n >= 1024 and _last["live_cells"] > 0:
        _cells_per_point = min(_CPP_MAX, max(_CPP_MIN, 1.1 * _last["live_cells"] / n))
    return out
