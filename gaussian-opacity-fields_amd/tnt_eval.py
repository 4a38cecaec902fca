"""Tanks-and-Temples F-score evaluation on the GPU: the reference's eval_tnt/run.py (registration.py, evaluation.py) without Open3D.

    kept, index = crop(points, volume, transform=None)      # registration.py:118-120  (transform, polygon-volume crop)
    down, counts = voxel_down_sample(points, voxel)          # registration.py:123      (one mean point per voxel, ascending key)
    T, fitness, rmse, record = icp(source, target, threshold)   # registration.py:152-159 (point to point, with scale)
    T0 = align_trajectories(est, gt, gt_trans, seed)         # registration.py:65-108   (RANSAC over the camera centres, host)
    result = tnt_fscore(source, target, T, volume, tau)      # evaluation.py:60-170 without the normals
    python -m tnt_eval --dataset-dir <TNT>/Barn --traj-path Barn_COLMAP_SfM.log --ply-path mesh.ply     # run.py's command line

The kernels are ``gof_cloud_*`` of libgof_hip.so (csrc/cloud_reg.hip, include/gof_cloud_reg_hip.h, and the nearest-neighbour index
of csrc/cloud.hip); the contract is DESIGN.md §3.9: fp64 [N,3] tensors on a ROCm device in and out, results bit-equal to numpy's.
There is no host fallback: host tensors are refused.  Stated deviations: the RANSAC draws come from
``numpy.random.default_rng(seed)``, the voxel order is ascending key, ICP applies the accumulated transformation to the original
points, normals are not estimated.
"""
import contextlib
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn
import mesh_eval

__all__ = ["read_crop_volume", "read_log_trajectory", "crop", "voxel_down_sample", "uniform_down_sample", "transform_points", "icp",
           "umeyama_update", "align_trajectories", "registration_vol_ds", "registration_unif", "tnt_fscore", "run_evaluation", "main",
           "last_stats", "SCENES_TAU"]

# eval_tnt/config.py: the distance threshold tau of every scene, as data
SCENES_TAU = {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003, "Meetingroom": 0.01,
              "Truck": 0.005}
MAX_POINT_NUMBER = 4e6          # registration.py:41
MAX_POLYGON = 4096

lib = B.lib
_vp, _sz, _i64, _f64, _int = C.c_void_p, C.c_size_t, C.c_int64, C.c_double, C.c_int
_P64 = C.POINTER(C.c_int64)
gn.bind(lib, {_name: [_i64] for _name in ("gof_cloud_transform_ws_bytes", "gof_cloud_crop_ws_bytes", "gof_cloud_voxel_ws_bytes", "gof_cloud_icp_sums_ws_bytes")}, {
        "gof_cloud_transform": [_i64, _vp, _vp, _vp, _vp, _sz, _vp],
        "gof_cloud_crop": [_i64, _vp, _vp, _int, _f64, _f64, _i64, _vp, _vp, _vp, _vp, _sz, _P64, _vp],
        "gof_cloud_voxel": [_i64, _vp, _f64, _vp, _vp, _vp, _sz, _P64, _vp],
        "gof_cloud_icp_sums1": [_i64, _vp, _i64, _vp, _vp, _vp, _f64, _vp, _sz, _P64, _vp, _vp],
        "gof_cloud_icp_sums2": [_i64, _vp, _i64, _vp, _vp, _vp, _f64, _vp, _vp, _sz, _vp, _vp]})

_last = {}


def last_stats():
    """Statistics of the last crop / voxel_down_sample / icp / tnt_fscore calls (one sub-dictionary each)."""
    return {k: dict(v) for k, v in _last.items()}


# the device seams, by the names the host tests replace per module (tests/test_tnt_eval_host.py); one definition each: gof_native
# (tsdf_fusion and delaunay bind them the same way)
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "tnt_eval")


def _cloud(t, who, what="points", dtype=torch.float64):
    return gn.rows(t, who, what, dtype, on_device=_on_device)


def _matrix(m, who):
    """-> (4x4 float64 host array or None, pointer for the library)"""
    if m is None:
        return None, None
    a = np.ascontiguousarray(np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m, dtype=np.float64))
    if a.shape != (4, 4):
        raise RuntimeError("%s: the transformation must be a 4x4 matrix" % who)
    return a, a.ctypes.data_as(_vp)


# ---- files --------------------------------------------------------------------------------------------------------------------------
def read_crop_volume(path):
    """Open3D's SelectionPolygonVolume JSON -> {"axis": 0 | 1 | 2, "axis_min", "axis_max", "polygon": (K,3) float64}"""
    with open(path) as f:
        d = json.load(f)
    axis = str(d["orthogonal_axis"]).strip().upper()
    if axis not in ("X", "Y", "Z"):
        raise ValueError("%s: orthogonal_axis must be X, Y or Z, got %r" % (path, d["orthogonal_axis"]))
    poly = np.ascontiguousarray(np.asarray(d["bounding_polygon"], dtype=np.float64).reshape(-1, 3))
    return {"axis": "XYZ".index(axis), "axis_min": float(d["axis_min"]), "axis_max": float(d["axis_max"]), "polygon": poly}


def read_log_trajectory(path):
    """The .log trajectory format (a metadata line, four matrix rows per camera) -> (N,4,4) float64 camera-to-world matrices"""
    with open(path) as f:
        lines = [ln for ln in f.read().splitlines()]
    while lines and not lines[-1].strip():
        lines.pop()
    if len(lines) % 5:
        raise ValueError("%s: a .log trajectory has five lines per camera, this file has %d lines" % (path, len(lines)))
    mats = np.zeros((len(lines) // 5, 4, 4))
    for k in range(len(lines) // 5):
        for r in range(4):
            row = lines[5 * k + 1 + r].split()
            if len(row) != 4:
                raise ValueError("%s: line %d is not a matrix row" % (path, 5 * k + 2 + r))
            mats[k, r] = [float(x) for x in row]
    return mats


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------
def transform_points(points, matrix):
    """out = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3 per row of the 4x4 `matrix` (host) -> (N,3) float64 on points.device"""
    p = _cloud(points, "transform_points")
    m, mp = _matrix(matrix, "transform_points")
    n = int(p.size(0))
    with _device_of(p):
        nb = lib.gof_cloud_transform_ws_bytes(n)
        ws = torch.empty(nb, dtype=torch.uint8, device=p.device)
        out = torch.empty((n, 3), dtype=torch.float64, device=p.device)
        B._check(lib.gof_cloud_transform(n, _ptr(p), mp, _ptr(out), ws.data_ptr(), nb, _stream()))
    return out


def crop(points, volume, transform=None):
    """registration.py:118-120: the points (after `transform`, a 4x4 host matrix) inside the polygon volume, in input order
    -> ((M,3) float64, (M,) int64 rows of `points`) on points.device"""
    p = _cloud(points, "crop")
    m, mp = _matrix(transform, "crop")
    poly = np.ascontiguousarray(np.asarray(volume["polygon"], dtype=np.float64).reshape(-1, 3))
    n, k = int(p.size(0)), len(poly)
    with _device_of(p):
        nb = lib.gof_cloud_crop_ws_bytes(n)
        ws = torch.empty(nb, dtype=torch.uint8, device=p.device)
        pd = torch.from_numpy(poly).to(p.device)
        out = torch.empty((n, 3), dtype=torch.float64, device=p.device)
        idx = torch.empty(n, dtype=torch.int32, device=p.device)
        kept = C.c_int64()
        B._check(lib.gof_cloud_crop(n, _ptr(p), mp, int(volume["axis"]), float(volume["axis_min"]), float(volume["axis_max"]), k, _ptr(pd),
                                    _ptr(out), _ptr(idx), ws.data_ptr(), nb, C.byref(kept), _stream()))
    _last["crop"] = {"points": n, "kept": int(kept.value), "polygon": k, "workspace_bytes": int(nb)}
    return out[:kept.value].clone(), idx[:kept.value].long()


def voxel_down_sample(points, voxel):
    """registration.py:123: one point per occupied voxel of edge `voxel` (the mean of its points, added in input order), in ascending
    order of the voxel key -> ((M,3) float64, (M,) int64 points per voxel)"""
    p = _cloud(points, "voxel_down_sample")
    n = int(p.size(0))
    with _device_of(p):
        nb = lib.gof_cloud_voxel_ws_bytes(n)
        ws = torch.empty(nb, dtype=torch.uint8, device=p.device)
        out = torch.empty((n, 3), dtype=torch.float64, device=p.device)
        cnt = torch.empty(n, dtype=torch.int32, device=p.device)
        m = C.c_int64()
        B._check(lib.gof_cloud_voxel(n, _ptr(p), float(voxel), _ptr(out), _ptr(cnt), ws.data_ptr(), nb, C.byref(m), _stream()))
    _last["voxel"] = {"points": n, "voxels": int(m.value), "workspace_bytes": int(nb)}
    return out[:m.value].clone(), cnt[:m.value].long()


def uniform_down_sample(points, k):
    """every k-th point, starting with the first"""
    p = _cloud(points, "uniform_down_sample")
    if int(k) < 1:
        raise RuntimeError("uniform_down_sample: k must be at least 1")
    return p[::int(k)].contiguous()


def umeyama_update(n, sums1, sums2):
    """The similarity (with scale) that maps the transformed source onto its correspondences, from the 16 sums of one iteration
    (DESIGN.md §3.9, step by step; host numpy fp64) -> 4x4"""
    n = float(n)
    mu_s = np.array([sums1[0] / n, sums1[1] / n, sums1[2] / n])
    mu_t = np.array([sums1[3] / n, sums1[4] / n, sums1[5] / n])
    sigma = np.array(sums2[:9], dtype=np.float64).reshape(3, 3) / n
    var_s = sums2[9] / n
    U, D, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    c = ((D[0] * S[0] + D[1] * S[1]) + D[2] * S[2]) / var_s
    t = mu_t - c * (R @ mu_s)
    out = np.eye(4)
    out[:3, :3] = c * R
    out[:3, 3] = t
    return out


def icp(source, target, threshold, max_iteration=20, relative_fitness=1e-6, relative_rmse=1e-6):
    """registration.py:152-159: point-to-point ICP with scale from the identity -> (4x4 float64 host, fitness, inlier rmse, record).
    record[k] = {"transformation", "n", "sums1" (7), "sums2" (10) or None, "fitness", "rmse"} of the k-th evaluation."""
    s = _cloud(source, "icp", "source")
    t = _cloud(target, "icp", "target")
    if s.device != t.device:
        raise RuntimeError("icp: source and target are on different devices")
    ns, nt = int(s.size(0)), int(t.size(0))
    threshold = float(threshold)
    record = []
    with _device_of(s):
        ib = lib.gof_cloud_nn_index_bytes(nt)
        index = torch.empty(ib, dtype=torch.uint8, device=s.device)
        B._check(lib.gof_cloud_nn_build(nt, _ptr(t), index.data_ptr(), ib, _stream()))
        qb = lib.gof_cloud_nn_query_ws_bytes(ns)
        qws = torch.empty(qb, dtype=torch.uint8, device=s.device)
        sb = lib.gof_cloud_icp_sums_ws_bytes(ns)
        sws = torch.empty(sb, dtype=torch.uint8, device=s.device)
        tb = lib.gof_cloud_transform_ws_bytes(ns)
        tws = torch.empty(tb, dtype=torch.uint8, device=s.device)
        moved = torch.empty((ns, 3), dtype=torch.float64, device=s.device)
        dist = torch.empty(ns, dtype=torch.float64, device=s.device)
        near = torch.empty(ns, dtype=torch.int32, device=s.device)

        def evaluate(T):
            Tc = np.ascontiguousarray(T, dtype=np.float64)
            B._check(lib.gof_cloud_transform(ns, _ptr(s), Tc.ctypes.data_as(_vp), _ptr(moved), tws.data_ptr(), tb, _stream()))
            B._check(lib.gof_cloud_nn_query(nt, index.data_ptr(), ib, ns, _ptr(moved), _ptr(dist), _ptr(near), qws.data_ptr(), qb, _stream()))
            n = C.c_int64()
            s1 = (C.c_double * 7)()
            B._check(lib.gof_cloud_icp_sums1(ns, _ptr(moved), nt, _ptr(t), _ptr(dist), _ptr(near), threshold, sws.data_ptr(), sb, C.byref(n), s1,
                                             _stream()))
            n = int(n.value)
            s1 = [float(x) for x in s1]
            ev = {"transformation": Tc.copy(), "n": n, "sums1": s1, "sums2": None, "fitness": (n / ns if ns else 0.0),
                  "rmse": (float(np.sqrt(s1[6] / n)) if n else 0.0)}
            record.append(ev)
            return ev

        T = np.eye(4)
        ev = evaluate(T)
        for _ in range(int(max_iteration)):
            if ev["n"] < 3:
                break
            n, s1 = ev["n"], ev["sums1"]
            means = (C.c_double * 6)(*[s1[k] / float(n) for k in range(6)])
            s2 = (C.c_double * 10)()
            B._check(lib.gof_cloud_icp_sums2(ns, _ptr(moved), nt, _ptr(t), _ptr(dist), _ptr(near), threshold, means, sws.data_ptr(), sb, s2, _stream()))
            ev["sums2"] = [float(x) for x in s2]
            T = umeyama_update(n, s1, ev["sums2"]) @ T
            prev, ev = ev, evaluate(T)
            if abs(prev["fitness"] - ev["fitness"]) < relative_fitness and abs(prev["rmse"] - ev["rmse"]) < relative_rmse:
                break
    _last["icp"] = {"source": ns, "target": nt, "evaluations": len(record), "correspondences": ev["n"], "index_bytes": int(ib),
                    "workspace_bytes": int(qb + sb + tb)}
    return T, ev["fitness"], ev["rmse"], record


# ---- trajectory alignment (host) ----------------------------------------------------------------------------------------------------
def _similarity_batch(src, dst):
    """Umeyama with scale for a batch: src, dst (B,n,3) -> (c (B,), R (B,3,3), t (B,3)); sums run over the n points in their order"""
    n = src.shape[1]
    mu_s, mu_d = src[:, 0].copy(), dst[:, 0].copy()
    for k in range(1, n):
        mu_s = mu_s + src[:, k]
        mu_d = mu_d + dst[:, k]
    mu_s, mu_d = mu_s / float(n), mu_d / float(n)
    a, b = src - mu_s[:, None], dst - mu_d[:, None]
    cov = b[:, 0, :, None] * a[:, 0, None, :]
    var = (a[:, 0, 0] * a[:, 0, 0] + a[:, 0, 1] * a[:, 0, 1]) + a[:, 0, 2] * a[:, 0, 2]
    for k in range(1, n):
        cov = cov + b[:, k, :, None] * a[:, k, None, :]
        var = var + ((a[:, k, 0] * a[:, k, 0] + a[:, k, 1] * a[:, k, 1]) + a[:, k, 2] * a[:, k, 2])
    cov, var = cov / float(n), var / float(n)
    with np.errstate(all="ignore"):
        U, D, Vt = np.linalg.svd(cov)
        S = np.ones_like(D)
        S[np.linalg.det(U) * np.linalg.det(Vt) < 0, 2] = -1.0
        R = (U * S[:, None, :]) @ Vt
        c = ((D[:, 0] * S[:, 0] + D[:, 1] * S[:, 1]) + D[:, 2] * S[:, 2]) / var
        Rm = (R[:, :, 0] * mu_s[:, None, 0] + R[:, :, 1] * mu_s[:, None, 1]) + R[:, :, 2] * mu_s[:, None, 2]
        t = mu_d - c[:, None] * Rm
    return c, R, t


def _score_batch(c, R, t, est, gt, threshold):
    """-> (inlier counts (B,), rmse over the inliers (B,), finite (B,)) of the hypotheses over all N identity correspondences"""
    with np.errstate(all="ignore"):
        A = c[:, None, None] * R                                                        # (B,3,3)
        moved = ((A[:, None, :, 0] * est[None, :, None, 0] + A[:, None, :, 1] * est[None, :, None, 1]) + A[:, None, :, 2] * est[None, :, None, 2]) + t[:, None, :]
        e = moved - gt[None]
        d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        dist = np.sqrt(d2)
        finite = np.isfinite(c) & np.isfinite(R).all(axis=(1, 2)) & np.isfinite(t).all(axis=1)
        inl = dist < threshold
        cnt = inl.sum(axis=1)
        sq = np.where(inl, d2, 0.0)
        acc = np.zeros(len(c))
        for k in range(sq.shape[1]):                                                    # left to right over the cameras
            acc = acc + sq[:, k]
        rmse = np.sqrt(acc / np.maximum(cnt, 1))
    return cnt, rmse, finite


def align_trajectories(est, gt, gt_trans, seed, iterations=100000, threshold=0.2, n=6):
    """registration.py:65-108: RANSAC over the identity correspondences of the camera centres est[i] <-> gt_trans . gt[i].
    Host numpy, batched (a few thousand points: DESIGN.md §3.9).  Hypothesis h is fitted to the rows
    default_rng(seed).integers(0, N, (iterations, n))[h]; the winner has the most inliers (dist < threshold), then the lower rmse over
    them, then the lower h; non-finite hypotheses are skipped -> 4x4 float64 (the identity if no hypothesis is finite)."""
    est = np.ascontiguousarray(np.asarray(est, dtype=np.float64).reshape(-1, 3))
    gt = np.ascontiguousarray(np.asarray(gt, dtype=np.float64).reshape(-1, 3))
    if len(est) != len(gt):
        raise ValueError("align_trajectories: %d estimated and %d reference cameras" % (len(est), len(gt)))
    if gt_trans is not None:
        G = np.asarray(gt_trans, dtype=np.float64).reshape(4, 4)
        gt = np.stack([((G[r, 0] * gt[:, 0] + G[r, 1] * gt[:, 1]) + G[r, 2] * gt[:, 2]) + G[r, 3] for r in range(3)], axis=-1)
    N = len(est)
    out = np.eye(4)
    if N == 0:
        return out
    draws = np.random.default_rng(seed).integers(0, N, (int(iterations), int(n)))
    best = None
    chunk = max(1, min(int(iterations), 4_000_000 // max(N, 1)))
    for h0 in range(0, int(iterations), chunk):
        idx = draws[h0:h0 + chunk]
        c, R, t = _similarity_batch(est[idx], gt[idx])
        cnt, rmse, finite = _score_batch(c, R, t, est, gt, threshold)
        for h in np.nonzero(finite)[0]:
            key = (-int(cnt[h]), float(rmse[h]), h0 + int(h))
            if best is None or key < best[0]:
                best = (key, c[h], R[h].copy(), t[h].copy())
    if best is not None:
        out[:3, :3] = best[1] * best[2]
        out[:3, 3] = best[3]
        _last["ransac"] = {"cameras": N, "hypothesis": best[0][2], "inliers": -best[0][0], "rmse": best[0][1]}
    return out


# ---- registration and F-score ---------------------------------------------------------------------------------------------------------
def registration_vol_ds(source, target, init_trans, volume, voxel, threshold, max_iteration=20):
    """registration.py:164-200 -> (transformation . init_trans, fitness, rmse, record)"""
    s, _ = crop(source, volume, init_trans)
    s, _ = voxel_down_sample(s, voxel)
    t, _ = crop(target, volume)
    t, _ = voxel_down_sample(t, voxel)
    T, fit, rmse, rec = icp(s, t, threshold, max_iteration, 1e-6, 1e-6)
    return T @ np.asarray(init_trans, dtype=np.float64), fit, rmse, rec


def _uniform_if_large(p):
    n = int(p.size(0))
    if n > MAX_POINT_NUMBER:
        return uniform_down_sample(p, int(round(n / float(MAX_POINT_NUMBER))))
    return p


def registration_unif(source, target, init_trans, volume, threshold, max_iteration=20):
    """registration.py:132-161 -> (transformation . init_trans, fitness, rmse, record)"""
    s = _uniform_if_large(crop(source, volume, init_trans)[0])
    t = _uniform_if_large(crop(target, volume)[0])
    T, fit, rmse, rec = icp(s, t, threshold, max_iteration, 1e-6, 1e-6)
    return T @ np.asarray(init_trans, dtype=np.float64), fit, rmse, rec


def _counts(dist, tau, edges):
    """#(dist < tau) and numpy.histogram(dist, edges)'s counts (half-open bins, the last closed), on the device"""
    below = int((dist < tau).sum().item())
    e = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.float64)).to(dist.device)
    nb = len(edges) - 1
    b = torch.bucketize(dist, e, right=True) - 1                  # edges[b] <= d < edges[b + 1]
    b = torch.where(dist == e[-1], torch.full_like(b, nb - 1), b)
    ok = (b >= 0) & (b < nb)
    hist = torch.bincount(b[ok], minlength=nb)[:nb]
    return below, hist.cpu().numpy().astype(np.int64)


def tnt_fscore(source, target, transform, volume, tau, plot_stretch=5):
    """evaluation.py:60-170 without the normals: s = voxel(crop(transform . source), tau / 2), t = voxel(crop(target), tau / 2), the
    nearest distances in both directions, precision / recall / F-score at tau and the two cumulative histograms over
    numpy.arange(0, plot_stretch tau, tau / 100)."""
    tau = float(tau)
    s, _ = crop(source, volume, transform)
    s, _ = voxel_down_sample(s, tau / 2.0)
    t, _ = crop(target, volume)
    t, _ = voxel_down_sample(t, tau / 2.0)
    d1, _ = mesh_eval.nearest(s, t)
    d2, _ = mesh_eval.nearest(t, s)
    edges = np.arange(0, tau * plot_stretch, tau / 100)
    res = {"source": s, "target": t, "dist_source": d1, "dist_target": d2, "edges": edges, "tau": tau}
    if len(d1) and len(d2):
        n1, h1 = _counts(d1, tau, edges)
        n2, h2 = _counts(d2, tau, edges)
        recall = float(n2) / float(len(d2))
        precision = float(n1) / float(len(d1))
        fscore = 2 * recall * precision / (recall + precision) if recall + precision > 0 else 0.0
        res.update(precision=precision, recall=recall, fscore=fscore, below_source=n1, below_target=n2, hist_source=h1, hist_target=h2,
                   cum_source=np.cumsum(h1).astype(float) / len(d1), cum_target=np.cumsum(h2).astype(float) / len(d2))
    else:
        res.update(precision=0.0, recall=0.0, fscore=0.0, below_source=0, below_target=0, hist_source=np.zeros(0, np.int64),
                   hist_target=np.zeros(0, np.int64), cum_source=np.array([0.0]), cum_target=np.array([0.0]), edges=np.array([0.0]))
    _last["fscore"] = {"source": int(s.size(0)), "target": int(t.size(0)), "below_source": res["below_source"], "below_target": res["below_target"]}
    return res


def _write_cloud(path, points, dist, max_distance, cmap):
    p = points.detach().cpu().numpy()
    if cmap is not None:
        d = dist.detach().cpu().numpy()
        mesh_eval.write_vis_ply(path, p, cmap(np.minimum(d, max_distance) / max_distance)[:, :3])
        return
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\nend_header\n" % len(p)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(p, dtype="<f8").tobytes())


def _plot(scene, res, out_dir, plot_stretch, plt):
    """The precision / recall figure (contract: DESIGN.md §3.9): the two cumulative histograms in percent over the upper bin edges,
    a marker line at tau, the F-score in the title; written as PNG and PDF under the name the Tanks-and-Temples tools look for."""
    tau = res["tau"]
    fig, ax = plt.subplots(figsize=(8, 4.5))
    upper = res["edges"][1:]
    if len(upper):
        for key, colour, name in (("cum_source", "tab:red", "precision"), ("cum_target", "tab:blue", "recall")):
            ax.plot(upper, 100.0 * res[key], color=colour, lw=1.8, label=name)
    ax.axvline(tau, color="0.2", linestyle=":", lw=1.5, label="tau = %g" % tau)
    ax.set_xlim(0.0, plot_stretch * tau)
    ax.set_ylim(0.0, 100.0)
    ax.set_xlabel("distance")
    ax.set_ylabel("points within the distance (%)")
    ax.set_title("%s: F-score %.2f %% at tau" % (scene, 100.0 * res["fscore"]))
    ax.grid(alpha=0.4)
    ax.legend(loc="lower right")
    stem = os.path.join(out_dir, "PR_%s_@d_th_0_%04d" % (scene, tau * 10000))
    for ext in ("png", "pdf"):
        fig.savefig(stem + "." + ext, bbox_inches="tight")
    plt.close(fig)


def run_evaluation(dataset_dir, traj_path, ply_path, out_dir, seed=0, tau=None):
    """The sequence of eval_tnt/run.py: trajectory alignment, three ICP refinements, F-score.  Writes
    <scene>.precision.txt / .recall.txt / .prf_tau_plotstr.txt, the two clouds, results.json and (with matplotlib) the plot into
    out_dir -> the dictionary of tnt_fscore plus "transformation"."""
    scene = os.path.basename(os.path.normpath(dataset_dir))
    if tau is None:
        if scene not in SCENES_TAU:
            raise Exception("invalid dataset-dir, not in scenes_tau_dict")
        tau = SCENES_TAU[scene]
    tau = float(tau)
    dev = _device()
    if not str(traj_path).endswith(".log"):
        raise ValueError("%s: only .log trajectories are supported (DESIGN.md §7)" % traj_path)
    os.makedirs(out_dir, exist_ok=True)
    gt_file = os.path.join(dataset_dir, scene + ".ply")
    ref_log = os.path.join(dataset_dir, scene + "_COLMAP_SfM.log")
    print("tnt_eval: scene %s, tau %g\n  mesh        %s\n  scan        %s\n  trajectory  %s\n  reference   %s" % (scene, tau, ply_path, gt_file, traj_path, ref_log))
    vertices, faces = mesh_eval.read_ply(ply_path)
    if faces is not None and len(faces):
        tri = vertices[faces]
        vertices = np.concatenate([vertices, ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / 3.0], axis=0)      # the source: vertices + face centroids
    source = torch.from_numpy(np.ascontiguousarray(vertices)).to(dev)
    target = torch.from_numpy(mesh_eval.read_ply(gt_file)[0]).to(dev)
    gt_trans = np.loadtxt(os.path.join(dataset_dir, scene + "_trans.txt"))
    est = read_log_trajectory(traj_path)
    ref = read_log_trajectory(ref_log)
    T = align_trajectories(est[:, :3, 3], ref[:, :3, 3], gt_trans, seed)
    if "ransac" in _last:
        print("  alignment   %d of %d cameras within 0.2 (hypothesis %d)" % (_last["ransac"]["inliers"], len(est), _last["ransac"]["hypothesis"]))
    volume = read_crop_volume(os.path.join(dataset_dir, scene + ".json"))
    plot_stretch = 5
    for stage, (voxel, threshold) in enumerate(((tau, 80 * tau), (tau / 2.0, 20 * tau), (None, 2 * tau))):
        if voxel is None:
            T, fit, rmse, rec = registration_unif(source, target, T, volume, threshold, 20)
        else:
            T, fit, rmse, rec = registration_vol_ds(source, target, T, volume, voxel, threshold, 20)
        print("  icp stage %d voxel %s threshold %g: %d evaluations, fitness %.4f, rmse %.5g" % (stage + 1, "-" if voxel is None else "%g" % voxel, threshold, len(rec), fit, rmse))
    res = tnt_fscore(source, target, T, volume, tau, plot_stretch)
    res["transformation"] = T
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        cmap = plt.get_cmap("hot_r")
    except ImportError:
        plt = cmap = None
        print("matplotlib is not importable: the two clouds are written without colours and the plot is left out")
    base = os.path.join(out_dir, scene)
    _write_cloud(base + ".precision.ply", res["source"], res["dist_source"], 3 * tau, cmap)
    _write_cloud(base + ".recall.ply", res["target"], res["dist_target"], 3 * tau, cmap)
    np.savetxt(base + ".precision.txt", res["cum_source"])
    np.savetxt(base + ".recall.txt", res["cum_target"])
    np.savetxt(base + ".prf_tau_plotstr.txt", np.array([res["precision"], res["recall"], res["fscore"], tau, plot_stretch]))
    with open(os.path.join(out_dir, "results.json"), "w") as fp:
        json.dump({"precision": res["precision"], "recall": res["recall"], "fscore": res["fscore"], "tau": tau,
                   "transformation": [[float(x) for x in row] for row in T]}, fp, indent=True)
    print("  result      precision %.4f  recall %.4f  f-score %.4f  (%s)" % (res["precision"], res["recall"], res["fscore"], out_dir))
    if plt is not None:
        _plot(scene, res, out_dir, plot_stretch, plt)
    return res


def main(argv=None):
    """The command line of eval_tnt/run.py (the same argument names) plus --seed and --tau"""
    import argparse
    parser = argparse.ArgumentParser(prog="tnt_eval")
    parser.add_argument("--dataset-dir", required=True, help="scene directory <scene>/ with <scene>.ply, <scene>.json, <scene>_trans.txt, <scene>_COLMAP_SfM.log")
    parser.add_argument("--traj-path", required=True, help="camera trajectory of the reconstruction (.log)")
    parser.add_argument("--ply-path", required=True, help="the reconstructed mesh (PLY)")
    parser.add_argument("--out-dir", default=None, help="where the results go (default: evaluation/ next to the mesh)")
    parser.add_argument("--view-crop", type=int, default=0, help="accepted and ignored (no window)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the trajectory alignment's draws")
    parser.add_argument("--tau", type=float, default=None, help="distance threshold (default: the scene's, by the directory name)")
    args = parser.parse_args(argv)
    out_dir = args.out_dir.strip() if args.out_dir else ""
    if not out_dir:
        out_dir = os.path.join(os.path.dirname(os.path.abspath(args.ply_path)), "evaluation")
    return run_evaluation(args.dataset_dir, args.traj_path, args.ply_path, out_dir, seed=args.seed, tau=args.tau)


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main(sys.argv[1:])
