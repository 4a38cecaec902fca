"""The contract of the mesh simplification restated in numpy fp64, for the tests: cells and their numbering, the corner
quadrics and vertex sums in the written summation order (every run of a tile, every run of tile sums of a block and every run of block
sums added from left to right, one addition at a time; numpy only runs the independent runs side by side), the regularised Cholesky
solve with its fallback, the face remap, the degenerate and duplicate faces, and the compaction by boolean indexing.
Test infrastructure only."""
import numpy as np

from mesh_cull_restatement import ply_bytes  # noqa: F401  (the exported file's bytes)

SUM_TILE, SUM_BLOCK = 256, 65536
CELL_LIMIT = 2.0 ** 21
REG = 2.0 ** -10


class Refused(ValueError):
    pass


# ---- cells ---------------------------------------------------------------------------------------------------------------------------
def default_origin(V):
    V = np.asarray(V, np.float64).reshape(-1, 3)
    return V.min(axis=0) if len(V) else np.zeros(3)


def cells(V, origin, h):
    """(NV,3) float64: floor((x - o) / h) per axis; Refused for what the contract refuses"""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    o = np.asarray(origin, np.float64).reshape(3)
    if not (np.isfinite(o).all() and np.isfinite(h) and h > 0):
        raise Refused("grid")
    if not np.isfinite(V).all():
        raise Refused("finite")
    with np.errstate(over="ignore", invalid="ignore"):
        i = np.floor((V - o[None, :]) / h)
    if not ((i >= 0) & (i < CELL_LIMIT)).all():
        raise Refused("range")
    return i


def cluster(V, h, origin=None):
    """-> (vertex_cluster (NV,) int32, NC): occupied cells numbered in the order of their smallest vertex index"""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    i = cells(V, default_origin(V) if origin is None else origin, h).astype(np.int64)
    key = i[:, 0] * 2 ** 42 + i[:, 1] * 2 ** 21 + i[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32).reshape(len(V)), len(first)


# ---- sums in the written order -----------------------------------------------------------------------------------------------------------
def _runs(values, group):
    """values (N,K), group (N,) non-decreasing: every run of equal group added from left to right, starting from its first
    -> (sums (R,K), the position of every run's first item (R,))"""
    n = len(group)
    starts = np.flatnonzero(np.concatenate([[True], group[1:] != group[:-1]]))
    lens = np.diff(np.concatenate([starts, [n]]))
    acc = values[starts].copy()
    with np.errstate(all="ignore"):
        for j in range(1, int(lens.max())):
            m = lens > j
            acc[m] = acc[m] + values[starts[m] + j]
    return acc, starts


def segment_sums(values, keys, NC):
    """values (N,K) in sorted order, keys (N,) ascending cluster numbers -> (NC,K): tiles of 256 positions, blocks of 65536, the blocks;
    a cluster without an item sums to zero"""
    values = np.asarray(values)
    out = np.zeros((NC, values.shape[1]), values.dtype)
    if len(keys) == 0:
        return out
    keys = np.asarray(keys, np.int64)
    pos = np.arange(len(keys), dtype=np.int64)
    ntiles, nblocks = len(keys) // SUM_TILE + 1, len(keys) // SUM_BLOCK + 1
    s1, first1 = _runs(values, keys * ntiles + pos // SUM_TILE)
    k1, b1 = keys[first1], pos[first1] // SUM_BLOCK
    s2, first2 = _runs(s1, k1 * nblocks + b1)
    k2 = k1[first2]
    s3, first3 = _runs(s2, k2)
    out[k2[first3]] = s3
    return out


def corner_quadrics(V, F, centre_of_corner):
    """(3 NF, 10) per corner e = 3 f + k: A (xx xy xz yy yz zz), b, c of the plane of face f relative to centre_of_corner[e]"""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    f = np.repeat(np.arange(len(F)), 3)
    c = np.asarray(centre_of_corner, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q0, q1, q2 = V[F[f, 0]] - c, V[F[f, 1]] - c, V[F[f, 2]] - c
        e1, e2 = q1 - q0, q2 - q0
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        L = np.sqrt((nx * nx + ny * ny) + nz * nz)
        w = 0.5 / L
        d = -((nx * q0[:, 0] + ny * q0[:, 1]) + nz * q0[:, 2])
        wx, wy, wz, wd = w * nx, w * ny, w * nz, w * d
        Q = np.stack([wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, wd * nx, wd * ny, wd * nz, wd * d], axis=1)
    Q[L == 0.0] = 0.0
    return Q.reshape(-1, 10)


def sums(V, F, Col, vc, NC, h, origin):
    """-> dict: count (NC,), centre (NC,3), qsum (NC,3), csum (NC,3) int64, quadric (NC,10)"""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    vc = np.asarray(vc, np.int64)
    o = np.asarray(origin, np.float64).reshape(3)
    order = np.argsort(vc, kind="stable")
    count = np.bincount(vc, minlength=NC).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    centre = np.zeros((NC, 3))
    have = count > 0
    first = order[start[have]]
    centre[have] = o[None, :] + (cells(V[first], o, h) + 0.5) * h
    first_of = np.zeros(NC, np.int64)
    first_of[have] = first
    qsum = segment_sums((V - centre[vc])[order], vc[order], NC)
    csum = np.zeros((NC, 3), np.int64)
    if Col is not None:
        for a in range(3):
            csum[:, a] = np.bincount(vc, weights=np.asarray(Col)[:, a].astype(np.float64), minlength=NC).astype(np.int64)      # (integers below 2^53: exact)
    cv = vc[F.reshape(-1)] if len(F) else np.zeros(0, np.int64)
    Q = corner_quadrics(V, F, centre[cv])
    corder = np.argsort(cv, kind="stable")
    quadric = segment_sums(Q[corder], cv[corder], NC)
    return {"count": count, "first": first_of, "centre": centre, "qsum": qsum, "csum": csum, "quadric": quadric}


# ---- solve ---------------------------------------------------------------------------------------------------------------------------
def solve(S, h, V=None):
    """-> (position (NC,3), mean (NC,3), used_mean (NC,) uint8, y (NC,3)): the operations in the order DESIGN.md §3.21 writes; with V, a
    cluster of one vertex skips the solve and its position is that vertex's own doubles"""
    n = S["count"].astype(np.float64)
    NC = len(n)
    m = np.zeros((NC, 3))
    have = n > 0
    m[have] = S["qsum"][have] / n[have, None]
    Q = S["quadric"]
    with np.errstate(all="ignore"):
        t = (Q[:, 0] + Q[:, 3]) + Q[:, 5]
        lam = t * REG
        a00, a11, a22, a01, a02, a12 = Q[:, 0] + lam, Q[:, 3] + lam, Q[:, 5] + lam, Q[:, 1], Q[:, 2], Q[:, 4]
        r0, r1, r2 = lam * m[:, 0] - Q[:, 6], lam * m[:, 1] - Q[:, 7], lam * m[:, 2] - Q[:, 8]
        l00 = np.sqrt(a00)
        l10, l20 = a01 / l00, a02 / l00
        l11 = np.sqrt(a11 - l10 * l10)
        l21 = (a12 - l20 * l10) / l11
        l22 = np.sqrt((a22 - l20 * l20) - l21 * l21)
        z0 = r0 / l00
        z1 = (r1 - l10 * z0) / l11
        z2 = ((r2 - l20 * z0) - l21 * z1) / l22
        y2 = z2 / l22
        y1 = (z1 - l21 * y2) / l11
        y0 = ((z0 - l10 * y1) - l20 * y2) / l00
        half = 0.5 * h
        ok = (t != 0.0) & (n != 1.0) & (np.abs(y0) <= half) & (np.abs(y1) <= half) & (np.abs(y2) <= half)
    y = np.where(ok[:, None], np.stack([y0, y1, y2], axis=1), m)
    pos = S["centre"] + y
    if V is not None:
        pos[n == 1.0] = np.asarray(V, np.float64).reshape(-1, 3)[S["first"][n == 1.0]]
    return pos, m, (~ok).astype(np.uint8), y


def colours(S):
    n = S["count"]
    out = np.zeros((len(n), 4), np.uint8)
    have = n > 0
    out[have, :3] = ((2 * S["csum"][have] + n[have, None]) // (2 * n[have, None])).astype(np.uint8)
    return out


def objective(Q, lam, m, y):
    """Q(y) + lam |y - m|^2 per cluster, Q(y) = y^T A y + 2 b.y + c"""
    A = np.stack([Q[:, [0, 1, 2]], Q[:, [1, 3, 4]], Q[:, [2, 4, 5]]], axis=1)
    Ay = np.einsum("nij,nj->ni", A, y)
    return np.einsum("ni,ni->n", y, Ay) + 2.0 * np.einsum("ni,ni->n", Q[:, 6:9], y) + Q[:, 9] + lam * ((y - m) ** 2).sum(axis=1)


# ---- faces ---------------------------------------------------------------------------------------------------------------------------
def cluster_faces(F, vc, dedupe=True):
    """-> (cluster_faces (NF,3) int32, face_keep (NF,) uint8, dropped degenerate, dropped duplicate)"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    cf = np.asarray(vc, np.int64)[F].reshape(-1, 3)
    distinct = (cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 0] != cf[:, 2])
    keep = distinct.copy()
    if dedupe and distinct.any():
        idx = np.flatnonzero(distinct)
        _, first = np.unique(np.sort(cf[idx], axis=1), axis=0, return_index=True)
        keep[:] = False
        keep[idx[first]] = True
    return cf.astype(np.int32), keep.astype(np.uint8), int((~distinct).sum()), int(distinct.sum() - keep.sum())


def simplify(V, F, N=None, Col=None, h=None, dedupe=True, origin=None):
    """-> dict with everything the product returns and the final mesh: v, f, n, c (after dropping the unreferenced clusters)"""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int32).reshape(-1, 3)
    o = default_origin(V) if origin is None else np.asarray(origin, np.float64)
    if len(F) and (F.min() < 0 or F.max() >= len(V)):
        raise Refused("index")
    vc, NC = cluster(V, h, o)
    col4 = None
    if Col is not None:
        col4 = np.zeros((len(V), 4), np.uint8)
        col4[:, :3] = np.asarray(Col, np.uint8).reshape(len(V), -1)[:, :3]
    S = sums(V, F, col4, vc, NC, h, o)
    pos, m, used, y = solve(S, h, V)
    cc = colours(S) if Col is not None else None
    cf, keep, ndeg, ndup = cluster_faces(F, vc, dedupe)
    f2 = cf[keep.astype(bool)]
    ref = np.zeros(NC, bool)
    ref[f2.reshape(-1)] = True
    new = np.cumsum(ref) - 1
    v_out, f_out = pos[ref], new[f2].astype(np.int32).reshape(-1, 3)
    c_out = None if cc is None else cc[ref][:, :3]
    n_out = None
    if N is not None:
        import mesh_render_restatement as RR
        n_out = RR.vertex_normals(v_out.astype(np.float32), f_out)
    return {"vertex_cluster": vc, "clusters": NC, "cluster_vertices": pos, "cluster_colors": cc, "used_mean": used, "cluster_faces": cf, "face_keep": keep,
            "dropped_degenerate": ndeg, "dropped_duplicate": ndup, "v": v_out, "f": f_out, "n": n_out, "c": c_out, "sums": S, "mean": m, "y": y}
