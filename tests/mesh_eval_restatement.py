"""The yardstick of the DTU Chamfer evaluation: the computation of the reference's dtu_eval/eval.py written anew
from the contract, as plain functions over numpy arrays -- scikit-learn's kd-tree for the radius and nearest queries, the
sequential loop for the thinning, the permutation as an argument.  Test infrastructure only; nothing here is used by the product."""
import numpy as np


def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def sample_triangles(vertices, triangles, thresh):
    """-> (samples (M,3) in triangle order then (i, j), counts per triangle (NT,))"""
    V = np.asarray(vertices, np.float64)
    T = np.asarray(triangles, np.int64).reshape(-1, 3)
    counts = np.zeros(len(T), np.int64)
    if len(T) == 0:
        return np.zeros((0, 3)), counts
    p0 = V[T[:, 0]]
    v1 = V[T[:, 1]] - p0
    v2 = V[T[:, 2]] - p0
    l1, l2 = _norm(v1), _norm(v2)
    area2 = _norm(_cross(v1, v2))
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        thr = thresh * np.sqrt(l1 * l2 / area2)
        n1 = np.floor(l1 / thr)
        n2 = np.floor(l2 / thr)
    for t in np.nonzero(area2 > 0)[0]:
        a = (np.arange(int(n1[t]) + 1, dtype=np.float64) + 0.5) / max(n1[t], 1e-7)
        b = (np.arange(int(n2[t]) + 1, dtype=np.float64) + 0.5) / max(n2[t], 1e-7)
        A, Bm = np.meshgrid(a, b, indexing="ij")
        sel = (A + Bm) < 1
        if not sel.any():
            continue
        ka, kb = A[sel][:, None], Bm[sel][:, None]             # row-major: i outer, j inner
        out.append((v1[t][None] * ka + v2[t][None] * kb) + p0[t][None])
        counts[t] = len(ka)
    return (np.concatenate(out, axis=0) if out else np.zeros((0, 3))), counts


def sample_mesh(vertices, triangles, thresh):
    return np.concatenate([np.asarray(vertices, np.float64), sample_triangles(vertices, triangles, thresh)[0]], axis=0)


def _engine(points, n_jobs=-1):
    import sklearn.neighbors as skln
    return skln.NearestNeighbors(n_neighbors=1, algorithm="kd_tree", n_jobs=n_jobs).fit(points)


def thin(points, r):
    """the sequential loop: visit in order, a kept point removes everything within r of it"""
    P = np.asarray(points, np.float64)
    mask = np.ones(len(P), np.bool_)
    if len(P) == 0:
        return mask
    idxs = _engine(P).radius_neighbors(P, radius=r, return_distance=False)
    for cur, ix in enumerate(idxs):
        if mask[cur]:
            mask[ix] = 0
            mask[cur] = 1
    return mask


def thin_brute(points, r):
    """the definition itself, O(N^2): keep[i] iff no kept j < i has (dx dx + dy dy) + dz dz <= r r"""
    P = np.asarray(points, np.float64)
    keep = np.zeros(len(P), np.bool_)
    r2 = r * r
    for i in range(len(P)):
        d = P[:i][keep[:i]] - P[i]
        keep[i] = not ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2).any()
    return keep


def pairs_near_radius(points, r, ulps=4):
    """number of pairs whose squared distance lies within `ulps` ulp of r r (where the two sides could legitimately differ)"""
    P = np.asarray(points, np.float64)
    if len(P) < 2:
        return 0
    r2 = r * r
    idxs = _engine(P).radius_neighbors(P, radius=r * (1 + 1e-9), return_distance=False)
    n = 0
    for i, ix in enumerate(idxs):
        ix = ix[ix > i]
        d = P[ix] - P[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        n += int((np.abs(d2 - r2) <= ulps * np.spacing(r2)).sum())
    return n


def nearest(query, ref):
    """-> (dist (NQ,), index (NQ,)); an empty ref gives +inf and -1"""
    Q = np.asarray(query, np.float64).reshape(-1, 3)
    S = np.asarray(ref, np.float64).reshape(-1, 3)
    if len(S) == 0 or len(Q) == 0:
        return np.full(len(Q), np.inf), np.full(len(Q), -1, np.int64)
    d, i = _engine(S).kneighbors(Q, n_neighbors=1, return_distance=True)
    return d[:, 0], i[:, 0].astype(np.int64)


def nearest_brute(query, ref):
    Q = np.asarray(query, np.float64).reshape(-1, 3)
    S = np.asarray(ref, np.float64).reshape(-1, 3)
    dist = np.empty(len(Q))
    idx = np.empty(len(Q), np.int64)
    for k, q in enumerate(Q):
        d = S - q
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        idx[k] = int(np.argmin(d2))                              # (the first, i.e. the smallest index, on a tie)
        dist[k] = np.sqrt(d2[idx[k]])
    return dist, idx


def dtu_chamfer(data_pcd, perm, obs_mask, bb, res, plane, stl, thresh=0.2, patch=60, max_dist=20):
    """everything behind the sampling: permute, thin, mask, the two directions -> dictionary as mesh_eval.dtu_chamfer's"""
    data_pcd = np.asarray(data_pcd, np.float64)[perm]
    data_down = data_pcd[thin(data_pcd, thresh)]
    BB = np.asarray(bb).astype(np.float32)
    inbound = ((data_down >= BB[:1] - np.float32(patch)) & (data_down < BB[1:] + np.float32(patch * 2))).sum(axis=-1) == 3
    data_in = data_down[inbound]
    data_grid = np.around((data_in - BB[:1]) / res).astype(np.int32)
    grid_inbound = ((data_grid >= 0) & (data_grid < np.expand_dims(obs_mask.shape, 0))).sum(axis=-1) == 3
    g = data_grid[grid_inbound]
    in_obs = obs_mask[g[:, 0], g[:, 1], g[:, 2]].astype(np.bool_)
    data_in_obs = data_in[grid_inbound][in_obs]
    dist_d2s, idx_d2s = nearest(data_in_obs, stl)
    mean_d2s = dist_d2s[dist_d2s < max_dist].mean()
    P = np.asarray(plane, np.float64).reshape(4)
    above = ((stl[:, 0] * P[0] + stl[:, 1] * P[1]) + stl[:, 2] * P[2]) + P[3] > 0        # the plane test, ((x a + y b) + z c) + d
    dist_s2d, idx_s2d = nearest(stl[above], data_in)
    mean_s2d = dist_s2d[dist_s2d < max_dist].mean()
    return {"mean_d2s": float(mean_d2s), "mean_s2d": float(mean_s2d), "overall": float((mean_d2s + mean_s2d) / 2),
            "data_down": data_down, "dist_d2s": dist_d2s, "idx_d2s": idx_d2s, "d2s_index": np.where(inbound)[0][grid_inbound][in_obs],
            "dist_s2d": dist_s2d, "idx_s2d": idx_s2d, "s2d_index": np.where(above)[0]}


# ---- a test cloud for the sort of the 3 x 21-bit cell keys (shared by the thinning and the voxel tests) ----------------------------
def straddle_cloud(n=5000, edge=0.5, seed=17):
    """A cloud for the sort of the 3 x 21-bit cell keys (x << 42 | y << 21 | z) that thin and voxel_down_sample share: the key's low
    word holds z and y's bits 0..10, its high word x and y's bits 11..20.  n points in 240 cells of edge `edge`: x in 0..3, z in 0..5,
    y in 0..3, 2046..2049 and 4095..4096 -- y straddles 2048 (bit 32 of the key) and 4096, so that cells agree in one word and differ
    in the other, in both directions; ~20 points per cell, in random order (a stable sort keeps them in input order).  More than one
    256-lane workgroup and more than one radix tile."""
    rng = np.random.default_rng(seed)
    ys = np.array([0, 1, 2, 3, 2046, 2047, 2048, 2049, 4095, 4096])
    cells = np.stack([rng.integers(0, 4, n), ys[rng.integers(0, len(ys), n)], rng.integers(0, 6, n)], -1)
    cells[0], cells[1] = (0, 0, 0), (3, 4096, 5)                       # the corners: the extent does not depend on the draws
    P = (cells + rng.uniform(0.3, 0.7, (n, 3))) * edge
    P[0] = 0.0                                                         # the minimum, on the lattice
    return np.ascontiguousarray(P)


def key_words(cells):
    """(low, high) 32-bit words of the keys of integer cells (n, 3)"""
    c = np.asarray(cells).astype(np.uint64)
    key = (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]
    return (key & np.uint64(0xFFFFFFFF)).astype(np.int64), (key >> np.uint64(32)).astype(np.int64)


def check_straddle(P, cells):
    """the preconditions of the units and what the case is for (see straddle_cloud); cells: floor coordinates as the unit forms them"""
    assert np.isfinite(P).all() and len(P) > 4096
    assert cells.min() >= 0 and cells.max() <= 2 ** 21 - 1
    y = cells[:, 1]
    assert (y < 2048).any() and (y >= 2048).any() and len(np.unique(cells[:, 0])) > 1
    lo, hi = key_words(cells)
    pairs = np.unique(np.stack([lo, hi], -1), axis=0)
    assert len(pairs) < len(P) / 4                                     # duplicated cells
    by_lo, by_hi = {}, {}
    for a, b in pairs.tolist():
        by_lo.setdefault(a, set()).add(b)
        by_hi.setdefault(b, set()).add(a)
    assert max(len(v) for v in by_lo.values()) > 1 and max(len(v) for v in by_hi.values()) > 1      # equal low / different high, and the reverse
    order_lo = np.argsort(lo, kind="stable")
    assert not (np.diff(hi[order_lo]) >= 0).all()                      # the two words disagree about the order
