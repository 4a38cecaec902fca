"""The Tanks-and-Temples F-score evaluation restated in numpy / SciPy from the contract of DESIGN.md §3.9, as plain functions over
numpy arrays: the crossing-number crop, the voxel means in ascending key order, the balanced-tree correspondence sums, ICP with
Umeyama's closed form, the RANSAC over drawn hypotheses and the F-score histograms.  The nearest neighbour comes from SciPy's
cKDTree; the distance is then evaluated again in the contract's order.  Test infrastructure only; nothing here imports the product
and nothing here is used by it."""
import numpy as np

WORKERS = 16


# ---- transformation, crop ---------------------------------------------------------------------------------------------------------
def transform(P, M):
    P = np.asarray(P, np.float64).reshape(-1, 3)
    if M is None:
        return P.copy()
    M = np.asarray(M, np.float64)
    return np.stack([((M[r, 0] * P[:, 0] + M[r, 1] * P[:, 1]) + M[r, 2] * P[:, 2]) + M[r, 3] for r in range(3)], axis=-1)


def crop(P, volume, M=None):
    """-> (kept transformed points in input order, their rows)"""
    Q = transform(P, M)
    w = volume["axis"]
    ua, va = (w + 1) % 3, (w + 2) % 3
    poly = np.asarray(volume["polygon"], np.float64).reshape(-1, 3)
    inside = (volume["axis_min"] <= Q[:, w]) & (Q[:, w] <= volume["axis_max"])
    pu, pv = Q[:, ua], Q[:, va]
    crossings = np.zeros(len(Q), np.int64)
    K = len(poly)
    with np.errstate(all="ignore"):
        for i in range(K):
            j = (i - 1) % K
            iu, iv, ju, jv = poly[i, ua], poly[i, va], poly[j, ua], poly[j, va]
            cond = ((iv < pv) & (jv >= pv)) | ((jv < pv) & (iv >= pv))
            x = iu + (pv - iv) / (jv - iv) * (ju - iu)
            crossings += cond & (x < pu)
    keep = inside & (crossings % 2 == 1)
    idx = np.nonzero(keep)[0]
    return Q[idx], idx


# ---- voxel down-sampling ------------------------------------------------------------------------------------------------------------
def voxel_down_sample(P, v):
    """-> (one mean per occupied voxel in ascending key order, counts)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    if len(P) == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64)
    o = P.min(axis=0) - 0.5 * v
    c = np.floor((P - o) / v)
    assert (c >= 0).all() and (c <= 2 ** 21 - 1).all()
    c = c.astype(np.uint64)
    key = (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    head = np.ones(len(P), bool)
    head[1:] = sk[1:] != sk[:-1]
    start = np.nonzero(head)[0]
    counts = np.diff(np.append(start, len(P)))
    S = P[order]
    acc = S[start].copy()
    for r in range(1, int(counts.max())):                   # left to right: the r-th point of every voxel that has one
        live = counts > r
        acc[live] = acc[live] + S[start[live] + r]
    return acc / counts[:, None].astype(np.float64), counts.astype(np.int64)


# ---- nearest neighbour --------------------------------------------------------------------------------------------------------------
def nearest(Q, S):
    """-> (dist, index): cKDTree's neighbour, the distance evaluated as sqrt((dx dx + dy dy) + dz dz)"""
    from scipy.spatial import cKDTree
    Q = np.asarray(Q, np.float64).reshape(-1, 3)
    S = np.asarray(S, np.float64).reshape(-1, 3)
    if len(S) == 0 or len(Q) == 0:
        return np.full(len(Q), np.inf), np.full(len(Q), -1, np.int64)
    _, i = cKDTree(S).query(Q, k=1, workers=WORKERS)
    e = S[i] - Q
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]), i.astype(np.int64)


# ---- the sums -------------------------------------------------------------------------------------------------------------------------
def tree_sum(v):
    """the balanced binary tree over the rows of v (N, C) in index order, padded with +0.0 to the next power of two"""
    v = np.asarray(v, np.float64)
    v = v.reshape(len(v), -1)
    n = 1
    while n < len(v):
        n *= 2
    w = np.zeros((n, v.shape[1]))
    w[:len(v)] = v
    while len(w) > 1:
        w = w[0::2] + w[1::2]
    return w[0]


def icp_sums1(S1, Tg, dist, idx, threshold):
    """-> (n, [sum s' (3), sum t (3), sum dist^2])"""
    m = (dist < threshold) & (idx >= 0)
    v = np.zeros((len(S1), 7))
    v[m, 0:3] = S1[m]
    v[m, 3:6] = Tg[idx[m]]
    v[m, 6] = dist[m] * dist[m]
    return int(m.sum()), tree_sum(v) if len(S1) else np.zeros(7)


def icp_sums2(S1, Tg, dist, idx, threshold, mu_s, mu_t):
    """-> [sum (t - mu_t)(s' - mu_s)^T row-major (9), sum |s' - mu_s|^2]"""
    m = (dist < threshold) & (idx >= 0)
    d = S1[m] - np.asarray(mu_s)
    e = Tg[idx[m]] - np.asarray(mu_t)
    v = np.zeros((len(S1), 10))
    for r in range(3):
        for c in range(3):
            v[m, 3 * r + c] = e[:, r] * d[:, c]
    v[m, 9] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return tree_sum(v) if len(S1) else np.zeros(10)


def umeyama_update(n, s1, s2):
    """DESIGN.md §3.9, step by step"""
    n = float(n)
    mu_s = np.array([s1[0] / n, s1[1] / n, s1[2] / n])
    mu_t = np.array([s1[3] / n, s1[4] / n, s1[5] / n])
    sigma = np.array(s2[:9], dtype=np.float64).reshape(3, 3) / n
    var_s = s2[9] / n
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


def icp_evaluate(source, target, T, threshold):
    """one evaluation at the accumulated transformation T -> dictionary as the product's record entries (sums2 filled when n >= 3)"""
    S1 = transform(source, T)
    dist, idx = nearest(S1, target)
    n, s1 = icp_sums1(S1, target, dist, idx, threshold)
    ev = {"transformation": np.array(T, dtype=np.float64), "n": n, "sums1": [float(x) for x in s1], "sums2": None,
          "fitness": (n / len(S1) if len(S1) else 0.0), "rmse": (float(np.sqrt(s1[6] / n)) if n else 0.0), "dist": dist}
    if n >= 3:
        mu = [s1[k] / float(n) for k in range(6)]
        ev["sums2"] = [float(x) for x in icp_sums2(S1, target, dist, idx, threshold, mu[:3], mu[3:])]
    return ev


def icp(source, target, threshold, max_iteration=20, relative_fitness=1e-6, relative_rmse=1e-6):
    """-> (T, fitness, rmse, record)"""
    T = np.eye(4)
    record = [icp_evaluate(source, target, T, threshold)]
    for _ in range(max_iteration):
        ev = record[-1]
        if ev["n"] < 3:
            break
        T = umeyama_update(ev["n"], ev["sums1"], ev["sums2"]) @ T
        record.append(icp_evaluate(source, target, T, threshold))
        if abs(ev["fitness"] - record[-1]["fitness"]) < relative_fitness and abs(ev["rmse"] - record[-1]["rmse"]) < relative_rmse:
            break
    return T, record[-1]["fitness"], record[-1]["rmse"], record


def registration_vol_ds(source, target, init, volume, voxel, threshold, max_iteration=20):
    s = voxel_down_sample(crop(source, volume, init)[0], voxel)[0]
    t = voxel_down_sample(crop(target, volume)[0], voxel)[0]
    T, fit, rmse, rec = icp(s, t, threshold, max_iteration)
    return T @ np.asarray(init, np.float64), fit, rmse, rec


def registration_unif(source, target, init, volume, threshold, max_iteration=20, max_points=4e6):
    def thin(p):
        return p[::int(round(len(p) / float(max_points)))] if len(p) > max_points else p
    T, fit, rmse, rec = icp(thin(crop(source, volume, init)[0]), thin(crop(target, volume)[0]), threshold, max_iteration)
    return T @ np.asarray(init, np.float64), fit, rmse, rec


# ---- RANSAC over the camera centres -----------------------------------------------------------------------------------------------------
def similarity(src, dst):
    """Umeyama with scale over n points, sums in their order -> (c, R, t)"""
    n = len(src)
    mu_s, mu_d = src[0].copy(), dst[0].copy()
    for k in range(1, n):
        mu_s = mu_s + src[k]
        mu_d = mu_d + dst[k]
    mu_s, mu_d = mu_s / float(n), mu_d / float(n)
    a, b = src - mu_s, dst - mu_d
    cov = np.outer(b[0], a[0])
    var = (a[0, 0] * a[0, 0] + a[0, 1] * a[0, 1]) + a[0, 2] * a[0, 2]
    for k in range(1, n):
        cov = cov + np.outer(b[k], a[k])
        var = var + ((a[k, 0] * a[k, 0] + a[k, 1] * a[k, 1]) + a[k, 2] * a[k, 2])
    cov, var = cov / float(n), var / float(n)
    with np.errstate(all="ignore"):
        U, D, Vt = np.linalg.svd(cov)
        S = np.ones(3)
        if np.linalg.det(U) * np.linalg.det(Vt) < 0:
            S[2] = -1.0
        R = (U * S[None, :]) @ Vt
        c = ((D[0] * S[0] + D[1] * S[1]) + D[2] * S[2]) / var
        Rm = (R[:, 0] * mu_s[0] + R[:, 1] * mu_s[1]) + R[:, 2] * mu_s[2]
        t = mu_d - c * Rm
    return c, R, t


def align_trajectories(est, gt, gt_trans, seed, iterations, threshold=0.2, n=6):
    """the exhaustive pass over the drawn hypotheses, one at a time -> (4x4, winning hypothesis, its inlier mask)"""
    est = np.asarray(est, np.float64).reshape(-1, 3)
    gt = transform(gt, gt_trans)
    N = len(est)
    draws = np.random.default_rng(seed).integers(0, N, (iterations, n))
    best = None
    for h in range(iterations):
        try:
            c, R, t = similarity(est[draws[h]], gt[draws[h]])
        except np.linalg.LinAlgError:
            continue
        if not (np.isfinite(c) and np.isfinite(R).all() and np.isfinite(t).all()):
            continue
        A = c * R
        moved = np.stack([((A[r, 0] * est[:, 0] + A[r, 1] * est[:, 1]) + A[r, 2] * est[:, 2]) + t[r] for r in range(3)], axis=-1)
        e = moved - gt
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        inl = np.sqrt(d2) < threshold
        acc = 0.0
        for x in np.where(inl, d2, 0.0):
            acc = acc + x
        key = (-int(inl.sum()), float(np.sqrt(acc / max(int(inl.sum()), 1))), h)
        if best is None or key < best[0]:
            best = (key, A, t, inl)
    out = np.eye(4)
    if best is None:
        return out, -1, np.zeros(N, bool)
    out[:3, :3] = best[1]
    out[:3, 3] = best[2]
    return out, best[0][2], best[3]


# ---- F-score ----------------------------------------------------------------------------------------------------------------------------
def tnt_fscore(source, target, T, volume, tau, plot_stretch=5):
    s = voxel_down_sample(crop(source, volume, T)[0], tau / 2.0)[0]
    t = voxel_down_sample(crop(target, volume)[0], tau / 2.0)[0]
    d1, _ = nearest(s, t)
    d2, _ = nearest(t, s)
    edges = np.arange(0, tau * plot_stretch, tau / 100)
    n1, n2 = int((d1 < tau).sum()), int((d2 < tau).sum())
    h1, h2 = np.histogram(d1, edges)[0], np.histogram(d2, edges)[0]
    recall, precision = float(n2) / float(len(d2)), float(n1) / float(len(d1))
    return {"source": s, "target": t, "dist_source": d1, "dist_target": d2, "below_source": n1, "below_target": n2, "hist_source": h1,
            "hist_target": h2, "precision": precision, "recall": recall, "fscore": 2 * recall * precision / (recall + precision),
            "cum_source": np.cumsum(h1).astype(float) / len(d1), "cum_target": np.cumsum(h2).astype(float) / len(d2), "edges": edges}
