"""Independent checker of a Delaunay tetrahedralization (test infrastructure).

It shares no code with csrc/delaunay.hip: orientation and in-sphere are evaluated in numpy fp64 with a generous error bound, and
what the bound cannot decide is evaluated exactly in Python integers (a float32 value times 2^149 is an integer).  No symbolic
perturbation: the checker asks for what holds whatever tie-breaking was used -- positive cells, faces paired with opposite
orientation, a convex boundary that every point lies inside, locally Delaunay interior faces (the opposite vertex not STRICTLY
inside), every distinct point used (the lowest index of duplicates), Euler characteristic 1."""
import numpy as np

_REL = 1e-10          # fp64 filter: |det| > _REL * permanent decides (far wider than the rounding can reach)
_SCALE = 2 ** 149


def _exact_rows(P, rows):
    return [[int(float(v) * _SCALE) for v in P[r]] for r in rows]


def _det3_int(u, v, w):
    return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0])


def _sign(x):
    return (x > 0) - (x < 0)


def orient(P, a, b, c, d):
    """sign det[b-a, c-a, d-a] for index arrays a..d into P (float32 [N,3])"""
    P64 = P.astype(np.float64)
    A = P64[a]
    u, v, w = P64[b] - A, P64[c] - A, P64[d] - A
    c1, c2, c3 = v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1], v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2], v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0]
    det = u[:, 0] * c1 + u[:, 1] * c2 + u[:, 2] * c3
    au, av, aw = np.abs(u), np.abs(v), np.abs(w)
    perm = au[:, 0] * (av[:, 1] * aw[:, 2] + av[:, 2] * aw[:, 1]) + au[:, 1] * (av[:, 2] * aw[:, 0] + av[:, 0] * aw[:, 2]) + \
        au[:, 2] * (av[:, 0] * aw[:, 1] + av[:, 1] * aw[:, 0])
    s = np.sign(det).astype(np.int64)
    und = ~(np.abs(det) > _REL * perm) | (perm < 1e-200)
    for i in np.nonzero(und)[0]:
        pa, pb, pc, pd = _exact_rows(P, [a[i], b[i], c[i], d[i]])
        s[i] = _sign(_det3_int([x - y for x, y in zip(pb, pa)], [x - y for x, y in zip(pc, pa)], [x - y for x, y in zip(pd, pa)]))
    return s, int(und.sum())


def insphere(P, a, b, c, d, e):
    """> 0: e strictly inside the circumsphere of the positively oriented (a, b, c, d)"""
    P64 = P.astype(np.float64)
    E = P64[e]
    R = [P64[x] - E for x in (a, b, c, d)]
    L = [(r * r).sum(1) for r in R]

    def d3(u, v, w):
        det = u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) - u[:, 1] * (v[:, 0] * w[:, 2] - v[:, 2] * w[:, 0]) + \
            u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])
        u, v, w = np.abs(u), np.abs(v), np.abs(w)
        perm = u[:, 0] * (v[:, 1] * w[:, 2] + v[:, 2] * w[:, 1]) + u[:, 1] * (v[:, 0] * w[:, 2] + v[:, 2] * w[:, 0]) + \
            u[:, 2] * (v[:, 0] * w[:, 1] + v[:, 1] * w[:, 0])
        return det, perm
    minors = [d3(R[1], R[2], R[3]), d3(R[0], R[2], R[3]), d3(R[0], R[1], R[3]), d3(R[0], R[1], R[2])]
    det = L[0] * minors[0][0] - L[1] * minors[1][0] + L[2] * minors[2][0] - L[3] * minors[3][0]
    perm = sum(L[i] * minors[i][1] for i in range(4))
    s = np.sign(det).astype(np.int64)
    und = ~(np.abs(det) > _REL * perm) | (perm < 1e-200)
    for i in np.nonzero(und)[0]:
        pe = _exact_rows(P, [e[i]])[0]
        rows = [[x - y for x, y in zip(r, pe)] for r in _exact_rows(P, [a[i], b[i], c[i], d[i]])]
        lift = [sum(x * x for x in r) for r in rows]
        D = lift[0] * _det3_int(rows[1], rows[2], rows[3]) - lift[1] * _det3_int(rows[0], rows[2], rows[3]) + \
            lift[2] * _det3_int(rows[0], rows[1], rows[3]) - lift[3] * _det3_int(rows[0], rows[1], rows[2])
        s[i] = _sign(D)
    return s, int(und.sum())


def representatives(P):
    """index of the lowest-index copy of every distinct point (exact float32 equality; -0 == +0)"""
    Q = np.ascontiguousarray(P.astype(np.float32) + np.float32(0.0))      # (-0 + 0 = +0)
    _, first = np.unique(Q.view(np.dtype((np.void, 12))).ravel(), return_index=True)
    return np.sort(first)


# outward-oriented faces of a positive cell (v0..v3): face i is opposite v_i
_FACES = np.array([[1, 2, 3], [0, 3, 2], [0, 1, 3], [0, 2, 1]])


def check(P, T, hull_sample=None):
    """Asserts the contract on points P [N,3] float32 and cells T [M,4]; returns a dict of counts"""
    P = np.asarray(P, np.float32)
    T = np.asarray(T).astype(np.int64)
    assert T.ndim == 2 and T.shape[1] == 4
    M = len(T)
    rep = representatives(P)
    used = np.unique(T)
    assert np.array_equal(used, rep), "used vertices != the lowest-index copies of the distinct points (%d used, %d distinct)" % (len(used), len(rep))
    o, ex_o = orient(P, T[:, 0], T[:, 1], T[:, 2], T[:, 3])
    assert (o > 0).all(), "%d cells are not positively oriented" % int((o <= 0).sum())
    # faces: outward triples, rotated so the smallest comes first; the sorted triple is the key, the rotation's parity the side
    F = T[:, _FACES].reshape(-1, 3)
    cell = np.repeat(np.arange(M), 4)
    opp = T.reshape(-1)
    key = np.sort(F, axis=1)
    r = np.argmin(F, axis=1)
    Fr = np.stack([F[np.arange(len(F)), (r + k) % 3] for k in range(3)], 1)
    parity = (Fr[:, 1] > Fr[:, 2]).astype(np.int64)       # 0: (min, mid, max), 1: (min, max, mid)
    kk = (key[:, 0] * (len(P) + 1) + key[:, 1]) * (len(P) + 1) + key[:, 2] if len(P) < 2 ** 20 else None
    if kk is None:
        order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))
        ks = key[order]
        same = np.r_[False, (ks[1:] == ks[:-1]).all(1)]
    else:
        order = np.argsort(kk, kind="stable")
        ks = kk[order]
        same = np.r_[False, ks[1:] == ks[:-1]]
    assert not (same[1:] & same[:-1]).any(), "a face is shared by more than two cells"
    second = np.nonzero(same)[0]
    first = second - 1
    fa, fb = order[first], order[second]
    assert (parity[fa] != parity[fb]).all(), "a shared face has the same orientation in both cells"
    interior = np.zeros(len(F), bool)
    interior[fa] = interior[fb] = True
    bnd = np.nonzero(~interior)[0]
    # convex boundary: every point on the inner side or on the plane of every boundary face (inner side: orient < 0)
    B = F[bnd]
    pts = rep if hull_sample is None or len(rep) <= hull_sample else rep[np.random.default_rng(0).choice(len(rep), hull_sample, replace=False)]
    ex_h = 0
    for start in range(0, len(B), max(1, 2_000_000 // max(1, len(pts)))):
        Bc = B[start:start + max(1, 2_000_000 // max(1, len(pts)))]
        a = np.repeat(Bc[:, 0], len(pts)); b = np.repeat(Bc[:, 1], len(pts)); c = np.repeat(Bc[:, 2], len(pts))
        q = np.tile(pts, len(Bc))
        s, ex = orient(P, a, b, c, q)
        ex_h += ex
        assert (s <= 0).all(), "a point lies outside a boundary face"
    # locally Delaunay: the opposite vertex of the neighbour is not strictly inside
    s1, ex1 = insphere(P, T[cell[fa], 0], T[cell[fa], 1], T[cell[fa], 2], T[cell[fa], 3], opp[fb])
    s2, ex2 = insphere(P, T[cell[fb], 0], T[cell[fb], 1], T[cell[fb], 2], T[cell[fb], 3], opp[fa])
    assert (s1 <= 0).all() and (s2 <= 0).all(), "%d interior faces are not locally Delaunay" % int((s1 > 0).sum() + (s2 > 0).sum())
    nF = len(second) + len(bnd)
    E = np.sort(T[:, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]].reshape(-1, 2), axis=1)
    nE = len(np.unique(E[:, 0] * (len(P) + 1) + E[:, 1]))
    V = len(used)
    assert V - nE + nF - M == 1, "Euler characteristic %d" % (V - nE + nF - M)
    return dict(cells=M, vertices=V, boundary_faces=len(bnd), exact=ex_o + ex_h + ex1 + ex2)


def as_sets(T):
    """the cells as a set of frozensets (for comparisons with SciPy, which orients and orders its simplices its own way)"""
    return set(map(frozenset, np.asarray(T).tolist()))
