"""Deterministic inputs of the Delaunay predicate tests (tests/test_delaunay_predicates_host.py).

Every generator returns (points float32 [N,3], idx int32 [Q,6]): query q reads points a, b, c, d, e = idx[q, :5] and aux = idx[q, 5]
(gof_debug_delaunay_predicates).  Every query owns its points, so a query may be scaled or permuted on its own.  CASES maps a class
name to (generator, ops it applies to).  No generator drops a query: a construction that fails (not representable, a flat cell where
a positive one is needed) is drawn again at generation time, and the counts are fixed (COUNT).  Where a construction needs to know a
sign (a cell turned positive), it asks the integer reference (tests/delaunay_exact.py), never the code under test."""
import itertools

import numpy as np

import delaunay_exact as X

COUNT = {"A1": 1000, "A2": 1000, "A3": 1000, "B_coplanar": 1000, "B_collinear": 1000, "B_cospherical": 1000,
         "C_coplanar": 1200, "C_collinear": 800, "C_cospherical": 1200, "D_orient": 1500, "D_insphere": 1500,
         "E_sphere": 1500, "E_circle": 960}


def _pack(quints, aux=None):
    """[Q][5][3] float64 values that are float32 numbers -> (points, idx)"""
    Q = np.asarray(quints, np.float64)
    P = Q.reshape(-1, 3).astype(np.float32)
    assert np.isfinite(P).all() and (P.astype(np.float64) == Q.reshape(-1, 3)).all(), "a coordinate is not a float32 number"
    idx = np.zeros((len(Q), 6), np.int32)
    idx[:, :5] = np.arange(5 * len(Q)).reshape(-1, 5)
    if aux is not None:
        idx[:, 5] = aux
    return np.ascontiguousarray(P), idx


# ---- A: general position -------------------------------------------------------------------------------------------------------
def _random_floats(rng, shape, lo, hi):
    """float32 numbers with a random sign and mantissa and the exponent field uniform in [lo, hi]"""
    bits = (rng.integers(0, 2, shape, dtype=np.uint32) << 31) | (rng.integers(lo, hi + 1, shape).astype(np.uint32) << 23) | \
        rng.integers(0, 1 << 23, shape, dtype=np.uint32)
    return bits.view(np.float32)


def gen_A(regime):
    lo, hi, seed = {"A1": (1, 254, 101), "A2": (97, 156, 102), "A3": (0, 2, 103)}[regime]
    rng = np.random.default_rng(seed)
    return _pack(_random_floats(rng, (COUNT[regime], 5, 3), lo, hi).astype(np.float64))


# ---- B: exactly degenerate -------------------------------------------------------------------------------------------------------
def _signed_perms(v):
    return sorted({tuple(s * x for s, x in zip(sg, p)) for p in itertools.permutations(v) for sg in itertools.product((1, -1), repeat=3)})


SPHERES = [sorted(itertools.product((1, -1), repeat=3)), _signed_perms((1, 2, 3)), _signed_perms((2, 3, 6))]   # 8, 48, 48 integer points each on a sphere about 0


def _place(rng, pts):
    """integer points [5][3] -> translated by an integer offset (every sum below 2^24) and multiplied by 2^k, k in [-140, 100]: exact"""
    off = rng.integers(-(1 << int(rng.integers(0, 21))), (1 << int(rng.integers(0, 21))) + 1, 3)
    k = int(rng.integers(-140, 101))
    out = (np.asarray(pts, np.int64) + off).astype(np.float64)
    assert np.abs(out).max() < 2 ** 24
    return out * 2.0 ** k


def _coplanar(rng):
    while True:
        a, u, v = rng.integers(-8, 9, 3), rng.integers(-4, 5, 3), rng.integers(-4, 5, 3)
        if not np.cross(u, v).any():
            continue
        st = rng.integers(-3, 4, (4, 2))
        pts = [a + s * u + t * v for s, t in st]
        if len({tuple(p) for p in pts}) == 4:
            return pts + [rng.integers(-8, 9, 3)]            # (e: not read by the orientation ops)


def _collinear(rng):
    while True:
        a, u = rng.integers(-8, 9, 3), rng.integers(-6, 7, 3)
        s = rng.integers(-5, 6, 3)
        if u.any() and len(set(s.tolist())) == 3:
            return [a + t * u for t in s] + [rng.integers(-8, 9, 3), rng.integers(-8, 9, 3)]


def _cospherical(rng, flat_cell_ok=False):
    """5 distinct integer points on a sphere about an integer centre; the cell (a, b, c, d) positively oriented unless flat"""
    while True:
        S = SPHERES[int(rng.integers(0, 3))]
        pts = [list(S[i]) for i in rng.choice(len(S), 5, replace=False)]
        o = X.orient_rows(*pts[:4])
        if o == 0 and not flat_cell_ok:
            continue
        if o < 0:
            pts[0], pts[1] = pts[1], pts[0]
        c = rng.integers(-8, 9, 3)
        return [np.array(p) + c for p in pts]


def gen_B(kind):
    rng = np.random.default_rng({"B_coplanar": 201, "B_collinear": 202, "B_cospherical": 203}[kind])
    make = {"B_coplanar": _coplanar, "B_collinear": _collinear, "B_cospherical": _cospherical}[kind]
    return _pack([_place(rng, make(rng)) for _ in range(COUNT[kind])])


# ---- C: one ulp off B ------------------------------------------------------------------------------------------------------------
def _one_ulp(rng, quint, rows, axes=(0, 1, 2)):
    """moves one coordinate (of the given axes) of one of the given rows of a placed quintuple to its float32 neighbour, up or down"""
    while True:
        q = np.array(quint, np.float64)
        r, k = int(rng.choice(rows)), int(rng.choice(axes))
        moved = float(np.nextafter(np.float32(q[r, k]), np.float32(np.inf if rng.integers(0, 2) else -np.inf)))
        if np.isfinite(moved):
            q[r, k] = moved
            return q


def gen_C(kind):
    rng = np.random.default_rng({"C_coplanar": 301, "C_collinear": 302, "C_cospherical": 303}[kind])
    make, rows = {"C_coplanar": (_coplanar, 4), "C_collinear": (_collinear, 3), "C_cospherical": (_cospherical, 5)}[kind]
    return _pack([_one_ulp(rng, _place(rng, make(rng)), rows) for _ in range(COUNT[kind])])


# ---- D: coordinate differences that round in fp64 --------------------------------------------------------------------------------
def _far(rng):
    """a float32 number of magnitude 2^20 .. 2^60, random sign and mantissa"""
    return float(_random_floats(rng, (), 127 + 20, 127 + 59))


def _D_orient(rng):
    """four points of a plane that contains the x direction, of magnitude 2^-20, one or two of them moved far along x (they stay in
    the plane); one query in three stays exactly coplanar, the others get one coordinate of a near vertex moved by one ulp"""
    while True:
        a, v = rng.integers(-30, 31, 3), rng.integers(-6, 7, 3)
        v[0] = 0
        st = rng.integers(-4, 5, (4, 2))
        if not v.any() or len({tuple(r) for r in st.tolist()}) < 4:
            continue
        q = np.array([a + np.array([s, 0, 0]) + t * v for s, t in st], np.float64) * 2.0 ** -26
        far = rng.choice(4, int(rng.integers(1, 3)), replace=False)
        for r in far:
            q[r, 0] = _far(rng)
        q = np.vstack([q, np.zeros((1, 3))])                    # (e: not read by the orientation ops)
        if rng.integers(0, 3):
            q = _one_ulp(rng, q, [r for r in range(4) if r not in far], axes=(1, 2))      # (a move along x stays in the plane)
        return q


CIRCLES = [[p for p in S if p[0] == x0] for S in SPHERES[1:] for x0 in sorted({p[0] for p in S})]     # 8 cocircular points of a plane x = x0 each


def _D_insphere(rng):
    """Four cocircular points of a plane x = x0 at magnitude 2^-20 and a far vertex: any fifth point off the plane is on a sphere with
    them, so the far vertex (any float32 numbers, its x of magnitude 2^20 .. 2^60) lies exactly on the common sphere.  One query in
    four stays so; two get a coordinate of a near vertex moved by one ulp; one is general: two far vertices on the same axis (no
    float32 point far out on a sphere through three near ones)."""
    mode = int(rng.integers(0, 4))
    C = CIRCLES[int(rng.integers(0, len(CIRCLES)))]
    near = (np.array([C[i] for i in rng.choice(len(C), 4, replace=False)], np.float64) + rng.integers(-8, 9, 3)) * 2.0 ** -26
    far = np.array([_far(rng), rng.integers(-8, 9) * 2.0 ** -26, rng.integers(-8, 9) * 2.0 ** -26])
    slot = int(rng.integers(0, 5))                       # the far vertex takes every role, the query's included
    q = np.insert(near, slot, far, axis=0)
    if mode == 3:
        other = int(rng.choice([r for r in range(5) if r != slot]))
        q[other, 0] = _far(rng)
    elif mode:
        q = _one_ulp(rng, q, [r for r in range(5) if r != slot])
    return q


def gen_D(kind):
    rng = np.random.default_rng({"D_orient": 401, "D_insphere": 402}[kind])
    make = {"D_orient": _D_orient, "D_insphere": _D_insphere}[kind]
    return _pack([make(rng) for _ in range(COUNT[kind])])


# ---- E: ties of the symbolic perturbation ----------------------------------------------------------------------------------------
def _positive(cell):
    """the four integer points in an order of positive orientation (None if flat)"""
    o = X.orient_rows(*[list(map(int, p)) for p in cell])
    if o == 0:
        return None
    return list(cell) if o > 0 else [cell[1], cell[0], cell[2], cell[3]]


def gen_E_sphere():
    """Cospherical quintuples, every point in the query role (the cell = the other four, shuffled, then turned positive).  Two
    families in turn: five points of which no four are coplanar (every coefficient non-zero: the largest point decides), and four
    cocircular points of the plane x = min with a fifth point of larger x -- the lexicographically largest, whose coefficient is the
    orientation of the other four, 0 -- where the second coefficient decides (the fifth point cannot be the query: its cell is flat)."""
    rng = np.random.default_rng(501)
    out = []
    while len(out) < COUNT["E_sphere"]:
        S = SPHERES[int(rng.integers(0, 3))]
        if (len(out) // 5) % 2 == 0:
            pts = [np.array(S[i]) for i in rng.choice(len(S), 5, replace=False)]
            roles = range(5)
        else:
            x0 = S[0][0]                                 # (sorted: the smallest x)
            ring = [p for p in S if p[0] == x0]
            rest = [p for p in S if p[0] != x0]
            pts = [np.array(ring[i]) for i in rng.choice(len(ring), 4, replace=False)] + [np.array(rest[int(rng.integers(0, len(rest)))])]
            roles = [0, 1, 2, 3, int(rng.integers(0, 4))]
        cells = [_positive([pts[i] for i in rng.permutation([k for k in range(5) if k != j])]) for j in roles]
        if any(c is None for c in cells):
            continue
        c = rng.integers(-8, 9, 3)
        placed = _place(rng, [p + c for p in pts])
        lookup = {tuple(p): placed[i] for i, p in enumerate(pts)}
        out.extend(np.array([lookup[tuple(v)] for v in cell] + [lookup[tuple(pts[j])]]) for cell, j in zip(cells, roles))
    return _pack(out[:COUNT["E_sphere"]])


def gen_E_circle():
    """A triangle and a fourth point p on its circle (a plane x = x0), an integer point d off the plane, d in every slot dk of a
    positively oriented cell, p and the triangle's vertices in every order."""
    rng = np.random.default_rng(502)
    out, aux = [], []
    while len(out) < COUNT["E_circle"]:
        C = CIRCLES[int(rng.integers(0, len(CIRCLES)))]
        ring = [np.array(C[i]) for i in rng.choice(len(C), 4, replace=False)]
        d = rng.integers(-8, 9, 3)
        if d[0] == C[0][0]:
            continue
        placed = _place(rng, ring + [d])
        for dk in range(4):
            cell = [0, 1, 2]
            cell.insert(dk, 4)
            if X.orient_rows(*[list(map(int, (ring + [d])[i])) for i in cell]) < 0:
                i, j = [k for k in range(4) if k != dk][:2]
                cell[i], cell[j] = cell[j], cell[i]
            out.append(placed[cell + [3]])
            aux.append(dk)
    return _pack(out[:COUNT["E_circle"]], aux[:COUNT["E_circle"]])


CASES = {
    "A1": (lambda: gen_A("A1"), (0, 1, 2, 3, 4)), "A2": (lambda: gen_A("A2"), (0, 1, 2, 3, 4)), "A3": (lambda: gen_A("A3"), (0, 1, 2, 3, 4)),
    "B_coplanar": (lambda: gen_B("B_coplanar"), (0, 2)), "B_collinear": (lambda: gen_B("B_collinear"), (4,)),
    "B_cospherical": (lambda: gen_B("B_cospherical"), (1, 3)),
    "C_coplanar": (lambda: gen_C("C_coplanar"), (0, 2)), "C_collinear": (lambda: gen_C("C_collinear"), (4,)),
    "C_cospherical": (lambda: gen_C("C_cospherical"), (1, 3)),
    "D_orient": (lambda: gen_D("D_orient"), (0, 2)), "D_insphere": (lambda: gen_D("D_insphere"), (1, 3)),
    "E_sphere": (gen_E_sphere, (5,)), "E_circle": (gen_E_circle, (6,)),
}


def scale_exponents(P, idx):
    """per query a power of two k != 0 (0 where none fits) by which all its points can be multiplied exactly -> int [Q]"""
    P64 = P.astype(np.float64)
    ks = np.zeros(len(idx), np.int64)
    for q, row in enumerate(idx):
        pts = P64[row[:5]]
        for k in (40, -40, 10, -10, 1, -1):
            s = pts * 2.0 ** k
            with np.errstate(over="ignore"):
                f = s.astype(np.float32)
            if np.isfinite(f).all() and (f.astype(np.float64) == s).all():
                ks[q] = k
                break
    return ks


def scaled(P, idx, ks):
    out = P.astype(np.float64)
    for q, row in enumerate(idx):
        out[row[:5]] *= 2.0 ** int(ks[q])
    f = out.astype(np.float32)
    assert (f.astype(np.float64) == out).all()
    return f
