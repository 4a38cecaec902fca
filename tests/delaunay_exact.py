"""Exact reference of the Delaunay predicates (test infrastructure) in Python integers.

A float32 value times 2^149 is an integer, so every determinant below is exact.  Nothing here is shared with
csrc/delaunay_predicates.h or csrc/delaunay.hip: the determinants are generic Laplace expansions, and the symbolic perturbation is
formulated on the 5x5 lifted determinant with an epsilon per perturbed point, not by the code's vertex replacement.

  orient(P, a, b, c, d)        sign det[b - a, c - a, d - a]
  insphere(P, a, b, c, d, e)   > 0: e strictly inside the sphere of the positively oriented (a, b, c, d)
  collinear(P, a, b, c)        1: (b - a) x (c - a) is the zero vector, 0: not
  perturbed(P, ids, mask)      the sign of det[x, y, z, x^2 + y^2 + z^2 + eps_i, 1] over the rows ids = (a, b, c, d, p), eps_i > 0 present
                               where mask[i], ordered like the points' lexicographic order (the largest point the largest eps, each eps
                               infinitely larger than the next): the first non-zero term among the constant term and the eps
                               coefficients in descending order.  -> (sign, term, row): term 0 = the constant, k = the k-th
                               coefficient; row = the row that decided (4 = the query point p), -1 for the constant, None if
                               every term is zero.
The overall sign of the two lifted determinants is fixed once, on the centroid of a positively oriented regular tetrahedron (in
conflict: +1)."""
import numpy as np

_SCALE = 2 ** 149


def ints(P, rows):
    """the coordinates of the given rows of P (float32 [N,3]) as integers (times 2^149)"""
    return [[int(float(v) * _SCALE) for v in P[int(r)]] for r in rows]


def det(M):
    """determinant of a square matrix of Python integers (Laplace expansion along the first row)"""
    n = len(M)
    if n == 1:
        return M[0][0]
    if n == 2:
        return M[0][0] * M[1][1] - M[0][1] * M[1][0]
    total = 0
    for j in range(n):
        if M[0][j]:
            total += (-1 if j & 1 else 1) * M[0][j] * det([row[:j] + row[j + 1:] for row in M[1:]])
    return total


def sign(x):
    return (x > 0) - (x < 0)


def _sub(p, q):
    return [x - y for x, y in zip(p, q)]


def orient_rows(a, b, c, d):
    return sign(det([_sub(b, a), _sub(c, a), _sub(d, a)]))


def _lifted4(a, b, c, d, e):
    rows = [_sub(p, e) for p in (a, b, c, d)]
    return det([r + [sum(x * x for x in r)] for r in rows])


def _lifted5(rows):
    return [[r[0], r[1], r[2], r[0] * r[0] + r[1] * r[1] + r[2] * r[2], 1] for r in rows]


def _calibrate():
    tet = [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]
    if orient_rows(*tet) < 0:
        tet[0], tet[1] = tet[1], tet[0]
    assert orient_rows(*tet) > 0
    centre = [0, 0, 0]
    s4 = sign(_lifted4(*tet, centre))
    s5 = sign(det(_lifted5(tet + [centre])))
    assert s4 != 0 and s5 != 0
    return s4, s5


_S4, _S5 = _calibrate()


def insphere_rows(a, b, c, d, e):
    return _S4 * sign(_lifted4(a, b, c, d, e))


def collinear_rows(a, b, c):
    u, v = _sub(b, a), _sub(c, a)
    cross = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    return int(not any(cross))


def perturbed_rows(rows, mask):
    M = _lifted5(rows)
    s = _S5 * sign(det(M))
    if s:
        return s, 0, -1
    order = sorted((i for i in range(5) if mask[i]), key=lambda i: rows[i], reverse=True)      # (lists compare lexicographically)
    for term, i in enumerate(order, 1):
        minor = [r[:3] + r[4:] for k, r in enumerate(M) if k != i]
        s = _S5 * (-1 if (i + 3) & 1 else 1) * sign(det(minor))                                 # the cofactor of entry (i, 3)
        if s:
            return s, term, i
    return 0, None, None


# ---- over index arrays ---------------------------------------------------------------------------------------------------------
def orient(P, idx):
    return np.array([orient_rows(*ints(P, q[:4])) for q in idx], np.int32)


def insphere(P, idx):
    return np.array([insphere_rows(*ints(P, q[:5])) for q in idx], np.int32)


def collinear(P, idx):
    return np.array([collinear_rows(*ints(P, q[:3])) for q in idx], np.int32)


def insphere_perturbed(P, idx):
    """op 5: all five points perturbed -> (sign [Q], term [Q], row [Q])"""
    out = [perturbed_rows(ints(P, q[:5]), (1, 1, 1, 1, 1)) for q in idx]
    return tuple(np.array([(-9 if v is None else v) for v in col], np.int32) for col in zip(*out))


def incircle_perturbed(P, idx):
    """op 6: the three face vertices (every slot of the cell but aux) and p perturbed"""
    out = [perturbed_rows(ints(P, q[:5]), tuple(int(k != q[5]) for k in range(4)) + (1,)) for q in idx]
    return tuple(np.array([(-9 if v is None else v) for v in col], np.int32) for col in zip(*out))
