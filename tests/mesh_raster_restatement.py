"""DESIGN.md §3.19 restated on the host, one face and one pixel at a time: Python floats (IEEE fp64, one rounding per operation, nothing
fused) and Python integers (no width at all) in the order the section writes down.  Written from the section, not from the kernel: no
fast path, no list, no tiles, no threshold -- a conservative box of pixels per fan triangle and the definition at each of them.

Beside it a brute-force fp64 ray cast through the pixel centres ties the definition to geometry (ray_cast, geometric_tolerance)."""
import math

import numpy as np

GUARD = 4096
EMPTY = 0xFFFFFFFF


def records(c2w_list, H, W, fx, fy, cx, cy, znear=0.01, zfar=20.0, convention="opengl"):
    """the view records as plain dictionaries: w2c = rows 0..2 of the fp64 inverse of the OpenCV camera-to-world"""
    out = []
    for c2w in c2w_list:
        m = np.eye(4)
        a = np.asarray(c2w, np.float64)
        m[:a.shape[0]] = a
        if convention == "opengl":
            m[:3, 1:3] *= -1.0
        out.append(dict(w2c=[float(x) for x in np.linalg.inv(m)[:3].reshape(12)], fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy),
                        znear=float(znear), zfar=float(zfar), W=int(W), H=int(H)))
    return out


def _div(a, b):
    """IEEE division of two floats (Python raises where IEEE answers)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def camera(rec, v):
    m = rec["w2c"]
    vx, vy, vz = float(v[0]), float(v[1]), float(v[2])
    with np.errstate(all="ignore"):
        vx, vy, vz = np.float64(vx), np.float64(vy), np.float64(vz)
        return tuple(float(((np.float64(m[4 * r]) * vx + np.float64(m[4 * r + 1]) * vy) + np.float64(m[4 * r + 2]) * vz) + np.float64(m[4 * r + 3])) for r in range(3))


def _clip(poly, inside, cross):
    out = []
    n = len(poly)
    for k in range(n):
        cur, nxt = poly[k], poly[(k + 1) % n]
        ci, ni = inside(cur), inside(nxt)
        if ci:
            out.append(cur)
        if ci != ni:
            out.append(cross(cur, nxt) if ci else cross(nxt, cur))          # always from the inside endpoint towards the outside one
    return out


def _side(axis, bound, upper):
    def inside(p):
        return p[axis] <= bound if upper else p[axis] >= bound

    def cross(a, b):
        t = (bound - a[axis]) / (b[axis] - a[axis])
        p = [a[c] + t * (b[c] - a[c]) for c in range(3)]
        p[axis] = bound
        return tuple(p)
    return inside, cross


def fan_triangles(rec, tri):
    """the fan triangles of one face in one view: [((sx, sy, w) x 3)], in the image plane, before the snap"""
    cam = [camera(rec, v) for v in tri]
    if not all(math.isfinite(float(x)) for v in tri for x in v) or not all(math.isfinite(x) for c in cam for x in c):
        return []
    zn = rec["znear"]

    def cross_near(a, b):
        t = (zn - a[2]) / (b[2] - a[2])
        return (a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), zn)
    poly = _clip(cam, lambda p: p[2] >= zn, cross_near)
    if not poly:
        return []
    with np.errstate(all="ignore"):
        img = [(float(np.float64(rec["fx"]) * np.float64(_div(x, z)) + np.float64(rec["cx"])), float(np.float64(rec["fy"]) * np.float64(_div(y, z)) + np.float64(rec["cy"])), _div(1.0, z))
               for x, y, z in poly]
    if not all(math.isfinite(p[0]) and math.isfinite(p[1]) for p in img):
        return []
    for axis, bound, upper in ((0, -float(GUARD), False), (0, float(rec["W"] + GUARD), True), (1, -float(GUARD), False), (1, float(rec["H"] + GUARD), True)):
        img = _clip(img, *_side(axis, bound, upper))
        if not img:
            return []
    return [(img[0], img[k], img[k + 1]) for k in range(1, len(img) - 1)]


def _top_left(dx, dy):
    return dy < 0 or (dy == 0 and dx > 0)


def pixel_depth(A, B, C, i, j, zfar):
    """A, B, C: (X, Y, w) snapped and oriented (area > 0) -> the float32 depth of pixel (i, j) or None"""
    px, py = 256 * i + 128, 256 * j + 128
    area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
    e = []
    for S, E in ((B, C), (C, A), (A, B)):
        dx, dy = E[0] - S[0], E[1] - S[1]
        v = dx * (py - S[1]) - dy * (px - S[0])
        if v < 0 or (v == 0 and not _top_left(dx, dy)):
            return None
        e.append(v)
    num = (float(e[0]) * A[2] + float(e[1]) * B[2]) + float(e[2]) * C[2]
    z = _div(float(area), num)
    if not (z > 0.0 and z <= zfar):
        return None
    with np.errstate(all="ignore"):
        return np.float32(z)


def snapped(tri):
    """-> (A, B, C) with integer X, Y (1/256 pixel) and positive area, or None for a zero-area triangle"""
    A, B, C = [(round(p[0] * 256.0), round(p[1] * 256.0), p[2]) for p in tri]          # round(): to nearest, ties to even, like rint
    area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0])
    if area == 0:
        return None
    return (A, C, B) if area < 0 else (A, B, C)


def render_view(V, F, rec, cover=None):
    """-> depth (H,W) float32.  cover (H,W) int: incremented per (fan triangle, covered pixel) before the depth range is looked at"""
    W, H = rec["W"], rec["H"]
    bits = np.full((H, W), EMPTY, np.uint32)
    for f in np.asarray(F).reshape(-1, 3):
        for tri in fan_triangles(rec, [V[int(k)] for k in f]):
            t = snapped(tri)
            if t is None:
                continue
            xs, ys = [p[0] for p in t], [p[1] for p in t]
            i0, i1 = max(0, min(xs) // 256 - 1), min(W - 1, max(xs) // 256 + 1)
            j0, j1 = max(0, min(ys) // 256 - 1), min(H - 1, max(ys) // 256 + 1)
            for j in range(j0, j1 + 1):
                for i in range(i0, i1 + 1):
                    if cover is not None and pixel_depth(t[0], t[1], t[2], i, j, math.inf) is not None:
                        cover[j, i] += 1
                    d = pixel_depth(t[0], t[1], t[2], i, j, rec["zfar"])
                    if d is not None:
                        bits[j, i] = min(int(bits[j, i]), int(np.float32(d).view(np.uint32)))
    bits[bits == EMPTY] = 0
    return bits.view(np.float32)


def render_depth(V, F, recs, stride_shape=None):
    if not recs:
        return np.zeros((0,) + (stride_shape or (0, 0)), np.float32)
    return np.stack([render_view(V, F, r) for r in recs])


def view_sees(rec, depth, v, eps):
    """-> (in_frustum and front, margins) of one vertex in one view; margins: (|z - (ds + eps)| or inf, distance of u, v from the bounds, |z|)"""
    x, y, Z = camera(rec, v)
    with np.errstate(all="ignore"):
        X = float(np.float64(rec["fx"]) * np.float64(x) + np.float64(rec["cx"]) * np.float64(Z))
        Y = float(np.float64(rec["fy"]) * np.float64(y) + np.float64(rec["cy"]) * np.float64(Z))
        z = float(np.float64(Z) + np.float64(1e-8))
    u, w = _div(X, z), _div(Y, z)
    W, H = rec["W"], rec["H"]
    inside = u >= 0.0 and u <= float(W - 1) and w >= 0.0 and w <= float(H - 1) and z > 0.0
    if not inside:
        return False, None
    x0, y0 = math.floor(u), math.floor(w)
    x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
    tx, ty = u - float(x0), w - float(y0)
    d00, d01, d10, d11 = float(depth[y0, x0]), float(depth[y0, x1]), float(depth[y1, x0]), float(depth[y1, x1])
    ds = ((d00 * ((1.0 - tx) * (1.0 - ty)) + d01 * (tx * (1.0 - ty))) + d10 * ((1.0 - tx) * ty)) + d11 * (tx * ty)
    front = (z < ds + eps) if ds > 0.0 else True
    return front, (u, w, z, ds)


def visible_count(V, recs, depth, eps=0.005):
    count = np.zeros(len(V), np.int32)
    for r, d in zip(recs, depth):
        for i, v in enumerate(V):
            if view_sees(r, d, v, eps)[0]:
                count[i] += 1
    return count


def visibility(V, F, recs, eps=0.005, min_views=20):
    count = visible_count(V, recs, render_depth(V, F, recs), eps)
    return count, count >= min_views


def cull(V, F, keep, normals=None, colors=None):
    """update_faces(keep[faces].all(1)) and remove_unreferenced_vertices -> (v, f, normals, colors)"""
    F = np.asarray(F).reshape(-1, 3)
    f = F[keep[F].all(axis=1)] if len(F) else F
    ref = np.zeros(len(V), bool)
    ref[f.reshape(-1)] = True
    new = np.cumsum(ref) - 1
    return (V[ref], new[f].astype(np.int32).reshape(-1, 3), None if normals is None else normals[ref], None if colors is None else colors[ref])


# ---- geometry: a brute-force ray cast through pixel centres ---------------------------------------------------------------------------
def ray_cast(V, F, rec, offsets=((0.0, 0.0),)):
    """-> (z (K,H,W) fp64 with inf for no hit, face (K,H,W) int) of the rays through pixel centre + offset (pixels), K = len(offsets):
    Moeller-Trumbore against every face, both sides, the nearest hit with znear <= z <= zfar"""
    W, H = rec["W"], rec["H"]
    cam = np.array([[camera(rec, V[int(k)]) for k in f] for f in np.asarray(F).reshape(-1, 3)], np.float64).reshape(-1, 3, 3)
    zs, fs = [], []
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for ox, oy in offsets:
        d = np.stack([(ii + 0.5 + ox - rec["cx"]) / rec["fx"], (jj + 0.5 + oy - rec["cy"]) / rec["fy"], np.ones((H, W))], axis=-1).reshape(-1, 1, 3)
        best = np.full(H * W, np.inf)
        face = np.full(H * W, -1)
        if len(cam):
            e1, e2 = cam[:, 1] - cam[:, 0], cam[:, 2] - cam[:, 0]
            with np.errstate(all="ignore"):
                p = np.cross(d, e2[None])
                det = (p * e1[None]).sum(-1)
                s = -cam[None, :, 0]
                uu = (p * s).sum(-1) / det
                q = np.cross(s, e1[None])
                vv = (q * d).sum(-1) / det
                t = (q * e2[None]).sum(-1) / det
                hit = (det != 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t >= rec["znear"]) & (t <= rec["zfar"])
            t = np.where(hit, t, np.inf)
            face = np.where(np.isfinite(t.min(axis=1)), t.argmin(axis=1), -1)
            best = t.min(axis=1)
        zs.append(best.reshape(H, W))
        fs.append(face.reshape(H, W))
    return np.stack(zs), np.stack(fs)


SNAP = 1.0 / 256.0
CLEAN = ((0.0, 0.0), (-2 * SNAP, -2 * SNAP), (2 * SNAP, -2 * SNAP), (-2 * SNAP, 2 * SNAP), (2 * SNAP, 2 * SNAP))


def geometric_tolerance(V, F, rec):
    """-> (z (H,W) of the ray cast at the centres, tol (H,W), clean (H,W) bool).  A vertex moves by at most half a unit of the 1/256-pixel
    grid in x and in y when it is snapped, so a point of its triangle moves by at most that, and the restated depth at a pixel centre
    is the true surface's depth somewhere within (+-1/512, +-1/512) pixel of it: tol = the largest change of the ray-cast depth over the
    corners of the four times larger square (+-1/128: the depth is not linear in the pixel, the square covers the curvature) plus the
    float32 rounding 2^-24 z.  clean: the same face (or none) answers at the centre and at all four corners -- no edge, no silhouette
    and no crossing of two surfaces within 1/128 pixel."""
    z, face = ray_cast(V, F, rec, CLEAN)
    clean = (face == face[0]).all(axis=0)
    with np.errstate(all="ignore"):
        tol = np.abs(z[1:] - z[0]).max(axis=0) + np.abs(z[0]) * 2.0 ** -24
    return z[0], np.where(clean & np.isfinite(z[0]), tol, 0.0), clean
