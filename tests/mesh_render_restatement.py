"""DESIGN.md §3.20 restated on the host in numpy fp64 and Python integers: vertex and face normals (g1), the face buffer (g2) and the
resolve pass (g3), in the order the section writes down (numpy's element-wise operations round once each and fuse nothing).  Geometry
and coverage are those of tests/mesh_raster_restatement.py (§3.19), reused as they are.  Nothing here calls the product.

Beside it a brute-force fp64 ray cast with the two nearest hits per pixel ties the face buffer to geometry (ray_cast2, anchor)."""
import numpy as np

import mesh_raster_restatement as R

NORMAL_WORLD, NORMAL_CAMERA, COLOR, SHADED = 0, 1, 2, 3
MODES = {"normal_world": NORMAL_WORLD, "normal_camera": NORMAL_CAMERA, "color": COLOR, "shaded": SHADED}
EMPTY64 = (1 << 64) - 1


def cross(a, b):
    """a, b: (..., 3) -> (..., 3)"""
    with np.errstate(all="ignore"):
        return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                         a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def dot(u, v):
    with np.errstate(all="ignore"):
        return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def unit(n):
    """the rule of (g1): n / len if len is finite and > 0, else (0, 0, 1)"""
    n = np.asarray(n, np.float64)
    with np.errstate(all="ignore"):
        ln = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        ok = np.isfinite(ln) & (ln > 0)
        out = n / np.where(ok, ln, 1.0)[..., None]
    out[~ok] = (0.0, 0.0, 1.0)
    return out


def face_vectors(V, F):
    """Nf = cross(v1 - v0, v2 - v0), (NF,3) fp64"""
    V = np.asarray(V, np.float32).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    if len(F) == 0:
        return np.zeros((0, 3))
    with np.errstate(all="ignore"):
        return cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])


def _f32(a):
    with np.errstate(all="ignore"):
        return np.asarray(a, np.float64).astype(np.float32)


def face_normals(V, F):
    return _f32(unit(face_vectors(V, F))).reshape(-1, 3)


def vertex_normals(V, F):
    """the sum over the incident corners in ascending 3 * face + corner order, one addition each, from 0"""
    nf = face_vectors(V, F)
    acc = np.zeros((len(np.asarray(V).reshape(-1, 3)), 3))
    with np.errstate(all="ignore"):
        for c, v in enumerate(np.asarray(F).reshape(-1)):
            acc[int(v)] = acc[int(v)] + nf[c // 3]
    return _f32(unit(acc)).reshape(-1, 3)


# ---- (g2) ------------------------------------------------------------------------------------------------------------------------------
def render_faces_view(V, F, rec):
    """-> (depth (H,W) float32, face (H,W) int32): per pixel the minimum of (bits(d) << 32) | face"""
    W, H = rec["W"], rec["H"]
    word = [[EMPTY64] * W for _ in range(H)]
    for fi, f in enumerate(np.asarray(F).reshape(-1, 3)):
        for tri in R.fan_triangles(rec, [V[int(k)] for k in f]):
            t = R.snapped(tri)
            if t is None:
                continue
            xs, ys = [p[0] for p in t], [p[1] for p in t]
            i0, i1 = max(0, min(xs) // 256 - 1), min(W - 1, max(xs) // 256 + 1)
            j0, j1 = max(0, min(ys) // 256 - 1), min(H - 1, max(ys) // 256 + 1)
            for j in range(j0, j1 + 1):
                for i in range(i0, i1 + 1):
                    d = R.pixel_depth(t[0], t[1], t[2], i, j, rec["zfar"])
                    if d is not None:
                        word[j][i] = min(word[j][i], (int(np.float32(d).view(np.uint32)) << 32) | fi)
    w = np.array(word, dtype=np.uint64).reshape(H, W)
    empty = w == np.uint64(EMPTY64)
    depth = np.where(empty, 0, w >> np.uint64(32)).astype(np.uint32).view(np.float32)
    face = np.where(empty, -1, (w & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return depth, face


def render_faces(V, F, recs, shape):
    if not recs:
        return np.zeros((0,) + shape, np.float32), np.zeros((0,) + shape, np.int32)
    out = [render_faces_view(V, F, r) for r in recs]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- (g3) ------------------------------------------------------------------------------------------------------------------------------
def camera_faces(V, F, rec):
    """(NF,3,3): the camera coordinates of every face's three vertices, as §3.19 step 1 forms them"""
    F = np.asarray(F).reshape(-1, 3)
    cam = np.array([R.camera(rec, v) for v in np.asarray(V, np.float32).reshape(-1, 3)], np.float64).reshape(-1, 3)
    return cam[F] if len(F) else np.zeros((0, 3, 3))


def barycentrics(V, F, rec, face):
    """face (H,W) int -> (lam (H,W,3) fp64 (0 where face < 0), cam (H,W,3,3) of the pixel's face)"""
    H, W = face.shape
    hit = face >= 0
    cam = np.zeros((H, W, 3, 3))
    cf = camera_faces(V, F, rec)
    if hit.any():
        cam[hit] = cf[face[hit]]
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        d = np.stack([((ii + 0.5) - rec["cx"]) / rec["fx"], ((jj + 0.5) - rec["cy"]) / rec["fy"], np.ones((H, W))], axis=-1)
        a, b, c = cam[:, :, 0], cam[:, :, 1], cam[:, :, 2]
        m0, m1, m2 = dot(d, cross(b, c)), dot(d, cross(c, a)), dot(d, cross(a, b))
        s = (m0 + m1) + m2
        lam = np.stack([m0 / s, m1 / s, m2 / s], axis=-1)
        lam = np.where(np.isnan(lam) | (lam < 0), 0.0, np.where(lam > 1, 1.0, lam))
        t = (lam[..., 0] + lam[..., 1]) + lam[..., 2]
        lam = np.where((t > 0)[..., None], lam / t[..., None], 1.0 / 3.0)
    lam[~hit] = 0.0
    return lam, cam


def _sum3(lam, q):
    """q (H,W,3 vertices,C) -> (H,W,C): (l0 q0 + l1 q1) + l2 q2"""
    with np.errstate(all="ignore"):
        return (lam[..., 0, None] * q[:, :, 0] + lam[..., 1, None] * q[:, :, 1]) + lam[..., 2, None] * q[:, :, 2]


def shade_view(V, F, rec, face, mode, normals=None, colors=None, flat=False, vertex_base=False, base=(0.8, 0.8, 0.8), ambient=0.25,
               background=(1.0, 1.0, 1.0)):
    """-> (image (3,H,W) float32, bary (3,H,W) float32)"""
    F = np.asarray(F).reshape(-1, 3)
    H, W = face.shape
    face = np.where((face >= 0) & (face < len(F)), face, -1)
    hit = face >= 0
    if not hit.any():
        img = np.empty((3, H, W), np.float32)
        img[:] = np.asarray(background, np.float64).astype(np.float32)[:, None, None]
        return img, np.zeros((3, H, W), np.float32)
    lam, cam = barycentrics(V, F, rec, face)
    fs = np.where(hit, face, 0)
    idx = F[fs] if len(F) else np.zeros((H, W, 3), int)
    col = None
    if mode == COLOR or (mode == SHADED and vertex_base):
        C = np.asarray(colors)[:, :3].astype(np.float64)
        with np.errstate(all="ignore"):
            col = _sum3(lam, C[idx]) / 255.0
    if mode == COLOR:
        out = col
    else:
        if flat:
            nw = face_vectors(V, F)[fs] if len(F) else np.zeros((H, W, 3))
        else:
            nw = _sum3(lam, np.asarray(normals, np.float32).astype(np.float64)[idx])
        nu = unit(nw)
        m = np.asarray(rec["w2c"], np.float64).reshape(3, 4)
        with np.errstate(all="ignore"):
            nc = np.stack([(m[r, 0] * nu[..., 0] + m[r, 1] * nu[..., 1]) + m[r, 2] * nu[..., 2] for r in range(3)], axis=-1)
            if mode == NORMAL_WORLD:
                out = (nu + 1.0) / 2.0
            elif mode == NORMAL_CAMERA:
                out = (nc + 1.0) / 2.0
            else:
                p = _sum3(lam, cam)
                v = unit(-p)
                lit = np.abs(dot(nc, v))
                k = ambient + (1.0 - ambient) * lit
                b = col if vertex_base else np.broadcast_to(np.asarray(base, np.float64), (H, W, 3))
                out = b * k[..., None]
    img = _f32(out)
    img[~hit] = np.asarray(background, np.float64).astype(np.float32)
    return np.ascontiguousarray(img.transpose(2, 0, 1)), np.ascontiguousarray(_f32(lam).transpose(2, 0, 1))


def shade(V, F, recs, faces, shape, mode, **kw):
    if not recs:
        return np.zeros((0, 3) + shape, np.float32), np.zeros((0, 3) + shape, np.float32)
    out = [shade_view(V, F, r, f, mode, **kw) for r, f in zip(recs, faces)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- geometry: the two nearest hits of a brute-force ray cast ----------------------------------------------------------------------------
def ray_cast2(V, F, rec, offset=(0.0, 0.0)):
    """-> (z1, z2 (H,W) fp64: the nearest and second nearest hit, inf for none; face (H,W) of the nearest, -1 for none; uv (H,W,2) of it):
    Moeller-Trumbore against every face, both sides, znear <= t <= zfar"""
    W, H = rec["W"], rec["H"]
    cam = camera_faces(V, F, rec)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(ii + 0.5 + offset[0] - rec["cx"]) / rec["fx"], (jj + 0.5 + offset[1] - rec["cy"]) / rec["fy"], np.ones((H, W))], axis=-1).reshape(-1, 1, 3)
    n = H * W
    if len(cam) == 0:
        return np.full((H, W), np.inf), np.full((H, W), np.inf), np.full((H, W), -1), np.zeros((H, W, 2))
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
    order = np.argsort(t, axis=1, kind="stable")
    first = order[:, 0]
    z1 = t[np.arange(n), first]
    z2 = t[np.arange(n), order[:, 1]] if t.shape[1] > 1 else np.full(n, np.inf)
    face = np.where(np.isfinite(z1), first, -1)
    uv = np.stack([uu[np.arange(n), first], vv[np.arange(n), first]], axis=-1)
    return z1.reshape(H, W), z2.reshape(H, W), face.reshape(H, W), uv.reshape(H, W, 2)


def anchor(V, F, rec):
    """-> (face (H,W) of the ray cast at the centres, uv, judged (H,W) bool, covered (H,W) bool).  judged: no projected edge within 1/128
    pixel (the same face, or none, answers at the centre and at the four corners of R.CLEAN) and the two nearest hits further apart
    than §3.19's depth tolerance (R.geometric_tolerance: snap x depth slope + float32 rounding) taken for both of them."""
    z, tol, clean = R.geometric_tolerance(V, F, rec)
    z1, z2, face, uv = ray_cast2(V, F, rec)
    with np.errstate(all="ignore"):
        apart = ~np.isfinite(z2) | (z2 - z1 > 2.0 * tol + np.abs(z2) * 2.0 ** -23)
    return face, uv, clean & (apart | (face < 0)), face >= 0
