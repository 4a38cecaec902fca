"""numpy restatement of DESIGN.md §3.11 (the tetra points, one bisection round, the edge filter, the mesh of the 8th round) -- the
contract in the plainest form it can take: ordered fp32 numpy for the point values, ordered fp64 numpy for the keep decisions, boolean
indexing for the compaction, the torch lines of extract_mesh.py:91-102 for the bisection.  The kernels of csrc/extract.hip are held to
it with equalities (tests/test_extract_host.py, tests/test_extract_gpu.py), and it is held to the reference through
tests/golden/ref_extract_golden.npz.  Also here: the synthetic scenes of those tests, the analytic field and the near-tie predicate.
Test infrastructure only."""
import types

import numpy as np

import mesh_cull_restatement as MR

f32 = np.float32
FINAL_ALPHA, FIRST, ALPHA = 0, 1, 2


# ---- the tetra points ------------------------------------------------------------------------------------------------------------------
def build_rotation(rotation):
    """utils/general_utils.py: build_rotation, operation by operation, in fp32 -> (P,3,3)"""
    q = np.asarray(rotation, f32)
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    q = q / n[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f32(1), f32(2)
    R = np.zeros((len(q), 3, 3), f32)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - r * z)
    R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y)
    R[:, 2, 1] = two * (y * z + r * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def candidates(xyz, scaling, rotation):
    """-> (points (9P,3) float32, scales (9P,) float32): 8 corners per Gaussian (corner c: signs = bits 2, 1, 0 of c), then the centres"""
    xyz, scaling = np.asarray(xyz, f32).reshape(-1, 3), np.asarray(scaling, f32).reshape(-1, 3)
    P = len(xyz)
    with np.errstate(all="ignore"):
        R = build_rotation(np.asarray(rotation, f32).reshape(-1, 4))
        s = scaling * f32(3.0)
        corners = np.zeros((P, 8, 3), f32)
        for c in range(8):
            a = [s[:, j] if (c >> (2 - j)) & 1 else -s[:, j] for j in range(3)]
            for k in range(3):
                corners[:, c, k] = ((R[:, k, 0] * a[0] + R[:, k, 1] * a[1]) + R[:, k, 2] * a[2]) + xyz[:, k]
        m = np.maximum(np.maximum(s[:, 0], s[:, 1]), s[:, 2])
    return np.concatenate([corners.reshape(-1, 3), xyz]), np.concatenate([np.repeat(m, 8), m])


def project(points, rec, W, H):
    """one view, fp64 in the contract's order -> (u, v, Z)"""
    p = np.asarray(points, f32).astype(np.float64)
    m, fx, fy = np.asarray(rec["m"], np.float64), float(rec["fx"]), float(rec["fy"])
    cx, cy = float(f32(W / 2.0)), float(f32(H / 2.0))
    with np.errstate(all="ignore"):
        X = ((m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]) + m[3]
        Y = ((m[4] * p[:, 0] + m[5] * p[:, 1]) + m[6] * p[:, 2]) + m[7]
        Z = ((m[8] * p[:, 0] + m[9] * p[:, 1]) + m[10] * p[:, 2]) + m[11]
        u = (fx * X + cx * Z) / Z
        v = (fy * Y + cy * Z) / Z
    return u, v, Z


def seen(points, records, W, H, near, far):
    keep = np.zeros(len(points), bool)
    for rec in records:
        u, v, Z = project(points, rec, W, H)
        with np.errstate(all="ignore"):
            keep |= (Z >= near) & (Z <= far) & (u >= 0.0) & (u <= float(W - 1)) & (v >= 0.0) & (v <= float(H - 1))
    return keep


def near_tie(points, records, W, H, near, far, px=1e-3, rel=1e-6):
    """the candidates for which, in some view, u or v lies within `px` of a bound or Z within `rel` (relative) of near / far"""
    tie = np.zeros(len(points), bool)
    for rec in records:
        u, v, Z = project(points, rec, W, H)
        with np.errstate(all="ignore"):
            tie |= (np.abs(u) <= px) | (np.abs(u - (W - 1)) <= px) | (np.abs(v) <= px) | (np.abs(v - (H - 1)) <= px)
            tie |= (np.abs(Z - near) <= rel * abs(near)) | (np.abs(Z - far) <= rel * abs(far))
    return tie


def tetra_points(xyz, scaling, rotation, records, W, H, near, far):
    pts, sc = candidates(xyz, scaling, rotation)
    keep = seen(pts, records, W, H, near, far)
    return pts[keep], sc[keep]


def frustum_records(cameras):
    """what mesh_extraction.frustum_records builds, restated: rows 0..2 of world_view_transform.T and the focal lengths, fp32 -> fp64"""
    rec = np.zeros(len(cameras), [("m", "<f8", (12,)), ("fx", "<f8"), ("fy", "<f8")])
    for i, cam in enumerate(cameras):
        w2c = np.asarray(cam.world_view_transform, f32).reshape(4, 4).T.astype(np.float64)
        rec[i] = (w2c[:3].reshape(12), float(f32(cam.focal_x)), float(f32(cam.focal_y)))
    W, H = (int(cameras[0].image_width), int(cameras[0].image_height)) if len(cameras) else (0, 0)
    return rec, W, H


# ---- the bisection, the filter, the mesh ----------------------------------------------------------------------------------------------
def bisect_step(left_pts, right_pts, left_sdf, right_sdf, value, mode):
    """extract_mesh.py:91-102 in numpy fp32, in place -> the next query points"""
    if mode != FIRST:
        with np.errstate(all="ignore"):
            alpha = value if mode == ALPHA else f32(1) - value
            mid = (left_pts + right_pts) / f32(2)
            mid_sdf = alpha - f32(0.5)
            mid_sdf = np.where(np.isnan(mid_sdf), np.array(0x7FC00000, np.uint32).view(f32), mid_sdf)     # the canonical quiet NaN (§3.11)
            low = ((mid_sdf < 0) & (left_sdf < 0)) | ((mid_sdf > 0) & (left_sdf > 0))
        left_sdf[low] = mid_sdf[low]
        right_sdf[~low] = mid_sdf[~low]
        left_pts[low] = mid[low]
        right_pts[~low] = mid[~low]
    with np.errstate(all="ignore"):
        return (left_pts + right_pts) / f32(2)


def edge_filter(end_points, end_scales):
    e = np.asarray(end_points, f32).reshape(-1, 2, 3)
    s = np.asarray(end_scales, f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        d = e[:, 0] - e[:, 1]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        return dist <= s[:, 0] + s[:, 1]


def edge_filter_near_tie(end_points, end_scales, ulps=4):
    """the edges whose length lies within `ulps` ulp (of the scales' sum) of the scales' sum"""
    e = np.asarray(end_points, f32).reshape(-1, 2, 3).astype(np.float64)
    s = np.asarray(end_scales, f32).reshape(-1, 2)
    total = s[:, 0] + s[:, 1]
    dist = np.sqrt(((e[:, 0] - e[:, 1]) ** 2).sum(-1))
    return np.abs(dist - total.astype(np.float64)) <= ulps * np.spacing(total).astype(np.float64)


def colors_u8(color):
    """(color * 255) truncated toward zero; outside [0, 256) the low 8 bits of the truncated integer; NaN and |value| >= 2^62 -> 0"""
    with np.errstate(all="ignore"):
        c = np.asarray(color, f32) * f32(255)
        c = np.where(np.abs(c) < f32(2.0 ** 62), c, f32(0))
    return (c.astype(np.int64) & 255).astype(np.uint8)


def bisect_and_mesh(end_points, end_sdf, end_scales, faces, final_alpha_of, color_of=None, filter_mesh=False, texture_mesh=False, steps=8):
    """extract_mesh.py:73-118 -> dict(end_vertices: the 8th round's midpoints of all edges, mask, vertices, faces, colors)"""
    e = np.asarray(end_points, f32).reshape(-1, 2, 3)
    sdf = np.asarray(end_sdf, f32).reshape(-1, 2)
    mask = edge_filter(e, end_scales)
    l, r, ls, rs = e[:, 0].copy(), e[:, 1].copy(), sdf[:, 0].copy(), sdf[:, 1].copy()
    pts = bisect_step(l, r, None, None, None, FIRST)
    for _ in range(steps):
        pts = bisect_step(l, r, ls, rs, final_alpha_of(pts), FINAL_ALPHA)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int32)
    out = {"end_vertices": pts, "mask": mask, "vertices": pts, "faces": faces, "colors": colors_u8(color_of(pts)) if texture_mesh else None}
    if filter_mesh:
        c = MR.compact(mask, faces, attrs=(pts,) + ((out["colors"],) if texture_mesh else ()))
        out["vertices"], out["faces"] = c["attrs"][0], c["faces"]
        if texture_mesh:
            out["colors"] = c["attrs"][1]
    return out


# ---- the analytic field: additions, multiplications and a clamp only, so numpy and torch (host or device) give the same bits -----------
def field_final_alpha(p):
    """the transmittance at p (N,3): 0 inside an ellipsoid around (0.125, -0.0625, 0.25), rising to 1; alpha = 1 - it crosses 0.5 on
    the ellipsoid 2 dx^2 + 1.5 dy^2 + 2.5 dz^2 = 0.5.  Works on float32 numpy arrays and torch tensors alike."""
    dx, dy, dz = p[:, 0] - 0.125, p[:, 1] + 0.0625, p[:, 2] - 0.25
    f = (dx * dx * 2.0 + dy * dy * 1.5) + dz * dz * 2.5
    return f.clip(0.0, 1.0)


def field_color(p):
    return (p * 0.5 + 0.5).clip(0.0, 1.0)


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------
def ring_cameras(n=8, sizes=((161, 120),)):
    """n cameras on a ring of radius 3 looking at the origin (mesh_cull_restatement.golden_scene's poses and focal lengths), image
    sizes taken in turn from `sizes` -> [namespace(world_view_transform (4,4) float32, focal_x, focal_y, image_width, image_height)]"""
    g = MR.golden_scene(num_vertices=1)
    return [types.SimpleNamespace(world_view_transform=g["world_view_transform"][i % 8].copy(), focal_x=float(g["focal"][i % 8, 0]), focal_y=float(g["focal"][i % 8, 1]),
                                  image_width=int(sizes[i % len(sizes)][0]), image_height=int(sizes[i % len(sizes)][1])) for i in range(n)]


def gaussians(P, seed=21, extent=2.5):
    """P seeded Gaussians: positions uniform in [-extent, extent]^3, scales log-normal around 0.03, random quaternions (not normalised)
    -> (xyz (P,3), scaling (P,3), rotation (P,4)) float32"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-extent, extent, (P, 3)).astype(f32)
    scaling = (0.03 * np.exp(0.5 * rng.normal(size=(P, 3)))).astype(f32)
    rotation = rng.normal(size=(P, 4)).astype(f32)
    return xyz, scaling, rotation


def edges(E, seed=31):
    """E synthetic crossing edges around the analytic surface: end points, their sdf (alpha - 0.5 of the field), scales such that about
    half of the edges pass the filter -> (end_points (E,2,3), end_sdf (E,2,1), end_scales (E,2,1), faces (2E,3) int64)"""
    rng = np.random.default_rng(seed + E)
    a = rng.uniform(-1.0, 1.0, (E, 3)).astype(f32)
    b = (a + rng.normal(size=(E, 3)).astype(f32) * f32(0.2)).astype(f32)
    e = np.stack([a, b], 1)
    sdf = ((f32(1) - field_final_alpha(e.reshape(-1, 3))) - f32(0.5)).reshape(E, 2, 1)
    length = np.sqrt(((a.astype(np.float64) - b) ** 2).sum(-1))
    sc = (length[:, None] * rng.uniform(0.2, 0.8, (E, 2))).astype(f32).reshape(E, 2, 1)
    faces = rng.integers(0, max(E, 1), (2 * E, 3)).astype(np.int64)
    return e, sdf, sc, faces
