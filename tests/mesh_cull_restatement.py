"""The yardstick of the mesh culling: the three computations of the reference's evaluate_dtu_mesh.py:77-131 written
anew from the contract, as plain functions over numpy arrays -- SciPy's binary dilation with the disk as structure, the ordered fp64
projection formulas, boolean indexing for the compaction.  Test infrastructure only; nothing here is used by the product."""
import numpy as np
from scipy import ndimage


def disk(r):
    """the footprint of skimage.morphology.disk: dx^2 + dy^2 <= r^2 on a (2r+1)^2 grid"""
    g = np.arange(-int(r), int(r) + 1)
    return (g[:, None] * g[:, None] + g[None, :] * g[None, :]) <= int(r) * int(r)


def mask_set(mask):
    """a pixel is set iff (float32) m / 256 != 0 (the script divides by 256. before it dilates)"""
    m = np.asarray(mask)
    return (m.astype(np.float32) / np.float32(256.0)) != 0


def dilate(mask, r):
    """-> (H,W) bool"""
    return ndimage.binary_dilation(mask_set(mask), structure=disk(r))


def pack(bits):
    """(H,W) bool -> (H, ceil(W/64)) uint64, pixel x = bit x % 64 of word x // 64, pad bits zero"""
    b = np.asarray(bits, bool)
    H, W = b.shape
    nw = (W + 63) // 64
    p = np.zeros((H, nw * 64), np.uint8)
    p[:, :W] = b
    return np.packbits(p.reshape(H, nw, 64), axis=-1, bitorder="little").view("<u8").reshape(H, nw)


def view_matrix(focal_x, focal_y, W, H, world_view_transform):
    """m = rows 0..2 of K W2C in fp64: K's entries and W2C = world_view_transform.T rounded to fp32 as the script stores them.
    K has two non-zero entries per row, so row r of the product is K[r,r] W2C[r] + K[r,2] W2C[2] (rows 0, 1) and W2C[2] (row 2)."""
    w2c = np.asarray(world_view_transform, np.float32).T.astype(np.float64)
    fx, fy, cx, cy = (float(np.float32(v)) for v in (focal_x, focal_y, W / 2.0, H / 2.0))
    return np.stack([fx * w2c[0] + cx * w2c[2], fy * w2c[1] + cy * w2c[2], w2c[2]])


def project(vertices, m, W, H):
    """-> (px, py) fp64 (N,), the contract's order of operations"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    m = np.asarray(m, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        x, y, z = (((m[r, 0] * v[:, 0] + m[r, 1] * v[:, 1]) + m[r, 2] * v[:, 2]) + m[r, 3] for r in range(3))
        d = z + 1e-6
        px = ((x / d) / float(W - 1) - 0.5) * 2.0
        py = ((y / d) / float(H - 1) - 0.5) * 2.0
    return px, py


def view_keeps(vertices, m, W, H, dilated):
    """-> (N,) bool: the view does not drop the vertex"""
    px, py = project(vertices, m, W, H)
    with np.errstate(all="ignore"):
        valid = (px > -1.0) & (px < 1.0) & (py > -1.0) & (py < 1.0)
        fx = np.rint((px + 1.0) / 2.0 * float(W - 1))
        fy = np.rint((py + 1.0) / 2.0 * float(H - 1))
    inside = valid & (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    ix = np.where(inside, fx, 0).astype(np.int64)
    iy = np.where(inside, fy, 0).astype(np.int64)
    hit = inside & np.asarray(dilated, bool)[iy, ix]
    return ~valid | hit


def cull(vertices, views):
    """views: [(m, W, H, dilated (H,W) bool)] -> keep (N,) bool"""
    keep = np.ones(len(vertices), bool)
    for m, W, H, dil in views:
        keep &= view_keeps(vertices, m, W, H, dil)
    return keep


def near_decision(vertices, views, eps=1e-3):
    """-> (N,) bool: in some view the fp64 pixel coordinate lies within eps px of a rounding tie or of a validity bound"""
    near = np.zeros(len(vertices), bool)
    for m, W, H, _ in views:
        px, py = project(vertices, m, W, H)
        with np.errstate(all="ignore"):
            for p, n in ((px, W - 1), (py, H - 1)):
                u = (p + 1.0) / 2.0 * n                       # pixel units; the bounds p = -1, 1 are u = 0, n
                ok = np.isfinite(u)
                frac = np.abs(u - np.floor(u) - 0.5)
                near |= ok & (u > -1.0) & (u < n + 1.0) & ((frac <= eps) | (np.abs(u) <= eps) | (np.abs(u - n) <= eps))
    return near


def compact(keep, faces, vertices=None, attrs=()):
    """-> dict(rows, faces, face_keep[, vertices][, attrs])"""
    keep = np.asarray(keep, bool)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    inverse = np.zeros(len(keep), np.int64)
    inverse[keep] = np.arange(int(keep.sum()))
    face_keep = keep[F].all(axis=1) if len(F) else np.zeros(0, bool)
    out = {"rows": np.nonzero(keep)[0].astype(np.int32), "face_keep": face_keep,
           "faces": inverse[F][face_keep].astype(np.int32).reshape(-1, 3),
           "faces_all": np.where(keep[F], inverse[F], 0).astype(np.int32).reshape(-1, 3) if len(F) else np.zeros((0, 3), np.int32)}
    if vertices is not None:
        out["vertices"] = np.asarray(vertices)[keep]
    out["attrs"] = [np.asarray(a)[keep] for a in attrs]
    return out


def ply_bytes(vertices, faces, normals=None, colors=None):
    """binary little-endian PLY: float x y z [nx ny nz] [uchar red green blue], list uchar int faces"""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(v)
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f)
    rec = np.zeros(len(v), fields)
    for i, k in enumerate("xyz"):
        rec[k] = v[:, i].astype(np.float32)
        if normals is not None:
            rec["n" + k] = np.asarray(normals, np.float32).reshape(-1, 3)[:, i]
    if colors is not None:
        for i, k in enumerate(("red", "green", "blue")):
            rec[k] = np.asarray(colors, np.uint8).reshape(-1, 3)[:, i]
    fr = np.zeros(len(f), [("n", "u1"), ("i", "<i4", (3,))])
    fr["n"], fr["i"] = 3, f
    return head.encode("ascii") + rec.tobytes() + fr.tobytes()


# ---- the scene of tests/golden/ref_dtu_cull_golden.npz (make_golden_cull.py builds the same one) -------------------------------------
def golden_scene(num_vertices=20000, seed=11):
    """8 views of 161 x 120 looking at the origin from a ring of radius 3, disc masks of radius 30 + 2 i px plus 0.1 % salt pixels,
    focal lengths ~150 px, vertices uniform in [-1.2, 1.2]^3 -> dict of arrays"""
    rng = np.random.default_rng(seed)
    W, H, n = 161, 120, 8
    wvt = np.zeros((n, 4, 4), np.float32)
    focal = np.zeros((n, 2), np.float32)
    masks = np.zeros((n, 1, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        a = 2 * np.pi * i / n
        C = np.array([3 * np.cos(a), 0.4 * np.sin(3 * a), 3 * np.sin(a)])
        zc = -C / np.linalg.norm(C)
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        yc = np.cross(zc, xc)
        R = np.stack([xc, yc, zc])                              # world -> camera
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = R, -R @ C
        wvt[i] = w2c.T.astype(np.float32)
        focal[i] = (150.0 + i, 148.5 - 0.5 * i)
        disc = (xx - W / 2.0 - 3 + i) ** 2 + (yy - H / 2.0 + 2 - i) ** 2 <= (30 + 2 * i) ** 2
        salt = rng.random((H, W)) < 0.001
        masks[i, 0] = (disc | salt) * rng.uniform(0.2, 1.0, (H, W))
    V = rng.uniform(-1.2, 1.2, (num_vertices, 3))
    return {"W": W, "H": H, "world_view_transform": wvt, "focal": focal, "masks": masks.astype(np.float32), "vertices": V}
