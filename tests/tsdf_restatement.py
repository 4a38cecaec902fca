"""Float64 numpy restatement of the TSDF fusion contract ("TSDF fusion"): touch, integrate and extract on small grids.

Test helper (not a test module).  It shares nothing with the product but the marching-cubes tables: ``gaussian-opacity-fields_amd/gen_tsdf_tables.py``
constructs them and writes ``csrc/tsdf_tables.h`` (tests/test_tsdf_host.py checks that the header holds them verbatim).

Conventions (Lorensen-Cline / Bourke numbering):
  corners 0..7 at (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); case bit i set iff corner i is inside (tsdf < 0);
  edges 0..11 = (0,1) (1,2) (3,2) (0,3) (4,5) (5,6) (7,6) (4,7) (0,4) (1,5) (2,6) (3,7), each written lower end first.
The triangle lists: see gen_tsdf_tables.py.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussian-opacity-fields_amd"))
R = 16
BIAS = 1 << 20
EMPTY = (1 << 64) - 1

from gen_tsdf_tables import CORNERS, EDGES, EDGE_OWNER, FACES, mc_tables, tables_header  # noqa: E402,F401  (the product's tables)


# ---------------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------------
def pack(b):
    b = np.asarray(b, dtype=np.int64)
    return ((b[..., 0] + BIAS).astype(np.uint64) | ((b[..., 1] + BIAS).astype(np.uint64) << np.uint64(21))
            | ((b[..., 2] + BIAS).astype(np.uint64) << np.uint64(42)))


def unpack(k):
    k = np.asarray(k, dtype=np.uint64)
    m = np.uint64((1 << 21) - 1)
    return np.stack([(k & m).astype(np.int64), ((k >> np.uint64(21)) & m).astype(np.int64), ((k >> np.uint64(42)) & m).astype(np.int64)], -1) - BIAS


# ---------------------------------------------------------------------------------------------------------------------------
# touch
# ---------------------------------------------------------------------------------------------------------------------------
def _camera(K, E):
    K = np.asarray(K, np.float64)
    E = np.asarray(E, np.float64)
    Rm, t = E[:3, :3], E[:3, 3]
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2], Rm, t, -Rm.T @ t


def _segments(depth, K, E, voxel_size, depth_scale, depth_max, trunc_mult):
    """-> (p0, p1) [N,3] in block units: the truncation segment of every valid pixel"""
    fx, fy, cx, cy, Rm, t, C = _camera(K, E)
    trunc = trunc_mult * voxel_size
    bs = voxel_size * R
    H, W = depth.shape
    d = depth.astype(np.float64) / depth_scale
    vv, uu = np.nonzero((d > 0) & (d <= depth_max))
    d = d[vv, uu]
    dc = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones(len(uu))], -1)
    dw = dc @ Rm                                                   # R^T dc, row by row
    t0, t1 = np.maximum(d - trunc, 0.0), np.minimum(d + trunc, depth_max)
    return (C + t0[:, None] * dw) / bs, (C + t1[:, None] * dw) / bs


def _walk(p0, p1):
    """exact 3-D DDA of every segment from its start block to its end block -> [M,3] blocks (with repeats)"""
    c = np.floor(p0).astype(np.int64)
    e = np.floor(p1).astype(np.int64)
    d = p1 - p0
    step = np.where(e > c, 1, -1)
    rem = np.abs(e - c)
    with np.errstate(divide="ignore", invalid="ignore"):
        tmax = np.where(rem > 0, (c + (step > 0) - p0) / d, np.inf)
        tdel = np.where(rem > 0, 1.0 / np.abs(d), np.inf)
    out = [c.copy()]
    n = rem.sum(1)
    for k in range(int(n.max()) if len(n) else 0):
        act = n > k
        tm = np.where(rem > 0, tmax, np.inf)
        a = np.argmin(tm, 1)                                        # first minimum: the lowest axis on ties
        rows = np.nonzero(act)[0]
        ax = a[rows]
        c[rows, ax] += step[rows, ax]
        rem[rows, ax] -= 1
        tmax[rows, ax] += tdel[rows, ax]
        out.append(c[rows].copy())
    return np.concatenate(out)


def _near_face(p0, p1, eps=1e-5):
    """-> bool [N]: the segment ends within eps of a block face, or crosses a face within eps of a block edge"""
    near = np.zeros(len(p0), bool)
    lo, hi = np.minimum(p0, p1), np.maximum(p0, p1)
    for a in range(3):
        near |= np.abs(p0[:, a] - np.round(p0[:, a])) < eps
        near |= np.abs(p1[:, a] - np.round(p1[:, a])) < eps
        base = np.floor(lo[:, a] - eps)
        span = int(np.max(np.floor(hi[:, a] + eps) - base)) + 2 if len(p0) else 0
        for k in range(span):
            f = base + k
            ok = (lo[:, a] - eps <= f) & (f <= hi[:, a] + eps)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = (f - p0[:, a]) / (p1[:, a] - p0[:, a])
            q = p0 + s[:, None] * (p1 - p0)
            for b in range(3):
                if b != a:
                    near |= ok & (np.abs(q[:, b] - np.round(q[:, b])) < eps)
    return near


def touch(depth, K, E, voxel_size, depth_scale=1.0, depth_max=6.0, trunc_mult=8.0, near_face=None):
    """-> set of block tuples of one frame.  near_face (a set, optional): receives the blocks of segments that pass within 1e-5
    (in block units) of a block face, where float32 and float64 walks may differ."""
    p0, p1 = _segments(depth, K, E, voxel_size, depth_scale, depth_max, trunc_mult)
    out = {tuple(b) for b in np.unique(_walk(p0, p1), axis=0).tolist()} if len(p0) else set()
    if near_face is not None and len(p0):
        sel = _near_face(p0, p1)
        if sel.any():
            near_face.update(tuple(b) for b in np.unique(_walk(p0[sel], p1[sel]), axis=0).tolist())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# volume and integrate
# ---------------------------------------------------------------------------------------------------------------------------
_ZYX = np.stack(np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij"), -1).reshape(-1, 3)   # (z, y, x), linear order
_XYZ = _ZYX[:, ::-1]


class Volume:
    """blocks: dict block tuple -> float64 array [5, R, R, R] (tsdf, weight, r, g, b), indexed [plane, z, y, x]"""

    def __init__(self, voxel_size, trunc_mult=8.0):
        self.v = float(voxel_size)
        self.trunc = trunc_mult * self.v
        self.trunc_mult = trunc_mult
        self.blocks = {}

    def integrate(self, depth, color_hw3, K, E, depth_scale=1.0, depth_max=6.0, ambiguous=None, frame=None, chunk=256):
        """Updates every voxel of the frame's blocks (`frame`: a given block set, else this frame's touch) -> the block set.
        ambiguous (dict block -> bool [R,R,R], optional): voxels whose float32 evaluation may take another branch (a projection
        within 1e-3 px of a pixel edge or of the image border, sdf within 1e-5 of -trunc, zc within 1e-6 of 0) are marked"""
        fx, fy, cx, cy, Rm, t, _ = _camera(K, E)
        if frame is None:
            frame = touch(depth, K, E, self.v, depth_scale, depth_max, self.trunc_mult)
        H, W = depth.shape
        keys = sorted(frame)
        for i0 in range(0, len(keys), chunk):
            ks = keys[i0:i0 + chunk]
            blk = np.stack([self.blocks.get(b, np.zeros((5, R, R, R))) for b in ks]).reshape(len(ks), 5, -1)
            p = self.v * (np.array(ks, np.int64)[:, None, :] * R + _XYZ[None]).astype(np.float64)       # [n, R^3, 3]
            xc = p @ Rm.T + t
            zc = xc[..., 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                u = fx * xc[..., 0] / zc + cx
                vv = fy * xc[..., 1] / zc + cy
            ok = (zc > 0) & (u >= 0) & (u <= W - 1) & (vv >= 0) & (vv <= H - 1)
            ui = np.where(ok, np.floor(np.where(ok, u, 0)), 0).astype(np.int64)
            vi = np.where(ok, np.floor(np.where(ok, vv, 0)), 0).astype(np.int64)
            d = depth[vi, ui].astype(np.float64) / depth_scale
            ok &= (d > 0) & (d <= depth_max)
            sdf = d - zc
            ok &= sdf >= -self.trunc
            if ambiguous is not None:
                with np.errstate(invalid="ignore"):
                    fu, fv = u - np.floor(u), vv - np.floor(vv)
                    amb = (np.abs(zc) < 1e-6) | (np.minimum(fu, 1 - fu) < 1e-3) | (np.minimum(fv, 1 - fv) < 1e-3)
                    amb |= (np.abs(u - (W - 1)) < 1e-3) | (np.abs(vv - (H - 1)) < 1e-3)
                    amb |= np.abs(sdf + self.trunc) < 1e-5
                for k, b in enumerate(ks):
                    ambiguous.setdefault(b, np.zeros((R, R, R), bool)).reshape(-1)[:] |= amb[k]
            s = np.minimum(sdf, self.trunc) / self.trunc
            w = blk[:, 1].copy()
            blk[:, 0] = np.where(ok, (w * blk[:, 0] + s) / (w + 1), blk[:, 0])
            for c in range(3):
                col = color_hw3[vi, ui, c].astype(np.float64)
                blk[:, 2 + c] = np.where(ok, (w * blk[:, 2 + c] + col) / (w + 1), blk[:, 2 + c])
            blk[:, 1] = np.where(ok, w + 1, w)
            for k, b in enumerate(ks):
                self.blocks[b] = blk[k].reshape(5, R, R, R)
        return set(frame)


# ---------------------------------------------------------------------------------------------------------------------------
# extract
# ---------------------------------------------------------------------------------------------------------------------------
def _padded(blocks, b, lo, hi, planes=5):
    """values [planes, n, n, n] and existence [n, n, n] of the voxels at block-local coordinates [lo, hi) (z, y, x order)"""
    n = hi - lo
    A = np.zeros((planes, n, n, n))
    X = np.zeros((n, n, n), bool)
    for dz in range(lo // R, (hi - 1) // R + 1):
        for dy in range(lo // R, (hi - 1) // R + 1):
            for dx in range(lo // R, (hi - 1) // R + 1):
                nb = blocks.get((b[0] + dx, b[1] + dy, b[2] + dz))
                if nb is None:
                    continue
                sl_dst, sl_src = [], []
                for d in (dz, dy, dx):
                    g0, g1 = max(lo, d * R), min(hi, d * R + R)
                    sl_dst.append(slice(g0 - lo, g1 - lo))
                    sl_src.append(slice(g0 - d * R, g1 - d * R))
                A[(slice(None),) + tuple(sl_dst)] = nb[(slice(0, planes),) + tuple(sl_src)]
                X[tuple(sl_dst)] = True
    return A, X


def extract(blocks, voxel_size, weight_threshold=3.0):
    """blocks: dict block tuple -> array [5, R, R, R] ([plane, z, y, x]).  -> (vertices [V,3], triangles [F,3], colors, normals)
    in the contract's order: blocks by ascending packed key, vertices by (block, voxel linear index, axis), triangles by
    (block, cube voxel, table order).  Block by block, over the voxels at local coordinates [-1, 18) of each."""
    em, tris = mc_tables()
    EM = np.array(em, np.int64)
    NT = np.array([len(t) for t in tris], np.int64)
    TRI = np.full((256, 3 * max(NT)), -1, np.int64)
    for c, t in enumerate(tris):
        TRI[c, :3 * len(t)] = [e for tri in t for e in tri]
    OWN = np.array([o[::-1] for o, _ in EDGE_OWNER], np.int64)      # (z, y, x) offsets
    AX = np.array([a for _, a in EDGE_OWNER], np.int64)
    keys = sorted(blocks, key=lambda b: int(pack(b)))
    tau = weight_threshold
    S = R + 1                                                          # cubes at local -1 .. 15
    per = []
    for b in keys:
        A, X = _padded(blocks, b, -1, R + 2)                           # local -1 .. 17 -> index +1
        T = A[0]
        good = X & (A[1] >= tau)
        allg = np.ones((S, S, S), bool)
        case = np.zeros((S, S, S), np.int64)
        for i, (cx_, cy_, cz_) in enumerate(CORNERS):
            sl = (slice(cz_, cz_ + S), slice(cy_, cy_ + S), slice(cx_, cx_ + S))
            allg &= good[sl]
            case |= (T[sl] < 0).astype(np.int64) << i
        emit = allg & (NT[case] > 0)
        case = np.where(emit, case, 0)
        flags = np.zeros((R, R, R, 3), bool)                          # owned voxels 0..15, [z, y, x, axis]
        for e in range(12):
            oz, oy, ox = OWN[e]
            ue = emit & (((EM[case] >> e) & 1) == 1)
            flags[..., AX[e]] |= ue[1 - oz:1 - oz + R, 1 - oy:1 - oy + R, 1 - ox:1 - ox + R]
        # gradients at local 0 .. 16 (index 1 .. 17)
        G = np.zeros((3, S, S, S))
        inner = (slice(1, S + 1),) * 3
        for ax in range(3):
            sp = [slice(1, S + 1)] * 3
            sm = [slice(1, S + 1)] * 3
            sp[2 - ax] = slice(2, S + 2)
            sm[2 - ax] = slice(0, S)
            Tp, Tm, Xp, Xm, T0 = T[tuple(sp)], T[tuple(sm)], X[tuple(sp)], X[tuple(sm)], T[inner]
            G[ax] = np.where(Xp & Xm, 0.5 * (Tp - Tm), np.where(Xp, Tp - T0, np.where(Xm, T0 - Tm, 0.0)))
        q = np.argwhere(flags)                                         # (z, y, x, axis) in (linear index, axis) order
        pa = q[:, :3]
        e3 = np.zeros((len(q), 3), np.int64)
        e3[np.arange(len(q)), 2 - q[:, 3]] = 1
        pb = pa + e3
        ta, tb = T[tuple((pa + 1).T)], T[tuple((pb + 1).T)]
        r = ta / (ta - tb)
        pos = voxel_size * (np.array(b, np.int64) * R + pa[:, ::-1]).astype(np.float64)
        pos[np.arange(len(q)), q[:, 3]] += r * voxel_size
        ca, cb = A[2:5][(slice(None),) + tuple((pa + 1).T)].T, A[2:5][(slice(None),) + tuple((pb + 1).T)].T
        ga, gb = G[(slice(None),) + tuple(pa.T)].T, G[(slice(None),) + tuple(pb.T)].T
        nrm = (1 - r)[:, None] * ga + r[:, None] * gb
        ln = np.sqrt(np.sum(nrm * nrm, 1))
        nrm = np.where(ln[:, None] > 0, nrm / np.where(ln > 0, ln, 1)[:, None], 0.0)
        per.append(dict(flags=flags, pos=pos, col=ca + r[:, None] * (cb - ca), nrm=nrm, case=case[1:, 1:, 1:]))
    off = np.cumsum([0] + [len(p["pos"]) for p in per])
    vmaps = {}
    for k, b in enumerate(keys):
        vm = -np.ones((R, R, R, 3), np.int64)
        f = per[k]["flags"]
        vm[f] = off[k] + np.arange(int(f.sum()))
        vmaps[b] = vm
    faces = []
    for k, b in enumerate(keys):
        VM = -np.ones((S, S, S, 3), np.int64)                          # local 0 .. 16
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    nb = vmaps.get((b[0] + dx, b[1] + dy, b[2] + dz))
                    if nb is not None:
                        VM[dz * R:dz * R + R, dy * R:dy * R + R, dx * R:dx * R + R][:S - dz * R, :S - dy * R, :S - dx * R] = nb[:S - dz * R, :S - dy * R, :S - dx * R]
        cs = per[k]["case"]
        cv = np.argwhere(NT[cs] > 0)                                   # cubes in linear order
        cc = cs[tuple(cv.T)]
        nt = NT[cc]
        rows = np.repeat(np.arange(len(cv)), nt)
        ti = np.arange(len(rows)) - np.repeat(np.cumsum(nt) - nt, nt)
        tri = np.zeros((len(rows), 3), np.int64)
        for j in range(3):
            e = TRI[cc[rows], 3 * ti + j]
            o = cv[rows] + OWN[e]
            tri[:, j] = VM[o[:, 0], o[:, 1], o[:, 2], AX[e]]
        faces.append(tri)
    z = np.zeros((0, 3))
    V = np.concatenate([p["pos"] for p in per]) if per else z
    F = np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)
    assert (F >= 0).all()
    return V, F, (np.concatenate([p["col"] for p in per]) if per else z), (np.concatenate([p["nrm"] for p in per]) if per else z)


# ---------------------------------------------------------------------------------------------------------------------------
# analytic test scenes: depth maps ray-cast in float64 (camera convention: x right, y down, z forward)
# ---------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """-> 4x4 world->camera"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross(z, (0.0, 1.0, 0.0))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def intrinsic(W, H, fov_deg=50.0):
    f = 0.5 * W / np.tan(np.radians(fov_deg) / 2)
    return np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1.0]])


def _rays(K, E, H, W):
    fx, fy, cx, cy, Rm, t, C = _camera(K, E)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    return C, dc @ Rm          # world direction per pixel, camera z component 1


def _hit_sphere(C, d, c, r):
    oc = C - np.asarray(c)
    a = np.sum(d * d, -1)
    b = 2 * np.sum(d * oc, -1)
    q = b * b - 4 * a * (oc @ oc - r * r)
    t = (-b - np.sqrt(np.maximum(q, 0))) / (2 * a)
    return np.where((q > 0) & (t > 0), t, np.inf)


def _hit_box(C, d, lo, hi):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (np.asarray(lo) - C) / d
        t2 = (np.asarray(hi) - C) / d
    tn = np.max(np.minimum(t1, t2), -1)
    tf = np.min(np.maximum(t1, t2), -1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def _hit_plane(C, d, n, extent):
    n = np.asarray(n, np.float64) / np.linalg.norm(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -(C @ n) / (d @ n)
    p = C + t[..., None] * d
    ok = (t > 0) & (np.abs(p[..., 0]) < extent) & (np.abs(p[..., 1]) < extent)
    return np.where(ok, t, np.inf)


SCENES = {
    "plane": lambda C, d: _hit_plane(C, d, (0.2, 0.3, 1.0), 1.2),
    "sphere": lambda C, d: _hit_sphere(C, d, (0.05, -0.03, 0.02), 0.7),
    "boxes": lambda C, d: np.minimum(_hit_box(C, d, (-0.9, -0.4, -0.5), (-0.1, 0.4, 0.3)), _hit_box(C, d, (0.2, -0.6, -0.3), (0.8, 0.1, 0.5))),
}


def render_scene(name, K, E, H, W):
    """-> depth [H,W] fp32 (0 where no hit; the camera-z of the hit), colour [H,W,3] fp32"""
    C, d = _rays(K, E, H, W)
    t = SCENES[name](C, d)
    depth = np.where(np.isfinite(t), t, 0.0).astype(np.float32)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    col = np.stack([0.5 + 0.5 * np.sin(0.15 * u), v / max(H - 1, 1), np.full(u.shape, 0.3)], -1).astype(np.float32)
    return depth, col


def ring_views(n, radius=3.0, height=1.2, seed=0):
    """n camera poses on a ring around the origin, looking at it"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        a = 2 * np.pi * i / n + 0.1 * rng.standard_normal()
        eye = (radius * np.cos(a), radius * np.sin(a), height + 0.3 * rng.standard_normal())
        out.append(look_at(eye, (0.02 * rng.standard_normal(), 0.02 * rng.standard_normal(), 0.0)))
    return out
