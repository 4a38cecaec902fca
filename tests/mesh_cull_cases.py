"""The case tables of the mesh culling tests, shared by the CPU suite (test_mesh_cull_host.py: the kernels through the
host emulator) and the GPU suite (test_mesh_cull_gpu.py: the real library).  run(M, up, case) drives mesh_cull's Python layer and
returns numpy arrays, want(case) is what tests/mesh_cull_restatement.py says they must be -- the tests compare the two with equalities.
Test infrastructure only."""
import numpy as np

import mesh_cull_restatement as R

RADII = (0, 1, 6, 31)
SIZES = ((1, 1), (63, 13), (64, 13), (65, 13), (161, 120), (130, 7))          # (W, H)


# ---- dilation ------------------------------------------------------------------------------------------------------------------------
def dilate_masks(W, H):
    """-> [(name, mask (H,W) float32 or uint8)]"""
    rng = np.random.default_rng(1000 * W + H)
    out = [("empty", np.zeros((H, W), np.float32)), ("full", np.ones((H, W), np.float32))]
    for name, (y, x) in (("corner00", (0, 0)), ("corner0w", (0, W - 1)), ("cornerh0", (H - 1, 0)), ("cornerhw", (H - 1, W - 1))):
        m = np.zeros((H, W), np.float32)
        m[y, x] = 1.0
        out.append((name, m))
    for x in (63, 64, 127, 128):
        if x < W:
            m = np.zeros((H, W), np.float32)
            m[H // 2, x] = 0.5
            out.append(("x%d" % x, m))
    out.append(("random", ((rng.random((H, W)) < 0.01) * rng.uniform(0.1, 1.0, (H, W))).astype(np.float32)))
    out.append(("random_u8", ((rng.random((H, W)) < 0.01) * rng.integers(1, 256, (H, W))).astype(np.uint8)))
    # values below 1 / 256 (and far below) that are still non-zero after the division by 256: set pixels
    out.append(("tiny", ((rng.random((H, W)) < 0.01) * rng.choice(np.array([1e-3, 3.9e-3, 1e-20, -1e-30], np.float32), (H, W))).astype(np.float32)))
    return out


def run_dilate(M, up, size):
    W, H = size
    res = {}
    for name, m in dilate_masks(W, H):
        for r in RADII:
            res["%s_r%d" % (name, r)] = M.dilate_mask(up(m), r).cpu().numpy().view(np.uint64)
    return res


def want_dilate(size):
    W, H = size
    return {"%s_r%d" % (name, r): R.pack(R.dilate(m, r)) for name, m in dilate_masks(W, H) for r in RADII}


# ---- culling -------------------------------------------------------------------------------------------------------------------------
def ring_views(n, sizes, seed, r=6):
    """n cameras on a ring of radius 3 looking at the origin, image sizes taken in turn from `sizes` -> [(m, W, H, mask (H,W) float32)]"""
    rng = np.random.default_rng(seed)
    views = []
    for i in range(n):
        W, H = sizes[i % len(sizes)]
        a = 2 * np.pi * i / max(n, 1) + 0.1
        C = np.array([3 * np.cos(a), 0.3 * np.sin(2 * a), 3 * np.sin(a)])
        zc = -C / np.linalg.norm(C)
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        w2c = np.eye(4)
        w2c[:3, :3] = np.stack([xc, np.cross(zc, xc), zc])
        w2c[:3, 3] = -w2c[:3, :3] @ C
        yy, xx = np.mgrid[0:H, 0:W]
        disc = (xx - W / 2.0) ** 2 + (yy - H / 2.0) ** 2 <= (0.3 * H + i % 5) ** 2
        mask = ((disc | (rng.random((H, W)) < 0.001)) * rng.uniform(0.2, 1.0, (H, W))).astype(np.float32)
        views.append((R.view_matrix(0.95 * W + i % 3, 0.93 * W, W, H, w2c.T), W, H, mask))
    return views


def _unit_depth_constant():
    """c with c + 1e-6 == 1.0 exactly in fp64"""
    c = 1.0 - 1e-6
    for _ in range(8):
        if c + 1e-6 == 1.0:
            return c
        c = np.nextafter(c, 2.0 if c + 1e-6 < 1.0 else 0.0)
    raise AssertionError("no fp64 c with c + 1e-6 == 1")


def edge_scene():
    """129 x 65 images (W - 1 and H - 1 powers of two: every operation of the contract is exact for the coordinates below).
    view A: x = vx, y = vy, d = 1 exactly: vertices on px, py = -1 and 1 (not valid: kept), on every .5 pixel tie (ties to even), next
    to them; view B: d = vz + 1e-6 with vertices behind the camera; view C: d = z + 1e-6 == 0 for every vertex (x / 0: kept).
    The mask is a random half of the pixels, not dilated, so that rounding a tie the wrong way changes the answer.
    -> (vertices (N,3) float32, [views A, B, C])"""
    W, H = 129, 65
    rng = np.random.default_rng(77)
    mask = (rng.random((H, W)) < 0.5).astype(np.float32)
    c = _unit_depth_constant()
    A = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, c]])
    B = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    Cm = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, -1e-6]])
    f32 = np.float32
    xs = np.concatenate([[0.0, 128.0, -0.0], np.arange(128) + 0.5, np.nextafter(f32(0), f32(1), dtype=f32)[None], np.nextafter(f32(128), f32(0), dtype=f32)[None],
                         np.nextafter((np.arange(128) + 0.5).astype(f32), f32(0)), np.nextafter((np.arange(128) + 0.5).astype(f32), f32(200)), [-3.0, 200.0]])
    ys = np.concatenate([[0.0, 64.0], np.arange(64) + 0.5, [31.0, 32.25, -1.0, 70.0]])
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    V = np.stack([gx.reshape(-1), gy.reshape(-1), np.ones(gx.size)], -1)
    # behind the camera (view B), at d == 0 for B up to rounding, non-finite
    extra = np.array([[40.0, 20.0, -1.0], [-40.0, -20.0, -1.0], [-40.5, -20.5, -1.0], [10.0, 10.0, -1e-6], [0.0, 0.0, 0.0], [5.0, 5.0, 0.0],
                      [np.nan, 1.0, 1.0], [1.0, np.nan, 1.0], [1.0, 1.0, np.nan], [np.inf, 1.0, 1.0], [1.0, -np.inf, 1.0], [1.0, 1.0, np.inf], [np.nan] * 3])
    V = np.vstack([V, extra]).astype(np.float32)
    return V, [(A, W, H, mask), (B, W, H, mask), (Cm, W, H, mask)]


def golden_views(g, r=6):
    return [(R.view_matrix(g["focal"][i, 0], g["focal"][i, 1], g["W"], g["H"], g["world_view_transform"][i]), int(g["W"]), int(g["H"]), g["masks"][i, 0])
            for i in range(len(g["masks"]))]


def cull_case(name, golden=None):
    """-> (vertices float32, views [(m, W, H, mask)], radius, list of view subsets to run)"""
    if name == "golden":
        return np.asarray(golden["vertices"], np.float32), golden_views(golden), 6, [list(range(8))]
    if name == "edges":
        V, views = edge_scene()
        return V, views, 0, [[0], [1], [2], [0, 1, 2]]
    if name == "counts":
        V = np.random.default_rng(5).uniform(-1.2, 1.2, (3000, 3)).astype(np.float32)
        return V, ring_views(70, ((161, 120), (64, 48)), 6), 6, [[], [3], list(range(70))]
    raise KeyError(name)


def run_cull(M, up, name, golden=None):
    V, views, r, subsets = cull_case(name, golden)
    packed = [M.dilate_mask(up(m), r) for _, _, _, m in views]
    v = up(V)
    return {"keep%d" % k: M.cull_vertices(v, [(views[i][0], views[i][1], views[i][2], packed[i]) for i in sub]).cpu().numpy() for k, sub in enumerate(subsets)}


def want_cull(name, golden=None):
    V, views, r, subsets = cull_case(name, golden)
    dil = [R.dilate(m, r) for _, _, _, m in views]
    return {"keep%d" % k: R.cull(V, [(views[i][0], views[i][1], views[i][2], dil[i]) for i in sub]) for k, sub in enumerate(subsets)}


# ---- compaction ----------------------------------------------------------------------------------------------------------------------
COMPACT_NV = (0, 1, 1023, 1024, 1025, 70001)


def compact_case(nv, pattern):
    rng = np.random.default_rng(nv * 7 + len(pattern))
    keep = {"all": np.ones(nv, bool), "none": np.zeros(nv, bool), "half": rng.random(nv) < 0.5}[pattern]
    faces = rng.integers(0, max(nv, 1), (2 * nv, 3)).astype(np.int32)
    V = rng.normal(size=(nv, 3))
    N = rng.normal(size=(nv, 3)).astype(np.float32)
    C = rng.integers(0, 256, (nv, 4)).astype(np.uint8)
    return keep, faces, V, N, C


def run_compact(M, up, nv):
    res = {}
    for pattern in ("all", "none", "half"):
        keep, faces, V, N, C = compact_case(nv, pattern)
        for tag, attrs in (("attrs", (V, N, C)), ("plain", ())):
            out = M.compact_mesh(up(keep), up(faces), [up(a) for a in attrs])
            p = "%s_%s_" % (pattern, tag)
            res[p + "rows"], res[p + "faces"], res[p + "face_keep"] = out["rows"].cpu().numpy(), out["faces"].cpu().numpy(), out["face_keep"].cpu().numpy()
            for i, a in enumerate(out["attrs"]):
                res[p + "attr%d" % i] = a.cpu().numpy()
        res[pattern + "_faces_all"] = M.compact_mesh(up(keep), up(faces), drop_faces=False)["faces"].cpu().numpy()
    return res


def want_compact(nv):
    res = {}
    for pattern in ("all", "none", "half"):
        keep, faces, V, N, C = compact_case(nv, pattern)
        for tag, attrs in (("attrs", (V, N, C)), ("plain", ())):
            out = R.compact(keep, faces, attrs=attrs)
            p = "%s_%s_" % (pattern, tag)
            res[p + "rows"], res[p + "faces"], res[p + "face_keep"] = out["rows"], out["faces"], out["face_keep"]
            for i, a in enumerate(out["attrs"]):
                res[p + "attr%d" % i] = a
        res[pattern + "_faces_all"] = R.compact(keep, faces)["faces_all"]
    return res


def same(got, want):
    """every array of `want` is in `got` with the same shape, type and bytes (NaN payloads included) -> list of the names that differ"""
    bad = []
    for k, w in want.items():
        g = got.get(k)
        w = np.ascontiguousarray(w)
        if g is None or g.shape != w.shape or g.dtype != w.dtype or np.ascontiguousarray(g).tobytes() != w.tobytes():
            bad.append(k)
    return bad
