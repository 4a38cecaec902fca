"""The cases of the mesh depth rasteriser and visibility cull, shared by tests/test_mesh_raster_host.py (the kernels
through the host emulator) and tests/test_mesh_raster_gpu.py: small scenes, what the product answers for them (run) and what
tests/mesh_raster_restatement.py answers (want, computed once per process), compared bit for bit (same).

Two cameras.  PIXEL: the identity pose in the OpenCV convention with fx = fy = 1, cx = cy = 0, so a vertex (x, y, 1) lies at pixel
coordinates (x, y) exactly and the coverage cases are written in pixels.  PERSPECTIVE: a pinhole in front of the scene."""
import functools

import numpy as np

import mesh_raster_restatement as R

SIZES = ((64, 48), (70, 33))           # (W, H); 70 is no multiple of the wave, 33 none of the tile
EPS = 0.005
CULL_EPS = 0.05         # the culled scene: at 64 x 48 the half pixel between render and sample is worth more depth than the script's 0.005


def pixel_views(W, H, n=1, zfar=20.0):
    return dict(c2w=[np.eye(4) for _ in range(n)], H=H, W=W, fx=1.0, fy=1.0, cx=0.0, cy=0.0, znear=0.01, zfar=zfar, convention="opencv")


def orbit(n, radius=3.0, height=0.6):
    """n OpenGL camera-to-world matrices on a circle, looking at the origin"""
    out = []
    for k in range(n):
        a = 2 * np.pi * k / max(n, 1) + 0.3
        eye = np.array([radius * np.cos(a), height * np.sin(3 * a), radius * np.sin(a)])
        back = eye / np.linalg.norm(eye)                      # the camera looks down -z
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, eye
        out.append(m.astype(np.float32).astype(np.float64))
    return out


def perspective_views(W, H, n, **kw):
    return dict(dict(c2w=orbit(n), H=H, W=W, fx=0.9 * W, fy=0.9 * W, cx=W / 2 - 0.3, cy=H / 2 + 0.2, znear=0.01, zfar=20.0, convention="opengl"), **kw)


def _mesh(tris):
    V = np.asarray(tris, np.float32).reshape(-1, 3)
    return V, np.arange(len(V), dtype=np.int32).reshape(-1, 3)


def _at(points, z=1.0):
    return [[(x * z, y * z, z) for x, y in points]]


def sphere(n_lat, n_lon, radius=1.0, centre=(0, 0, 0)):
    V, F = [], []
    for i in range(n_lat + 1):
        for j in range(n_lon):
            t, p = np.pi * i / n_lat, 2 * np.pi * j / n_lon
            V.append((radius * np.sin(t) * np.cos(p) + centre[0], radius * np.cos(t) + centre[1], radius * np.sin(t) * np.sin(p) + centre[2]))
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = i * n_lon + j, i * n_lon + (j + 1) % n_lon, (i + 1) * n_lon + j, (i + 1) * n_lon + (j + 1) % n_lon
            F += [(a, b, c), (b, d, c)]
    return np.asarray(V, np.float32), np.asarray(F, np.int32)


def soup(n, seed, spread=1.0, size=0.5):
    g = np.random.default_rng(seed)
    c = g.uniform(-spread, spread, (n, 1, 3))
    return _mesh((c + g.uniform(-size, size, (n, 3, 3))).reshape(-1, 3, 3))


def scenes(tiling):
    """-> {name: (V, F, views)}; `tiling` = mesh_cull.raster_tiling() (the threshold cases sit at its sizes)"""
    t = tiling["inline_max"]
    S = {}
    for W, H in SIZES:
        p = "%dx%d_" % (W, H)
        pv = pixel_views(W, H)
        # a quad whose diagonal runs through pixel centres, in two triangles; and its mirror image (the other diagonal, the other winding)
        q = [(2, 2), (30, 2), (30, 30), (2, 30)]
        S[p + "quad"] = _mesh(_at([q[0], q[1], q[2]]) + _at([q[0], q[2], q[3]])) + (pv,)
        S[p + "quad_other"] = _mesh(_at([q[1], q[0], q[3]]) + _at([q[3], q[2], q[1]])) + (pv,)
        # a vertex and edges exactly on pixel centres, both windings, and the neighbour across the hypotenuse
        a, b, c, d = (4.5, 4.5), (20.5, 4.5), (4.5, 20.5), (20.5, 20.5)
        S[p + "on_centres"] = _mesh(_at([a, b, c])) + (pv,)
        S[p + "on_centres_flipped"] = _mesh(_at([a, c, b])) + (pv,)
        S[p + "on_centres_pair"] = _mesh(_at([a, b, c], 1.0) + _at([b, d, c], 2.0)) + (pv,)
        # below a pixel: no centre covered (four of them), one centre covered (the fifth)
        tiny = [[(x + 0.05, y + 0.05), (x + 0.45, y + 0.1), (x + 0.1, y + 0.45)] for x, y in ((3, 3), (10, 7), (11.5, 7.5), (W - 1, H - 1))] + [[(8.3, 9.3), (8.8, 9.4), (8.4, 9.9)]]
        S[p + "subpixel"] = _mesh([_at(tri)[0] for tri in tiny]) + (pv,)
        S[p + "whole_image"] = _mesh(_at([(-10, -10), (3 * W, -10), (-10, 3 * H)], 2.0)) + (pv,)
        # boxes of pixel centres just below, at and just above the threshold, and at and above one and two tiles
        boxes, x = [], 1.25
        for k, n in enumerate((t - 1, t, t + 1, tiling["tile_w"], tiling["tile_w"] + 1, 2 * tiling["tile_w"] + 1)):
            boxes += _at([(x, 3.25), (x + n, 3.25), (x, 3.25 + n)], 1.0 + k)
            x += n + 1
        S[p + "threshold"] = _mesh(boxes) + (pv,)
        # the far plane: exactly at it (kept), one float above (gone), across it (cut along the plane)
        S[p + "zfar"] = _mesh(_at([(2, 2), (12, 2), (2, 12)], 20.0) + _at([(14, 2), (24, 2), (14, 12)], float(np.nextafter(np.float32(20), np.float32(30))))
                              + [[(26.0 * 15, 2.0 * 15, 15.0), (40.0 * 25, 2.0 * 25, 25.0), (26.0 * 15, 20.0 * 15, 15.0)]]) + (pv,)
        # far outside the guard band, up to the largest float
        big = float(np.finfo(np.float32).max)
        S[p + "outside_guard"] = _mesh(_at([(5, 5), (1e7, 6), (5, 1e7)], 1.0) + _at([(-1e30, 10), (1e30, 11), (20, 1e30)], 2.0) + _at([(-big, -big), (big, -big), (12.25, big)], 0.5)
                                       + _at([(-big, 40), (big, 40.5), (-big, big)], 0.25)) + (pv,)
        # degenerate: repeated indices, collinear and coincident vertices, beside a proper face
        V = np.asarray([(3, 3, 1), (20, 3, 1), (3, 20, 1), (10, 10, 1), (30, 30, 1), (10, 10, 1)], np.float32)
        S[p + "degenerate"] = (V, np.asarray([(0, 0, 1), (2, 2, 2), (0, 3, 4), (3, 5, 1), (0, 1, 2), (1, 0, 1)], np.int32), pv)
        # NaN and Inf vertices: their faces vanish, the others stay
        V = np.asarray([(3, 3, 1), (20, 3, 1), (3, 20, 1), (np.nan, 5, 1), (np.inf, 5, 1), (5, 5, -np.inf), (25, 25, 2), (40, 25, 2), (25, 31, 2)], np.float32)
        S[p + "nonfinite"] = (V, np.asarray([(0, 1, 3), (0, 4, 2), (5, 1, 2), (6, 7, 8), (0, 1, 2)], np.int32), pv)
        S[p + "nothing"] = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), pv)
        S[p + "no_faces"] = (np.asarray([(3, 3, 1), (5, 5, 1)], np.float32), np.zeros((0, 3), np.int32), pv)
        S[p + "no_views"] = _mesh(_at([a, b, c])) + (pixel_views(W, H, 0),)
        # the near plane: one vertex behind, two behind, all behind, and a fan of faces around an edge that crosses it
        pp = perspective_views(W, H, 1, c2w=[np.eye(4)], convention="opencv")
        near = [[(-0.3, -0.2, 1.0), (0.3, -0.2, 1.0), (0.0, 0.1, -1.0)], [(-0.3, 0.25, 1.5), (0.0, 0.2, -0.5), (0.3, 0.25, -2.0)], [(0, 0, -1.0), (1, 0, -1.0), (0, 1, -2.0)]]
        S[p + "near"] = _mesh(near) + (pp,)
        V = np.asarray([(0.0, 0.0, 1.2), (0.02, 0.01, -0.7), (-0.5, -0.3, 0.6), (0.5, -0.35, 0.5), (0.45, 0.3, 0.7), (-0.4, 0.35, 0.4)], np.float32)
        S[p + "near_fan"] = (V, np.asarray([(0, 1, 2), (1, 0, 3), (0, 1, 4), (5, 1, 0)], np.int32), pp)
        # more views than one batch holds: a sphere in front of a soup, 7 views in batches of 3
        Vs, Fs = sphere(6, 8, 0.8)
        Vb, Fb = soup(24, 5, 1.0, 0.6)
        S[p + "views"] = (np.concatenate([Vs, Vb]), np.concatenate([Fs, Fb + len(Vs)]), perspective_views(W, H, 7))
    return S


BATCH = 3


def recs_of(views):
    return R.records(views["c2w"], views["H"], views["W"], views["fx"], views["fy"], views["cx"], views["cy"], views["znear"], views["zfar"], views["convention"])


@functools.lru_cache(maxsize=None)
def _want(name, key):
    V, F, views = scenes(dict(key))[name]
    recs = recs_of(views)
    depth = R.render_depth(V, F, recs, (views["H"], views["W"]))
    count = R.visible_count(V, recs, depth, EPS)
    return {"depth": depth, "count": count}


def want(name, tiling):
    return _want(name, tuple(sorted(tiling.items())))


def _kw(views):
    return dict(H=views["H"], W=views["W"], fx=views["fx"], fy=views["fy"], cx=views["cx"], cy=views["cy"], znear=views["znear"], zfar=views["zfar"],
                convention=views["convention"])


def run(M, up, scene, down=lambda t: t.cpu().numpy()):
    """the product's answers for one scene: render_depth, visible_count against those images, and the batched driver"""
    V, F, views = scene
    mesh = M.DeviceMesh.from_device(up(V), up(F))
    depth = M.render_depth(mesh, views["c2w"], **_kw(views))
    count = M.visible_count(up(V), views["c2w"], depth=depth, eps=EPS, **_kw(views))
    count2, keep = M.visibility(mesh, views["c2w"], eps=EPS, min_views=1, batch=BATCH, **_kw(views))
    return {"depth": down(depth), "count": down(count), "driver_count": down(count2), "driver_keep": down(keep)}


def same(got, wanted, prefix=""):
    """-> the list of what differs (bit patterns for the depth)"""
    bad = []
    if got["depth"].shape != wanted["depth"].shape or not np.array_equal(got["depth"].view(np.uint32), wanted["depth"].view(np.uint32)):
        bad.append(prefix + "depth")
    for k in ("count", "driver_count"):
        if not np.array_equal(got[k], wanted["count"]):
            bad.append(prefix + k)
    if not np.array_equal(got["driver_keep"], wanted["count"] >= 1):
        bad.append(prefix + "driver_keep")
    return bad


# ---- the mesh that is culled -----------------------------------------------------------------------------------------------------------
def cull_scene(W=64, H=48):
    """a sphere hidden behind a larger open shell for most cameras, with normals and colours -> (V, F, N, Col, views)"""
    Vs, Fs = sphere(7, 10, 0.5)
    Vo, Fo = sphere(6, 9, 1.2)
    Fo = Fo[: len(Fo) * 2 // 3]                                   # the shell is open below: some cameras see inside
    V = np.concatenate([Vs, Vo])
    F = np.concatenate([Fs, Fo + len(Vs)])
    g = np.random.default_rng(3)
    N = g.standard_normal((len(V), 3)).astype(np.float32)
    Col = g.integers(0, 256, (len(V), 3)).astype(np.uint8)
    return V, F, N, Col, perspective_views(W, H, 9)
