"""The cases of the mesh renderer, shared by tests/test_mesh_render_host.py (the kernels through the host emulator) and
tests/test_mesh_render_gpu.py: the scenes of tests/mesh_raster_cases.py and the new ones below, what the product answers for them (run)
and what tests/mesh_render_restatement.py answers (want, computed once per process), compared bit for bit (same)."""
import functools

import numpy as np

import mesh_raster_cases as K
import mesh_render_restatement as RR

# (name, mode, flat, base = the vertex colours): every mode, smooth and flat; the two that read colours only where a scene has them
CONFIGS = (("normal_world", "normal_world", False, False), ("normal_world_flat", "normal_world", True, False),
           ("normal_camera", "normal_camera", False, False), ("normal_camera_flat", "normal_camera", True, False),
           ("shaded", "shaded", False, False), ("shaded_flat", "shaded", True, False),
           ("color", "color", False, False), ("shaded_vertex", "shaded", False, True), ("shaded_vertex_flat", "shaded", True, True))
BASE, AMBIENT, BACKGROUND = (0.8, 0.7, 0.6), 0.25, (1.0, 0.5, 0.25)
W0, H0 = K.SIZES[0]


def configs(colors):
    return [c for c in CONFIGS if colors is not None or c[1] != "color" and not c[3]]


def fan_mesh():
    """70 faces round vertex 0 (a segment longer than a wave), one of them degenerate (a repeated index), the last with a NaN vertex;
    vertex 72 is referenced by no face"""
    ring = [(0.9 * np.cos(2 * np.pi * k / 70), 0.9 * np.sin(2 * np.pi * k / 70), 0.15 * np.sin(7.0 * k)) for k in range(70)]
    V = np.asarray([(0.0, 0.0, 0.3)] + ring + [(np.nan, 0.0, 0.0), (0.5, 0.5, 0.5)], np.float32)
    F = [(0, 1 + k, 1 + (k + 1) % 70) for k in range(69)] + [(0, 71, 70)]
    F[33] = (0, 34, 34)
    return V, np.asarray(F, np.int32)


def closed_mesh():
    """a closed mesh of 220 vertices (the poles repeat) with per-vertex RGBA"""
    V, F = K.sphere(10, 20, 0.9)
    g = np.random.default_rng(11)
    V = (V + g.uniform(-0.03, 0.03, V.shape)).astype(np.float32)
    col = g.integers(0, 256, (len(V), 4)).astype(np.uint8)
    return V, F, col


def scenes(tiling):
    """-> {name: (V, F, views, colours or None)}"""
    S = {k: v + (None,) for k, v in K.scenes(tiling).items()}
    for W, H in K.SIZES:
        p = "%dx%d_" % (W, H)
        pv = K.pixel_views(W, H)
        # two coincident faces with different indices; a face that crosses another along the pixel column 16 (1 / z is linear in the
        # pixel: 1 at x = 0.5, 1/4 at x = 24.5, so 1/2 = the other face's at x = 16.5)
        a, b, c = (4.5, 4.5), (30.5, 4.5), (4.5, 30.5)
        tri = K._at([a, b, c], 2.0)
        tilt = [[(0.5 * 1.0, 2.0 * 1.0, 1.0), (24.5 * 4.0, 2.0 * 4.0, 4.0), (0.5 * 1.0, 40.0 * 1.0, 1.0)], [(24.5 * 4.0, 2.0 * 4.0, 4.0), (24.5 * 4.0, 40.0 * 4.0, 4.0), (0.5 * 1.0, 40.0 * 1.0, 1.0)]]
        S[p + "ties"] = K._mesh(tri + tri + tilt) + (pv, None)
    V, F, col = closed_mesh()
    S["closed"] = (V, F, K.perspective_views(W0, H0, 2), col)
    S["closed_plain"] = (V, F, K.perspective_views(70, 33, 1), None)
    V, F = fan_mesh()
    g = np.random.default_rng(12)
    S["fan"] = (V, F, K.perspective_views(W0, H0, 2), g.integers(0, 256, (len(V), 3)).astype(np.uint8))
    line = np.asarray([(0, 0, 1), (1, 1, 1), (2, 2, 1), (3, 3, 1), (1, 1, 1)], np.float32)
    S["zero_area"] = (line, np.asarray([(0, 1, 2), (1, 2, 3), (0, 4, 1), (2, 2, 2)], np.int32), K.pixel_views(W0, H0), None)
    return S


NEW = ("64x48_ties", "70x33_ties", "closed", "closed_plain", "fan", "zero_area")
KEYS = ("normals", "face_normals", "depth", "face", "bary")


def _kw(views):
    return K._kw(views)


@functools.lru_cache(maxsize=None)
def _want(name, key):
    V, F, views, col = scenes(dict(key))[name]
    recs = K.recs_of(views)
    shape = (views["H"], views["W"])
    depth, face = RR.render_faces(V, F, recs, shape)
    out = {"normals": RR.vertex_normals(V, F), "face_normals": RR.face_normals(V, F), "depth": depth, "face": face}
    for tag, mode, flat, vbase in configs(col):
        img, bary = RR.shade(V, F, recs, face, shape, RR.MODES[mode], normals=out["normals"], colors=col, flat=flat, vertex_base=vbase, base=BASE,
                             ambient=AMBIENT, background=BACKGROUND)
        out["image_" + tag], out["bary"] = img, bary
    return out


def want(name, tiling):
    return _want(name, tuple(sorted(tiling.items())))


def run(MR, M, up, scene, down=lambda t: t.cpu().numpy()):
    """the product's answers for one scene through its Python layer"""
    V, F, views, col = scene
    mesh = M.DeviceMesh.from_device(up(V), up(F), colors=None if col is None else up(col))
    out = {"normals": down(MR.vertex_normals(mesh)), "face_normals": down(MR.face_normals(mesh)), "depth_entry": down(M.render_depth(mesh, views["c2w"], **_kw(views)))}
    for tag, mode, flat, vbase in configs(col):
        img, aux = MR.render(mesh, views["c2w"], mode=mode, flat=flat, base="vertex" if vbase else BASE, ambient=AMBIENT, background=BACKGROUND, aux=True,
                             batch=0 if flat else 2, **_kw(views))
        out["image_" + tag] = down(img)
        for k in ("depth", "face", "bary"):
            a = down(aux[k])
            assert k not in out or np.array_equal(out[k].view(np.uint8), a.view(np.uint8)), (k, tag)      # every mode sees the same buffers
            out[k] = a
    return out


def same(got, wanted, prefix=""):
    """-> the list of what differs, by bit pattern; `depth_entry` (gof_mesh_render_depth) against the face buffer's depth"""
    bad = []
    for k, w in wanted.items():
        g = got.get(k)
        if g is None or g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(g.view(np.uint8), w.view(np.uint8)):
            bad.append(prefix + k)
    if "depth_entry" in got and not np.array_equal(got["depth_entry"].view(np.uint8), wanted["depth"].view(np.uint8)):
        bad.append(prefix + "depth_entry")
    return bad
