"""Writes tests/golden/tnt_cull_scene.npz: the reference's own Mesher.point_masks (eval_tnt/cull_mesh.py:117-175) on a small scene.

    python tests/golden/make_golden_tnt_cull.py /path/to/gaussian-opacity-fields

Runs on the CPU.  The reference's eval_tnt/cull_mesh.py is imported as it is, with this package's import stand-ins for pyrender, open3d,
trimesh and cv2 where they are missing, and Mesher.device = 'cpu'.  point_masks is fed the depth images of
tests/mesh_raster_restatement.py for 24 views at 64 x 48 of a mesh of about 2 000 vertices; the file holds the inputs,
those depth images, the reference's mask and `decided`: the vertices on which an fp64 evaluation must agree with the reference's
float32 one.  The file holds data only.

decided.  The reference evaluates the test in float32: the inverse of the pose, the transform, K, the division, grid_sample's
normalisation of u and v and its weights.  Fewer than OPS = 32 roundings lie between the inputs and any compared quantity, each of
relative size U = 2^-24, so with S the largest magnitude that enters (the scene's camera-space coordinates, bounded by ZMAX)
  u, v carry at most T_UV = OPS * U * max(W, H) pixels,
  z and the sampled depth at most OPS * U * (|z| + |ds|), and the sample moves with u, v by at most T_UV * 2 * (largest - smallest of
  the four texels) more.
A view is in doubt for a vertex when u or v lies within T_UV of a frustum bound, z within OPS * U * |z| of 0, or |z - (ds + eps)| within
that depth threshold (or ds within it of 0).  A vertex is decided when, with n the fp64 count of the views that are not in doubt and
m the number in doubt, n >= MIN_VIEWS (kept whatever the doubtful views say) or n + m < MIN_VIEWS (dropped).  The generator fails
unless the reference's mask equals the fp64 one on every decided vertex and at most 2 % of the vertices are undecided."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
PKG = os.path.join(os.path.dirname(TESTS), "gaussian-opacity-fields_amd")
sys.path[:0] = [TESTS, PKG]

import mesh_raster_cases as K  # noqa: E402
import mesh_raster_restatement as R  # noqa: E402

W, H, VIEWS, MIN_VIEWS, EPS = 64, 48, 24, 20, 0.005
OPS, U = 32, 2.0 ** -24
OUT = os.path.join(HERE, "tnt_cull_scene.npz")


def scene():
    """two spheres, one partly behind the other, seen from an arc of cameras on one side.  The scene is small (a pixel is worth about
    0.0025 of depth, half the script's eps): at 64 x 48 the half pixel between the render and the sample would otherwise drop nearly everything"""
    Va, Fa = K.sphere(20, 50, 0.035, (-0.0175, 0.0, 0.0))
    Vb, Fb = K.sphere(18, 50, 0.0275, (0.0275, 0.005, -0.025))
    V, F = np.concatenate([Va, Vb]), np.concatenate([Fa, Fb + len(Va)])
    c2w = []
    for k in range(VIEWS):
        a = np.deg2rad(65.0 + 50.0 * k / (VIEWS - 1))
        eye = np.array([0.15 * np.cos(a), 0.025 * np.sin(9 * a), 0.15 * np.sin(a)])
        back = eye / np.linalg.norm(eye)
        right = np.cross([0.0, 1.0, 0.0], back)
        right /= np.linalg.norm(right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, np.cross(back, right), back, eye
        c2w.append(m.astype(np.float32))
    return V, F, np.stack(c2w), dict(fx=0.95 * W, fy=0.95 * W, cx=W / 2 - 0.4, cy=H / 2 + 0.3)


def decided_vertices(V, recs, depth):
    """-> (count fp64 restatement, decided (NV,) bool, thresholds)"""
    t_uv = OPS * U * max(W, H)
    count = np.zeros(len(V), int)
    sure = np.zeros(len(V), int)
    doubt = np.zeros(len(V), int)
    for r, d in zip(recs, depth):
        for i, v in enumerate(V):
            x, y, Z = R.camera(r, v)
            z = Z + 1e-8
            u, w = (r["fx"] * x + r["cx"] * Z) / z, (r["fy"] * y + r["cy"] * Z) / z
            seen, info = R.view_sees(r, d, v, EPS)
            count[i] += seen
            t_z = OPS * U * abs(z)
            in_doubt = abs(z) <= t_z or min(abs(u), abs(u - (W - 1)), abs(w), abs(w - (H - 1))) <= t_uv
            if info is not None:
                ds = info[3]
                x0, y0 = int(np.floor(info[0])), int(np.floor(info[1]))
                tex = d[y0:y0 + 2, x0:x0 + 2].astype(np.float64)
                t_d = OPS * U * (abs(z) + abs(ds)) + t_uv * 2.0 * float(tex.max() - tex.min())
                in_doubt = in_doubt or abs(ds) <= t_d or abs(z - (ds + EPS)) <= t_d
            doubt[i] += in_doubt
            sure[i] += seen and not in_doubt
    return count, (sure >= MIN_VIEWS) | (sure + doubt < MIN_VIEWS), dict(t_uv=t_uv, ops=OPS, unit=U)


def reference_module(root):
    for shim in (os.path.join(PKG, "shims"), os.path.join(PKG, "shims_dtu", "trimesh"), os.path.join(PKG, "shims_dtu", "cv2")):
        sys.path.append(shim)                     # last: an installed package wins
    sys.path.insert(0, os.path.join(root, "eval_tnt"))
    spec = importlib.util.spec_from_file_location("reference_cull_mesh", os.path.join(root, "eval_tnt", "cull_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(root):
    import torch
    V, F, c2w, k = scene()
    recs = R.records(list(c2w), H, W, k["fx"], k["fy"], k["cx"], k["cy"])
    depth = R.render_depth(V, F, recs)
    ref = reference_module(root)
    mesher = ref.Mesher(H, W, k["fx"], k["fy"], k["cx"], k["cy"], 20.0, points_batch_size=5e5)
    mesher.device = "cpu"
    mask, _ = mesher.point_masks(V.copy(), [torch.from_numpy(d.copy()) for d in depth], [torch.from_numpy(m.copy()) for m in c2w])
    count, decided, thr = decided_vertices(V, recs, depth)
    keep = count >= MIN_VIEWS
    share = 1.0 - decided.mean()
    print("vertices %d, faces %d, kept by the reference %d, by fp64 %d, undecided %d (%.2f %%), thresholds %s" % (len(V), len(F), mask.sum(), keep.sum(), (~decided).sum(), 100 * share, thr))
    assert min(mask.sum(), (~mask).sum()) >= 100, "the scene must keep a hundred vertices and drop a hundred, or one answer passes"
    assert np.array_equal(mask[decided], keep[decided]), "the reference and the fp64 restatement disagree on a decided vertex"
    assert share <= 0.02, "more than 2 % of the vertices are undecided"
    np.savez_compressed(OUT, vertices=V, faces=F, c2w=c2w, depth=depth, mask=mask, decided=decided, count=count.astype(np.int32), H=H, W=W, min_views=MIN_VIEWS,
                        eps=EPS, t_uv=thr["t_uv"], ops=OPS, unit=U, **k)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
