"""CPU tests of the Tanks-and-Temples F-score evaluation: the kernels of csrc/cloud_reg.hip (and cloud.hip's
nearest-neighbour index) through the host emulator (tests/hipemu) behind tnt_eval's own Python layer, each run in a child process,
held to tests/tnt_eval_restatement.py with equalities: kept rows, voxel means, the 16 correspondence sums and the F-score integers
bit for bit.

In the child the product modules run unchanged except for the test seams of tests/test_mesh_eval_host.py: GOF_HIP_LIB names the
emulated library, the device check / stream / device context are replaced by host stand-ins, and every workspace is filled with
0xA5 and followed by guard bytes that are checked after the run.  Sizes stay at or below 50 k points per case."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import host_child  # noqa: E402
from host_child import PKG  # noqa: E402
import tnt_eval_restatement as R  # noqa: E402

TAU = 0.5


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def surface(n, seed):
    """n points of a closed surface without any symmetry (a torus whose two radii, height and aspect vary with the angle)"""
    rng = np.random.default_rng(seed)
    u, v = rng.random(n) * 2 * np.pi, rng.random(n) * 2 * np.pi
    R0 = 20 + 3 * np.sin(3 * u + 0.3)
    r0 = 6 + 2 * np.cos(u) + 1.5 * np.sin(2 * u + 0.7)
    return np.stack([(R0 + r0 * np.cos(v)) * np.cos(u), 0.8 * (R0 + r0 * np.cos(v)) * np.sin(u), r0 * np.sin(v) + 2 * np.cos(u)], -1)


def similarity_matrix(scale, degrees, axis, translation):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.radians(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rm = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    M = np.eye(4)
    M[:3, :3] = scale * Rm
    M[:3, 3] = translation
    return M


KNOWN = similarity_matrix(1.03, 3.0, [0.3, -0.5, 0.8], [0.8, -0.5, 0.4])      # maps the source's frame onto the target's


def volume_for(axis=2):
    """a concave polygon around the surface (it cuts a part of it off) with the slab along `axis`; the polygon's coordinates along
    the orthogonal axis are junk on purpose"""
    uv = np.array([[-34, -27], [0, -21.5], [33, -28], [36, 4], [31, 27], [3, 24.5], [-12, 12], [-33, 26], [-29.5, 0]], np.float64)
    poly = np.zeros((len(uv), 3))
    poly[:, (axis + 1) % 3], poly[:, (axis + 2) % 3], poly[:, axis] = uv[:, 0], uv[:, 1], 1e3
    return {"axis": axis, "axis_min": -12.0, "axis_max": 100.0, "polygon": poly}


def registration_case(n_target=40000, n_source=30000, seed=11, n_far=None):
    """-> (source in its own frame, target): the source is a second sampling of the surface with noise, a patch of far outliers
    (beyond every threshold) and a set of points lifted off the surface by 0.3 .. 14 (the masks of stages 2 and 3 bite), moved by the
    inverse of KNOWN.  n_far: the size of the far patch (a kd-tree answers a query that is about equally far from the whole target
    by visiting most of it, so the large cases keep the patch small)"""
    rng = np.random.default_rng(seed)
    target = surface(n_target, seed)
    n_far, n_off = (n_source // 60 if n_far is None else n_far), n_source // 20
    s = surface(n_source - n_far - n_off, seed + 1)
    off = surface(n_off, seed + 2)
    off[:, 2] += rng.uniform(0.3, 14.0, n_off) * np.where(rng.random(n_off) < 0.5, -1.0, 1.0)
    far = rng.normal(size=(n_far, 3)) + [3.0, -2.0, 78.0]
    q = np.vstack([s, off, far])[rng.permutation(n_source)]
    q = q + rng.normal(scale=0.05, size=q.shape)
    return R.transform(q, np.linalg.inv(KNOWN)), target


def crop_case(name):
    """-> (points, volume, transformation or None)"""
    kind, axis, tr = name.split("_")
    axis = "xyz".index(axis)
    rng = np.random.default_rng(5 + axis)
    if kind == "empty":
        return np.zeros((0, 3)), volume_for(axis), None
    vol = volume_for(axis)
    if kind == "circle":                                        # the largest polygon the kernel takes: 4096 vertices = 64 KB of LDS
        a = np.arange(4096) * (2 * np.pi / 4096)
        poly = np.zeros((4096, 3))
        poly[:, (axis + 1) % 3], poly[:, (axis + 2) % 3], poly[:, axis] = 30 * np.cos(a) + 2, 26 * np.sin(a) - 1, -7.0
        vol["polygon"] = poly
    if kind == "nopoly":
        vol["polygon"] = np.zeros((0, 3))
    P = rng.random((20000, 3)) * 90 - 45
    ua, va = (axis + 1) % 3, (axis + 2) % 3
    # points exactly on the two faces of the slab (kept), just outside them, and on the height of polygon vertices
    special = np.zeros((8, 3))
    special[:, ua], special[:, va] = [0, 0, 0, 0, -20, 10, 20, -31], [0, 0, 0, 0, -21.5, -21.5, 4, 0]
    special[:, axis] = [-12.0, 100.0, np.nextafter(-12.0, -np.inf), np.nextafter(100.0, np.inf), 0, 0, 0, 0]
    P = np.vstack([special, P])
    P[8:, axis] = rng.random(20000) * 130 - 20
    M = None
    if tr == "moved":
        M = similarity_matrix(0.97, 11.0, [0.2, 0.9, -0.4], [1.5, -2.0, 0.7])
        P[:8] = R.transform(special, np.linalg.inv(M))          # (no longer exact: ordinary points)
    return np.ascontiguousarray(P), vol, M


def voxel_case(name):
    """-> (points, voxel)"""
    rng = np.random.default_rng(13)
    if name in ("n0", "n1"):
        return np.zeros((int(name[1]), 3)) + 0.25, 0.5
    if name == "straddle":                                       # the 63-bit key sort where its two words disagree
        from mesh_eval_restatement import straddle_cloud
        return straddle_cloud(), 0.5
    if name == "surface":
        return surface(40000, 3), 0.5
    if name == "one":
        return rng.random((3000, 3)) * 0.2 + 5.0, 0.5
    if name == "lattice":
        g = np.arange(20, dtype=np.float64) * 0.25               # binary-exact multiples of v / 2 and of v
        L = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return L[rng.permutation(len(L))], 0.5
    if name == "skew":                                           # one voxel with 12 000 points among 10 000 voxels with one
        g = np.stack(np.meshgrid(np.arange(25.0), np.arange(20.0), np.arange(20.0), indexing="ij"), -1).reshape(-1, 3) * 2.0 + 0.3
        big = rng.random((12000, 3)) * 0.4 + [60.1, 7.1, 7.1]
        P = np.vstack([g, big])
        return P[rng.permutation(len(P))], 0.5
    raise KeyError(name)


def sums_case(name):
    """-> (source, target, threshold)"""
    src, tgt = registration_case(20000, 15001 if name != "pow2" else 16384)
    src = R.transform(src, KNOWN @ similarity_matrix(1.01, 1.0, [0, 0, 1], [0.1, 0.05, -0.1]))
    if name == "torus":
        return src, tgt, 1.0
    if name == "pow2":
        return src, tgt, 1.0
    if name == "ragged":
        return src[:1000 + 77], tgt, 1.0
    if name == "n0":
        return src[:3000], tgt, 1e-9
    if name == "n1":
        s = src[:3000] + [0.0, 0.0, 500.0]
        s[1234] = tgt[17] + [0.01, 0.0, 0.0]
        return s, tgt, 1.0
    if name == "single":
        return tgt[5:6] + 0.01, tgt, 1.0
    raise KeyError(name)


def trajectory_case(displaced=0.0, n=200, seed=4):
    """-> (estimated centres, reference centres, gt_trans, mask of the displaced ones)"""
    rng = np.random.default_rng(seed)
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    gt = np.stack([4 * np.cos(a), 3 * np.sin(a), 0.5 * np.sin(3 * a) + 0.2 * a], -1)
    gt_trans = similarity_matrix(1.0, 25.0, [0.1, 0.2, 1.0], [0.5, 1.0, -0.3])
    est = R.transform(R.transform(gt, gt_trans), np.linalg.inv(similarity_matrix(2.5, -40.0, [1.0, 0.3, 0.2], [3.0, 0.0, 1.0])))
    bad = np.zeros(n, bool)
    if displaced:
        bad[rng.permutation(n)[:int(displaced * n)]] = True
        est[bad] += rng.normal(size=(int(bad.sum()), 3)) * 5 + 10
    return est, gt, gt_trans, bad


def write_scene(root, scene="Barn"):
    """a synthetic scene directory in TNT's layout -> dict(dir, mesh, traj, source vertices + centroids, target, ...)"""
    import mesh_eval
    d = os.path.join(root, scene)
    os.makedirs(d, exist_ok=True)
    tau = 0.01
    k = tau / TAU                                                # the registration case scaled so that the scene's tau fits it
    src, tgt = registration_case(24000, 9000, seed=21)
    tgt = (tgt * k).astype(np.float32).astype(np.float64)
    src = src * k
    # a mesh whose vertices + face centroids are the source cloud: every third point a vertex triple's centroid is extra
    V = src.astype(np.float32).astype(np.float64)
    F = np.arange(len(V) // 3 * 3, dtype=np.int32).reshape(-1, 3)[:200]
    mesh = os.path.join(root, "mesh.ply")
    with open(mesh, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(V), len(F))).encode())
        f.write(V.astype("<f4").tobytes())
        fr = np.zeros(len(F), [("n", "u1"), ("i", "<i4", 3)])
        fr["n"], fr["i"] = 3, F
        f.write(fr.tobytes())
    mesh_eval.write_vis_ply(os.path.join(d, scene + ".ply"), tgt, np.zeros_like(tgt))
    vol = volume_for(2)
    with open(os.path.join(d, scene + ".json"), "w") as f:
        json.dump({"axis_max": vol["axis_max"] * k, "axis_min": vol["axis_min"] * k, "bounding_polygon": (vol["polygon"] * k).tolist(),
                   "class_name": "SelectionPolygonVolume", "orthogonal_axis": "Z", "version_major": 1, "version_minor": 0}, f)
    # cameras: reference centres c (COLMAP frame), gt_trans maps them into the target's frame; the estimated ones are in the mesh's
    est_c, gt_c, gt_trans, _ = trajectory_case(n=60)
    Ks = KNOWN.copy()
    Ks[:3, 3] *= k
    cam_target = R.transform(gt_c, gt_trans) * 0.05
    gt_trans = gt_trans.copy()
    gt_trans[:3] *= 0.05
    cam_source = R.transform(cam_target, np.linalg.inv(Ks))
    np.savetxt(os.path.join(d, scene + "_trans.txt"), gt_trans)

    def write_log(path, centres):
        with open(path, "w") as f:
            for i, c in enumerate(centres):
                m = np.eye(4)
                m[:3, 3] = c
                f.write("%d %d 0\n" % (i, i))
                f.write("\n".join(" ".join(repr(float(x)) for x in row) for row in m) + "\n")
    write_log(os.path.join(d, scene + "_COLMAP_SfM.log"), gt_c)
    traj = os.path.join(root, "estimated.log")
    write_log(traj, cam_source)
    tri = V[F]
    source = np.concatenate([V, ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / 3.0])
    vol_s = {"axis": 2, "axis_min": vol["axis_min"] * k, "axis_max": vol["axis_max"] * k, "polygon": vol["polygon"] * k}
    return dict(dir=d, mesh=mesh, traj=traj, source=source, target=tgt, volume=vol_s, tau=tau, est=cam_source, gt=gt_c, gt_trans=gt_trans, scene=scene)


def restated_run(sc, seed):
    """run.py's sequence on the restatement -> (transformation, F-score dictionary)"""
    T, _, _ = R.align_trajectories(sc["est"], sc["gt"], sc["gt_trans"], seed, 100000)
    tau, vol = sc["tau"], sc["volume"]
    T = R.registration_vol_ds(sc["source"], sc["target"], T, vol, tau, 80 * tau)[0]
    T = R.registration_vol_ds(sc["source"], sc["target"], T, vol, tau / 2, 20 * tau)[0]
    T = R.registration_unif(sc["source"], sc["target"], T, vol, 2 * tau)[0]
    return T, R.tnt_fscore(sc["source"], sc["target"], T, vol, tau)


# ---------------------------------------------------------------------------------------------------------------------------
# the child: tnt_eval over the emulated library
# ---------------------------------------------------------------------------------------------------------------------------
def pack_record(record):
    """the per-evaluation record as arrays (a missing sums2 is NaN)"""
    return {"rec_T": np.array([e["transformation"] for e in record]).reshape(-1, 4, 4), "rec_n": np.array([e["n"] for e in record], np.int64),
            "rec_s1": np.array([e["sums1"] for e in record]).reshape(-1, 7),
            "rec_s2": np.array([e["sums2"] if e["sums2"] is not None else [np.nan] * 10 for e in record]).reshape(-1, 10)}


def sums2_means(n, s1):
    """the six means pass 2 is given: the sums of pass 1 over n (zeros when there is no correspondence)"""
    return [float(x) / float(n) for x in s1[:6]] if n else [0.0] * 6


def direct_sums2(M, s, t, thr, means):
    """gof_cloud_icp_sums2 called as icp calls it (transformation by the identity, query, pass 2) -> the 10 sums"""
    import ctypes as C
    import mesh_eval
    L = M.lib
    moved = M.transform_points(s, np.eye(4))
    dist, near = mesh_eval.nearest(moved, t)
    near = near.int()
    nb = L.gof_cloud_icp_sums_ws_bytes(len(s))
    ws = M.torch.empty(nb, dtype=M.torch.uint8, device=s.device)
    out, mu = (C.c_double * 10)(), (C.c_double * 6)(*means)
    with M._device_of(s):
        rc = L.gof_cloud_icp_sums2(len(s), moved.data_ptr(), len(t), t.data_ptr(), dist.data_ptr(), near.data_ptr(), float(thr), mu, ws.data_ptr(), nb, out,
                                   M._stream())
    assert rc == 0, L.gof_last_error()
    return np.array(list(out))


def run_case(M, case, workdir, tt):
    """one case on the product module M (tt: numpy array -> tensor on the device under test) -> dictionary of numpy arrays"""
    kind, name = case.split(":", 1)
    res = {}
    if kind == "crop":
        P, vol, T = crop_case(name)
        pts, idx = M.crop(tt(P), vol, T)
        res["points"], res["index"] = pts.cpu().numpy(), idx.cpu().numpy()
    elif kind == "voxel":
        P, v = voxel_case(name)
        pts, cnt = M.voxel_down_sample(tt(P), v)
        res["points"], res["counts"] = pts.cpu().numpy(), cnt.cpu().numpy()
    elif kind == "sums":
        s, t, thr = sums_case(name)
        res.update(pack_record(M.icp(tt(s), tt(t), thr, max_iteration=1)[3][:1]))
        if res["rec_n"][0] < 3:                                   # icp stops below 3 correspondences: pass 2 through the ABI itself
            res["rec_s2"][0] = direct_sums2(M, tt(s), tt(t), thr, sums2_means(res["rec_n"][0], res["rec_s1"][0]))
    elif kind == "icp":                                           # teacher-forced: one stage, the record is what is compared
        s, t = registration_case()
        s = R.transform(s, KNOWN @ similarity_matrix(1.02, 2.0, [0.5, 0.2, 1.0], [0.4, -0.3, 0.2]))
        T, fit, rmse, rec = M.icp(tt(s[:20000]), tt(t[:25000]), float(name), max_iteration=6)
        res.update(pack_record(rec))
        res["T"], res["fitness"], res["rmse"] = T, np.array(fit), np.array(rmse)
    elif kind == "stages":
        s, t = registration_case()
        vol = volume_for(2)
        T = np.eye(4)
        out = []
        s_d, t_d = tt(s), tt(t)
        for voxel, thr in ((TAU, 80 * TAU), (TAU / 2, 20 * TAU)):
            T = M.registration_vol_ds(s_d, t_d, T, vol, voxel, thr, 20)[0]
            out.append(T)
        out.append(M.registration_unif(s_d, t_d, T, vol, 2 * TAU, 20)[0])
        res["T"] = np.array(out)
    elif kind == "fscore":
        s, t = registration_case()
        r = M.tnt_fscore(tt(s), tt(t), KNOWN @ similarity_matrix(1.0, 0.2, [0, 1, 0], [0.05, 0.0, 0.1]), volume_for(2), TAU)
        res = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.array(v)) for k, v in r.items()}
    elif kind == "cli":
        root = os.path.join(workdir, "scene_" + name)
        sc = write_scene(root)
        for run in ("a", "b"):
            M.main(["--dataset-dir", sc["dir"], "--traj-path", sc["traj"], "--ply-path", sc["mesh"], "--out-dir", os.path.join(root, "out_" + run),
                    "--seed", "5"])
        try:
            M.main(["--dataset-dir", os.path.join(root, "Shed"), "--traj-path", sc["traj"], "--ply-path", sc["mesh"]])
            res["error"] = np.array("")
        except Exception as e:
            res["error"] = np.array(str(e))
        res["root"] = np.array(root)
    else:
        raise KeyError(case)
    return res


def _child(case, out):
    import torch
    import mesh_eval
    import tnt_eval as M
    check = host_child.install_seams(mesh_eval, M)          # (tnt_eval and the mesh_eval it calls)
    res = run_case(M, case, os.path.dirname(out), lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    res["workspaces"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path, order=None):
    res = host_child.run_child(__file__, case, tmp_path, order=order, timeout=3000)
    assert int(res["workspaces"]) > 0
    return res


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
# the checks, shared with tests/test_tnt_eval_gpu.py (res: what run_case returned)
# ---------------------------------------------------------------------------------------------------------------------------
def check_crop(name, res):
    P, vol, T = crop_case(name)
    want, idx = R.crop(P, vol, T)
    kind, _, tr = name.split("_")
    if kind in ("poly", "circle"):
        assert 0.2 * len(P) < len(idx) < 0.8 * len(P)
        assert kind == "poly" or len(vol["polygon"]) == 4096
        if tr == "plain" and kind == "poly":
            assert {0, 1} <= set(idx[:8].tolist()) and not ({2, 3} & set(idx[:8].tolist()))      # the slab is closed on both sides
    else:
        assert len(idx) == 0
    assert np.array_equal(res["index"], idx), "%d rows kept, the restatement keeps %d" % (len(res["index"]), len(idx))
    assert np.array_equal(bits(res["points"]), bits(want))


def check_voxel(name, res):
    P, v = voxel_case(name)
    want, counts = R.voxel_down_sample(P, v)
    if name == "skew":
        assert counts.max() >= 10 ** 4 and (counts == 1).sum() >= 10 ** 4
    if name == "one":
        assert len(counts) == 1
    if name == "lattice":
        assert len(counts) == 11 ** 3 and counts.max() == 8 and counts.min() == 1      # (the origin lies half a voxel below the minimum)
    if name == "straddle":
        from mesh_eval_restatement import check_straddle
        check_straddle(P, np.floor((P - (P.min(0) - 0.5 * v)) / v).astype(np.int64))    # the voxels
        assert counts.max() > 1
    assert res["points"].shape == want.shape, "%d voxels, the restatement has %d" % (len(res["points"]), len(want))
    assert np.array_equal(res["counts"], counts)
    assert np.array_equal(bits(res["points"]), bits(want))


def check_record(res, source, target, threshold, exact_update=True):
    """teacher-forced: the restatement, fed the product's transformation of every evaluation, reproduces n and the 16 sums bit for
    bit, and its own update from those sums is the product's next transformation"""
    K = len(res["rec_n"])
    for k in range(K):
        ev = R.icp_evaluate(source, target, res["rec_T"][k], threshold)
        assert ev["n"] == res["rec_n"][k], (k, ev["n"], int(res["rec_n"][k]))
        assert np.array_equal(bits(ev["sums1"]), bits(res["rec_s1"][k])), (k, ev["sums1"], res["rec_s1"][k])
        if ev["sums2"] is None and not np.isnan(res["rec_s2"][k]).all():      # (pass 2 called directly: sums_case n0 / n1 / single)
            S1 = R.transform(source, res["rec_T"][k])
            d, i = R.nearest(S1, target)
            mu = sums2_means(ev["n"], ev["sums1"])
            ev["sums2"] = [float(x) for x in R.icp_sums2(S1, target, d, i, threshold, mu[:3], mu[3:])]
        if not np.isnan(res["rec_s2"][k]).all():
            assert np.array_equal(bits(ev["sums2"]), bits(res["rec_s2"][k])), (k, ev["sums2"], res["rec_s2"][k])
            if k + 1 < K:
                nxt = R.umeyama_update(ev["n"], ev["sums1"], ev["sums2"]) @ res["rec_T"][k]
                if exact_update:
                    assert np.array_equal(bits(nxt), bits(res["rec_T"][k + 1])), (k, nxt, res["rec_T"][k + 1])
                else:
                    assert np.abs(nxt - res["rec_T"][k + 1]).max() <= 1e-12 * np.abs(nxt).max()
    return K


def restated_stages(source, target):
    """the three stages of run.py:156-160 on the restatement, with the conditions that make the comparison meaningful
    -> [T after each stage]"""
    vol = volume_for(2)
    T, out, margin = np.eye(4), [], np.inf
    for stage, (voxel, thr) in enumerate(((TAU, 80 * TAU), (TAU / 2, 20 * TAU), (None, 2 * TAU))):
        if voxel is None:
            T, _, _, rec = R.registration_unif(source, target, T, vol, thr)
        else:
            T, _, _, rec = R.registration_vol_ds(source, target, T, vol, voxel, thr)
        for ev in rec:
            margin = min(margin, np.abs(ev["dist"] / thr - 1).min())
            assert 0 < ev["n"] < len(ev["dist"]), "stage %d: the mask does not bite (%d of %d)" % (stage, ev["n"], len(ev["dist"]))
        out.append(T)
    moved = np.linalg.norm(R.transform(target, out[-1] @ np.linalg.inv(KNOWN)) - target, axis=1).max()
    print("restated stages: largest target movement %.4f (tau / 4 = %.4f), smallest |dist / threshold - 1| %.3g" % (moved, TAU / 4, margin))
    assert moved <= TAU / 4, moved
    assert margin > 1e-9, margin
    return out


def check_fscore(res, want):
    for k in ("below_source", "below_target"):
        assert int(res[k]) == want[k], k
    for k in ("hist_source", "hist_target"):
        assert np.array_equal(res[k], want[k]), k
    assert 0 < want["below_source"] < len(want["dist_source"]) and 0 < want["below_target"] < len(want["dist_target"])
    for k in ("source", "target", "dist_source", "dist_target", "cum_source", "cum_target", "precision", "recall", "fscore"):
        assert np.array_equal(bits(res[k]), bits(want[k])), k


CROP_CASES = ["circle_z_moved", "poly_x_plain", "poly_y_plain", "poly_z_plain", "poly_x_moved", "poly_z_moved", "nopoly_z_plain", "empty_z_plain"]
VOXEL_CASES = ["surface", "one", "lattice", "skew", "n0", "n1", "straddle"]
SUMS_CASES = ["torus", "pow2", "ragged", "n0", "n1", "single"]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CROP_CASES)
def test_crop_is_bit_equal(name, tmp_path):
    check_crop(name, _emulate("crop:" + name, tmp_path))


@pytest.mark.parametrize("name", VOXEL_CASES)
def test_voxel_means_are_bit_equal(name, tmp_path):
    check_voxel(name, _emulate("voxel:" + name, tmp_path))


@pytest.mark.parametrize("name", SUMS_CASES)
def test_correspondence_sums_are_the_tree(name, tmp_path):
    s, t, thr = sums_case(name)
    res = _emulate("sums:" + name, tmp_path)
    n = int(res["rec_n"][0])
    assert n == {"n0": 0, "n1": 1, "single": 1}.get(name, n) and (name in ("n0", "n1", "single") or 3 <= n < len(s))
    assert not np.isnan(res["rec_s2"][0]).any()                  # all 16 sums were produced and are compared
    assert check_record(res, s, t, thr) == 1


@pytest.mark.parametrize("order", ["reverse", "random:5"])
def test_sums_do_not_depend_on_the_schedule(order, tmp_path):
    s, t, thr = sums_case("torus")
    a, b = _emulate("sums:torus", tmp_path), _emulate("sums:torus", tmp_path, order=order)
    for k in ("rec_n", "rec_s1", "rec_s2"):
        assert np.array_equal(bits(a[k]) if a[k].dtype == np.float64 else a[k], bits(b[k]) if b[k].dtype == np.float64 else b[k]), k


def test_tree_sum_is_the_definition():
    """the yardstick against the definition it restates: explicit recursion, and the padding's one visible effect.  (This one test
    checks tests/tnt_eval_restatement.py alone and does not touch the product.)"""
    def rec(v):
        return v[0] if len(v) == 1 else rec(v[:len(v) // 2]) + rec(v[len(v) // 2:])
    v = np.random.default_rng(0).normal(size=(37, 1)) * 10.0 ** np.random.default_rng(1).integers(-8, 8, (37, 1))
    pad = np.vstack([v, np.zeros((64 - 37, 1))])
    assert R.tree_sum(v)[0] == rec(pad[:, 0])
    assert np.signbit(R.tree_sum(np.array([[-0.0]]))[0]) and not np.signbit(R.tree_sum(np.array([[-0.0], [-0.0], [-0.0]]))[0])


@pytest.mark.parametrize("threshold", ["10.0", "1.0"])
def test_icp_teacher_forced(threshold, tmp_path):
    s, t = registration_case()
    s = R.transform(s, KNOWN @ similarity_matrix(1.02, 2.0, [0.5, 0.2, 1.0], [0.4, -0.3, 0.2]))
    res = _emulate("icp:" + threshold, tmp_path)
    assert check_record(res, s[:20000], t[:25000], float(threshold)) == 7
    assert np.array_equal(bits(res["T"]), bits(res["rec_T"][-1]))


def test_icp_three_stages_free_running(tmp_path):
    s, t = registration_case()
    want = restated_stages(s, t)
    got = _emulate("stages:run", tmp_path)["T"]
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, got[k], want[k])


def test_ransac_identical_trajectories():
    import tnt_eval
    est, gt, gt_trans, _ = trajectory_case()
    T = tnt_eval.align_trajectories(gt, gt, gt_trans, seed=3, iterations=2000)
    assert np.abs(T - gt_trans).max() < 1e-9, T - gt_trans
    assert tnt_eval.align_trajectories(gt, gt, gt_trans, seed=3, iterations=2000).tobytes() == T.tobytes()


def test_ransac_finds_the_undisplaced_cameras():
    import tnt_eval
    est, gt, gt_trans, bad = trajectory_case(displaced=0.3)
    T = tnt_eval.align_trajectories(est, gt, gt_trans, seed=7, iterations=3000)
    want, h, inl = R.align_trajectories(est, gt, gt_trans, 7, 3000)
    assert np.array_equal(inl, ~bad) and bad.sum() == 60
    assert tnt_eval.last_stats()["ransac"]["hypothesis"] == h and tnt_eval.last_stats()["ransac"]["inliers"] == int(inl.sum())
    # the batched and the one-at-a-time pass call the same LAPACK / BLAS routines on the same 3x3 matrices, and with this numpy the
    # two transformations agree bit for bit; a numpy build that sends stacked and single 3x3 products down different paths would
    # round differently, which is no fault of the product: then the project's bar for fp64 results of equal terms in different
    # orders holds, 1e-12 relative (tests/test_mesh_eval_host.py, the two means)
    if not np.array_equal(bits(T), bits(want)):
        assert np.abs(T - want).max() <= 1e-12 * np.abs(want).max(), (T, want)
    d = np.linalg.norm(R.transform(est, T) - R.transform(gt, gt_trans), axis=1)
    assert (d[~bad] < 1e-6).all() and (d[bad] > 0.2).all()


def test_fscore_equals_the_restatement(tmp_path):
    s, t = registration_case()
    want = R.tnt_fscore(s, t, KNOWN @ similarity_matrix(1.0, 0.2, [0, 1, 0], [0.05, 0.0, 0.1]), volume_for(2), TAU)
    check_fscore(_emulate("fscore:run", tmp_path), want)


def check_cli(root, error):
    import mesh_eval
    sc = write_scene(os.path.join(os.path.dirname(root), "again"))
    T, want = restated_run(sc, 5)
    a, b = os.path.join(root, "out_a"), os.path.join(root, "out_b")
    got = json.load(open(os.path.join(a, "results.json")))
    assert sorted(got) == ["fscore", "precision", "recall", "tau", "transformation"]
    assert got["tau"] == 0.01 and 0.3 < want["fscore"] < 1.0
    assert np.array_equal(bits(np.array(got["transformation"])), bits(T))
    for k in ("precision", "recall", "fscore"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(np.loadtxt(os.path.join(a, "Barn.precision.txt")), want["cum_source"])
    assert np.array_equal(np.loadtxt(os.path.join(a, "Barn.recall.txt")), want["cum_target"])
    assert np.array_equal(np.loadtxt(os.path.join(a, "Barn.prf_tau_plotstr.txt")), np.array([want["precision"], want["recall"], want["fscore"], 0.01, 5]))
    for f, pts in (("Barn.precision.ply", want["source"]), ("Barn.recall.ply", want["target"])):
        assert np.array_equal(bits(mesh_eval.read_ply(os.path.join(a, f))[0]), bits(pts)), f
    for f in ("results.json", "Barn.precision.txt", "Barn.recall.txt", "Barn.prf_tau_plotstr.txt", "Barn.precision.ply", "Barn.recall.ply"):
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    assert "invalid dataset-dir, not in scenes_tau_dict" in error
    return a, want


def test_command_line_on_a_synthetic_scene(tmp_path):
    res = _emulate("cli:barn", tmp_path)
    check_cli(str(res["root"]), str(res["error"]))


def test_command_line_colours_and_plot(tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib.pyplot as plt
    res = _emulate("cli:barn", tmp_path)
    a, want = check_cli(str(res["root"]), str(res["error"]))
    assert os.path.getsize(os.path.join(a, "PR_Barn_@d_th_0_0100.png")) > 1000 and os.path.getsize(os.path.join(a, "PR_Barn_@d_th_0_0100.pdf")) > 1000
    raw = open(os.path.join(a, "Barn.precision.ply"), "rb").read()
    body = raw[raw.find(b"end_header\n") + 11:]
    rec = np.frombuffer(body, dtype=[("p", "<f8", 3), ("c", "u1", 3)])
    colour = plt.get_cmap("hot_r")(np.minimum(want["dist_source"], 0.03) / 0.03)[:, :3]
    assert np.array_equal(rec["c"], np.clip(colour * 255.0, 0, 255).astype(np.uint8))


def test_files_are_read_as_written(tmp_path):
    import tnt_eval
    sc = write_scene(str(tmp_path))
    vol = tnt_eval.read_crop_volume(os.path.join(sc["dir"], "Barn.json"))
    assert vol["axis"] == 2 and vol["axis_min"] == sc["volume"]["axis_min"] and np.array_equal(vol["polygon"], sc["volume"]["polygon"])
    traj = tnt_eval.read_log_trajectory(sc["traj"])
    assert traj.shape == (60, 4, 4) and np.array_equal(bits(traj[:, :3, 3]), bits(sc["est"])) and (traj[:, 3] == [0, 0, 0, 1]).all()
    assert tnt_eval.SCENES_TAU == {"Barn": 0.01, "Caterpillar": 0.005, "Church": 0.025, "Courthouse": 0.025, "Ignatius": 0.003,
                                   "Meetingroom": 0.01, "Truck": 0.005}


def test_host_tensors_are_refused():
    import torch
    import tnt_eval
    p = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        tnt_eval.crop(p, volume_for(2))
    with pytest.raises(RuntimeError, match="ROCm device"):
        tnt_eval.voxel_down_sample(p, 0.5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        tnt_eval.icp(p, p, 1.0)
    with pytest.raises(RuntimeError, match="ROCm device"):
        tnt_eval.tnt_fscore(p, p, np.eye(4), volume_for(2), 0.5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        tnt_eval.transform_points(p, np.eye(4))


def test_size_queries_and_argument_checks():
    import ctypes as C
    import tnt_eval
    L = tnt_eval.lib
    for q in (L.gof_cloud_crop_ws_bytes, L.gof_cloud_voxel_ws_bytes, L.gof_cloud_icp_sums_ws_bytes):
        assert 0 < q(0) <= q(1000) < q(100000) < q(10_000_000)
    assert L.gof_cloud_transform_ws_bytes(10 ** 6) > 0
    assert L.gof_cloud_voxel_ws_bytes(1_000_000) < 64 * 1_000_000 and L.gof_cloud_crop_ws_bytes(1_000_000) < 8 * 1_000_000
    assert L.gof_cloud_icp_sums_ws_bytes(1_000_000) < 1_000_000
    n = C.c_int64()
    assert L.gof_cloud_crop(5, None, None, 2, 0.0, 1.0, 4097, None, None, None, None, 0, C.byref(n), None) == -5 and b"4097" in L.gof_last_error()
    assert L.gof_cloud_crop(5, None, None, 3, 0.0, 1.0, 4, None, None, None, None, 0, C.byref(n), None) < 0 and b"axis" in L.gof_last_error()
    assert L.gof_cloud_voxel(5, None, 0.0, None, None, None, 0, C.byref(n), None) < 0 and b"positive" in L.gof_last_error()
    assert L.gof_cloud_voxel(5, None, -1.0, None, None, None, 0, C.byref(n), None) < 0
    assert L.gof_cloud_voxel(2 ** 31, None, 0.5, None, None, None, 0, C.byref(n), None) < 0
    assert L.gof_cloud_crop(2 ** 31, None, None, 2, 0.0, 1.0, 0, None, None, None, None, 0, C.byref(n), None) < 0
    assert L.gof_cloud_transform(2 ** 31, None, None, None, None, 0, None) < 0
    s = (C.c_double * 10)()
    assert L.gof_cloud_icp_sums1(2 ** 31, None, 0, None, None, None, 1.0, None, 0, C.byref(n), s, None) < 0
    assert L.gof_cloud_icp_sums2(5, None, 0, None, None, None, 1.0, None, None, 0, s, None) < 0
    bad = (C.c_double * 16)(*([float("nan")] * 16))
    assert L.gof_cloud_transform(5, None, bad, None, None, 0, None) < 0 and b"finite" in L.gof_last_error()


def test_launcher_sends_the_evaluation_in_process(tmp_path, monkeypatch):
    """given eval_tnt/run.py, the launcher runs tnt_eval's command line with the same arguments; GOF_TNT_EVAL_SUBPROCESS=1 leaves the
    script alone"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher_tnt", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    import tnt_eval
    calls = []
    monkeypatch.setattr(tnt_eval, "main", lambda argv=None: calls.append(list(argv)))
    script = tmp_path / "eval_tnt" / "run.py"
    script.parent.mkdir()
    script.write_text("raise SystemExit('the stand-in script itself was run')\n")
    argv = ["--dataset-dir", "/d/Barn", "--traj-path", "/d/Barn/Barn_COLMAP_SfM.log", "--ply-path", "/o/mesh.ply"]
    monkeypatch.delenv("GOF_TNT_EVAL_SUBPROCESS", raising=False)
    rb = L.tnt_eval_rebinding(str(script))
    assert list(rb) == ["main"]
    monkeypatch.setattr(sys, "argv", ["run_reference_script.py", str(script)] + argv)
    L.main()
    assert calls == [argv]
    monkeypatch.setenv("GOF_TNT_EVAL_SUBPROCESS", "1")
    assert L.tnt_eval_rebinding(str(script)) == {}
    monkeypatch.delenv("GOF_TNT_EVAL_SUBPROCESS")
    assert L.tnt_eval_rebinding("train.py") == {} and L.tnt_eval_rebinding(str(tmp_path / "run.py")) == {}


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
