"""CPU tests of the mesh depth rasteriser and visibility cull: the kernels of csrc/mesh_raster.hip through the host
emulator (tests/hipemu) behind mesh_cull's own Python layer, each group of cases in a child process, held to
tests/mesh_raster_restatement.py bit for bit: every depth image, every count, the culled mesh and its exported bytes.  The
restatement itself is held to a brute-force ray cast, so that the contract is tied to geometry.

In the child the product module runs unchanged except for its test seams; every buffer it allocates is filled with 0xA5 and followed by
guard bytes that are checked after the run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import mesh_raster_cases as K  # noqa: E402
import mesh_raster_restatement as R  # noqa: E402
import mesh_components_restatement as RC  # noqa: E402

FILLS = (0x00, 0xA5, 0xFF)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def _down(t):
    return t.detach().numpy().copy()


def tiling():
    import mesh_cull
    return mesh_cull.raster_tiling()


def run_abi(M, alloc, down, V, F, views, fill, batch=K.BATCH, min_views=1, mutate=None):
    """the three entry points over buffers of the case's own: workspace and outputs filled with `fill`, guard bytes behind every one
    -> depth, count (added to zeros), driver count and keep, the status codes and whether the guards held"""
    import torch
    L = M.lib
    rec = M.raster_views(views["c2w"], views["H"], views["W"], views["fx"], views["fy"], views["cx"], views["cy"], views["znear"], views["zfar"], views["convention"])
    if mutate:
        mutate(rec)
    n, nv, nf, stride = len(rec), len(V), len(F), views["H"] * views["W"]
    v, f, r = _up_like(alloc, V), _up_like(alloc, F), _up_like(alloc, rec.view(np.uint8).reshape(-1))
    G = 256

    def buf(nbytes):
        b = alloc(nbytes + G)
        b.fill_(fill)
        return b
    ws1, ws2 = buf(L.gof_mesh_render_depth_ws_bytes(nf)), buf(L.gof_mesh_visibility_ws_bytes(nf, stride, batch))
    depth, count, count2, keep = buf(4 * n * stride), buf(4 * nv), buf(4 * nv), buf(nv)
    count[:4 * nv] = 0
    ptr = lambda t: t.data_ptr() if t.numel() else None
    rc1 = L.gof_mesh_render_depth(nv, ptr(v), nf, ptr(f), n, ptr(r), stride, depth.data_ptr(), None, ws1.data_ptr(), ws1.numel() - G, None)
    rc2 = L.gof_mesh_visible_count(nv, ptr(v), n, ptr(r), stride, depth.data_ptr(), K.EPS, count.data_ptr(), ws1.data_ptr(), ws1.numel() - G, None)
    rc3 = L.gof_mesh_visibility(nv, ptr(v), nf, ptr(f), n, ptr(r), stride, batch, K.EPS, min_views, count2.data_ptr(), keep.data_ptr(), None, ws2.data_ptr(),
                                ws2.numel() - G, None)
    guards = all(bool((down(b)[-G:] == fill).all()) for b in (ws1, ws2, depth, count, count2, keep))
    return {"depth": down(depth)[:-G].view(np.float32).reshape(n, views["H"], views["W"]), "count": down(count)[:-G].view(np.int32), "driver_count": down(count2)[:-G].view(np.int32),
            "driver_keep": down(keep)[:-G].astype(bool), "rc": np.array([rc1, rc2, rc3]), "guards": np.array(guards), "error": np.array(L.gof_last_error().decode())}


def _up_like(alloc, a):
    import torch
    a = np.ascontiguousarray(a)
    t = alloc(max(a.nbytes, 1))
    t[:a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1))
    return t[:a.nbytes]


def bad_inputs(V, F):
    """-> [(tag, V, F, what to do to the records, the text of the error)]"""
    hi, neg = F.copy(), F.copy()
    hi[1, 2], neg[0, 0] = len(V), -1

    def setter(field, value):
        def go(rec):
            rec[field][-1] = value
        return go
    return [("index_high", V, hi, None, "outside [0"), ("index_negative", V, neg, None, "outside [0"), ("width", V, F, setter("W", 0), "view record"),
            ("height", V, F, setter("H", -3), "view record"), ("znear", V, F, setter("znear", 0.0), "view record"), ("znear_nan", V, F, setter("znear", np.nan), "view record"),
            ("zfar", V, F, setter("zfar", 0.01), "view record"), ("too_wide", V, F, setter("W", 20000), "view record")]


def _pivot(count):
    """the count of the first vertex that some but not all of the 9 cameras see"""
    return int(count[np.argmax((count > 0) & (count < 9))])


def cull_runs(M, up, down, tmp):
    """cull_by_visibility at min_views around a vertex's count, the exported bytes, and TntMesher over a file"""
    V, F, N, Col, views = K.cull_scene()
    kw = dict(H=views["H"], W=views["W"], fx=views["fx"], fy=views["fy"], cx=views["cx"], cy=views["cy"])
    res = {}
    mesh = M.DeviceMesh(V, F, N, Col)
    count = down(M.visible_count(mesh, views["c2w"], eps=K.CULL_EPS, **kw))
    res["count"] = count
    for mv in sorted({_pivot(count) - 1, _pivot(count), _pivot(count) + 1, 0, 2}):
        mesh = M.DeviceMesh(V, F, N, Col)
        c = mesh.cull_by_visibility(views["c2w"], eps=K.CULL_EPS, min_views=mv, **kw)
        path = os.path.join(tmp, "cull_%d.ply" % mv)
        mesh.export(path)
        res["ply_%d" % mv] = np.frombuffer(open(path, "rb").read(), np.uint8)
        res["count_%d" % mv] = down(c)
    src = os.path.join(tmp, "scene.ply")
    M.DeviceMesh(V, F, N, Col).export(src)
    mesher = M.TntMesher(views["H"], views["W"], views["fx"], views["fy"], views["cx"], views["cy"], 20.0)
    mesher.verbose, mesher.min_views, mesher.eps = False, 2, K.CULL_EPS
    import torch
    mesher(src, [torch.from_numpy(m).float() for m in views["c2w"]])
    res["mesher_ply"] = np.frombuffer(open(os.path.join(tmp, "scene_cull.ply"), "rb").read(), np.uint8)
    mesher.components = dict(largest=1)
    mesher(src, [torch.from_numpy(m).float() for m in views["c2w"]])
    res["mesher_largest_ply"] = np.frombuffer(open(os.path.join(tmp, "scene_cull.ply"), "rb").read(), np.uint8)
    return res


def want_cull():
    V, F, N, Col, views = K.cull_scene()
    count, _ = R.visibility(V, F, K.recs_of(views), K.CULL_EPS, 0)
    return V, F, N, Col, count


def check_cull(res):
    V, F, N, Col, count = want_cull()
    assert np.array_equal(res["count"], count)
    c0 = _pivot(count)
    assert 0 < c0 < 9 and len(np.unique(count)) > 3                                   # the scene bites: hidden, partly seen and seen vertices
    sizes = []
    for mv in sorted({c0 - 1, c0, c0 + 1, 0, 2}):
        v, f, n, c = R.cull(V, F, count >= mv, N, Col)
        assert np.array_equal(res["count_%d" % mv], count)
        assert res["ply_%d" % mv].tobytes() == RC.ply_bytes(v.astype(np.float64), f, n, c), mv
        sizes.append((mv, len(v)))
    by = dict(sizes)
    assert by[0] == len(np.unique(F)) and by[c0 - 1] >= by[c0] > by[c0 + 1] > 0                        # the pivot vertex leaves exactly above its own count
    k = int(np.argmax((count > 0) & (count < 9)))
    assert [bool((count >= mv)[k]) for mv in (c0 - 1, c0, c0 + 1)] == [True, True, False]
    v, f, n, c = R.cull(V.astype(np.float32), F, count >= 2, N, Col)                    # (the file holds float32 coordinates)
    assert res["mesher_ply"].tobytes() == RC.ply_bytes(v.astype(np.float64), f, n, c)
    v2, f2, n2, c2, kept, _ = RC.keep_components(v.astype(np.float64), f, n, c, largest=1)
    assert res["mesher_largest_ply"].tobytes() == RC.ply_bytes(v2, f2, n2, c2) and kept == 1


# ---------------------------------------------------------------------------------------------------------------------------
def _child(case, out):
    import mesh_cull as M
    import mesh_components as MC
    check = host_child.install_seams(M, MC, buffers="all")
    alloc, down = host_child.host_buffers(M)
    kind, name = case.split(":", 1)
    T = M.raster_tiling()
    S = K.scenes(T)
    res = {}
    if kind == "cases":
        for tag, sc in S.items():
            if tag.startswith(name):
                res.update({"%s_%s" % (tag, k): v for k, v in K.run(M, _up, sc, _down).items()})
    elif kind == "order":
        V, F, views = S["64x48_views"]
        perm = np.random.default_rng(1).permutation(len(F))
        for tag, f in (("first", F), ("again", F), ("permuted", F[perm]), ("reversed", F[::-1])):
            res.update({"%s_%s" % (tag, k): v for k, v in K.run(M, _up, (V, f, views), _down).items()})
    elif kind == "fills":
        for tag in ("64x48_views", "70x33_threshold", "70x33_near_fan"):
            for fill in FILLS:
                res.update({"%s_%02x_%s" % (tag, fill, k): v for k, v in run_abi(M, alloc, down, *S[tag], fill).items()})
    elif kind == "errors":
        V, F, views = S["70x33_views"]
        for tag, v, f, mutate, _ in bad_inputs(V, F):
            res.update({"%s_%s" % (tag, k): v2 for k, v2 in run_abi(M, alloc, down, v, f, views, 0x5C, mutate=mutate).items()})
    elif kind == "cull":
        res = cull_runs(M, _up, _down, os.path.dirname(out))
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=900)
    assert int(res["buffers"]) > 0
    return res


def check_cases(got_of, prefix, T):
    """every scene of one image size against the restatement, and that the scenes show what they are for"""
    S = K.scenes(T)
    for tag in S:
        if tag.startswith(prefix):
            assert K.same(got_of(tag), K.want(tag, T), tag + " ") == []
    d = lambda tag: K.want(prefix + tag, T)["depth"][0]
    W, H = (int(x) for x in prefix.rstrip("_").split("x"))
    # the quad: every pixel centre inside is covered, once: 28 x 28, whichever diagonal and winding
    for tag in ("quad", "quad_other"):
        V, F, views = S[prefix + tag]
        cover = np.zeros((H, W), int)
        R.render_view(V, F, K.recs_of(views)[0], cover)
        inside = np.zeros((H, W), bool)
        inside[2:30, 2:30] = True
        assert np.array_equal(cover == 1, inside) and cover.max() == 1
    # top-left rule: the vertex on a centre and the top and left edges belong to the triangle, the hypotenuse to its neighbour
    for tag in ("on_centres", "on_centres_flipped"):
        img = d(tag)
        assert img[4, 4] == 1 and img[4, 19] == 1 and img[19, 4] == 1 and img[4, 20] == 0 and img[20, 4] == 0 and img[12, 12] == 0 and img[11, 12] == 1
    pair = d("on_centres_pair")
    assert pair[12, 12] == 2 and pair[4, 20] == 0 and pair[20, 20] == 0 and pair[19, 19] == 2 and (pair > 0).sum() == 256
    assert np.argwhere(d("subpixel") > 0).tolist() == [[9, 8]]
    assert (d("whole_image") == 2).all()
    t = T["inline_max"]
    assert (d("threshold") > 0).sum() == sum(n * (n + 1) // 2 for n in (t - 1, t, t + 1, T["tile_w"], T["tile_w"] + 1, 2 * T["tile_w"] + 1))
    z = d("zfar")
    assert (z[2:12, 2:12] == 20).sum() == 45 and not z[2:12, 14:24].any() and 0 < (z[:, 26:] > 0).sum() and z.max() == 20 and (z[2, 26:] > 15).any()
    g = d("outside_guard")
    assert g[5, 5] == 0.5 and (g > 0).all() and (H < 42 or (g[42:] == 0.25).any())
    assert np.array_equal(d("degenerate") > 0, d("on_centres") * 0 + (K.want(prefix + "degenerate", T)["depth"][0] > 0)) and (d("degenerate") > 0).sum() == 136
    assert (d("nonfinite") == 1).sum() == 136 and (d("nonfinite") == 2).sum() == 16
    assert K.want(prefix + "nothing", T)["depth"].shape == (1, H, W) and K.want(prefix + "no_views", T)["depth"].shape == (0, H, W)
    assert (d("near") > 0).sum() > 100 and d("near")[d("near") > 0].min() >= np.float32(0.01)
    # no crack along the clipped shared edge: every clean ray-cast hit of the fan is covered in the restated image
    V, F, views = S[prefix + "near_fan"]
    z, tol, clean = R.geometric_tolerance(V, F, K.recs_of(views)[0])
    fan = d("near_fan")
    assert (clean & np.isfinite(z)).sum() > 300 and (fan[clean & np.isfinite(z)] > 0).all() and not fan[clean & ~np.isfinite(z)].any()
    cnt = K.want(prefix + "views", T)["count"]
    assert cnt.max() > K.BATCH and cnt.min() == 0 and len(S[prefix + "views"][2]["c2w"]) > 2 * K.BATCH


@pytest.mark.parametrize("size", ["%dx%d_" % s for s in K.SIZES])
def test_every_case_equals_the_restatement(size, tmp_path):
    got = _emulate("cases:" + size, tmp_path)
    check_cases(lambda tag: {k: got["%s_%s" % (tag, k)] for k in ("depth", "count", "driver_count", "driver_keep")}, size, tiling())


def test_face_order_and_repetition_do_not_matter(tmp_path):
    got = _emulate("order:all", tmp_path)
    for tag in ("again", "permuted", "reversed"):
        for k in ("depth", "count", "driver_count", "driver_keep"):
            assert np.array_equal(got["first_" + k].view(np.uint8), got[tag + "_" + k].view(np.uint8)), (tag, k)


def test_workspace_and_output_contents_do_not_matter(tmp_path):
    got = host_child.run_child(__file__, "fills:all", tmp_path, timeout=900)
    T = tiling()
    for tag in ("64x48_views", "70x33_threshold", "70x33_near_fan"):
        for fill in FILLS:
            p = "%s_%02x_" % (tag, fill)
            assert got[p + "rc"].tolist() == [0, 0, 0] and bool(got[p + "guards"]), p
            assert K.same({k: got[p + k] for k in ("depth", "count", "driver_count", "driver_keep")}, K.want(tag, T)) == [], p


def check_errors(got, V, F):
    for tag, _, _, _, text in bad_inputs(V, F):
        rc = got[tag + "_rc"].tolist()
        assert rc[0] < 0 and rc[2] < 0 and (rc[1] < 0) == (text == "view record"), (tag, rc)
        assert text in str(got[tag + "_error"]) and bool(got[tag + "_guards"]), tag
        assert (got[tag + "_depth"].view(np.uint32) == 0x5C5C5C5C).all() and (got[tag + "_driver_count"].view(np.uint32) == 0x5C5C5C5C).all(), tag
        assert (got[tag + "_driver_keep"].view(np.uint8) == 1).all() and (rc[1] == 0 or not got[tag + "_count"].any()), tag      # (0x5C as bool)


def test_bad_input_is_refused_with_nothing_written(tmp_path):
    got = host_child.run_child(__file__, "errors:all", tmp_path, timeout=900)
    V, F, _ = K.scenes(tiling())["70x33_views"]
    check_errors(got, V, F)


def test_cull_by_visibility_and_the_exported_bytes(tmp_path):
    check_cull(_emulate("cull:all", tmp_path))


# ---- without the emulator ----------------------------------------------------------------------------------------------------
def test_the_restatement_agrees_with_a_ray_cast():
    """The contract against geometry: on every pixel that no edge, silhouette or crossing comes within 1/128 pixel of, the restated
    depth equals the ray cast's within the snap's worth of depth slope (R.geometric_tolerance), and background equals background."""
    T = tiling()
    S = K.scenes(T)
    worst = 0.0
    for tag in ("64x48_views", "70x33_views", "64x48_near_fan", "70x33_near", "64x48_quad", "70x33_whole_image", "64x48_zfar"):
        V, F, views = S[tag]
        for r, img in zip(K.recs_of(views), K.want(tag, T)["depth"]):
            z, tol, clean = R.geometric_tolerance(V, F, r)
            hit = clean & np.isfinite(z)
            assert clean.mean() > 0.5, tag
            assert not img[clean & ~hit].any(), tag
            err = np.abs(img[hit].astype(np.float64) - z[hit])
            assert (img[hit] > 0).all() and (err <= tol[hit]).all(), (tag, float((err - tol[hit]).max()))
            if hit.any():
                worst = max(worst, float(tol[hit].max()))
    print("largest tolerance used (snap x depth slope + float32 rounding): %.3g" % worst)
    assert worst > 0


def test_host_tensors_and_bad_arguments_are_refused():
    import torch
    import mesh_cull as M
    eye = [np.eye(4)]
    with pytest.raises(RuntimeError, match="ROCm device"):
        M.visible_count(torch.zeros((1, 3)), eye, 4, 4, 1.0, 1.0, 0.0, 0.0, depth=torch.zeros((1, 4, 4)))
    with pytest.raises(ValueError, match="convention"):
        M.raster_views(eye, 4, 4, 1.0, 1.0, 0.0, 0.0, convention="vulkan")
    with pytest.raises(ValueError, match="camera 0"):
        M.raster_views([np.eye(3)], 4, 4, 1.0, 1.0, 0.0, 0.0)
    m = M.TntMesher(4, 4, 1.0, 1.0, 0.0, 0.0, 20.0)
    m.forecast_radius = 2
    with pytest.raises(NotImplementedError, match="forecast_radius"):
        m("mesh.ply", eye)


def test_size_queries_versions_and_records():
    import mesh_cull as M
    L = M.lib
    assert L.gof_mesh_raster_abi_version() == 3 and L.gof_mesh_abi_version() == 2 and L.gof_abi_version() == 12
    T = M.raster_tiling()
    assert T["guard"] == R.GUARD and T["inline_max"] >= 2 and T["tile_w"] * T["tile_h"] == 64 and 256 * (T["max_side"] + T["guard"]) < 2 ** 23
    assert 0 < L.gof_mesh_render_depth_ws_bytes(0) < L.gof_mesh_render_depth_ws_bytes(10 ** 6) < 16 * 10 ** 6
    one = L.gof_mesh_visibility_ws_bytes(1000, 1920 * 1080, 1) - L.gof_mesh_render_depth_ws_bytes(1000)
    assert abs(one - 4 * 1920 * 1080) < 1024 and L.gof_mesh_visibility_ws_bytes(1000, 1920 * 1080, 0) == L.gof_mesh_visibility_ws_bytes(1000, 1920 * 1080, T["batch"])
    assert L.gof_mesh_visibility_ws_bytes(1000, 64, -1) == 0 and L.gof_mesh_visibility_ws_bytes(1000, -1, 1) == 0
    assert L.gof_mesh_render_depth(-1, None, 0, None, 0, None, 0, None, None, None, 0, None) < 0
    assert L.gof_mesh_render_depth(3, None, (2 ** 31 + 2) // 3, None, 0, None, 0, None, None, None, 0, None) < 0 and b"2^31" in L.gof_last_error()
    assert L.gof_mesh_visibility(3, None, 0, None, 1, None, 16, 5000, 0.005, 1, None, None, None, None, 0, None) < 0 and b"batch" in L.gof_last_error()
    # the records: the OpenGL pose the script hands to pyrender and the OpenCV pose point_masks forms from it are one camera
    c2w = K.orbit(3)
    gl = M.raster_views(c2w, 48, 64, 50.0, 51.0, 31.0, 23.0)
    flipped = [m.copy() for m in c2w]
    for m in flipped:
        m[:3, 1:3] *= -1
    cv = M.raster_views(flipped, 48, 64, 50.0, 51.0, 31.0, 23.0, convention="opencv")
    assert gl.tobytes() == cv.tobytes() and gl.dtype.itemsize == C.sizeof(M.GofRasterView) == 152
    want = R.records(c2w, 48, 64, 50.0, 51.0, 31.0, 23.0)
    assert all(r["w2c"] == list(g["w2c"]) and r["fx"] == g["fx"] and r["W"] == g["W"] and r["zfar"] == g["zfar"] == 20.0 for r, g in zip(want, gl))
    eye = np.array([0.3, -0.2, 0.9, 1.0])
    assert np.allclose(np.asarray(gl[0]["w2c"]).reshape(3, 4) @ (c2w[0] @ eye), eye[:3] * [1, -1, -1])
    for name in ("cull_by_visibility",):
        assert hasattr(M.DeviceMesh, name)


def test_trajectories_load_through_numpy(tmp_path):
    import json
    import mesh_cull as M
    poses = np.stack(K.orbit(5)).astype(np.float32)
    np.save(tmp_path / "traj.npy", poses[:, :3])
    traj = M.get_traj(str(tmp_path / "traj.npy"))
    assert len(traj) == 5 and all(tuple(t.shape) == (4, 4) for t in traj) and np.array_equal(traj[2].numpy(), poses[2])
    frames = [{"file_path": "images/frame_%05d.png" % (i + 1), "transform_matrix": poses[i].tolist()} for i in (3, 0, 4, 1, 2)]
    (tmp_path / "transforms.json").write_text(json.dumps({"frames": frames}))
    traj = np.stack([t.numpy() for t in M.get_traj(str(tmp_path / "transforms.json"))])
    assert np.abs(traj[:, :3, 3]).max() == pytest.approx(1.0, abs=1e-6) and np.abs(traj[:, :3, 3].mean(axis=0)).max() < 1e-6
    up = traj[:, :3, 1].mean(axis=0)
    assert up[2] > 0 and abs(up[0]) < 1e-6 and abs(up[1]) < 1e-6                           # the mean up vector points along +z
    rot = traj[:, :3, :3]
    assert np.allclose(rot @ rot.transpose(0, 2, 1), np.eye(3), atol=1e-5)
    # the order is the files' numbers, not the list's: camera 0 of the file is pose 0
    d = np.linalg.norm(traj[0, :3, 3] - traj[1, :3, 3]) / np.linalg.norm(traj[0, :3, 3] - traj[2, :3, 3])
    assert d == pytest.approx(np.linalg.norm(poses[0, :3, 3] - poses[1, :3, 3]) / np.linalg.norm(poses[0, :3, 3] - poses[2, :3, 3]), rel=1e-4)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
