"""CPU tests of the mesh renderer: the kernels of csrc/mesh_render.hip through the host emulator (tests/hipemu) behind
mesh_render's own Python layer, each group of cases in a child process, held to tests/mesh_render_restatement.py bit for bit: vertex and
face normals, depth, face, barycentrics and the image of every mode.  The restatement itself is held to a brute-force ray cast and to
an independent form of the normals.

In the child the product modules run unchanged except for their test seams; every buffer they allocate is filled with 0xA5 and followed
by guard bytes that are checked after the run."""
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
import mesh_render_cases as KR  # noqa: E402
import mesh_render_restatement as RR  # noqa: E402
from test_mesh_raster_host import FILLS, _up, _down, _up_like, tiling  # noqa: E402

G = 256
ORDER_SCENES = ("64x48_views", "64x48_ties")
FILL_SCENES = ("closed", "70x33_threshold", "70x33_near_fan")
FILL_CONFIG = ("shaded_vertex", "shaded", False, True)


def run_abi(M, MR, alloc, down, scene, fill, config=("shaded", "shaded", False, False), mutate=None, params=None, drop_colors=False):
    """the entry points of (g) over buffers of the case's own: workspaces and outputs filled with `fill`, guard bytes behind every one ->
    every output, the status codes and whether the guards held"""
    L = M.lib
    V, F, views, col = scene
    rec = M.raster_views(views["c2w"], views["H"], views["W"], views["fx"], views["fy"], views["cx"], views["cy"], views["znear"], views["zfar"], views["convention"])
    if mutate:
        mutate(rec)
    n, nv, nf, stride = len(rec), len(V), len(F), views["H"] * views["W"]
    v, f, r = _up_like(alloc, V), _up_like(alloc, F), _up_like(alloc, rec.view(np.uint8).reshape(-1))
    c4 = None
    if col is not None and not drop_colors:
        c4 = np.zeros((nv, 4), np.uint8)
        c4[:, :3] = col[:, :3]
        c4 = _up_like(alloc, c4)

    def buf(nbytes):
        b = alloc(nbytes + G)
        b.fill_(fill)
        return b
    ws_n, ws_fn = buf(L.gof_mesh_vertex_normals_ws_bytes(nv, nf)), buf(L.gof_mesh_face_normals_ws_bytes())
    ws_f, ws_s = buf(L.gof_mesh_render_faces_ws_bytes(nf, n, stride)), buf(L.gof_mesh_shade_ws_bytes())
    normals, fnormals, depth, face, image, bary = buf(12 * nv), buf(12 * nf), buf(4 * n * stride), buf(4 * n * stride), buf(12 * n * stride), buf(12 * n * stride)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    P = MR.GofShadeParams()
    P.mode, P.flags = MR.MODES[config[1]], (MR.FLAT if config[2] else 0) | (MR.VERTEX_BASE if config[3] else 0)
    P.base[:], P.background[:], P.ambient = KR.BASE, KR.BACKGROUND, KR.AMBIENT
    if params:
        params(P)
    rc = [L.gof_mesh_vertex_normals(nv, ptr(v), nf, ptr(f), normals.data_ptr(), ws_n.data_ptr(), ws_n.numel() - G, None),
          L.gof_mesh_face_normals(nv, ptr(v), nf, ptr(f), fnormals.data_ptr(), ws_fn.data_ptr(), ws_fn.numel() - G, None),
          L.gof_mesh_render_faces(nv, ptr(v), nf, ptr(f), n, ptr(r), stride, depth.data_ptr(), face.data_ptr(), None, ws_f.data_ptr(), ws_f.numel() - G, None)]
    err = [L.gof_last_error().decode()]
    shade_face = face
    if rc[2] != 0:                                  # the face buffer was refused: the resolve pass is asked over a valid (empty) one
        shade_face = buf(4 * n * stride)
        shade_face[:4 * n * stride] = 0xFF
    rc.append(L.gof_mesh_shade(nv, ptr(v), nf, ptr(f), normals.data_ptr(), ptr(c4), n, ptr(r), stride, shade_face.data_ptr(), C.byref(P), image.data_ptr(),
                               bary.data_ptr(), ws_s.data_ptr(), ws_s.numel() - G, None))
    err.append(L.gof_last_error().decode())
    guards = all(bool((down(b)[-G:] == fill).all()) for b in (ws_n, ws_fn, ws_f, ws_s, normals, fnormals, depth, face, image, bary))
    H, W = views["H"], views["W"]
    return {"normals": down(normals)[:-G].view(np.float32).reshape(nv, 3), "face_normals": down(fnormals)[:-G].view(np.float32).reshape(nf, 3),
            "depth": down(depth)[:-G].view(np.float32).reshape(n, H, W), "face": down(face)[:-G].view(np.int32).reshape(n, H, W),
            "image_" + config[0]: down(image)[:-G].view(np.float32).reshape(n, 3, H, W), "bary": down(bary)[:-G].view(np.float32).reshape(n, 3, H, W),
            "rc": np.array(rc), "guards": np.array(guards), "error": np.array(" | ".join(err))}


def bad_inputs(scene):
    """-> [(tag, scene, config, what to do to the records, what to do to the parameters, drop the colours, the entries that refuse
    (normals, face normals, faces, shade), the text of the error)]: the issue's six and their neighbours"""
    V, F, views, col = scene
    hi = F.copy()
    hi[1, 2] = len(V)

    def setter(field, value):
        def go(rec):
            rec[field][-1] = value
        return go

    def param(field, value):
        def go(P):
            setattr(P, field, value)
        return go
    shaded, color = ("shaded", "shaded", False, False), ("color", "color", False, False)
    return [("index_high", (V, hi, views, col), shaded, None, None, False, (1, 1, 1, 1), "outside [0"),
            ("too_wide", scene, shaded, setter("W", 20000), None, False, (0, 0, 1, 1), "view record"),
            ("znear", scene, shaded, setter("znear", 0.0), None, False, (0, 0, 1, 1), "view record"),
            ("znear_negative", scene, shaded, setter("znear", -1.0), None, False, (0, 0, 1, 1), "view record"),
            ("no_colors", scene, color, None, None, True, (0, 0, 0, 1), "colours"),
            ("mode", scene, shaded, None, param("mode", 4), False, (0, 0, 0, 1), "mode"),
            ("ambient_nan", scene, shaded, None, param("ambient", float("nan")), False, (0, 0, 0, 1), "ambient"),
            ("ambient_inf", scene, shaded, None, param("ambient", float("inf")), False, (0, 0, 0, 1), "ambient")]


ERROR_OUTPUTS = (("normals", 0), ("face_normals", 1), ("depth", 2), ("face", 2), ("image_", 3), ("bary", 3))


def check_errors(got, scene):
    for tag, _, config, _, _, _, refuses, text in bad_inputs(scene):
        rc = got[tag + "_rc"].tolist()
        assert [r < 0 for r in rc] == [bool(x) for x in refuses], (tag, rc)
        assert all(r in (0, -1) for r in rc), (tag, rc)                                  # GOF_E_INVALID
        assert text in str(got[tag + "_error"]) and bool(got[tag + "_guards"]), (tag, str(got[tag + "_error"]))
        for name, entry in ERROR_OUTPUTS:
            if refuses[entry]:
                a = got[tag + "_" + (name + config[0] if name == "image_" else name)]
                assert (a.view(np.uint8) == 0x5C).all(), (tag, name)


# ---------------------------------------------------------------------------------------------------------------------------
def order_runs(MR, M, up, down, S):
    res = {}
    for name in ORDER_SCENES:
        V, F, views, col = S[name]
        perm = np.random.default_rng(1).permutation(len(F))
        for tag, f in (("first", F), ("again", F), ("permuted", F[perm]), ("reversed", F[::-1])):
            res.update({"%s_%s_%s" % (name, tag, k): v for k, v in KR.run(MR, M, up, (V, np.ascontiguousarray(f), views, col), down).items()})
    return res


def check_order(got, T):
    """permuting the faces leaves depth alone; face, bary and the images equal the restatement run on the permuted faces"""
    S = KR.scenes(T)
    for name in ORDER_SCENES:
        V, F, views, col = S[name]
        perm = np.random.default_rng(1).permutation(len(F))
        recs, shape = K.recs_of(views), (views["H"], views["W"])
        first = {k[len(name) + 7:]: v for k, v in got.items() if k.startswith(name + "_first_")}
        assert KR.same(first, KR.want(name, T)) == []
        for tag, f in (("again", F), ("permuted", F[perm]), ("reversed", F[::-1])):
            g = {k[len(name) + len(tag) + 2:]: v for k, v in got.items() if k.startswith("%s_%s_" % (name, tag))}
            assert np.array_equal(g["depth"].view(np.uint32), first["depth"].view(np.uint32)), (name, tag)
            depth, face = RR.render_faces(V, f, recs, shape)
            assert np.array_equal(g["face"], face) and np.array_equal(g["depth"].view(np.uint32), depth.view(np.uint32)), (name, tag)
            normals = RR.vertex_normals(V, f)
            assert np.array_equal(g["normals"].view(np.uint32), normals.view(np.uint32)), (name, tag)
            for ctag, mode, flat, vbase in KR.configs(col):
                img, bary = RR.shade(V, f, recs, face, shape, RR.MODES[mode], normals=normals, colors=col, flat=flat, vertex_base=vbase, base=KR.BASE,
                                     ambient=KR.AMBIENT, background=KR.BACKGROUND)
                assert np.array_equal(g["image_" + ctag].view(np.uint32), img.view(np.uint32)), (name, tag, ctag)
                assert np.array_equal(g["bary"].view(np.uint32), bary.view(np.uint32)), (name, tag)
            if tag == "again":
                assert all(np.array_equal(g[k].view(np.uint8), first[k].view(np.uint8)) for k in first), (name, tag)
    # the scene bites: pixels whose two nearest faces have the same depth bits, decided by the face index
    V, F, views, col = S["64x48_ties"]
    rec = K.recs_of(views)[0]
    alone = [RR.render_faces_view(V, F[k:k + 1], rec)[0].view(np.uint32) for k in range(len(F))]
    face = KR.want("64x48_ties", T)["face"][0]
    twins = (alone[0] == alone[1]) & (alone[0] != 0)
    crossing = (alone[0] == alone[2]) & (alone[0] != 0) | (alone[0] == alone[3]) & (alone[0] != 0)
    assert twins.sum() > 100 and crossing.sum() >= 5 and (face[crossing] == 0).all() and not (face == 1).any()
    rev = RR.render_faces_view(V, F[::-1], rec)[1]
    assert (rev[crossing] < 2).all() and not (rev == 3).any()                          # reversed: the tilted faces come first and win the tie


def _child(case, out):
    import mesh_cull as M
    import mesh_components as MC
    import mesh_render as MR
    check = host_child.install_seams(M, MC, MR, buffers="all")
    alloc, down = host_child.host_buffers(M)
    kind, name = case.split(":", 1)
    S = KR.scenes(M.raster_tiling())
    res = {}
    if kind == "cases":
        for tag, sc in S.items():
            if tag.startswith(name) and tag not in KR.NEW:
                res.update({"%s_%s" % (tag, k): v for k, v in KR.run(MR, M, _up, sc, _down).items()})
    elif kind == "new":
        for tag in KR.NEW:
            res.update({"%s_%s" % (tag, k): v for k, v in KR.run(MR, M, _up, S[tag], _down).items()})
    elif kind == "order":
        res = order_runs(MR, M, _up, _down, S)
    elif kind == "fills":
        for tag in FILL_SCENES:
            for fill in FILLS:
                cfg = FILL_CONFIG if S[tag][3] is not None else ("shaded", "shaded", False, False)
                res.update({"%s_%02x_%s" % (tag, fill, k): v for k, v in run_abi(M, MR, alloc, down, S[tag], fill, cfg).items()})
    elif kind == "errors":
        for tag, sc, cfg, mutate, params, drop, _, _ in bad_inputs(S["closed"]):
            res.update({"%s_%s" % (tag, k): v for k, v in run_abi(M, MR, alloc, down, sc, 0x5C, cfg, mutate, params, drop).items()})
    elif kind == "python":
        res = python_runs(MR, M, _up, _down, os.path.dirname(out), device=False)
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=900)
    assert int(res["buffers"]) > 0
    return res


def check_scenes(got_of, names, T):
    for tag in names:
        assert KR.same(got_of(tag), KR.want(tag, T), tag + " ") == []


def _got_of(got):
    return lambda tag: {k[len(tag) + 1:]: v for k, v in got.items() if k.startswith(tag + "_") and not k[len(tag) + 1:].split("_")[0].isdigit()}


def old_names(size, T):
    return [t for t in KR.scenes(T) if t.startswith(size) and t not in KR.NEW]


def check_new(got_of, T):
    check_scenes(got_of, KR.NEW, T)
    S = KR.scenes(T)
    fan = KR.want("fan", T)["normals"]
    up = np.array([0, 0, 1], np.float32)
    assert np.array_equal(fan[72], up) and np.array_equal(fan[0], up) and np.array_equal(fan[71], up)      # unreferenced; poisoned by the NaN face; NaN itself
    assert np.abs(np.linalg.norm(fan[1:70].astype(np.float64), axis=1) - 1).max() < 1e-6 and len(np.unique(fan[1:70], axis=0)) > 60
    assert np.array_equal(KR.want("fan", T)["face_normals"][33], up)                                           # the degenerate face
    z = KR.want("zero_area", T)
    assert (z["normals"] == up).all() and (z["face_normals"] == up).all() and (z["face"] == -1).all()
    c = KR.want("closed", T)
    assert (c["face"] >= 0).mean() > 0.2 and len(np.unique(c["face"])) > 50
    bg = np.asarray(KR.BACKGROUND, np.float32)
    for tag, *_ in KR.configs(S["closed"][3]):
        img = c["image_" + tag]
        assert (img.transpose(0, 2, 3, 1)[c["face"] < 0] == bg).all() and np.isfinite(img).all() and img.min() >= 0 and img.max() <= 1, tag
    assert np.abs(c["bary"].sum(axis=1)[c["face"] >= 0] - 1).max() < 1e-6


@pytest.mark.parametrize("size", ["%dx%d_" % s for s in K.SIZES])
def test_every_case_equals_the_restatement(size, tmp_path):
    got = _emulate("cases:" + size, tmp_path)
    T = tiling()
    check_scenes(_got_of(got), old_names(size, T), T)
    empty = KR.want(size + "nothing", T)
    assert empty["face"].shape == (1,) + K.SIZES[0 if size.startswith("64") else 1][::-1] and (empty["face"] == -1).all() and empty["normals"].shape == (0, 3)
    assert KR.want(size + "no_views", T)["face"].shape[0] == 0 and KR.want(size + "no_views", T)["image_shaded"].shape[0] == 0


def test_the_new_scenes_equal_the_restatement(tmp_path):
    check_new(_got_of(_emulate("new:all", tmp_path)), tiling())


def test_face_order_and_repetition(tmp_path):
    check_order(_emulate("order:all", tmp_path), tiling())


def check_fills(got, T):
    S = KR.scenes(T)
    for tag in FILL_SCENES:
        cfg = FILL_CONFIG if S[tag][3] is not None else ("shaded", "shaded", False, False)
        w = KR.want(tag, T)
        keys = KR.KEYS + ("image_" + cfg[0],)
        for fill in FILLS:
            p = "%s_%02x_" % (tag, fill)
            assert got[p + "rc"].tolist() == [0, 0, 0, 0] and bool(got[p + "guards"]), (p, str(got[p + "error"]))
            assert KR.same({k: got[p + k] for k in keys}, {k: w[k] for k in keys}) == [], p


def test_workspace_and_output_contents_do_not_matter(tmp_path):
    check_fills(host_child.run_child(__file__, "fills:all", tmp_path, timeout=900), tiling())


def test_bad_input_is_refused_with_nothing_written(tmp_path):
    got = host_child.run_child(__file__, "errors:all", tmp_path, timeout=900)
    check_errors(got, KR.scenes(tiling())["closed"])


# ---- the Python layer and the command line -----------------------------------------------------------------------------------------------
def write_cameras_json(path, c2w_list, W, H, fx, fy):
    """what train.py's camera_to_JSON writes: the camera-to-world rotation and position (OpenCV), fx, fy, width, height"""
    import json
    cams = [{"id": i, "img_name": "%05d" % i, "width": W, "height": H, "position": m[:3, 3].tolist(), "rotation": [r.tolist() for r in m[:3, :3]], "fy": fy, "fx": fx}
            for i, m in enumerate(c2w_list)]
    with open(path, "w") as fh:
        json.dump(cams, fh)


def cv_poses(n):
    out = []
    for m in K.orbit(n):
        m = m.copy()
        m[:3, 1:3] *= -1.0
        out.append(m)
    return out


def python_runs(MR, M, up, down, tmp, device):
    """cameras_from_json, turntable, compute_vertex_normals + export, and (on the device) the command line's PNG files"""
    V, F, col = KR.closed_mesh()
    res = {}
    poses = cv_poses(3)
    path = os.path.join(tmp, "cameras.json")
    write_cameras_json(path, poses, 64, 48, 57.6, 57.6)
    cams = MR.cameras_from_json(path)
    rec = np.concatenate([M.raster_views([c["c2w"]], c["H"], c["W"], c["fx"], c["fy"], c["cx"], c["cy"], convention="opencv") for c in cams])
    res["records"] = np.frombuffer(rec.tobytes(), np.uint8)
    res["records_want"] = np.frombuffer(M.raster_views(poses, 48, 64, 57.6, 57.6, 32.0, 24.0, convention="opencv").tobytes(), np.uint8)
    mesh = M.DeviceMesh(V, F, colors=col)
    t = MR.turntable(mesh, 5, 48, 64)
    res["turntable"] = np.stack(t["c2w"])
    res["turntable_centre"], res["turntable_radius"], res["turntable_fx"] = np.asarray(t["centre"]), np.asarray(t["radius"]), np.asarray(t["fx"])
    img, aux = MR.render(mesh, t["c2w"], 48, 64, t["fx"], t["fy"], t["cx"], t["cy"], mode="shaded", aux=True)
    res["turntable_image"], res["turntable_face"] = down(img), down(aux["face"])
    assert mesh.vertex_normals is not None                                                # computed once, kept
    res["mesh_normals"] = mesh.vertex_normals
    plain = M.DeviceMesh(V, F)
    assert plain.vertex_normals is None and plain.compute_vertex_normals() is plain
    ply = os.path.join(tmp, "with_normals.ply")
    plain.export(ply)
    res["ply_normals"] = M.load(ply).vertex_normals
    return res


def check_python(res):
    V, F, col = KR.closed_mesh()
    assert res["records"].tobytes() == res["records_want"].tobytes()
    c2w, centre, radius = res["turntable"], res["turntable_centre"], float(res["turntable_radius"])
    lo, hi = V.astype(np.float64).min(axis=0), V.astype(np.float64).max(axis=0)
    assert np.allclose(centre, (lo + hi) / 2) and radius == pytest.approx(1.5 * np.linalg.norm(hi - lo) / 2)
    assert float(res["turntable_fx"]) == pytest.approx(32.0 / np.tan(np.radians(25.0)))
    for m in c2w:
        eye, fwd = m[:3, 3], m[:3, 2]
        assert np.allclose(m[:3, :3] @ m[:3, :3].T, np.eye(3), atol=1e-12) and np.linalg.det(m[:3, :3]) == pytest.approx(1.0)
        assert np.allclose(eye + fwd * radius, centre, atol=1e-9)                         # looks at the centre from the radius
        assert (eye - centre)[2] / radius == pytest.approx(np.sin(np.radians(20.0))) and m[2, 1] < 0      # raised by 20 degrees; +y (down) points down
    assert len(np.unique(np.round(c2w[:, :3, 3], 9), axis=0)) == 5
    recs = R.records(list(c2w), 48, 64, float(res["turntable_fx"]), float(res["turntable_fx"]), 32.0, 24.0, 0.01, 1e3, "opencv")
    depth, face = RR.render_faces(V, F, recs, (48, 64))
    normals = RR.vertex_normals(V, F)
    img, _ = RR.shade(V, F, recs, face, (48, 64), RR.SHADED, normals=normals, base=(0.8, 0.8, 0.8), ambient=0.25, background=(1.0, 1.0, 1.0))
    assert np.array_equal(res["turntable_face"], face) and (face >= 0).mean() > 0.1
    assert np.array_equal(res["turntable_image"].view(np.uint32), img.view(np.uint32))
    assert np.array_equal(res["mesh_normals"].view(np.uint32), normals.view(np.uint32)) and np.array_equal(res["ply_normals"].view(np.uint32), normals.view(np.uint32))


def test_python_layer(tmp_path):
    check_python(_emulate("python:all", tmp_path))


# ---- without the emulator ----------------------------------------------------------------------------------------------------
ANCHOR_SCENES = ("64x48_views", "70x33_views", "closed", "closed_plain", "64x48_near_fan", "70x33_near", "64x48_quad", "70x33_whole_image", "fan")


def test_the_restatement_agrees_with_a_ray_cast():
    """The contract against geometry: at every pixel that no projected edge comes within 1/128 pixel of and whose two nearest hits
    differ by more than §3.19's depth tolerance, the restated face is the ray cast's nearest, so the barycentrics -- the same formula
    over the same face -- have the same bits; they also are the ray cast's own (Moeller-Trumbore u, v) to rounding.  The share of the
    covered pixels left out is printed and stays below 25 % on every scene."""
    T = tiling()
    S = KR.scenes(T)
    worst = 0.0
    for tag in ANCHOR_SCENES:
        V, F, views, _ = S[tag]
        w = KR.want(tag, T)
        for k, rec in enumerate(K.recs_of(views)):
            face, uv, judged, covered = RR.anchor(V, F, rec)
            left_out = float((covered & ~judged).sum()) / max(int(covered.sum()), 1)
            print("%s view %d: %d covered pixels, %.1f %% left out" % (tag, k, int(covered.sum()), 100 * left_out))
            assert left_out < 0.25, (tag, k, left_out)
            assert np.array_equal(w["face"][k][judged], face[judged]), (tag, k)
            lam, _ = RR.barycentrics(V, F, rec, np.where(judged, face, -1))
            got = w["bary"][k].transpose(1, 2, 0)
            hit = judged & (face >= 0)
            assert np.array_equal(got[hit].view(np.uint32), lam[hit].astype(np.float32).view(np.uint32)), (tag, k)
            mt = np.stack([1 - uv[..., 0] - uv[..., 1], uv[..., 0], uv[..., 1]], axis=-1)
            if hit.any():
                worst = max(worst, float(np.abs(lam[hit] - mt[hit]).max()))
    print("largest difference between the restated barycentrics and Moeller-Trumbore's: %.3g" % worst)
    assert worst < 1e-9


def test_normals_against_an_independent_form():
    """the closed mesh: np.add.at over unnormalised face crosses in fp64, another summation order: within 4 ulp of float32"""
    V, F, _ = KR.closed_mesh()
    V64 = V.astype(np.float64)
    n = np.cross(V64[F[:, 1]] - V64[F[:, 0]], V64[F[:, 2]] - V64[F[:, 0]])
    acc = np.zeros_like(V64)
    for k in (2, 1, 0):
        np.add.at(acc, F[:, k], n)
    ref = acc / np.linalg.norm(acc, axis=1, keepdims=True)
    got = RR.vertex_normals(V, F).astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(got - ref) / ulp).max())
    print("largest difference from np.add.at: %.3f ulp of float32" % worst)
    assert np.isfinite(ref).all() and worst <= 4.0


def test_size_queries_and_versions():
    import mesh_cull as M
    import mesh_render as MR
    L = M.lib
    assert L.gof_mesh_render_abi_version() == 4
    assert L.gof_mesh_raster_abi_version() == 3 and L.gof_mesh_abi_version() == 2 and L.gof_abi_version() == 12
    per_pixel = L.gof_mesh_render_faces_ws_bytes(1000, 2, 1920 * 1080) - L.gof_mesh_render_depth_ws_bytes(1000)
    assert abs(per_pixel - 8 * 2 * 1920 * 1080) < 1024                                   # 8 bytes per pixel and view on top of (e)'s
    assert L.gof_mesh_render_faces_ws_bytes(1000, -1, 64) == 0 and L.gof_mesh_render_faces_ws_bytes(1000, 1, -1) == 0
    assert 0 < L.gof_mesh_shade_ws_bytes() < 4096 and 0 < L.gof_mesh_face_normals_ws_bytes() < 4096
    assert 0 < L.gof_mesh_vertex_normals_ws_bytes(0, 0) < L.gof_mesh_vertex_normals_ws_bytes(10 ** 6, 2 * 10 ** 6) < 256 * 10 ** 6
    assert L.gof_mesh_vertex_normals(-1, None, 0, None, None, None, 0, None) < 0
    assert L.gof_mesh_render_faces(3, None, (2 ** 31 + 2) // 3, None, 0, None, 0, None, None, None, None, 0, None) < 0 and b"2^31" in L.gof_last_error()
    assert C.sizeof(MR.GofShadeParams) == 64 and hasattr(M.DeviceMesh, "compute_vertex_normals")
    with pytest.raises(ValueError, match="mode"):
        MR.render(None, [], 4, 4, 1.0, 1.0, 0.0, 0.0, mode="wireframe")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
