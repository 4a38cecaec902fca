"""CPU tests of the DTU Chamfer evaluation: the kernels of csrc/cloud.hip through the host emulator
(tests/hipemu) behind mesh_eval's own Python layer, each run in a child process (an emulator abort fails one test, not the
session), held to tests/mesh_eval_restatement.py with equalities: sample coordinates, keep masks and nearest distances bit for bit.

In the child the product module runs unchanged except for three test seams (tests/hipemu/host_child.py): GOF_HIP_LIB names the
emulated library, the device check / stream / device context are replaced by host stand-ins, and every workspace mesh_eval
allocates is filled with 0xA5 and followed by guard bytes that are checked after the run.  Sizes stay at or below 50 k points per case."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import host_child  # noqa: E402
from host_child import PKG  # noqa: E402
import mesh_eval_restatement as R  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def torus(nu, nv, R0=20.0, r0=6.0, noise=0.0, seed=0):
    """a torus mesh with float32-rounded vertices -> (vertices float64 (nu nv, 3), triangles int32)"""
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    P = np.stack([(R0 + r0 * np.cos(v)) * np.cos(u), (R0 + r0 * np.cos(v)) * np.sin(u), r0 * np.sin(v)], -1).reshape(-1, 3)
    if noise:
        P = P + np.random.default_rng(seed).normal(scale=noise, size=P.shape)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    T = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return P.astype(np.float32).astype(np.float64), T.astype(np.int32)


def sample_case(name):
    """-> (vertices, triangles, thresh)"""
    rng = np.random.default_rng(3)
    if name == "torus":
        return torus(48, 24) + (0.5,)
    if name == "degenerate":
        V, T = torus(12, 8)
        extra = np.array([[0, 0, 0], [0, 1, 1], [5, 5, 5], [3, 3, 7],          # repeated vertices: zero area
                          [0, 1, 2]], np.int32)
        V = np.vstack([V, [[1, 1, 1], [2, 2, 2], [3, 3, 3],                     # a collinear triple (zero area with distinct vertices)
                           [0, 0, 0], [0.3, 0, 0], [0, 0.3, 0],                   # a triangle smaller than the lattice: n1 = n2 = 0
                           [0, 0, 0], [30, 0, 0], [0, 0.6, 0]]])                  # a sliver: n2 small, n1 large
        n = len(V) - 9
        extra = np.vstack([extra, [[n, n + 1, n + 2], [n + 3, n + 4, n + 5], [n + 6, n + 7, n + 8], [n + 7, n + 8, n + 6]]]).astype(np.int32)
        return V, np.vstack([T[:40], extra, T[40:]]).astype(np.int32), 0.5
    if name == "balance":
        # one triangle with ~4e4 samples between 10^4 triangles that are too small for any
        small = rng.random((10000, 3, 3)) * 0.05 + rng.random((10000, 1, 3)) * 50
        V = np.vstack([small.reshape(-1, 3), [[0, 0, 0], [150, 0, 3], [0, 150, 5]]])
        T = np.arange(30000, dtype=np.int32).reshape(-1, 3)
        T = np.vstack([T[:5000], [[30000, 30001, 30002]], T[5000:]]).astype(np.int32)
        return V, T, 0.5
    raise KeyError(name)


def thin_case(name):
    """-> (points in visiting order, r)"""
    if name in ("n0", "n1"):
        return np.zeros((int(name[1]), 3)) + 0.25, 0.5
    if name == "straddle":
        return R.straddle_cloud(), 0.5
    if name == "lattice":
        g = np.arange(16, dtype=np.float64) * 0.5              # exact in binary: every neighbour pair is an equality of the <=
        L = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return L[np.random.default_rng(2).permutation(len(L))], 0.5
    V, T, th = sample_case("torus")
    P = R.sample_mesh(V, T, th)
    if name.startswith("rand"):
        return P[np.random.default_rng(int(name[4:])).permutation(len(P))], 0.5
    if name == "morton":
        q = ((P - P.min(0)) / (P.max(0) - P.min(0)) * 1023).astype(np.int64)
        code = np.zeros(len(P), np.int64)
        for b in range(10):
            for c in range(3):
                code |= ((q[:, c] >> b) & 1) << (3 * b + c)
        return P[np.argsort(code, kind="stable")], 0.5
    if name == "dups":
        rng = np.random.default_rng(9)
        Q = np.vstack([P[:6000], P[:6000], P[:3000]])
        return Q[rng.permutation(len(Q))], 0.5
    raise KeyError(name)


def nn_case(name):
    """-> (query, ref)"""
    rng = np.random.default_rng(5)
    if name == "clouds":
        V, T, th = sample_case("torus")
        S = R.sample_mesh(V, T, th)
        Q = S[rng.permutation(len(S))[:20000]]
        Q = Q + rng.normal(scale=0.3, size=Q.shape)
        return Q, S
    if name == "ties":
        g = np.arange(12, dtype=np.float64)
        S = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        S = np.vstack([S, S])[rng.permutation(2 * len(S))]                      # every point twice: each minimum is a tie
        Q = np.vstack([S[:500] + 0.5, rng.random((1500, 3)) * 11])              # cell centres: eight-fold ties
        return Q, S
    if name == "far":
        S = rng.random((5000, 3))
        Q = np.vstack([rng.random((500, 3)) * 2e3 - 1e3, rng.random((500, 3)) + [50, 0, 0], rng.random((100, 3))])
        return Q, S
    if name == "one":
        return rng.random((700, 3)), rng.random((1, 3))
    if name == "empty":
        return rng.random((300, 3)), np.zeros((0, 3))
    if name == "scales":
        S = np.vstack([rng.random((3000, 3)) * 1e-3, rng.random((3000, 3)) * 1e3])
        Q = np.vstack([rng.random((1000, 3)) * 1e-3, rng.random((1000, 3)) * 1e3, rng.random((500, 3))])
        return Q, S
    if name == "groups":                                  # 32 full boxes = one full group, then a 33rd box of one point in a second group
        return rng.random((257, 3)), rng.random((8193, 3))
    raise KeyError(name)


def write_scan(root, scan=7):
    """a synthetic scan in DTU's file layout under `root`; -> dict(mesh=path, pcd=path, obs, bb, res, plane, stl, V, T)"""
    from scipy.io import savemat
    import mesh_eval
    rng = np.random.default_rng(21)
    u, v = rng.random(15000) * 2 * np.pi, rng.random(15000) * 2 * np.pi
    stl = np.stack([(20 + 6 * np.cos(v)) * np.cos(u), (20 + 6 * np.cos(v)) * np.sin(u), 6 * np.sin(v)], -1).astype(np.float32).astype(np.float64)
    bb = np.array([[-24.0, -30.0, -8.0], [30.0, 30.0, 8.0]])
    res = 1.0
    obs = np.ones((55, 61, 17), np.uint8)
    obs[:10, :, :] = 0
    obs[:, 40:45, 3:9] = 0
    plane = np.array([[0.01], [0.02], [1.0], [4.5]])
    os.makedirs(os.path.join(root, "ObsMask"), exist_ok=True)
    os.makedirs(os.path.join(root, "Points", "stl"), exist_ok=True)
    savemat(os.path.join(root, "ObsMask", "ObsMask%d_10.mat" % scan), {"ObsMask": obs, "BB": bb, "Res": np.array([[res]])})
    savemat(os.path.join(root, "ObsMask", "Plane%d.mat" % scan), {"P": plane})
    mesh_eval.write_vis_ply(os.path.join(root, "Points", "stl", "stl%03d_total.ply" % scan), stl, np.zeros_like(stl))
    V, T = torus(40, 20, noise=0.15, seed=4)
    mesh = os.path.join(root, "mesh.ply")
    with open(mesh, "wb") as f:                                                 # binary, float coordinates + colours, uchar/int faces
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(V), len(T))).encode())
        vr = np.zeros(len(V), [("p", "<f4", 3), ("c", "u1", 3)])
        vr["p"] = V
        f.write(vr.tobytes())
        fr = np.zeros(len(T), [("n", "u1"), ("i", "<i4", 3)])
        fr["n"], fr["i"] = 3, T
        f.write(fr.tobytes())
    pcd = os.path.join(root, "cloud.ply")
    cloud = R.sample_mesh(V, T, 0.5)[::3]
    with open(pcd, "w") as f:                                                   # ASCII, double coordinates + normals
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(cloud))
        for p in cloud:
            f.write("%r %r %r 0 0 1\n" % (float(p[0]), float(p[1]), float(p[2])))
    return dict(mesh=mesh, pcd=pcd, cloud=cloud, obs=obs, bb=bb, res=res, plane=plane.reshape(-1), stl=stl, V=V, T=T, scan=scan)


# ---------------------------------------------------------------------------------------------------------------------------
# the child: mesh_eval over the emulated library
# ---------------------------------------------------------------------------------------------------------------------------
def _child(case, out):
    import torch
    import mesh_eval as M
    check = host_child.install_seams(M)
    kind, name = case.split(":", 1)
    res = {}
    tt = torch.from_numpy
    if kind == "sample":
        V, T, th = sample_case(name)
        res["points"] = M.sample_mesh(tt(V), tt(T), th).numpy()
    elif kind == "sample_bad":
        V, T, th = sample_case("degenerate")
        if name == "nan":
            V = V.copy()
            V[5, 1] = np.nan
        else:
            T = T.copy()
            T[7, 2] = len(V)
        try:
            M.sample_mesh(tt(V), tt(T), th)
            res["error"] = np.array("")
        except RuntimeError as e:
            res["error"] = np.array(str(e))
    elif kind == "thin":
        P, r = thin_case(name)
        res["keep"] = M.thin(tt(np.ascontiguousarray(P)), r).numpy()
        res["stats"] = np.array(json.dumps(M.last_stats()["thin"]))
    elif kind == "nn":
        Q, S = nn_case(name)
        d, i = M.nearest(tt(np.ascontiguousarray(Q)), tt(np.ascontiguousarray(S)))
        res["dist"], res["idx"] = d.numpy(), i.numpy()
        res["stats"] = np.array(json.dumps(M.last_stats()["nearest"]))
    elif kind == "chamfer":
        sc = write_scan(os.path.join(os.path.dirname(out), "scan_" + name))
        data = (tt(sc["V"]), tt(sc["T"])) if name == "mesh" else tt(np.ascontiguousarray(sc["cloud"]))
        r = M.dtu_chamfer(data, sc["obs"], sc["bb"], sc["res"], sc["plane"], tt(sc["stl"]), mode=name, downsample_density=0.5, seed=3)
        res = {k: (v.numpy() if isinstance(v, torch.Tensor) else np.array(v)) for k, v in r.items()}
    elif kind == "cli":
        root = os.path.join(os.path.dirname(out), "scan_cli_" + name)
        sc = write_scan(root)
        for run in ("a", "b"):
            vis = os.path.join(root, "vis_" + run)
            M.main(["--data", sc["mesh"] if name == "mesh" else sc["pcd"], "--scan", str(sc["scan"]), "--mode", name, "--dataset_dir", root,
                    "--vis_out_dir", vis, "--downsample_density", "0.5", "--seed", "3"])
        res["root"] = np.array(root)
    else:
        raise KeyError(case)
    res["workspaces"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path, order=None):
    res = host_child.run_child(__file__, case, tmp_path, order=order, timeout=1800)
    assert int(res["workspaces"]) > 0 or case.startswith("cli")
    return res


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["torus", "degenerate", "balance"])
def test_sampling_is_bit_equal(name, tmp_path):
    V, T, th = sample_case(name)
    want, counts = R.sample_triangles(V, T, th)
    if name == "balance":
        assert counts.max() > 30000 and (counts > 0).sum() == 1
    if name == "degenerate":
        assert (counts == 0).sum() >= 6 and counts.max() > 20      # 4 repeated-vertex, 1 collinear, 1 below the lattice
    got = _emulate("sample:" + name, tmp_path)["points"]
    assert got.shape == (len(V) + len(want), 3), "%d samples, the restatement has %d" % (len(got) - len(V), len(want))
    assert np.array_equal(bits(got[:len(V)]), bits(V))
    assert np.array_equal(bits(got[len(V):]), bits(want))


@pytest.mark.parametrize("name", ["nan", "index"])
def test_bad_meshes_are_refused(name, tmp_path):
    err = str(_emulate("sample_bad:" + name, tmp_path)["error"])
    assert ("not finite" in err) if name == "nan" else ("outside" in err), err


THIN_CASES = ["rand1", "rand2", "rand3", "morton", "dups", "lattice", "n0", "n1", "straddle"]


def check_thin_case(name, P, r):
    """what a case promises before anything is compared"""
    if name.startswith("rand") or name in ("morton", "straddle"):
        assert R.pairs_near_radius(P, r) == 0          # no pair within 4 ulp of r^2: nothing may be left out of the comparison
    if name == "straddle":
        R.check_straddle(P, np.floor((P - P.min(0)) / (r * (1.0 + 1.0 / 1048576.0))).astype(np.int64))      # thin's cells


@pytest.mark.parametrize("name", THIN_CASES)
def test_thinning_equals_the_sequential_loop(name, tmp_path):
    P, r = thin_case(name)
    want = R.thin(P, r)
    check_thin_case(name, P, r)
    res = _emulate("thin:" + name, tmp_path)
    assert np.array_equal(res["keep"], want), "%d of %d points differ" % ((res["keep"] != want).sum(), len(P))
    st = json.loads(str(res["stats"]))
    assert st["kept"] == want.sum()
    if len(P) > 1:
        assert st["rounds"] >= 1 and st["distance_evaluations"] > 0 and st["read_backs"] <= st["rounds"]


def test_the_loop_is_the_definition():
    """the yardstick against the definition it restates (brute force, small)"""
    P, r = thin_case("rand1")
    assert np.array_equal(R.thin(P[:3000], r), R.thin_brute(P[:3000], r))
    Q, S = nn_case("clouds")
    d, i = R.nearest(Q[:300], S)
    db, ib = R.nearest_brute(Q[:300], S)
    assert np.array_equal(bits(d), bits(db)) and np.array_equal(i, ib)


@pytest.mark.parametrize("order", ["reverse", "random:5"])
@pytest.mark.parametrize("name", ["rand1", "lattice"])
def test_thinning_does_not_depend_on_the_schedule(name, order, tmp_path):
    P, r = thin_case(name)
    assert np.array_equal(_emulate("thin:" + name, tmp_path, order=order)["keep"], R.thin(P, r))


@pytest.mark.parametrize("name", ["clouds", "ties", "far", "one", "empty", "scales", "groups"])
def test_nearest_is_exact(name, tmp_path):
    Q, S = nn_case(name)
    res = _emulate("nn:" + name, tmp_path)
    d, i = R.nearest(Q, S)
    assert np.array_equal(bits(res["dist"]), bits(d))
    if name == "empty":
        assert np.isinf(res["dist"]).all() and (res["idx"] == -1).all()
        return
    pick = np.random.default_rng(0).permutation(len(Q))[:400]
    db, ib = R.nearest_brute(Q[pick], S)
    assert np.array_equal(bits(res["dist"][pick]), bits(db))
    assert np.array_equal(res["idx"][pick], ib), "not the smallest index of the minimisers"
    if name in ("clouds", "far", "scales", "groups"):    # unique minima: the kd-tree's index as well
        assert np.array_equal(res["idx"], i)
    if name == "clouds":
        st = json.loads(str(res["stats"]))
        assert 0 < st["boxes_per_query"] < 0.5 * (len(S) / 256), "the pruning does not prune"


@pytest.mark.parametrize("mode", ["mesh", "pcd"])
def test_dtu_chamfer_equals_the_restatement(mode, tmp_path):
    res = _emulate("chamfer:" + mode, tmp_path)
    sc = write_scan(str(tmp_path / "again"))
    cloud = R.sample_mesh(sc["V"], sc["T"], 0.5) if mode == "mesh" else sc["cloud"]
    perm = np.random.default_rng(3).permutation(len(cloud))
    want = R.dtu_chamfer(cloud, perm, sc["obs"], sc["bb"], sc["res"], sc["plane"], sc["stl"], thresh=0.5)
    for k in ("data_down", "dist_d2s", "dist_s2d"):
        assert np.array_equal(bits(res[k]), bits(want[k])), k
    for k in ("idx_d2s", "idx_s2d", "d2s_index", "s2d_index"):
        assert np.array_equal(res[k], want[k]), k
    assert 0 < len(want["d2s_index"]) < len(want["data_down"]) and 0 < len(want["s2d_index"]) < len(sc["stl"])      # the masks and the plane bite
    # the two means: torch and numpy add the same terms in different orders (fp64 sums of <= 10^7 terms of one sign): 1e-12 relative
    for k in ("mean_d2s", "mean_s2d", "overall"):
        assert abs(float(res[k]) - want[k]) <= 1e-12 * abs(want[k]), (k, float(res[k]), want[k])


@pytest.mark.parametrize("mode", ["mesh", "pcd"])
def test_command_line_writes_results_and_clouds(mode, tmp_path):
    import mesh_eval
    root = str(_emulate("cli:" + mode, tmp_path)["root"])
    sc = write_scan(str(tmp_path / "again"))
    # the file readers give back what was written (float coordinates widen exactly)
    v, t = mesh_eval.read_ply(sc["mesh"])
    assert np.array_equal(v, sc["V"]) and np.array_equal(t, sc["T"])
    v, t = mesh_eval.read_ply(sc["pcd"])
    assert np.array_equal(bits(v), bits(sc["cloud"])) and t is None
    cloud = R.sample_mesh(sc["V"], sc["T"], 0.5) if mode == "mesh" else sc["cloud"]
    want = R.dtu_chamfer(cloud, np.random.default_rng(3).permutation(len(cloud)), sc["obs"], sc["bb"], sc["res"], sc["plane"], sc["stl"], thresh=0.5)
    got = json.load(open(os.path.join(root, "vis_a", "results.json")))
    assert sorted(got) == ["mean_d2s", "mean_s2d", "overall"]
    for k in got:
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k])
    d2s, _ = mesh_eval.read_ply(os.path.join(root, "vis_a", "vis_%03d_d2s.ply" % sc["scan"]))
    s2d, _ = mesh_eval.read_ply(os.path.join(root, "vis_a", "vis_%03d_s2d.ply" % sc["scan"]))
    assert np.array_equal(bits(d2s), bits(want["data_down"])) and np.array_equal(bits(s2d), bits(sc["stl"]))
    for f in ("results.json", "vis_%03d_d2s.ply" % sc["scan"], "vis_%03d_s2d.ply" % sc["scan"]):      # two runs, identical bytes
        assert open(os.path.join(root, "vis_a", f), "rb").read() == open(os.path.join(root, "vis_b", f), "rb").read(), f


def test_host_tensors_are_refused():
    import torch
    import mesh_eval
    with pytest.raises(RuntimeError, match="ROCm device"):
        mesh_eval.thin(torch.zeros((4, 3), dtype=torch.float64), 0.5)
    with pytest.raises(RuntimeError, match="ROCm device"):
        mesh_eval.nearest(torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="ROCm device"):
        mesh_eval.sample_mesh(torch.zeros((4, 3), dtype=torch.float64), torch.zeros((1, 3), dtype=torch.int32), 0.5)


def test_size_queries_and_argument_checks():
    import mesh_eval
    L = mesh_eval.lib
    assert 0 < L.gof_cloud_thin_ws_bytes(1000) < L.gof_cloud_thin_ws_bytes(100000)
    assert L.gof_cloud_thin_ws_bytes(1_000_000) < 120 * 1_000_000
    assert 0 < L.gof_cloud_nn_index_bytes(0) < L.gof_cloud_nn_index_bytes(100000)
    assert 0 < L.gof_cloud_sample_ws_bytes(0) < L.gof_cloud_sample_ws_bytes(100000)
    import ctypes as C
    n = C.c_int64()
    assert L.gof_cloud_thin(5, None, -1.0, None, None, 0, C.byref(n), None) < 0 and b"positive" in L.gof_last_error()
    assert L.gof_cloud_sample_count(0, None, -1, None, 0.5, None, 0, C.byref(n), None) < 0
    assert L.gof_cloud_nn_build(2 ** 31, None, None, 0, None) < 0


def test_launcher_sends_the_evaluation_in_process(tmp_path, monkeypatch):
    """evaluate_dtu_mesh.py shells out to dtu_eval/eval.py (os.system): under the launcher that command runs mesh_eval's command line
    in-process, every other command reaches the real os.system, and GOF_DTU_EVAL_SUBPROCESS=1 leaves the script alone."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher_eval", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    import mesh_eval
    calls, real = [], []
    monkeypatch.setattr(mesh_eval, "main", lambda argv=None: calls.append(list(argv)))
    monkeypatch.setattr(os, "system", lambda cmd: real.append(cmd) or 0)
    script = tmp_path / "evaluate_dtu_mesh.py"
    script.write_text(
        "import os\n"
        "def run():\n"
        "    cmd = f\"python dtu_eval/eval.py --data {'a b.ply'!r} --scan 24 --mode mesh --dataset_dir /d --vis_out_dir /o\"\n"
        "    rc = os.system(cmd)\n"
        "    os.system('echo other')\n"
        "    assert os.path.basename('/x/y') == 'y' and rc == 0\n"
        "if __name__ == '__main__':\n"
        "    run()\n")
    monkeypatch.delenv("GOF_DTU_EVAL_SUBPROCESS", raising=False)
    L.run_script(str(script), L.dtu_eval_rebinding(str(script)))
    assert calls == [["--data", "a b.ply", "--scan", "24", "--mode", "mesh", "--dataset_dir", "/d", "--vis_out_dir", "/o"]]
    assert real == ["echo other"]
    monkeypatch.setenv("GOF_DTU_EVAL_SUBPROCESS", "1")
    L.run_script(str(script), L.dtu_eval_rebinding(str(script)))
    assert len(calls) == 1 and len(real) == 3 and real[1].startswith("python dtu_eval/eval.py")
    assert L.dtu_eval_rebinding(str(tmp_path / "train.py")) == {}


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
