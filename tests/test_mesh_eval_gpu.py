"""GPU tests of the DTU Chamfer evaluation: the cases of tests/test_mesh_eval_host.py on the device, a
marching-cubes mesh from tsdf_fusion, and one large case (>= 5 M sampled points thinned, a 2 M-point scan, both directions), all
held to tests/mesh_eval_restatement.py with the same equalities: coordinates, masks and distances bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mesh_eval_restatement as R  # noqa: E402
import test_mesh_eval_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
bits = H.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["torus", "degenerate", "balance", "balance_1m"])
def test_sampling_is_bit_equal(name):
    import mesh_eval as M
    if name == "balance_1m":                              # one triangle with 10^6 samples next to 10^4 with none
        V, T, th = H.sample_case("balance")
        V = V.copy()
        V[-2:] = [[710, 0, 3], [0, 710, 5]]
    else:
        V, T, th = H.sample_case(name)
    want, counts = R.sample_triangles(V, T, th)
    if name == "balance_1m":
        assert counts.max() >= 10 ** 6 and (counts > 0).sum() == 1
    got = M.sample_mesh(dev(V), dev(T), th).cpu().numpy()
    assert got.shape == (len(V) + len(want), 3), "%d samples, the restatement has %d" % (len(got) - len(V), len(want))
    assert np.array_equal(bits(got[:len(V)]), bits(V)) and np.array_equal(bits(got[len(V):]), bits(want))


def test_sampling_a_marching_cubes_mesh():
    """a mesh as extract_mesh_tsdf.py writes it: fused depth maps of a sphere, marching cubes on the device"""
    import mesh_eval as M
    from tsdf_fusion import TSDFVolume
    Hh, Ww, f = 120, 160, 140.0
    K = torch.tensor([[f, 0, Ww / 2], [0, f, Hh / 2], [0, 0, 1]], dtype=torch.float64)
    v, u = torch.meshgrid(torch.arange(Hh, dtype=torch.float64), torch.arange(Ww, dtype=torch.float64), indexing="ij")
    d = torch.stack([(u - Ww / 2) / f, (v - Hh / 2) / f, torch.ones_like(u)], -1)
    # ray / sphere (centre (0,0,2), radius 0.5): depth = z of the first hit
    c = torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64)
    b = (d * c).sum(-1)
    disc = b * b - (d * d).sum(-1) * ((c * c).sum() - 0.25)
    t = torch.where(disc > 0, (b - disc.clamp(min=0).sqrt()) / (d * d).sum(-1), torch.zeros_like(b))
    depth = t.float().cuda()
    color = torch.full((Hh, Ww, 3), 0.5, dtype=torch.float32).cuda()
    vol = TSDFVolume(voxel_size=0.02, device="cuda")
    for _ in range(4):                                    # (extract_triangle_mesh wants weight >= 3)
        vol.integrate(depth, color, K.float().cuda(), torch.eye(4, dtype=torch.float32).cuda())
    mesh = vol.extract_triangle_mesh()
    V = mesh.vertices.double().cpu().numpy()
    T = mesh.triangles.cpu().numpy().astype(np.int32)
    assert len(T) > 1000
    want, _ = R.sample_triangles(V, T, 0.004)
    got = M.sample_mesh(dev(V), dev(T), 0.004).cpu().numpy()
    assert len(want) > 10000 and got.shape == (len(V) + len(want), 3)
    assert np.array_equal(bits(got[len(V):]), bits(want))


@pytest.mark.parametrize("name", H.THIN_CASES)
def test_thinning_equals_the_sequential_loop(name):
    import mesh_eval as M
    P, r = H.thin_case(name)
    want = R.thin(P, r)
    H.check_thin_case(name, P, r)
    got = M.thin(dev(P), r).cpu().numpy()
    assert np.array_equal(got, want), "%d of %d points differ" % ((got != want).sum(), len(P))
    assert M.last_stats()["thin"]["kept"] == want.sum()


@pytest.mark.parametrize("name", ["clouds", "ties", "far", "one", "empty", "scales", "groups"])
def test_nearest_is_exact(name):
    import mesh_eval as M
    Q, S = H.nn_case(name)
    d, i = M.nearest(dev(Q), dev(S))
    d, i = d.cpu().numpy(), i.cpu().numpy()
    dr, ir = R.nearest(Q, S)
    assert np.array_equal(bits(d), bits(dr))
    if name == "empty":
        assert np.isinf(d).all() and (i == -1).all()
        return
    pick = np.random.default_rng(0).permutation(len(Q))[:400]
    db, ib = R.nearest_brute(Q[pick], S)
    assert np.array_equal(bits(d[pick]), bits(db)) and np.array_equal(i[pick], ib)
    if name in ("clouds", "far", "scales", "groups"):
        assert np.array_equal(i, ir)


@pytest.mark.parametrize("mode", ["mesh", "pcd"])
def test_command_line_equals_the_restatement(mode, tmp_path):
    import mesh_eval as M
    sc = H.write_scan(str(tmp_path / "scan"))
    outs = []
    for run in ("a", "b"):
        vis = str(tmp_path / ("vis_" + run))
        res = M.main(["--data", sc["mesh"] if mode == "mesh" else sc["pcd"], "--scan", str(sc["scan"]), "--mode", mode, "--dataset_dir", str(tmp_path / "scan"),
                      "--vis_out_dir", vis, "--downsample_density", "0.5", "--seed", "3"])
        outs.append(vis)
    cloud = R.sample_mesh(sc["V"], sc["T"], 0.5) if mode == "mesh" else sc["cloud"]
    want = R.dtu_chamfer(cloud, np.random.default_rng(3).permutation(len(cloud)), sc["obs"], sc["bb"], sc["res"], sc["plane"], sc["stl"], thresh=0.5)
    for k in ("data_down", "dist_d2s", "dist_s2d"):
        assert np.array_equal(bits(res[k].cpu().numpy()), bits(want[k])), k
    for k in ("idx_d2s", "idx_s2d", "d2s_index", "s2d_index"):
        assert np.array_equal(res[k].cpu().numpy(), want[k]), k
    got = json.load(open(os.path.join(outs[0], "results.json")))
    assert sorted(got) == ["mean_d2s", "mean_s2d", "overall"]
    for k in got:                                          # the device's sum and numpy's add the same terms in different orders: 1e-12 relative
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    for f in ("vis_%03d_d2s.ply" % sc["scan"], "vis_%03d_s2d.ply" % sc["scan"]):
        pts, _ = M.read_ply(os.path.join(outs[0], f))
        assert len(pts) == (len(want["data_down"]) if "d2s" in f else len(sc["stl"]))
    for f in ("results.json", "vis_%03d_d2s.ply" % sc["scan"], "vis_%03d_s2d.ply" % sc["scan"]):
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f


def test_large_cloud_both_directions():
    """>= 5 M sampled points thinned, a 2 M-point scan, nearest distances in both directions, against the restatement on the CPUs"""
    import mesh_eval as M
    V, T = H.torus(400, 200)
    th = 0.0232
    pts = M.sample_mesh(dev(V), dev(T), th)
    n = int(pts.size(0))
    assert n - len(V) >= 5_000_000, n
    want_pts = R.sample_mesh(V, T, th)
    assert np.array_equal(bits(pts.cpu().numpy()), bits(want_pts))
    perm = np.random.default_rng(1).permutation(n)
    shuffled = pts[torch.from_numpy(perm).cuda()]
    keep = M.thin(shuffled, th)
    st = M.last_stats()["thin"]
    print("thin:", st)
    want_keep = R.thin(want_pts[perm], th)
    got_keep = keep.cpu().numpy()
    assert np.array_equal(got_keep, want_keep), "%d of %d points differ" % ((got_keep != want_keep).sum(), n)
    down = shuffled[keep]
    rng = np.random.default_rng(8)
    u, v = rng.random(2_000_000) * 2 * np.pi, rng.random(2_000_000) * 2 * np.pi
    stl = np.stack([(20 + 6.05 * np.cos(v)) * np.cos(u), (20 + 6.05 * np.cos(v)) * np.sin(u), 6.05 * np.sin(v)], -1).astype(np.float32).astype(np.float64)
    down_np = down.cpu().numpy()
    for q, s in ((down, dev(stl)), (dev(stl), down)):
        d, i = M.nearest(q, s)
        print("nearest:", M.last_stats()["nearest"])
        dr, ir = R.nearest(q.cpu().numpy(), s.cpu().numpy())
        assert np.array_equal(bits(d.cpu().numpy()), bits(dr))
        # indices: equal where the minimum is unique; where they differ the two candidates are equally far and ours is the smaller
        i_np, q_np, s_np = i.cpu().numpy(), q.cpu().numpy(), s.cpu().numpy()
        diff = np.nonzero(i_np != ir)[0]
        if len(diff):
            def d2(a, b):
                e = a - b
                return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            assert np.array_equal(d2(q_np[diff], s_np[i_np[diff]]), d2(q_np[diff], s_np[ir[diff]])) and (i_np[diff] < ir[diff]).all()
    assert len(down_np) > 1_000_000
