"""GPU tests of the mesh culling: the case tables of tests/mesh_cull_cases.py through the real library, the golden
fixture, one medium mesh whose exported PLY must be byte-identical to the restatement's, and cull_mesh chained with
mesh_eval.sample_mesh on the device -- all held to tests/mesh_cull_restatement.py with equalities."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mesh_cull_cases as K  # noqa: E402
import mesh_cull_restatement as R  # noqa: E402
import test_mesh_cull_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "%dx%d" % s)
def test_dilation_is_bit_equal(size):
    import mesh_cull as M
    assert K.same(K.run_dilate(M, dev, size), K.want_dilate(size)) == []


def test_dilation_into_a_poisoned_buffer_writes_the_pad_bits():
    import mesh_cull as M
    name, m = K.dilate_masks(161, 120)[-3]
    out = torch.full((120 * 3,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    got = M.dilate_mask(dev(m), 6, out=out).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, R.pack(R.dilate(m, 6)))


@pytest.mark.parametrize("name", ["golden", "edges", "counts"])
def test_culling_is_bit_equal(name):
    import mesh_cull as M
    g = H.golden()
    assert K.same(K.run_cull(M, dev, name, g), K.want_cull(name, g)) == []


@pytest.mark.parametrize("nv", K.COMPACT_NV)
def test_compaction_is_bit_equal(nv):
    import mesh_cull as M
    assert K.same(K.run_compact(M, dev, nv), K.want_compact(nv)) == []


def test_bad_indices_are_refused():
    import mesh_cull as M
    keep, faces, _, _, _ = K.compact_case(1025, "half")
    faces = faces.copy()
    faces[100, 1] = 1025
    with pytest.raises(RuntimeError, match=r"outside \[0, 1025\)"):
        M.compact_mesh(dev(keep), dev(faces))


def test_golden_fixture_through_cull_mesh():
    """the product on the recorded inputs: equal to the restatement, and to the reference's own mask wherever no fp64 pixel coordinate
    lies within 1e-3 px of a tie or bound (test_mesh_cull_host.py: on this fixture the two agree everywhere)"""
    import mesh_cull as M
    g = H.golden()
    keep = K.want_cull("golden", g)["keep0"]
    mesh = M.cull_mesh(H._cameras(g), M.DeviceMesh(g["vertices"].astype(np.float64), g["faces"]))
    want = R.compact(keep, g["faces"], attrs=(g["vertices"].astype(np.float64),))
    assert np.array_equal(mesh.vertices, want["attrs"][0]) and np.array_equal(mesh.faces, want["faces"])
    views = K.golden_views(g)
    near = R.near_decision(g["vertices"], views, 1e-3)
    assert not ((keep != g["vertex_mask"]) & ~near).any() and (keep != g["vertex_mask"]).sum() <= 0.001 * len(keep)


@pytest.fixture(scope="module")
def medium():
    """200 000 vertices, 400 000 faces, 16 views of 400 x 300 -> (vertices, faces, normals, colours, cameras, the restatement's mesh)"""
    import types
    rng = np.random.default_rng(31)
    V = rng.uniform(-1.2, 1.2, (200000, 3)).astype(np.float32).astype(np.float64)
    F = np.minimum(rng.integers(0, 200000, (400000, 1)) + rng.integers(0, 40, (400000, 3)), 199999).astype(np.int32)
    order = np.argsort(V[:, 0], kind="stable")                  # neighbouring indices are neighbours in space: faces survive the culling
    V = V[order]
    N = rng.normal(size=V.shape).astype(np.float32)
    C3 = rng.integers(0, 256, V.shape).astype(np.uint8)
    views = K.ring_views(16, ((400, 300),), 32)
    cams, dil = [], []
    for i, (m, W, Hh, mask) in enumerate(views):
        # a camera whose view_matrix is m: K = diag(fx, fy) with the principal point, world_view_transform = W2C^T in float32
        a = 2 * np.pi * i / 16 + 0.1
        C = np.array([3 * np.cos(a), 0.3 * np.sin(2 * a), 3 * np.sin(a)])
        zc = -C / np.linalg.norm(C)
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        w2c = np.eye(4)
        w2c[:3, :3] = np.stack([xc, np.cross(zc, xc), zc])
        w2c[:3, 3] = -w2c[:3, :3] @ C
        fx, fy = 0.95 * W + i % 3, 0.93 * W
        assert np.array_equal(R.view_matrix(fx, fy, W, Hh, w2c.T), m)
        cams.append(types.SimpleNamespace(world_view_transform=torch.from_numpy(w2c.T.astype(np.float32)), gt_alpha_mask=torch.from_numpy(mask[None]).cuda(),
                                          focal_x=fx, focal_y=fy, image_width=W, image_height=Hh, image_name="v%d" % i))
        dil.append((m, W, Hh, R.dilate(mask, 6)))
    keep = R.cull(V, dil)
    want = R.compact(keep, F, attrs=(V, N, C3))
    assert 0.02 * len(V) < keep.sum() < 0.6 * len(V) and len(want["faces"]) > 1000
    return V, F, N, C3, cams, want


def test_medium_mesh_exports_the_restatements_bytes(medium, tmp_path):
    import mesh_cull as M
    V, F, N, C3, cams, want = medium
    mesh = M.cull_mesh(cams, M.DeviceMesh(V, F, N, C3))
    path = str(tmp_path / "culled.ply")
    mesh.export(path)
    assert open(path, "rb").read() == R.ply_bytes(want["attrs"][0], want["faces"], want["attrs"][1], want["attrs"][2][:, :3])
    st = M.last_stats()
    assert st["cull"]["views"] == 16 and st["compact"]["kept_vertices"] == len(want["attrs"][0]) and st["compact"]["kept_faces"] == len(want["faces"])


def test_culling_chains_with_the_sampling_on_the_device(medium):
    """evaluate_dtu_mesh.py's next stage (mesh_eval) takes the culled mesh's device tensors as they are"""
    import mesh_cull as M
    import mesh_eval
    import mesh_eval_restatement as ER
    V, F, N, C3, cams, want = medium
    mesh = M.cull_mesh(cams, M.DeviceMesh(V, F))
    assert mesh._v.is_cuda and mesh._v.dtype == torch.float64 and mesh._f.dtype == torch.int32
    nf = min(2000, int(mesh._f.size(0)))
    got = mesh_eval.sample_mesh(mesh._v, mesh._f[:nf].contiguous(), 0.05).cpu().numpy()
    ref = ER.sample_mesh(want["attrs"][0], want["faces"][:nf], 0.05)
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint64), ref.view(np.uint64))
