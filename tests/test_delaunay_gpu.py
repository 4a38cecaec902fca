"""GPU tests of the Delaunay tetrahedralization: delaunay.triangulate on the device, held to the independent checker
(tests/delaunay_check.py), to SciPy in general position, and to a closed, consistently wound surface through the product's marching
tetrahedra."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
for _p in (HERE, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import delaunay_check as K  # noqa: E402
import test_delaunay_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


def _tri(P):
    import delaunay
    return delaunay.triangulate(torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda())


@pytest.mark.parametrize("name", ["uniform_2k", "tetra_2k", "lattice", "sphere", "dup", "scales"])
def test_small_inputs_valid_and_reproducible(name):
    import delaunay
    P = H.case_points(name)
    T0 = _tri(P)
    st = delaunay.last_stats()
    T1 = _tri(P)
    assert T0.dtype == torch.int32 and T0.device.type == "cuda"
    assert torch.equal(T0, T1)
    K.check(P, T0.cpu().numpy(), hull_sample=4000)
    if name == "lattice":
        assert st["exact_evaluations"] > 0
    if name == "sphere":
        assert st["slow_insertions"] > 0


@pytest.mark.parametrize("name", ["coplanar", "three", "dup4"])
def test_degenerate_dimension_gives_no_cells(name):
    T = _tri(H.case_points(name))
    assert tuple(T.shape) == (0, 4) and T.dtype == torch.int32


def test_non_finite_input_raises():
    with pytest.raises(RuntimeError):
        _tri(H.case_points("nan"))


def test_host_tensor_is_refused():
    import delaunay
    with pytest.raises(RuntimeError):
        delaunay.triangulate(torch.zeros((10, 3)))


def test_200k_uniform_matches_scipy():
    from scipy.spatial import Delaunay
    P = np.random.default_rng(1).random((200_000, 3)).astype(np.float32)
    T = _tri(P).cpu().numpy()
    assert K.as_sets(T) == K.as_sets(Delaunay(P.astype(np.float64)).simplices)


def _surface(n, seed):
    import tetmesh
    P = torch.from_numpy((np.random.default_rng(seed).random((n, 3)) * 2 - 1).astype(np.float32)).cuda()
    T = _tri(P.cpu().numpy()).long()
    sdf = 0.5 - P.norm(dim=1)
    (pos, esdf), _, faces, _ = [x[0] for x in tetmesh.marching_tetrahedra(P[None], T, sdf[None], torch.ones_like(sdf)[None])]
    s0, s1 = esdf[:, 0, 0].double(), esdf[:, 1, 0].double()
    t = (s0 / (s0 - s1))[:, None]
    V = pos[:, 0].double() + (pos[:, 1].double() - pos[:, 0].double()) * t
    return V, faces


def test_marching_tets_surface_is_closed_and_consistently_wound():
    """Through the product's marching tetrahedra on 1 M random points, SDF 0.5 - |x| (> 0 inside): every undirected edge of the
    surface lies in two faces, every directed edge appears once, and the face normals point toward sdf > 0 (the triangle table winds
    each triangle by the cell's vertex order).  SciPy's cells are not consistently oriented, so the same check on
    them is expected to fail the winding assertion; that is why the positive orientation is part of the contract."""
    V, F = _surface(1_000_000, 2)
    assert F.shape[0] > 10000
    E = torch.cat([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    und = torch.sort(E, dim=1).values
    _, cnt = torch.unique(und, dim=0, return_counts=True)
    assert (cnt == 2).all(), "surface not closed: undirected edge counts %s" % torch.unique(cnt).tolist()
    _, dcnt = torch.unique(E, dim=0, return_counts=True)
    assert (dcnt == 1).all(), "inconsistent winding: a directed edge appears twice"
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    nrm = torch.cross(b - a, c - a, dim=1)
    dot = (nrm * (a + b + c)).sum(1)
    assert (dot < 0).double().mean().item() > 0.999, "face normals do not point toward sdf > 0"


def test_tetra_points_1m_gaussians():
    """9 M tetra points of a 1 M-Gaussian synthetic scene: every cell positively oriented (fp64 on the device, the undecided
    remainder exactly on the host), faces paired, Euler characteristic 1."""
    import synthetic_scenes as S
    import delaunay
    sc = S.scene_frustum(1_000_000, seed=5)
    P = S.tetra_points(sc)
    Pd = torch.from_numpy(P).cuda()
    T = delaunay.triangulate(Pd).long()
    M = T.shape[0]
    assert M > 5 * len(P)
    X = Pd.double()
    A = X[T[:, 0]]
    u, v, w = X[T[:, 1]] - A, X[T[:, 2]] - A, X[T[:, 3]] - A
    det = (u * torch.cross(v, w, dim=1)).sum(1)
    av, aw = v.abs(), w.abs()
    cperm = torch.stack([av[:, 1] * aw[:, 2] + av[:, 2] * aw[:, 1], av[:, 2] * aw[:, 0] + av[:, 0] * aw[:, 2],
                         av[:, 0] * aw[:, 1] + av[:, 1] * aw[:, 0]], 1)
    perm = (u.abs() * cperm).sum(1)
    und = ~(det.abs() > 1e-10 * perm) | (perm < 1e-200)
    assert (det[~und] > 0).all()
    iu = torch.nonzero(und).flatten().cpu().numpy()
    if len(iu):
        Tu = T[und].cpu().numpy()
        s, _ = K.orient(P, Tu[:, 0], Tu[:, 1], Tu[:, 2], Tu[:, 3])
        assert (s > 0).all()
    # faces: each sorted triple in one or two cells; Euler: V - E + F - T = 1
    Fc = torch.sort(T[:, [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]].reshape(-1, 3), dim=1).values
    n = len(P) + 1
    _, fcnt = torch.unique(torch.stack([Fc[:, 0] * n + Fc[:, 1], Fc[:, 2]], 1), dim=0, return_counts=True)
    del Fc
    assert int(fcnt.max()) <= 2
    Ec = torch.sort(T[:, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]].reshape(-1, 2), dim=1).values
    nE = torch.unique(Ec[:, 0] * n + Ec[:, 1]).numel()
    nV = torch.unique(T).numel()
    assert nV == delaunay.last_stats()["distinct_points"]
    assert nV - nE + fcnt.numel() - M == 1


def test_shim_device_tensor():
    sys.path.insert(0, os.path.join(PKG, "shims"))
    try:
        from tetranerf.utils.extension import cpp
    finally:
        sys.path.remove(os.path.join(PKG, "shims"))
    P = torch.rand((5000, 3), device="cuda")
    T = cpp.triangulate(P)
    assert T.dtype == torch.int32 and T.device == P.device and T.shape[1] == 4 and T.shape[0] > 5000
