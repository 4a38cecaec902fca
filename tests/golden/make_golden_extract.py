"""Generates tests/golden/ref_extract_golden.npz by EXECUTING the reference's own GaussianModel.get_tetra_points
(scene/gaussian_model.py:433-463 with get_frustum_mask, :31-72) and extract_mesh.marching_tetrahedra_with_binary_search
(extract_mesh.py:36-120) where they lie (the reference checkout next to this repository, build container only -- the tests read the
committed .npz), on the CPU.  No reference code is copied.

The two modules import packages that are not part of this project's environment and modules the two functions never touch; they are
replaced by stand-ins in sys.modules before the import:
  * scene: a package stand-in whose path is the reference's scene/ (scene.gaussian_model, scene.cameras and scene.appearance_network
    are the reference's own files; scene/__init__.py with its dataset readers is not executed);
  * plyfile, simple_knn._C, utils.vis_utils, gaussian_renderer, tetranerf.utils.extension: stand-ins; `cpp.triangulate` is SciPy's
    Delaunay;
  * trimesh: this project's import stand-in (shims_dtu/trimesh).  ASSUMPTION, stated: trimesh.creation.box() lists its 8 vertices
    with x slowest and z fastest, each from -0.5 to 0.5, which is the order the stand-in reproduces and DESIGN.md §3.11 defines the
    corner index by.  `trimesh.Trimesh` in extract_mesh's namespace is a recorder.
The reference hard-codes `.cuda()` and `device="cuda"`; Tensor.cuda and the device argument of torch.zeros / ones are redirected to the
CPU for this run.  `evaluage_alpha` is the analytic field of tests/extract_restatement.py (additions, multiplications and a clamp:
the same bits in numpy and torch), since the opacity field itself is not what is recorded here.

(a) 600 seeded Gaussians (extract_restatement.gaussians), 8 views of 161 x 120 on a ring of radius 3 (extract_restatement.ring_cameras),
    (near, far) = (0.02, 1e6) and (2.0, 3.5): the inputs, the reference's vertex mask and the points / scales it returns.
(b) 3000 seeded points in [-1, 1]^3 with scales, SciPy's cells, the reference's marching tetrahedra (its crossing edges' vertex ids
    are recorded; the end points are the input points at those ids), the 8 rounds, with and without filter_mesh / texture_mesh: the
    final vertices, faces, vertex mask, face mask and colours."""
import os
import sys
import tempfile
import types

import numpy as np
import torch
from scipy.spatial import Delaunay

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.append(os.path.join(ROOT, "gaussian-opacity-fields_amd", "shims_dtu", "trimesh"))

import extract_restatement as R  # noqa: E402

f32 = np.float32
torch.Tensor.cuda = lambda self, *a, **k: self
for _name in ("zeros", "ones"):
    def _on_cpu(*a, _f=getattr(torch, _name), **k):
        if str(k.get("device", "cpu")).startswith("cuda"):
            k["device"] = "cpu"
        return _f(*a, **k)
    setattr(torch, _name, _on_cpu)


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stand_in("scene", Scene=None).__path__ = [os.path.join(REF, "scene")]
_stand_in("plyfile", PlyData=None, PlyElement=None)
_stand_in("simple_knn")
_stand_in("simple_knn._C", distCUDA2=None)
import utils  # noqa: E402,F401  (the reference's package; one of its modules needs matplotlib and open3d and is never called here)
_stand_in("utils.vis_utils", save_points=None)
_stand_in("gaussian_renderer", render=None, integrate=None, GaussianModel=None)
_stand_in("tetranerf")
_stand_in("tetranerf.utils")
_stand_in("tetranerf.utils.extension", cpp=types.SimpleNamespace(
    triangulate=lambda points: torch.from_numpy(Delaunay(points.detach().cpu().double().numpy()).simplices.astype(np.int32))))

from scene.gaussian_model import GaussianModel  # noqa: E402
import extract_mesh as EM  # noqa: E402

out = {}

# ---- (a) --------------------------------------------------------------------------------------------------------------------------------
xyz, scaling, rotation = R.gaussians(600)
cams = R.ring_cameras(8)
for cam in cams:
    cam.world_view_transform = torch.from_numpy(cam.world_view_transform)
model = types.SimpleNamespace(get_xyz=torch.from_numpy(xyz), get_scaling_with_3D_filter=torch.from_numpy(scaling), _rotation=torch.from_numpy(rotation))
out.update(tp_xyz=xyz, tp_scaling=scaling, tp_rotation=rotation)
for tag, (near, far) in (("a", (0.02, 1e6)), ("b", (2.0, 3.5))):
    import scene.gaussian_model as GM
    masks = []
    frustum = GM.get_frustum_mask
    GM.get_frustum_mask = lambda *a, **k: masks.append(frustum(*a, **k)) or masks[-1]
    pts, sc = GaussianModel.get_tetra_points(model, cams, near, far)
    GM.get_frustum_mask = frustum
    mask = masks[0].numpy()
    assert pts.dtype == torch.float32 and tuple(sc.shape) == (int(mask.sum()), 1) and len(mask) == 9 * 600
    print("(a) near %g far %g: the reference keeps %d of %d candidates" % (near, far, mask.sum(), len(mask)))
    out.update({"tp_%s_near_far" % tag: np.array([near, far]), "tp_%s_mask" % tag: np.packbits(mask), "tp_%s_points" % tag: pts.numpy(),
                "tp_%s_scales" % tag: sc.numpy().reshape(-1)})

# ---- (b) --------------------------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(41)
N = 3000
points = rng.uniform(-1.0, 1.0, (N, 3)).astype(f32)
scales = rng.uniform(0.05, 0.2, (N, 1)).astype(f32)


def evaluage_alpha(pts, views, gaussians, pipeline, background, kernel_size, return_color=False):
    p = pts.detach().numpy()
    alpha = torch.from_numpy(f32(1) - R.field_final_alpha(p))
    return (alpha, torch.from_numpy(R.field_color(p))) if return_color else alpha


class Recorder:
    last = None

    def __init__(self, vertices=None, faces=None, vertex_colors=None, process=True):
        assert process is False
        self.vertices, self.faces, self.vertex_colors = np.asarray(vertices).copy(), np.asarray(faces).copy(), None if vertex_colors is None else np.asarray(vertex_colors).copy()
        self.vertex_mask = self.face_mask = None
        Recorder.last = self

    def update_vertices(self, mask):
        self.vertex_mask = np.asarray(mask).copy()

    def update_faces(self, mask):
        self.face_mask = np.asarray(mask).copy()

    def export(self, path):
        self.path = path


recorded = {}
marching = EM.marching_tetrahedra


def marching_recorded(vertices, tets, sdf, scales_):
    res = marching(vertices, tets, sdf, scales_)
    (end_points, end_sdf), end_scales, ids = res[0][0], res[1][0], res[3][0]
    assert torch.equal(end_points, vertices[0][ids.reshape(-1)].reshape(-1, 2, 3)) and torch.equal(end_sdf, sdf[0][ids.reshape(-1)].reshape(-1, 2, 1))
    assert torch.equal(end_scales, scales_[0][ids.reshape(-1)].reshape(-1, 2, 1))
    recorded["ids"] = ids.numpy().copy()
    return res


EM.evaluage_alpha, EM.marching_tetrahedra = evaluage_alpha, marching_recorded
EM.trimesh = types.SimpleNamespace(Trimesh=Recorder)
gaussians = types.SimpleNamespace(get_tetra_points=lambda views, near, far: (torch.from_numpy(points), torch.from_numpy(scales)))
with tempfile.TemporaryDirectory() as tmp:
    runs = {}
    for filter_mesh, texture_mesh in ((False, False), (True, True)):
        EM.marching_tetrahedra_with_binary_search(tmp, "test", 7, [], gaussians, None, None, 0.0, filter_mesh, texture_mesh, 0.02, 1e6)
        runs[filter_mesh] = Recorder.last
    cells = torch.load(os.path.join(tmp, "test", "ours_7", "fusion", "cells.pt")).numpy()
plain, full = runs[False], runs[True]
assert plain.vertex_mask is None and plain.vertex_colors is None and np.array_equal(plain.vertices, full.vertices) and np.array_equal(plain.faces, full.faces)
E, F = len(full.vertices), len(full.faces)
assert N < 65536 and E < 65536 and full.vertices.dtype == np.float32 and full.vertex_colors.dtype == np.uint8
print("(b) %d points, %d cells, %d edges, %d faces; the filter keeps %d vertices and %d faces" % (N, len(cells), E, F, full.vertex_mask.sum(), full.face_mask.sum()))
out.update(bs_points=points, bs_scales=scales.reshape(-1), bs_cells=cells.astype(np.uint16), bs_edge_ids=recorded["ids"].astype(np.uint16),
           bs_faces=full.faces.astype(np.uint16), bs_vertices=full.vertices, bs_vertex_mask=np.packbits(full.vertex_mask),
           bs_face_mask=np.packbits(full.face_mask), bs_colors=full.vertex_colors)
path = os.path.join(HERE, "ref_extract_golden.npz")
np.savez_compressed(path, **out)
print("%s: %d bytes" % (path, os.path.getsize(path)))
