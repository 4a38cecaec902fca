"""Generates tests/golden/ref_dtu_cull_golden.npz by EXECUTING the reference's own evaluate_dtu_mesh.cull_mesh (:77-139) where it lies
(the reference checkout next to this repository, build container only -- the tests read the committed .npz).  No reference code is
copied.

The script's module imports packages that are not part of this project's environment and modules that cull_mesh never touches; they
are replaced by stand-ins in sys.modules before the import:
  * scene, gaussian_renderer, arguments, cv2, trimesh: empty stand-ins (cull_mesh uses none of them: the mesh is a plain object
    with `vertices`, `faces`, `update_vertices`, `update_faces`);
  * skimage.morphology: `disk(r)` = the (2r+1)^2 footprint dx^2 + dy^2 <= r^2 (scikit-image's definition) and `binary_dilation`
    = scipy.ndimage.binary_dilation(image != 0, structure=footprint).  ASSUMPTION, stated: for a footprint with odd sides
    scikit-image's binary_dilation is SciPy's with the footprint as structure (scikit-image documents it as a wrapper of
    scipy.ndimage with the image converted to bool first; its centring correction only concerns even-sided footprints).
The reference hard-codes `.cuda()`; Tensor.cuda is redirected to the CPU for this run.

The scene (tests/mesh_cull_restatement.golden_scene): 8 views of 161 x 120 looking at the origin from a ring of radius 3, disc masks of
radius 30 + 2 i px plus 0.1 % salt pixels, focal lengths ~150 px, 20 000 vertices uniform in [-1.2, 1.2]^3 (float32 values, as the
meshes of this pipeline have).  Recorded: the inputs and the reference's vertex mask (and its face mask for a random face list)."""
import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

import mesh_cull_restatement as R  # noqa: E402

torch.Tensor.cuda = lambda self, *a, **k: self


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


for _name, _attrs in (("scene", {"Scene": None}), ("gaussian_renderer", {"GaussianModel": None}), ("cv2", {}), ("trimesh", {}),
                      ("arguments", {"ModelParams": None, "PipelineParams": None, "get_combined_args": None})):
    _stand_in(_name, **_attrs)
_stand_in("skimage")
_stand_in("skimage.morphology", disk=lambda r: R.disk(r).astype(np.uint8),
          binary_dilation=lambda image, footprint=None: ndimage.binary_dilation(np.asarray(image) != 0, structure=np.asarray(footprint) != 0))

from evaluate_dtu_mesh import cull_mesh  # noqa: E402


class Mesh:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces

    def update_vertices(self, mask):
        self.vertex_mask = np.asarray(mask).copy()

    def update_faces(self, mask):
        self.face_mask = np.asarray(mask).copy()


g = R.golden_scene()
V32 = g["vertices"].astype(np.float32)
faces = np.random.default_rng(12).integers(0, len(V32), (30000, 3)).astype(np.int32)
cameras = [types.SimpleNamespace(world_view_transform=torch.from_numpy(g["world_view_transform"][i].copy()), gt_alpha_mask=torch.from_numpy(g["masks"][i].copy()),
                                 focal_x=float(g["focal"][i, 0]), focal_y=float(g["focal"][i, 1]), image_width=g["W"], image_height=g["H"])
           for i in range(len(g["masks"]))]
mesh = cull_mesh(cameras, Mesh(V32.astype(np.float64), faces))
print("reference keeps %d of %d vertices, %d of %d faces" % (mesh.vertex_mask.sum(), len(V32), mesh.face_mask.sum(), len(faces)))
np.savez_compressed(os.path.join(HERE, "ref_dtu_cull_golden.npz"), W=np.int32(g["W"]), H=np.int32(g["H"]), world_view_transform=g["world_view_transform"],
                    focal=g["focal"], masks=g["masks"], vertices=V32, faces=faces, vertex_mask=mesh.vertex_mask, face_mask=mesh.face_mask)
