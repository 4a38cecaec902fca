"""Generates tests/golden/ref_model_ply_golden.npz by running the reference's OWN GaussianModel.save_ply / save_fused_ply / load_ply
(scene/gaussian_model.py:374-430, 486-530) where they lie, in /root/reference (run in the build container only; the GPU machine only reads
the committed .npz).

The reference's methods hand a structured array to plyfile (PlyElement.describe) and take one from it (PlyData.read): a recording stub
stands in for plyfile, so what is pinned is exactly what the reference would have written and what it makes of what it reads.  Absent
third-party modules are stubbed and device='cuda' is redirected to the CPU, as tests/golden/make_golden.py does.  No reference code is
copied.

Per model of tests/model_io_cases.py (sh degree 0..3 with P = 5, degree 3 with P = 130), under the prefix <tag>_:
  raw, fused            the bytes of the arrays save_ply / save_fused_ply describe (uint8)
  load_<field>          the seven tensors load_ply makes of the raw array
  load64_<field>        the same from the variant whose opacity and scale columns are float64 (model_io_cases.f64_variant)
  act_opacity, act_scaling   get_opacity_with_3D_filter, get_scaling_with_3D_filter
  roundtrip_rel         max relative difference between sigmoid64(fused opacity) / exp64(fused scales) and those activated tensors: what the
                        reference's own log-then-exp loses
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, REF)
sys.path.insert(0, TESTS)

import model_io_cases as K  # noqa: E402

for name in ("plyfile", "trimesh", "simple_knn", "simple_knn._C", "open3d", "cv2"):
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)
sys.modules["simple_knn._C"].distCUDA2 = lambda *a, **k: None

tape = {}


class _Property:
    def __init__(self, name):
        self.name = name


class PlyElement:
    def __init__(self, data):
        self.data = data
        self.properties = [_Property(n) for n in data.dtype.names]

    @staticmethod
    def describe(data, name):
        tape["described"] = (name, data.copy())
        return PlyElement(data)

    def __getitem__(self, key):
        return np.ascontiguousarray(self.data[key])        # (torch.tensor refuses the strides of a packed record with float64 fields)


class PlyData:
    def __init__(self, elements):
        self.elements = elements

    def write(self, path):
        tape["written"] = path

    @staticmethod
    def read(path):
        return PlyData([PlyElement(tape["to_read"])])


sys.modules["plyfile"].PlyData = PlyData
sys.modules["plyfile"].PlyElement = PlyElement


def _cpu(fn):
    def wrapped(*a, **k):
        k.pop("device", None)
        return fn(*a, **k)
    return wrapped


for _f in ("zeros", "ones", "tensor", "empty"):
    setattr(torch, _f, _cpu(getattr(torch, _f)))

from scene.gaussian_model import GaussianModel  # noqa: E402


def reference_model(m, degree):
    g = GaussianModel.__new__(GaussianModel)        # (__init__ builds the appearance network on 'cuda'; none of it is touched here)
    g.max_sh_degree, g.active_sh_degree = degree, 0
    g.setup_functions()
    for attr, key in (("_xyz", "xyz"), ("_features_dc", "f_dc"), ("_features_rest", "f_rest"), ("_opacity", "opacity"),
                      ("_scaling", "scaling"), ("_rotation", "rotation")):
        setattr(g, attr, torch.nn.Parameter(torch.from_numpy(m[key].copy())))
    g.filter_3D = torch.from_numpy(m["filter_3D"].copy())
    return g


def loaded(g):
    t = {"xyz": g._xyz, "f_dc": g._features_dc, "f_rest": g._features_rest, "opacity": g._opacity, "scaling": g._scaling,
         "rotation": g._rotation, "filter_3D": g.filter_3D}
    for k, v in t.items():
        assert v.dtype == torch.float32 and v.is_contiguous(), k
        assert (k == "filter_3D") != (isinstance(v, torch.nn.Parameter) and v.requires_grad), k
    return {k: v.detach().numpy().copy() for k, v in t.items()}


out = {}
tmp = tempfile.mkdtemp()
for i, (tag, degree, P) in enumerate(K.GOLDEN_MODELS):
    m = K.make_model(degree, P, i)
    Kc = m["f_rest"].shape[1]
    g = reference_model(m, degree)
    g.save_ply(os.path.join(tmp, tag, "point_cloud.ply"))
    name, raw = tape["described"]
    assert name == "vertex" and raw.dtype.names == tuple(K.names(Kc)) and all(raw.dtype[n] == np.dtype("<f4") for n in raw.dtype.names)
    g.save_fused_ply(os.path.join(tmp, tag, "fused.ply"))
    _, fused = tape["described"]
    assert fused.dtype.names == tuple(K.names(Kc, fused=True))
    out[tag + "_raw"] = np.frombuffer(raw.tobytes(), np.uint8)
    out[tag + "_fused"] = np.frombuffer(fused.tobytes(), np.uint8)
    with torch.no_grad():
        ao, asc = g.get_opacity_with_3D_filter.numpy().copy(), g.get_scaling_with_3D_filter.numpy().copy()
    out[tag + "_act_opacity"], out[tag + "_act_scaling"] = ao, asc
    fr = np.frombuffer(fused.tobytes(), np.float32).reshape(P, 17 + 3 * Kc)
    out[tag + "_roundtrip_rel"] = np.float64(max(K.fused_errors(fr, Kc, ao, asc)))
    assert 0.0 < ao.min() and ao.max() < 1.0 and np.isfinite(fr).all()
    for prefix, arr in (("load", raw), ("load64", K.f64_variant(m)[0])):
        h = GaussianModel.__new__(GaussianModel)
        h.max_sh_degree, h.active_sh_degree = degree, 0
        tape["to_read"] = arr
        h.load_ply("unused")
        assert h.active_sh_degree == degree
        for k, v in loaded(h).items():
            out["%s_%s_%s" % (tag, prefix, k)] = v
    print("%s: degree %d, P %d, roundtrip_rel %.3g, opacity in [%.4g, %.4g]" % (tag, degree, P, out[tag + "_roundtrip_rel"], ao.min(), ao.max()))

path = os.path.join(HERE, "ref_model_ply_golden.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 200 * 1024
