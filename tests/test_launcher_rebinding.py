"""CPU-only, needs the reference's Python scripts as __graft_entry__.build() stages them (oracle/_ref/refpy, byte-identical copies;
skipped where they were not staged): launch/run_reference_script.py rebinds the RIGHT names of the unchanged reference -- every
attribute it replaces exists in the reference with the same call signature."""
import importlib.util
import inspect
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "refpy")
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="oracle/_ref/refpy not staged (build() stages it where the reference exists)")


def _load_launcher():
    spec = importlib.util.spec_from_file_location("gof_launcher", os.path.join(ROOT, "gaussian-opacity-fields_amd", "launch", "run_reference_script.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture()
def reference_on_path(monkeypatch):
    for name in ("plyfile", "trimesh", "open3d", "cv2"):                 # third-party packages the reference imports at module top
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    sys.modules["plyfile"].PlyData = getattr(sys.modules["plyfile"], "PlyData", object)
    sys.modules["plyfile"].PlyElement = getattr(sys.modules["plyfile"], "PlyElement", object)
    monkeypatch.syspath_prepend(REF)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "gaussian-opacity-fields_amd"))
    before = set(sys.modules)
    yield
    for k in set(sys.modules) - before:
        if k.split(".")[0] in ("utils", "scene", "gaussian_renderer", "arguments"):
            sys.modules.pop(k, None)


def test_train_epilogue_rebinding_hits_existing_reference_names(reference_on_path):
    import utils.loss_utils as ref_loss
    import utils.depth_utils as ref_depth
    from scene.gaussian_model import GaussianModel
    props = {p_: getattr(GaussianModel, p_) for p_ in ("get_scaling_with_3D_filter", "get_opacity_with_3D_filter", "get_rotation", "get_features")}
    assert all(isinstance(v, property) for v in props.values())          # they are properties in the reference too
    orig = {"ssim": ref_loss.ssim, "l1": ref_loss.l1_loss, "d2n": ref_depth.depth_to_normal, "d2p": ref_depth.depths_to_points,
            "setup": GaussianModel.training_setup, "f3d": GaussianModel.compute_3D_filter, "stats": GaussianModel.add_densification_stats}
    import scene.cameras as ref_cameras
    orig["camera_init"] = ref_cameras.Camera.__init__
    L = _load_launcher()
    L.rebind_train_epilogue()
    import train_epilogue as T
    from train_epilogue import deferred as Dl
    import diff_gaussian_rasterization as DGR
    try:
        # the three loss helpers in their deferred form (train_epilogue/deferred.py: the script's inline loss becomes one fused call),
        # switched on; GOF_EAGER_LOSS=1 leaves the same names bound but every call eager
        assert Dl._ENABLED and DGR._slice_hook is Dl._on_slice
        # Camera.world_view_transform -> train_epilogue.PoseMatrix (train.py:177-179): the constructor is wrapped, its signature kept
        assert ref_cameras.Camera.__init__ is not orig["camera_init"]
        assert "world_view_transform" in inspect.getsource(orig["camera_init"])              # the attribute the wrapper replaces exists in the reference
        assert ref_loss.l1_loss is Dl.l1_loss and ref_loss.ssim is Dl.ssim and ref_depth.depth_to_normal is Dl.depth_to_normal and ref_depth.depths_to_points is T.depths_to_points
        assert Dl.impl["l1"] is T.l1_loss and Dl.impl["ssim"] is T.ssim and Dl.impl["depth_to_normal"] is T.depth_to_normal      # what they fall back to
        assert GaussianModel.compute_3D_filter is T.compute_3D_filter and GaussianModel.add_densification_stats is T.add_densification_stats
        assert GaussianModel.training_setup is not orig["setup"]
        for prop in ("get_scaling_with_3D_filter", "get_opacity_with_3D_filter", "get_rotation"):
            assert isinstance(getattr(GaussianModel, prop), property) and getattr(GaussianModel, prop).fget is getattr(T.activations, prop)
        # get_features: the two stored tensors as they are; every other use of the object sees the reference's concatenation
        import torch
        import types
        from diff_gaussian_rasterization import SplitSH
        fake = types.SimpleNamespace(_features_dc=torch.randn(5, 1, 3), _features_rest=torch.randn(5, 15, 3))
        got = GaussianModel.get_features.fget(fake)
        want = props["get_features"].fget(fake)
        assert isinstance(got, SplitSH) and got.native() and got.dc is fake._features_dc and got.rest is fake._features_rest
        assert got.shape == want.shape and torch.equal(got.transpose(1, 2).view(-1, 3, 16), want.transpose(1, 2).view(-1, 3, 16))   # gaussian_renderer/__init__.py:84
        assert not SplitSH(torch.randn(5, 1, 3), torch.randn(5, 8, 3)).native()       # fewer stored bands: the rasterizer concatenates
        # same call signatures as the functions they replace
        for new, old in ((T.ssim, orig["ssim"]), (T.l1_loss, orig["l1"]), (T.depth_to_normal, orig["d2n"]), (T.depths_to_points, orig["d2p"]),
                         (Dl.ssim, orig["ssim"]), (Dl.l1_loss, orig["l1"]), (Dl.depth_to_normal, orig["d2n"]),
                         (T.compute_3D_filter, orig["f3d"]), (T.add_densification_stats, orig["stats"])):
            assert list(inspect.signature(new).parameters) == list(inspect.signature(old).parameters), (new, old)
    finally:
        Dl.enable(False)
        ref_cameras.Camera.__init__ = orig["camera_init"]
        ref_loss.ssim, ref_loss.l1_loss, ref_depth.depth_to_normal, ref_depth.depths_to_points = orig["ssim"], orig["l1"], orig["d2n"], orig["d2p"]
        GaussianModel.training_setup, GaussianModel.compute_3D_filter, GaussianModel.add_densification_stats = orig["setup"], orig["f3d"], orig["stats"]
        for k_, v_ in props.items():
            setattr(GaussianModel, k_, v_)


def test_integrate_wrapper_and_marching_tets_rebinding(reference_on_path):
    import gaussian_renderer as GR
    import utils.tetmesh as ref_tetmesh
    import tetmesh as hip_tetmesh
    orig = GR.integrate
    L = _load_launcher()
    L.rebind_integrate_with_view_cache()
    try:
        assert GR.integrate is not orig
        assert list(inspect.signature(GR.integrate).parameters) == list(inspect.signature(orig).parameters)
    finally:
        GR.integrate = orig
    assert list(inspect.signature(hip_tetmesh.marching_tetrahedra).parameters) == list(inspect.signature(ref_tetmesh.marching_tetrahedra).parameters)
    # the names the scripts import (train.py:20,38; extract_mesh.py:5,14) exist where the launcher patches them
    src_train = open(os.path.join(REF, "train.py")).read()
    assert "from utils.loss_utils import l1_loss, ssim" in src_train and "from utils.depth_utils import depths_to_points, depth_to_normal" in src_train
    src_mesh = open(os.path.join(REF, "extract_mesh.py")).read()
    assert "from gaussian_renderer import render, integrate" in src_mesh and "from utils.tetmesh import marching_tetrahedra" in src_mesh


def test_script_level_functions_are_rebound_without_touching_the_script(tmp_path, monkeypatch):
    """extract_mesh.py defines evaluage_alpha ITSELF (extract_mesh.py:17): the launcher executes the module body without the
    `if __name__ == "__main__":` block, replaces the name, then runs the block -- every statement once, in order; a script that
    does not define the name (or whose guard is not at the end) goes through runpy unchanged."""
    L = _load_launcher()
    out = tmp_path / "out.txt"
    script = tmp_path / "toy_extract.py"
    script.write_text(
        "import sys\n"
        "LOG = []\n"
        "def evaluage_alpha(points, views):\n"
        "    return 'script'\n"
        "def driver():\n"
        "    LOG.append(evaluage_alpha(1, 2))\n"
        "LOG.append('body')\n"
        "if __name__ == \"__main__\":\n"
        "    LOG.append(__name__)\n"
        "    driver()\n"
        "    open(%r, 'w').write(','.join(LOG) + ',' + sys.modules['__main__'].__file__)\n" % str(out))
    main_before = sys.modules.get("__main__")
    L.run_script(str(script), {"evaluage_alpha": lambda points, views: "rebound"})
    assert out.read_text() == "body,__main__,rebound," + str(script)
    assert sys.modules.get("__main__") is main_before
    L.run_script(str(script), {"some_other_name": lambda: None})          # nothing to rebind: plain runpy
    assert out.read_text().startswith("body,__main__,script,")
    # a guard that is not the last statement: the order of execution must not change -> runpy, no rebinding
    script.write_text(script.read_text() + "LOG.append('after')\n")
    L.run_script(str(script), {"evaluage_alpha": lambda points, views: "rebound"})
    assert out.read_text().startswith("body,__main__,script,")
    # the reference's extract_mesh.py has the shape the split needs
    import ast
    ref = os.path.join(REF, "extract_mesh.py") if os.path.isdir(REF) else None
    if ref and os.path.exists(ref):
        tree = ast.parse(open(ref).read())
        assert any(isinstance(n, ast.FunctionDef) and n.name == "evaluage_alpha" for n in tree.body)
        assert L._is_main_guard(tree.body[-1]) and sum(L._is_main_guard(n) for n in tree.body) == 1
