"""CPU-only, needs the reference's Python scripts as __graft_entry__.build() stages them (oracle/_ref/refpy, byte-identical copies;
skipped where they were not staged): launch/run_reference_script.py binds the mesh extraction to the RIGHT names
of the unchanged reference -- GaussianModel.get_tetra_points and extract_mesh.py's marching_tetrahedra_with_binary_search exist there
with the signatures the drop-ins take; without trimesh the two modules still import; GOF_TORCH_EXTRACT=1 leaves both names alone; the
bound function queries the field through the script's `evaluage_alpha` as it is bound when it is called."""
import ast
import importlib.util
import inspect
import os
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "refpy")
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="oracle/_ref/refpy not staged (build() stages it where the reference exists)")


def _load_launcher():
    spec = importlib.util.spec_from_file_location("gof_launcher_extract", os.path.join(PKG, "launch", "run_reference_script.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture()
def reference_on_path(monkeypatch):
    """the launcher's path arrangement (the package first, the reference second) with stand-ins for the third-party packages the
    reference imports at module top -- except trimesh, which is the launcher's business here"""
    for name in ("plyfile", "open3d", "cv2"):
        if name not in sys.modules:
            monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    sys.modules["plyfile"].PlyData = getattr(sys.modules["plyfile"], "PlyData", object)
    sys.modules["plyfile"].PlyElement = getattr(sys.modules["plyfile"], "PlyElement", object)
    monkeypatch.syspath_prepend(REF)
    monkeypatch.syspath_prepend(PKG)
    before, path_before = set(sys.modules), list(sys.path)
    yield
    sys.path[:] = path_before
    for k in set(sys.modules) - before:
        if k.split(".")[0] in ("utils", "scene", "gaussian_renderer", "arguments", "trimesh", "tetranerf"):
            sys.modules.pop(k, None)


def _script_function(name):
    tree = ast.parse(open(os.path.join(REF, "extract_mesh.py")).read())
    return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)


@needs_reference
def test_both_names_exist_in_the_reference_with_the_drop_ins_signatures(reference_on_path):
    import mesh_extraction as ME
    L = _load_launcher()
    L.add_trimesh_stand_in()
    from scene.gaussian_model import GaussianModel
    ref = inspect.signature(GaussianModel.get_tetra_points)
    new = inspect.signature(ME.get_tetra_points)
    assert list(new.parameters) == list(ref.parameters) and [p.default for p in new.parameters.values()] == [p.default for p in ref.parameters.values()]
    params = [a.arg for a in _script_function("marching_tetrahedra_with_binary_search").args.args]
    assert params == list(inspect.signature(L._marching_tetrahedra_with_binary_search).parameters)
    assert params + ["evaluate_alpha"] == list(inspect.signature(ME.marching_tetrahedra_with_binary_search).parameters)
    assert [a.arg for a in _script_function("evaluage_alpha").args.args] == list(inspect.signature(L._fused_evaluate_alpha).parameters)
    src = open(os.path.join(REF, "extract_mesh.py")).read()
    assert "gaussians.get_tetra_points(views, near, far)" in src and "import trimesh" in src


@needs_reference
def test_the_modules_import_without_trimesh_and_the_method_is_rebound(reference_on_path, monkeypatch):
    if importlib.util.find_spec("trimesh") is not None and not (importlib.util.find_spec("trimesh").origin or "").startswith(os.path.join(PKG, "shims_dtu")):
        pytest.skip("trimesh is installed here: an installed trimesh wins")
    import mesh_extraction as ME
    L = _load_launcher()
    if importlib.util.find_spec("tetranerf") is None:
        sys.path.append(os.path.join(PKG, "shims"))
    L.add_trimesh_stand_in()
    assert sys.path[-1] == os.path.join(PKG, "shims_dtu", "trimesh")                 # last: whatever is installed comes first
    n = len(sys.path)
    L.add_trimesh_stand_in()
    assert len(sys.path) == n
    import scene.gaussian_model as GM
    import trimesh
    assert (trimesh.__file__ or "").startswith(os.path.join(PKG, "shims_dtu")) and len(trimesh.creation.box().vertices) == 8
    original = GM.GaussianModel.get_tetra_points
    try:
        monkeypatch.setenv("GOF_TORCH_EXTRACT", "1")
        L.rebind_tetra_points()
        assert GM.GaussianModel.get_tetra_points is original and L.extract_rebinding("extract_mesh.py") == {}
        monkeypatch.delenv("GOF_TORCH_EXTRACT")
        L.rebind_tetra_points()
        assert GM.GaussianModel.get_tetra_points is L._get_tetra_points
        assert list(inspect.signature(L._get_tetra_points).parameters) == list(inspect.signature(original).parameters)
        monkeypatch.setattr(ME, "get_tetra_points", lambda self, views, near, far: ("called", self, views, near, far))
        assert GM.GaussianModel.get_tetra_points("model", ["v"], 0.5) == ("called", "model", ["v"], 0.5, 1e6)
        assert set(L.extract_rebinding("extract_mesh.py")) == {"marching_tetrahedra_with_binary_search"}
    finally:
        GM.GaussianModel.get_tetra_points = original
    # extract_mesh.py's module body (everything but its `if __name__ == "__main__":` block) runs
    script = os.path.join(REF, "extract_mesh.py")
    tree = ast.parse(open(script).read(), filename=script)
    head = ast.Module(body=[b for b in tree.body if not L._is_main_guard(b)], type_ignores=[])
    ns = {"__name__": "extract_mesh_body", "__file__": script}
    exec(compile(head, script, "exec"), ns)
    assert callable(ns["marching_tetrahedra_with_binary_search"]) and callable(ns["evaluage_alpha"]) and ns["trimesh"] is trimesh


def test_the_bound_function_takes_evaluage_alpha_at_call_time(tmp_path, monkeypatch):
    """a synthetic extract_mesh.py: under the launcher's rebinding its marching_tetrahedra_with_binary_search is mesh_extraction's, and
    the field is queried through the `evaluage_alpha` of the script's namespace at the moment of the call: None (mesh_extraction's
    own view loop) where the launcher's fused loop is bound, the script's own function where that rebinding is switched off
    (GOF_TORCH_VIEW_REDUCE=1), and whatever the script itself binds later"""
    monkeypatch.syspath_prepend(PKG)
    import mesh_extraction as ME
    L = _load_launcher()
    calls = []

    def recorder(*a, evaluate_alpha=None):
        calls.append((a, evaluate_alpha))
        return "mesh"
    monkeypatch.setattr(ME, "marching_tetrahedra_with_binary_search", recorder)
    script = tmp_path / "extract_mesh.py"
    script.write_text(
        "def evaluage_alpha(points, views, gaussians, pipeline, background, kernel_size, return_color=False):\n"
        "    return 'script'\n"
        "def later(*a, **k):\n"
        "    return 'later'\n"
        "def marching_tetrahedra_with_binary_search(model_path, name, iteration, views, gaussians, pipeline, background, kernel_size, filter_mesh, texture_mesh, near, far):\n"
        "    raise AssertionError('the script own function ran')\n"
        "if __name__ == '__main__':\n"
        "    marching_tetrahedra_with_binary_search(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)\n"
        "    evaluage_alpha = later\n"
        "    marching_tetrahedra_with_binary_search(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)\n")
    monkeypatch.delenv("GOF_TORCH_EXTRACT", raising=False)
    L.run_script(str(script), dict({"evaluage_alpha": L._fused_evaluate_alpha}, **L.extract_rebinding(str(script))))
    assert [c[0] for c in calls] == [tuple(range(1, 13))] * 2
    assert calls[0][1] is None and calls[1][1] is not None and calls[1][1]() == "later"
    del calls[:]
    L.run_script(str(script), L.extract_rebinding(str(script)))                      # the script's own view loop stays bound
    assert calls[0][1] is not None and calls[0][1](0, 0, 0, 0, 0, 0) == "script" and calls[1][1]() == "later"
    del calls[:]
    monkeypatch.setenv("GOF_TORCH_EXTRACT", "1")
    with pytest.raises(AssertionError, match="own function ran"):
        L.run_script(str(script), L.extract_rebinding(str(script)))
    assert calls == []
