"""Import stand-in for `trimesh` where it is not installed (launch/run_reference_script.py appends this directory to sys.path last,
for every script it runs): a top-level `import trimesh` (evaluate_dtu_mesh.py's, extract_mesh.py:12, scene/gaussian_model.py:23) succeeds,
the launcher points evaluate_dtu_mesh.py's `trimesh.load` at mesh_cull.load and binds the mesh extraction to mesh_extraction (no trimesh), `creation.box()` works (scene/gaussian_model.py:434), and everything
else raises when called."""
from . import creation  # noqa: F401
from ._missing import Missing


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return Missing("trimesh." + name)
