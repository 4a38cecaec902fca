"""Import stand-in for `trimesh` where it is not installed (launch/run_reference_script.py appends this directory to sys.path last,
for evaluate_dtu_mesh.py only): the script's top-level `import trimesh` (its own and scene/gaussian_model.py:23) succeeds, the
launcher points the script's `trimesh.load` at mesh_cull.load, `creation.box()` works (scene/gaussian_model.py:434), and everything
else raises when called."""
from . import creation  # noqa: F401
from ._missing import Missing


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return Missing("trimesh." + name)
