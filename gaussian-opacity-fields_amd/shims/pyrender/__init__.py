"""Import stand-in for ``pyrender`` (eval_tnt/cull_mesh.py:9 imports it at module level).  pyrender renders through OpenGL, which an
MI355X machine does not have, and the only function of that script that uses it, ``extract_depth_from_mesh``, is rebound to the HIP
depth rasteriser (mesh_cull.render_depth) by launch/run_reference_script.py, which puts this package on sys.path only when a real
pyrender is not importable.  Every attribute exists so that the import succeeds; calling one raises."""
from ._missing import Missing

Scene = Missing("pyrender.Scene")
Mesh = Missing("pyrender.Mesh")
Node = Missing("pyrender.Node")
IntrinsicsCamera = Missing("pyrender.IntrinsicsCamera")
OffscreenRenderer = Missing("pyrender.OffscreenRenderer")
RenderFlags = Missing("pyrender.RenderFlags")


def __getattr__(name):
    return Missing("pyrender." + name)
