"""Import stand-in for ``open3d`` (extract_mesh_tsdf.py:12-13 imports it at module level).  Open3D has no HIP device, and the only
function of that script that uses it, ``tsdf_fusion``, is rebound to the HIP TSDF fusion (tsdf_fusion.py) by
launch/run_reference_script.py, which puts this package on sys.path only when a real open3d is not importable.  Every attribute
exists so that the imports succeed; calling one raises."""
from ._missing import Missing

from . import core  # noqa: E402,F401  (``import open3d.core as o3c``)

geometry = Missing("open3d.geometry")
camera = Missing("open3d.camera")
io = Missing("open3d.io")
t = Missing("open3d.t")
utility = Missing("open3d.utility")
visualization = Missing("open3d.visualization")


def __getattr__(name):
    return Missing("open3d." + name)
