"""``open3d.core`` stand-in (extract_mesh_tsdf.py:13): see the package docstring."""
from ._missing import Missing

Device = Missing("open3d.core.Device")
Tensor = Missing("open3d.core.Tensor")
Dtype = Missing("open3d.core.Dtype")
float32 = Missing("open3d.core.float32")
float64 = Missing("open3d.core.float64")


def __getattr__(name):
    return Missing("open3d.core." + name)
