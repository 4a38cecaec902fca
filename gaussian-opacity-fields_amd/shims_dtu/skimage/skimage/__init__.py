"""Import stand-in for `skimage` where it is not installed (launch/run_reference_script.py appends this directory to sys.path last,
for evaluate_dtu_mesh.py only): `from skimage.morphology import binary_dilation, disk` succeeds; the launcher's cull_mesh dilates on
the device (mesh_cull.dilate_mask), so nothing here is called -- and whatever is called raises."""
from ._missing import Missing


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return Missing("skimage." + name)
