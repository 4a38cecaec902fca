"""Import stand-in for `cv2` where it is not installed (launch/run_reference_script.py appends this directory to sys.path last, for
evaluate_dtu_mesh.py only): `import cv2` succeeds; the launcher binds mesh_cull.load_dtu_camera (a numpy RQ decomposition) in place of
the script's, so nothing here is called -- and whatever is called raises."""
from ._missing import Missing


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    return Missing("cv2." + name)
