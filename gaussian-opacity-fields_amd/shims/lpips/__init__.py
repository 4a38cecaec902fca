"""Stand-in for the ``lpips`` pip package (metrics.py:19 imports it, :100 builds ``lpips.LPIPS(net='vgg')``): the model is this
backend's HIP implementation (image_metrics.py, csrc/lpips.hip).  launch/run_reference_script.py puts this directory LAST on
sys.path and only when no real lpips is importable, so an installed package wins."""
from image_metrics import LPIPS  # noqa: F401

__all__ = ["LPIPS"]


def __getattr__(name):
    from ._missing import Missing
    return Missing("lpips." + name)
