"""Import stand-in for ``torchvision`` (render.py:18, metrics.py:16 import it at module level).  It provides the two functions those
scripts call, with torchvision's arithmetic, over Pillow (which metrics.py imports itself): ``utils.save_image`` and
``transforms.functional.to_tensor``.  launch/run_reference_script.py puts this directory LAST on sys.path and only when no real
torchvision is importable, so an installed package wins.  Every other attribute exists so that imports succeed; calling one raises."""
from ._missing import Missing

from . import utils  # noqa: E402,F401
from . import transforms  # noqa: E402,F401


def __getattr__(name):
    return Missing("torchvision." + name)
