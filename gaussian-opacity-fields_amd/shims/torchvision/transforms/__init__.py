"""``torchvision.transforms`` of the stand-in: only ``functional.to_tensor``."""
from .._missing import Missing

from . import functional  # noqa: E402,F401


def __getattr__(name):
    return Missing("torchvision.transforms." + name)
