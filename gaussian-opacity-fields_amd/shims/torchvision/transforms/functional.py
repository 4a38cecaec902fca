"""``torchvision.transforms.functional`` of the stand-in: to_tensor as metrics.py:33-34 calls it."""
from .._missing import Missing


def to_tensor(pic):
    """a PIL image (modes L, LA, RGB, RGBA: 8 bits per channel) or an (H,W[,C]) uint8 numpy array -> (C,H,W) float32, divided by 255"""
    import numpy as np
    import torch
    if isinstance(pic, np.ndarray):
        a = pic if pic.ndim == 3 else pic[:, :, None]
        if a.dtype != np.uint8:
            return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    else:
        if getattr(pic, "mode", None) not in ("L", "LA", "RGB", "RGBA", "1"):
            raise RuntimeError("torchvision.transforms.functional.to_tensor (stand-in): image mode %r is not provided (8-bit L, LA, RGB, RGBA)" % getattr(pic, "mode", None))
        if pic.mode == "1":
            a = 255 * np.asarray(pic, np.uint8)[:, :, None]
        else:
            a = np.asarray(pic, np.uint8)
            a = a if a.ndim == 3 else a[:, :, None]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)


def __getattr__(name):
    return Missing("torchvision.transforms.functional." + name)
