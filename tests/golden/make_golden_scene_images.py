"""Writes tests/golden/ref_scene_images_golden.npz: for every case of tests/scene_images_cases.py (inputs regenerated from their seeds, not
stored) the bytes of Pillow's Image.resize and the float tensor of the reference's own PILtoTorch (the staged
oracle/_ref/refpy/utils/general_utils.py), composed as loadCam composes them: an L or RGB image in one call, a 4-channel image as four L
bands resized separately and concatenated (utils/camera_utils.py:41-49).  Needs Pillow, torch and the staged reference scripts.

    python tests/golden/make_golden_scene_images.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_images_cases as K  # noqa: E402


def main():
    import PIL
    from PIL import Image
    import torch
    spec = importlib.util.spec_from_file_location("ref_general_utils", os.path.join(ROOT, "oracle", "_ref", "refpy", "utils", "general_utils.py"))
    gu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gu)
    out = {"pillow_version": np.array(PIL.__version__), "torch_version": np.array(torch.__version__)}
    for (tag, W, H, w, h, C), kind, a in K.inputs():
        if C == 4:
            bands = Image.fromarray(a, "RGBA").split()
            assert len(bands) == 4
            planes = torch.cat([gu.PILtoTorch(b, (w, h)) for b in bands], dim=0)
            by = np.stack([np.array(b.resize((w, h))) for b in bands], axis=-1)
        else:
            im = Image.fromarray(a[..., 0], "L") if C == 1 else Image.fromarray(a, "RGB")
            planes = gu.PILtoTorch(im, (w, h))
            by = np.array(im.resize((w, h))).reshape(h, w, C)
        planes = planes.contiguous().numpy()
        assert planes.shape == (C, h, w) and planes.dtype == np.float32 and by.dtype == np.uint8
        out["bytes_%s_%s" % (tag, kind)] = by
        out["planar_%s_%s" % (tag, kind)] = planes
    path = K.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes (Pillow %s)" % (path, len(out), os.path.getsize(path), PIL.__version__))


if __name__ == "__main__":
    main()
