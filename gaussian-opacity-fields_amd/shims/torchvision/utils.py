"""``torchvision.utils`` of the stand-in: save_image for one image, as render.py:35-36 calls it."""
from ._missing import Missing


def save_image(tensor, fp, format=None, **kwargs):
    """tensor (3,H,W), (1,H,W), (H,W) or (1,C,H,W) float in [0,1] -> an image file, with torchvision's arithmetic:
    mul(255).add_(0.5).clamp_(0, 255), to uint8, channels last, then Pillow.  A batch of more than one image (torchvision tiles
    it into a grid) is not provided."""
    import torch
    from PIL import Image
    t = tensor.detach()
    if t.dim() == 4:
        if t.size(0) != 1:
            raise RuntimeError("torchvision.utils.save_image (stand-in): a batch of %d images would need make_grid, which is not provided" % t.size(0))
        t = t[0]
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.size(0) not in (1, 3, 4):
        raise RuntimeError("torchvision.utils.save_image (stand-in): expected (C,H,W) with C in (1, 3, 4), got %s" % (tuple(tensor.shape),))
    if t.size(0) == 1:
        t = t.expand(3, -1, -1)          # (make_grid turns a single-channel image into three equal channels)
    nd = t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
    Image.fromarray(nd).save(fp, format=format)


def __getattr__(name):
    return Missing("torchvision.utils." + name)
