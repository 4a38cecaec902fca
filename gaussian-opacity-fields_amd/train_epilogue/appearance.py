"""The decoupled-appearance L1 of the reference's train.py:67-88 on the GPU, forward and backward, without MIOpen or torch's resampling.

    Ll1 = L1_loss_appearance(image, gt_image, gaussians, view_idx)            # train.py:159 (the launcher rebinds the name)
    loss = appearance_l1(image, gt_image, embedding, params)                  # the autograd function under it: 14 parameter tensors

    conv3x3 / conv3x3_wgrad / weight_transpose / materialize / bilinear / up2_backward      # the pieces, as the library exports them

The kernels are ``gof_app_*`` of libgof_hip.so (csrc/appearance.hip, include/gof_appearance_hip.h); the contract is DESIGN.md §3.13:
fp32 tensors on a ROCm device in and out, the convolutions and their gradients on the exact fp32 matrix instruction in a fixed order,
every sum in a fixed order (bit-reproducible, no atomics).  There is no host fallback.  The network stays the reference's module:
its parameters are read by the reference's names, so its state dict, optimizer groups and checkpoints are untouched.
"""
import ctypes as C
import functools

import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["appearance_l1", "L1_loss_appearance", "network_params", "conv3x3", "conv3x3_wgrad", "weight_transpose", "materialize", "bilinear",
           "up2_backward", "head_forward", "head_backward", "image_grad", "stats", "GofAppNet", "MODES", "WGRAD_CHUNK", "PARAM_NAMES"]

lib = B.lib
_vp, _sz, _i64, _i32 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32


class GofAppNet(C.Structure):
    """Mirror of ``GofAppNet`` in include/gof_appearance_hip.h."""
    _fields_ = [("n_embed", C.c_int32), ("width", C.c_int32 * 6)]


_PN = C.POINTER(GofAppNet)
_PP = C.POINTER(C.c_void_p)
gn.bind(lib, {"gof_app_wgrad_workspace_bytes": [_i32, _i32, _i32, _i32], "gof_app_saved_bytes": [_i32, _i32, _PN], "gof_app_head_workspace_bytes": [_i32, _i32],
              "gof_app_workspace_bytes": [_i32, _i32, _PN]}, {
        "gof_app_conv3x3": [_i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp],
        "gof_app_materialize": [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
        "gof_app_weight_transpose": [_i32, _i32, _vp, _vp, _vp],
        "gof_app_conv3x3_wgrad": [_i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp],
        "gof_app_bilinear": [_i32, _i32, _i32, _i64, _i64, _vp, _i32, _i32, _vp, _vp],
        "gof_app_up2_backward": [_i32, _i32, _i32, _vp, _vp, _vp],
        "gof_app_head_forward": [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
        "gof_app_head_backward": [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
        "gof_app_image_grad": [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
        "gof_app_l1_forward": [_i32, _i32, _PN, _vp, _vp, _vp, _PP, _vp, _vp, _vp, _sz, _vp, _sz, _vp],
        "gof_app_l1_backward": [_i32, _i32, _PN, _vp, _vp, _vp, _PP, _vp, _vp, _sz, _vp, _vp, _PP, _vp, _sz, _vp]})

MODES = {"plain": 0, "shuffle": 1, "unshuffle": 2, "up2": 3, "embed": 4}       # GOF_APP_SRC_*
WGRAD_CHUNK = 4096                                                             # GOF_APP_WGRAD_CHUNK
# the reference's names (scene/appearance_network.py), in the order of the library's 14 parameter pointers
PARAM_NAMES = ("conv1", "up1.conv", "up2.conv", "up3.conv", "up4.conv", "conv2", "conv3")

# the device seams, by the names the host tests replace (tests/test_appearance_host.py); one definition each: gof_native
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "appearance")


def _tensor(t, who, what, dims):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s: %s must be a torch tensor" % (who, what))
    if not _on_device(t):
        raise RuntimeError("%s (gfx950 backend) needs %s on a ROCm device, got %s" % (who, what, t.device))
    if t.dtype != torch.float32:
        raise RuntimeError("%s: %s must be torch.float32, got %s" % (who, what, t.dtype))
    if t.dim() != dims:
        raise RuntimeError("%s: %s must have %d dimensions, got %s" % (who, what, dims, tuple(t.shape)))
    return t.detach().contiguous()


def _view_shape(who, mode, stored, emb):
    """(C, H, W) of the view `mode` of a stored (C_s, H_s, W_s) tensor"""
    if mode not in MODES:
        raise RuntimeError("%s: unknown operand view %r (one of %s)" % (who, mode, ", ".join(MODES)))
    cs, hs, ws = (int(v) for v in stored)
    if mode == "shuffle":
        if cs % 4:
            raise RuntimeError("%s: a pixel-shuffle needs a channel count that is a multiple of 4, got %d" % (who, cs))
        return cs // 4, 2 * hs, 2 * ws
    if mode == "unshuffle":
        if hs % 2 or ws % 2:
            raise RuntimeError("%s: the inverse pixel-shuffle needs even H and W, got %d x %d" % (who, hs, ws))
        return 4 * cs, hs // 2, ws // 2
    if mode == "up2":
        return cs, 2 * hs, 2 * ws
    if mode == "embed":
        if cs != 3 or emb is None:
            raise RuntimeError("%s: the embedding view takes a (3, H, W) tensor and the embedding" % who)
        return 3 + int(emb.numel()), hs, ws
    return cs, hs, ws


def _operand(who, x, mode, emb, mask, what="x"):
    x = _tensor(x, who, what, 3)
    emb = _tensor(emb, who, "the embedding", 1) if emb is not None else None
    shape = _view_shape(who, mode, x.shape, emb)
    if mask is not None:
        mask = _tensor(mask, who, "mask", 3)
        if tuple(mask.shape) != shape:
            raise RuntimeError("%s: mask %s does not fit the view %s of %s" % (who, tuple(mask.shape), shape, what))
    return x, emb, mask, shape


def conv3x3(x, weight, bias=None, relu=False, mode="plain", emb=None, mask=None):
    """out (C_out, H, W) = conv3x3(view `mode` of x, weight (C_out, C_in, 3, 3), zero padding 1) (+ bias), max(., 0) if `relu`; the view
    is (C_in, H, W) and never materialised (include/gof_appearance_hip.h: GOF_APP_SRC_*); mask: (C_in, H, W), values where it is <= 0
    are read as 0."""
    x, emb, mask, (ci, h, wd) = _operand("conv3x3", x, mode, emb, mask)
    w = _tensor(weight, "conv3x3", "weight", 4)
    co = int(w.size(0))
    b = _tensor(bias, "conv3x3", "bias", 1) if bias is not None else None
    if tuple(w.shape) != (co, ci, 3, 3) or (b is not None and int(b.numel()) != co):
        raise RuntimeError("conv3x3: weight %s / bias do not fit an input of %d channels" % (tuple(w.shape), ci))
    with _device_of(x):
        out = torch.empty((co, h, wd), dtype=torch.float32, device=x.device)
        B._check(lib.gof_app_conv3x3(ci, co, wd, h, _ptr(x), MODES[mode], _ptr(emb), _ptr(mask), _ptr(w), _ptr(b), 1 if relu else 0, _ptr(out), _stream()))
    return out


def materialize(x, mode, emb=None, mask=None):
    """the view itself as a (C, H, W) tensor: exactly the values the convolutions stage"""
    x, emb, mask, (c, h, wd) = _operand("materialize", x, mode, emb, mask)
    with _device_of(x):
        out = torch.empty((c, h, wd), dtype=torch.float32, device=x.device)
        B._check(lib.gof_app_materialize(MODES[mode], c, wd, h, _ptr(x), _ptr(emb), _ptr(mask), _ptr(out), _stream()))
    return out


def weight_transpose(weight):
    """(C_out, C_in, 3, 3) -> (C_in, C_out, 3, 3) with both taps flipped: the weight of the data gradient"""
    w = _tensor(weight, "weight_transpose", "weight", 4)
    co, ci = int(w.size(0)), int(w.size(1))
    if tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError("weight_transpose: weight must be (C_out, C_in, 3, 3), got %s" % (tuple(w.shape),))
    with _device_of(w):
        out = torch.empty((ci, co, 3, 3), dtype=torch.float32, device=w.device)
        B._check(lib.gof_app_weight_transpose(ci, co, _ptr(w), _ptr(out), _stream()))
    return out


def conv3x3_wgrad(x, dy, mode="plain", emb=None, dy_mode="plain", mask=None):
    """(dW (C_out, C_in, 3, 3), db (C_out,)) of a 3x3 convolution from the view `mode` of its input x and the view `dy_mode` of the
    gradient of its output, masked by `mask` (the layer's ReLU output) if given"""
    x, emb, _, (ci, h, wd) = _operand("conv3x3_wgrad", x, mode, emb, None)
    dy, _, mask, (co, h2, w2) = _operand("conv3x3_wgrad", dy, dy_mode, None, mask, "dy")
    if (h2, w2) != (h, wd) or dy_mode == "embed":
        raise RuntimeError("conv3x3_wgrad: dy is %d x %d through its view, x %d x %d" % (w2, h2, wd, h))
    with _device_of(x):
        nb = lib.gof_app_wgrad_workspace_bytes(ci, co, wd, h)
        ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=x.device)
        dW = torch.empty((co, ci, 3, 3), dtype=torch.float32, device=x.device)
        db = torch.empty((co,), dtype=torch.float32, device=x.device)
        B._check(lib.gof_app_conv3x3_wgrad(ci, co, wd, h, _ptr(x), MODES[mode], _ptr(emb), _ptr(dy), MODES[dy_mode], _ptr(mask), _ptr(dW), _ptr(db),
                                           ws.data_ptr(), int(nb), _stream()))
    return dW, db


def bilinear(x, size):
    """x (C, H, W) (a crop of a contiguous tensor is taken as it lies) -> (C, size[0], size[1]): F.interpolate(x[None], size=size,
    mode="bilinear", align_corners=True)[0]"""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.stride(2) != 1 or x.numel() == 0:
        x = _tensor(x, "bilinear", "x", 3)
    else:
        _tensor(x[:, :1, :1], "bilinear", "x", 3)
        x = x.detach()
    c, h, wd = (int(v) for v in x.shape)
    oh, ow = int(size[0]), int(size[1])
    with _device_of(x):
        out = torch.empty((c, oh, ow), dtype=torch.float32, device=x.device)
        B._check(lib.gof_app_bilinear(c, wd, h, int(x.stride(1)), int(x.stride(0)), x.data_ptr(), ow, oh, _ptr(out), _stream()))
    return out


def up2_backward(g):
    """g (C, 2H, 2W) -> (C, H, W): the transpose of the bilinear x2 up-sample (align_corners=True), as a gather in a fixed order"""
    g = _tensor(g, "up2_backward", "g", 3)
    c, h2, w2 = (int(v) for v in g.shape)
    if h2 % 2 or w2 % 2:
        raise RuntimeError("up2_backward: g must have even H and W, got %d x %d" % (h2, w2))
    with _device_of(g):
        out = torch.empty((c, h2 // 2, w2 // 2), dtype=torch.float32, device=g.device)
        B._check(lib.gof_app_up2_backward(c, w2 // 2, h2 // 2, _ptr(g), _ptr(out), _stream()))
    return out


def _images(who, image, gt):
    image, gt = _tensor(image, who, "image", 3), _tensor(gt, who, "gt_image", 3)
    if image.shape != gt.shape or int(image.size(0)) != 3:
        raise RuntimeError("%s: image and gt_image must both be (3, H, W), got %s and %s" % (who, tuple(image.shape), tuple(gt.shape)))
    h, w = int(image.size(1)), int(image.size(2))
    return image, gt, h, w, (3, h // 32 * 32, w // 32 * 32)


def _cropped(who, t, what, crop):
    t = _tensor(t, who, what, 3)
    if tuple(t.shape) != crop:
        raise RuntimeError("%s: %s must be %s (the crop of the image to multiples of 32), got %s" % (who, what, crop, tuple(t.shape)))
    return t


def head_forward(z, image, gt_image):
    """z (3, Hc, Wc): conv3's output on the crop -> (loss (0-dim), m = sigmoid(z), transformed = m * crop(image)): the arithmetic of
    conv3's epilogue on a stored z"""
    image, gt, h, w, crop = _images("head_forward", image, gt_image)
    z = _cropped("head_forward", z, "z", crop)
    with _device_of(z):
        nb = int(lib.gof_app_head_workspace_bytes(w, h))
        if nb == 0:
            raise RuntimeError(lib.gof_last_error().decode())
        ws = torch.empty(nb, dtype=torch.uint8, device=z.device)
        m = torch.empty(crop, dtype=torch.float32, device=z.device)
        t = torch.empty(crop, dtype=torch.float32, device=z.device)
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        B._check(lib.gof_app_head_forward(w, h, _ptr(z), _ptr(image), _ptr(gt), _ptr(m), _ptr(t), _ptr(loss), ws.data_ptr(), nb, _stream()))
    return loss.reshape(()), m, t


def head_backward(m, image, gt_image, dL):
    """m (3, Hc, Wc): the saved sigmoid, dL (0-dim) -> dz (3, Hc, Wc) = ((g I) m) (1 - m), g = sign(m I - G) dL / (3 Hc Wc): what
    conv3's gradient kernels stage"""
    image, gt, h, w, crop = _images("head_backward", image, gt_image)
    m = _cropped("head_backward", m, "m", crop)
    dL = _tensor(dL, "head_backward", "dL", 0).reshape(1)
    with _device_of(m):
        dz = torch.empty(crop, dtype=torch.float32, device=m.device)
        B._check(lib.gof_app_head_backward(w, h, _ptr(m), _ptr(image), _ptr(gt), _ptr(dL), _ptr(dz), _stream()))
    return dz


def image_grad(m, image, gt_image, dL, d_down):
    """-> d_image (3, H, W): 0 outside the crop, inside g m + the transpose of the bilinear down-sample applied to d_down (3, Hc/32, Wc/32)"""
    image, gt, h, w, crop = _images("image_grad", image, gt_image)
    m = _cropped("image_grad", m, "m", crop)
    dL = _tensor(dL, "image_grad", "dL", 0).reshape(1)
    d_down = _tensor(d_down, "image_grad", "d_down", 3)
    if tuple(d_down.shape) != (3, crop[1] // 32, crop[2] // 32):
        raise RuntimeError("image_grad: d_down must be %s, got %s" % ((3, crop[1] // 32, crop[2] // 32), tuple(d_down.shape)))
    with _device_of(m):
        out = torch.empty((3, h, w), dtype=torch.float32, device=m.device)
        B._check(lib.gof_app_image_grad(w, h, _ptr(m), _ptr(image), _ptr(gt), _ptr(dL), _ptr(d_down), _ptr(out), _stream()))
    return out


# ---- the loss -------------------------------------------------------------------------------------------------------------------
stats = {"forwards": 0, "backwards": 0}          # calls of the two entry points (the launcher writes them next to the binding's counters)


def _describe(who, image, gt, embedding, params):
    """checked, contiguous (image, gt, embedding, params) and the network description"""
    image, gt = _tensor(image, who, "image", 3), _tensor(gt, who, "gt_image", 3)
    if image.shape != gt.shape or int(image.size(0)) != 3:
        raise RuntimeError("%s: image and gt_image must both be (3, H, W), got %s and %s" % (who, tuple(image.shape), tuple(gt.shape)))
    embedding = _tensor(embedding, who, "the embedding", 1)
    if len(params) != 14:
        raise RuntimeError("%s: the network has 14 parameter tensors (weight, bias of %s), got %d" % (who, ", ".join(PARAM_NAMES), len(params)))
    ws = [_tensor(p, who, "%s.weight" % n, 4) for p, n in zip(params[0::2], PARAM_NAMES)]
    bs = [_tensor(p, who, "%s.bias" % n, 1) for p, n in zip(params[1::2], PARAM_NAMES)]
    widths = [int(w.size(0)) for w in ws]
    c_in = [3 + int(embedding.numel())] + [v // 4 for v in widths[:4]] + [widths[4], widths[5]]
    for n, w, b, ci in zip(PARAM_NAMES, ws, bs, c_in):
        if tuple(w.shape) != (int(w.size(0)), ci, 3, 3) or int(b.numel()) != int(w.size(0)):
            raise RuntimeError("%s: %s.weight %s / bias %s do not fit %d input channels" % (who, n, tuple(w.shape), tuple(b.shape), ci))
    if widths[6] != 3:
        raise RuntimeError("%s: conv3 must give 3 channels, got %d" % (who, widths[6]))
    net = GofAppNet(int(embedding.numel()), (C.c_int32 * 6)(*widths[:6]))
    flat = [t for pair in zip(ws, bs) for t in pair]
    return image, gt, embedding, flat, net


def _pointers(tensors):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _forward(image, gt, embedding, params, want_transformed, who="appearance_l1"):
    image, gt, embedding, flat, net = _describe(who, image, gt, embedding, params)
    h, w = int(image.size(1)), int(image.size(2))
    with _device_of(image):
        sb, wb = int(lib.gof_app_saved_bytes(w, h, net)), int(lib.gof_app_workspace_bytes(w, h, net))
        if sb == 0 or wb == 0:
            raise RuntimeError(lib.gof_last_error().decode())
        saved = torch.empty(sb, dtype=torch.uint8, device=image.device)
        ws = torch.empty(wb, dtype=torch.uint8, device=image.device)
        loss = torch.empty(1, dtype=torch.float32, device=image.device)
        transformed = torch.empty((3, h // 32 * 32, w // 32 * 32), dtype=torch.float32, device=image.device) if want_transformed else None
        stats["forwards"] += 1
        B._check(lib.gof_app_l1_forward(w, h, net, _ptr(image), _ptr(gt), _ptr(embedding), _pointers(flat), _ptr(loss), _ptr(transformed),
                                        saved.data_ptr(), sb, ws.data_ptr(), wb, _stream()))
    return loss.reshape(()), transformed, saved, (image, gt, embedding, flat, net)


class _AppearanceL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, embedding, *params):
        loss, _, saved, (image, gt, embedding, flat, net) = _forward(image, gt, embedding, params, False)
        ctx.net, ctx.saved_buffer = net, saved
        ctx.save_for_backward(image, gt, embedding, *flat)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dL):
        image, gt, embedding = ctx.saved_tensors[:3]
        flat = list(ctx.saved_tensors[3:])
        net, saved = ctx.net, ctx.saved_buffer
        h, w = int(image.size(1)), int(image.size(2))
        dL = _tensor(dL, "appearance_l1 backward", "the incoming gradient", 0).reshape(1)
        with _device_of(image):
            wb = int(lib.gof_app_workspace_bytes(w, h, net))
            ws = torch.empty(wb, dtype=torch.uint8, device=image.device)
            d_image = torch.empty((3, h, w), dtype=torch.float32, device=image.device)
            d_emb = torch.empty((int(embedding.numel()),), dtype=torch.float32, device=image.device)
            d_params = [torch.empty(tuple(p.shape), dtype=torch.float32, device=image.device) for p in flat]
            stats["backwards"] += 1
            B._check(lib.gof_app_l1_backward(w, h, net, _ptr(image), _ptr(gt), _ptr(embedding), _pointers(flat), _ptr(dL), saved.data_ptr(),
                                             int(saved.numel()), _ptr(d_image), _ptr(d_emb), _pointers(d_params), ws.data_ptr(), wb, _stream()))
        return (d_image, None, d_emb) + tuple(d_params)


def appearance_l1(image, gt_image, embedding, params):
    """image, gt_image (3, H, W), embedding (E,), params: the 14 tensors of `network_params` -> the 0-dim loss of train.py:67-85
    (crop to multiples of 32, down-sample by 32, the network, sigmoid, product with the crop of the image, L1 against the crop of
    gt_image), differentiable with respect to image, embedding and params"""
    return _AppearanceL1.apply(image, gt_image, embedding, *params)


def network_params(network):
    """the 14 parameter tensors of a scene.appearance_network.AppearanceNetwork, by the reference's names, in the library's order"""
    out = []
    for name in PARAM_NAMES:
        m = network
        for part in name.split("."):
            m = getattr(m, part)
        out += [m.weight, m.bias]
    return out


def L1_loss_appearance(image, gt_image, gaussians, view_idx, return_transformed_image=False):
    """train.py:67-88 with the reference's signature: `gaussians.appearance_network` and `gaussians.get_apperance_embedding(view_idx)`
    are read as the reference reads them; return_transformed_image=True (train.py:200, forward only) gives the transformed image resized
    to the image's size."""
    embedding = gaussians.get_apperance_embedding(view_idx)
    params = network_params(gaussians.appearance_network)
    if type(image) is not torch.Tensor:                 # (a channel slice of the rasterizer's image: the same tensor, the same graph)
        with torch._C.DisableTorchFunctionSubclass():
            image = image.as_subclass(torch.Tensor)
    if not return_transformed_image:
        return appearance_l1(image, gt_image, embedding, params)
    _, transformed, _, _ = _forward(image, gt_image, embedding, params, True, "L1_loss_appearance")
    return bilinear(transformed, (int(image.size(1)), int(image.size(2))))
