"""The LPIPS metric of the reference's metrics.py on the GPU, without the `lpips` pip package and torchvision.

    lpips_fn = LPIPS(net='vgg').to(device)                 # metrics.py:100
    d = lpips_fn(render, gt)                               # metrics.py:76: (N,3,H,W) in [0,1] -> (N,1,1,1)

    conv3x3(x, weight, bias, relu) / maxpool2(x)           # the pieces, as the library exports them
    network_distance(img0, img1, layers, ...)              # any network of 3x3 convolutions, pools and taps

The kernels are ``gof_lpips_*`` of libgof_hip.so (csrc/lpips.hip, include/gof_lpips_hip.h); the contract is DESIGN.md §3.12: fp32
tensors on a ROCm device in and out, the convolutions on the exact fp32 matrix instruction in a fixed order of K, every sum in a
fixed order (bit-reproducible).  There is no host fallback and no download: the two weight files are the user's own, as they are
for the pip package, and a missing one is a FileNotFoundError at construction that lists every place searched.
"""
import ctypes as C
import functools
import importlib.util
import os

import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["LPIPS", "VGG_LAYERS", "VGG_FEATURE_INDICES", "SHIFT", "SCALE", "conv3x3", "maxpool2", "network_distance", "GofLpipsLayer",
           "find_weight_files"]

lib = B.lib
_vp, _sz, _i64, _i32 = C.c_void_p, C.c_size_t, C.c_int64, C.c_int32


class GofLpipsLayer(C.Structure):
    """Mirror of ``GofLpipsLayer`` in include/gof_lpips_hip.h."""
    _fields_ = [("c_in", C.c_int32), ("c_out", C.c_int32), ("pool_before", C.c_int32), ("tap_after", C.c_int32)]


_PL = C.POINTER(GofLpipsLayer)
_PF = C.POINTER(C.c_float)
_PP = C.POINTER(C.c_void_p)
gn.bind(lib, {"gof_lpips_workspace_bytes": [_i32, _i32, _i32, _PL]}, {
        "gof_lpips_conv3x3": [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp],
        "gof_lpips_maxpool2": [_i64, _i32, _i32, _vp, _vp, _vp],
        "gof_lpips_forward": [_i32, _i32, _vp, _vp, _PF, _PF, _i32, _PL, _PP, _PP, _PP, _vp, _vp, _vp, _sz, _vp]})

# the scaling layer of the pip package (lpips/lpips.py: ScalingLayer)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# VGG16's convolutions as (c_in, c_out, pool_before, tap_after): taps after relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
VGG_LAYERS = ((3, 64, 0, 0), (64, 64, 0, 1),
              (64, 128, 1, 0), (128, 128, 0, 1),
              (128, 256, 1, 0), (256, 256, 0, 0), (256, 256, 0, 1),
              (256, 512, 1, 0), (512, 512, 0, 0), (512, 512, 0, 1),
              (512, 512, 1, 0), (512, 512, 0, 0), (512, 512, 0, 1))
# where torchvision's vgg16().features keeps them (the keys `features.N.weight / .bias` of vgg16-397923af.pth)
VGG_FEATURE_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG16_FILE = "vgg16-397923af.pth"
LIN_FILE = "vgg.pth"

# the device seams, by the names the host tests replace (tests/test_lpips_host.py); one definition each: gof_native
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "image_metrics")


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


def conv3x3(x, weight, bias, relu=True):
    """x (N,C_in,H,W), weight (C_out,C_in,3,3), bias (C_out,), fp32 on one ROCm device -> (N,C_out,H,W): the 3x3 convolution with zero
    padding 1 plus bias, max(., 0) applied if `relu`.  C_out must be a multiple of 32."""
    x, w, b = _tensor(x, "conv3x3", "x", 4), _tensor(weight, "conv3x3", "weight", 4), _tensor(bias, "conv3x3", "bias", 1)
    n, ci, h, wd = (int(s) for s in x.shape)
    co = int(w.size(0))
    if tuple(w.shape) != (co, ci, 3, 3) or int(b.numel()) != co:
        raise RuntimeError("conv3x3: weight %s / bias %s do not fit an input of %d channels" % (tuple(w.shape), tuple(b.shape), ci))
    with _device_of(x):
        out = torch.empty((n, co, h, wd), dtype=torch.float32, device=x.device)
        B._check(lib.gof_lpips_conv3x3(n, ci, co, wd, h, _ptr(x), _ptr(w), _ptr(b), 1 if relu else 0, _ptr(out), _stream()))
    return out


def maxpool2(x):
    """x (N,C,H,W) fp32 on a ROCm device -> (N,C,H//2,W//2): nn.MaxPool2d(2, 2)"""
    x = _tensor(x, "maxpool2", "x", 4)
    n, c, h, w = (int(s) for s in x.shape)
    with _device_of(x):
        out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
        B._check(lib.gof_lpips_maxpool2(n * c, w, h, _ptr(x), _ptr(out), _stream()))
    return out


def network_distance(img0, img1, layers, conv_weights, conv_biases, lin_weights, shift=SHIFT, scale=SCALE):
    """img0, img1 (3,H,W) fp32 on a ROCm device; layers: (c_in, c_out, pool_before, tap_after) per convolution; conv_weights /
    conv_biases: one tensor per layer, lin_weights: one (c_out,) tensor per tap -> (value: 0-dim tensor, per_tap: (n_taps,) tensor)"""
    a, b = _tensor(img0, "network_distance", "img0", 3), _tensor(img1, "network_distance", "img1", 3)
    if a.shape != b.shape or int(a.size(0)) != 3:
        raise RuntimeError("network_distance: the images must both be (3, H, W), got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    h, w = int(a.size(1)), int(a.size(2))
    n = len(layers)
    n_taps = sum(1 for L in layers if L[3])
    if len(conv_weights) != n or len(conv_biases) != n or len(lin_weights) != n_taps:
        raise RuntimeError("network_distance: %d layers with %d taps need as many weights / biases / lin weights" % (n, n_taps))
    desc = (GofLpipsLayer * max(n, 1))(*[GofLpipsLayer(int(L[0]), int(L[1]), 1 if L[2] else 0, 1 if L[3] else 0) for L in layers])
    held = []

    def pointers(tensors, shapes, what):
        arr = (C.c_void_p * max(len(tensors), 1))()
        for i, (t, shape) in enumerate(zip(tensors, shapes)):
            t = _tensor(t, "network_distance", what, len(tuple(t.shape)) if isinstance(t, torch.Tensor) else 1)
            if t.numel() != shape:
                raise RuntimeError("network_distance: %s %d has %d elements, the layer needs %d" % (what, i, t.numel(), shape))
            held.append(t)
            arr[i] = t.data_ptr()
        return arr
    pw = pointers(conv_weights, [L[0] * L[1] * 9 for L in layers], "conv weight")
    pb = pointers(conv_biases, [L[1] for L in layers], "conv bias")
    plin = pointers(lin_weights, [L[1] for L in layers if L[3]], "lin weight")
    sh, sc = (C.c_float * 3)(*shift), (C.c_float * 3)(*scale)
    with _device_of(a):
        nb = lib.gof_lpips_workspace_bytes(w, h, n, desc)
        ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=a.device)
        out = torch.empty(1 + max(n_taps, 1), dtype=torch.float32, device=a.device)
        B._check(lib.gof_lpips_forward(w, h, _ptr(a), _ptr(b), sh, sc, n, desc, pw, pb, plin, out.data_ptr(), out.data_ptr() + 4,
                                       ws.data_ptr(), int(nb), _stream()))
    return out[0], out[1:1 + n_taps]


# ---- the weight files -------------------------------------------------------------------------------------------------------------
def _lpips_package_weights():
    """the weights directory of an installed `lpips` package (not this backend's stand-in of that name), or None"""
    shims = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shims")
    try:
        spec = importlib.util.find_spec("lpips")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.origin or os.path.abspath(spec.origin).startswith(shims):
        return None
    return os.path.join(os.path.dirname(spec.origin), "weights", "v0.1")


def find_weight_files():
    """-> (path of torchvision's VGG16 checkpoint, path of the lpips package's lin weights), searched in this order: the environment
    (GOF_LPIPS_VGG16, GOF_LPIPS_LIN), torch's hub cache ($TORCH_HOME/hub/checkpoints, default ~/.cache/torch/hub/checkpoints), an
    installed lpips package's own weights directory.  Nothing is downloaded: FileNotFoundError lists every place searched."""
    hub = os.path.join(os.environ.get("TORCH_HOME") or os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.expanduser("~/.cache"), "torch"),
                       "hub", "checkpoints")
    pkg = _lpips_package_weights()
    found, searched = [], []
    for env, fname, what in (("GOF_LPIPS_VGG16", VGG16_FILE, "torchvision's VGG16 checkpoint (keys features.N.weight / .bias)"),
                             ("GOF_LPIPS_LIN", LIN_FILE, "the lpips package's weights/v0.1/vgg.pth (keys lin{k}.model.1.weight)")):
        places = []
        if os.environ.get(env):
            places.append("%s = %s" % (env, os.environ[env]))
        else:
            places.append("%s (not set)" % env)
        candidates = [os.environ[env]] if os.environ.get(env) else []
        candidates.append(os.path.join(hub, fname))
        places.append(candidates[-1])
        if pkg is not None:
            candidates.append(os.path.join(pkg, fname))
            places.append(candidates[-1])
        else:
            places.append("an installed lpips package's weights/v0.1/%s (no such package)" % fname)
        hit = next((p for p in candidates if os.path.isfile(p)), None)
        found.append(hit)
        if hit is None:
            searched.append("%s: searched %s" % (what, "; ".join(places)))
    if searched:
        raise FileNotFoundError("LPIPS(net='vgg'): weight file(s) not found, and nothing is downloaded.  " + "  ".join(searched))
    return tuple(found)


def _load_vgg_weights(vgg_path, lin_path):
    sd = torch.load(vgg_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    conv_w, conv_b, lin_w = [], [], []
    for (ci, co, _, _), idx in zip(VGG_LAYERS, VGG_FEATURE_INDICES):
        w, b = sd["features.%d.weight" % idx], sd["features.%d.bias" % idx]
        if tuple(w.shape) != (co, ci, 3, 3) or tuple(b.shape) != (co,):
            raise RuntimeError("%s: features.%d has shapes %s / %s, VGG16 has (%d, %d, 3, 3) / (%d,)" % (vgg_path, idx, tuple(w.shape), tuple(b.shape), co, ci, co))
        conv_w.append(w.float().contiguous())
        conv_b.append(b.float().contiguous())
    for k, co in enumerate(L[1] for L in VGG_LAYERS if L[3]):
        w = lin["lin%d.model.1.weight" % k]
        if w.numel() != co:
            raise RuntimeError("%s: lin%d.model.1.weight has %d elements, the tap has %d channels" % (lin_path, k, w.numel(), co))
        lin_w.append(w.float().reshape(co).contiguous())
    return conv_w, conv_b, lin_w


class LPIPS:
    """Takes the place of the pip package's ``lpips.LPIPS`` for what metrics.py does with it: ``LPIPS(net='vgg').to(device)`` and
    ``model(in0, in1)`` on (N,3,H,W) fp32 device tensors -> (N,1,1,1).  As in the package, the inputs are used as given unless
    ``normalize=True`` (then 2 x - 1 first); metrics.py passes [0,1] images without it, and so does this."""

    def __init__(self, net="vgg", version="0.1", **kwargs):
        if net != "vgg" or str(version) != "0.1":
            raise NotImplementedError("LPIPS(net=%r, version=%r): this backend implements net='vgg', version='0.1' (what metrics.py uses)" % (net, version))
        self.net, self.version = net, str(version)
        self.weight_files = find_weight_files()
        self._cpu = _load_vgg_weights(*self.weight_files)
        self._on = {}

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def cuda(self, *a, **k):
        return self

    def train(self, mode=True):
        return self

    def requires_grad_(self, flag=False):
        return self

    def _weights(self, device):
        if device not in self._on:
            self._on[device] = tuple([t.to(device) for t in group] for group in self._cpu)
        return self._on[device]

    def forward(self, in0, in1, normalize=False):
        a, b = _tensor(in0, "LPIPS", "in0", 4), _tensor(in1, "LPIPS", "in1", 4)
        if a.shape != b.shape or int(a.size(1)) != 3:
            raise RuntimeError("LPIPS: the inputs must both be (N, 3, H, W), got %s and %s" % (tuple(a.shape), tuple(b.shape)))
        if normalize:
            a, b = 2 * a - 1, 2 * b - 1
        conv_w, conv_b, lin_w = self._weights(a.device)
        vals = [network_distance(a[i], b[i], VGG_LAYERS, conv_w, conv_b, lin_w)[0] for i in range(int(a.size(0)))]
        return torch.stack(vals).reshape(-1, 1, 1, 1)

    __call__ = forward
