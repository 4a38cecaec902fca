"""The LPIPS contract restated in torch on the CPU, in this project's own words: scaling layer, 3x3 convolutions
with zero padding 1 + bias + ReLU, flooring 2x2 max-pools, and at every tap

    sum_px sum_c w_c (f0_c / (||f0|| + 1e-10) - f1_c / (||f1|| + 1e-10))^2 / (H_l W_l),      ||.|| = sqrt(sum over the channels)

summed over the taps.  Run at torch.float64 it is the truth, at torch.float32 the yardstick (what an fp32 framework computes).
Networks are data: (c_in, c_out, pool_before, tap_after) per convolution, seeded random weights."""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
VGG_WIDTHS = (64, 128, 256, 512, 512)
THIN_WIDTHS = (32, 32, 64, 64, 128)          # one instance of every tile shape of the convolution kernel (C_out % 32, % 64, % 128)


def vgg_layers(widths=VGG_WIDTHS):
    """the VGG16 structure 2-2-3-3-3 with the given width per block, taps at the end of every block"""
    layers, c = [], 3
    for block, (n, w) in enumerate(zip((2, 2, 3, 3, 3), widths)):
        for i in range(n):
            layers.append((c, w, 1 if (i == 0 and block > 0) else 0, 1 if i == n - 1 else 0))
            c = w
    return tuple(layers)


def make_weights(layers, seed):
    """conv weights ~ N(0, 2 / (9 C_in)), small biases, lin weights uniform in [0, 1): fp32 tensors"""
    g = torch.Generator().manual_seed(seed)
    conv_w = [(torch.randn((co, ci, 3, 3), generator=g, dtype=torch.float64) * (2.0 / (9 * ci)) ** 0.5).float() for ci, co, _, _ in layers]
    conv_b = [(0.05 * torch.randn((co,), generator=g, dtype=torch.float64)).float() for _, co, _, _ in layers]
    lin_w = [torch.rand((co,), generator=g, dtype=torch.float64).float() for _, co, _, tap in layers if tap]
    return conv_w, conv_b, lin_w


def make_images(W, H, seed, n=1):
    """(n,3,H,W) fp32 in [0,1]: a smooth pattern plus noise, and a perturbed copy of it"""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    a = torch.empty((n, 3, H, W), dtype=torch.float64)
    for i in range(n):
        for c in range(3):
            a[i, c] = 0.5 + 0.35 * torch.sin(0.21 * (c + 1) * x + 0.13 * y * (i + 1) + c) * torch.cos(0.17 * y - 0.05 * x * (c + 1))
    a = (a + 0.08 * torch.randn(a.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    b = (a + 0.06 * torch.randn(a.shape, generator=g, dtype=torch.float64) + 0.03 * torch.sin(0.4 * x)).clamp(0, 1)
    return a.float(), b.float()


def scale_layer(x, dtype):
    sh = torch.tensor(SHIFT, dtype=torch.float32).to(dtype).view(1, 3, 1, 1).to(x.device)
    sc = torch.tensor(SCALE, dtype=torch.float32).to(dtype).view(1, 3, 1, 1).to(x.device)
    return (x.to(dtype) - sh) / sc


def conv(x, w, b, dtype):
    """the layer before its ReLU"""
    return F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=1)


def conv_magnitude(x, w, b):
    """sum_k |w_k x_k| + |b| per output element, fp64: what the rounding-error bound of a K-term chain is proportional to"""
    return F.conv2d(x.double().abs(), w.double().abs(), None, padding=1) + b.double().abs().view(1, -1, 1, 1)


def pool(x):
    return F.max_pool2d(x, 2, 2)


def tap_value(f, w):
    """f (2,C,h,w): the two images' features -> the tap's value"""
    f0, f1 = f[0], f[1]
    n0 = torch.sqrt((f0 * f0).sum(0, keepdim=True)) + 1e-10
    n1 = torch.sqrt((f1 * f1).sum(0, keepdim=True)) + 1e-10
    d = (f0 / n0 - f1 / n1) ** 2
    return (d * w.to(f.dtype).view(-1, 1, 1)).sum() / (f.shape[1:][1] * f.shape[1:][2])


def forward(img0, img1, layers, weights, dtype):
    """img0, img1 (3,H,W) -> dict(value, per_tap [n_taps], layer_in [per layer: (2,C_in,h,w)], pre_relu [per layer], pooled [per pool])
    all computed at `dtype`"""
    conv_w, conv_b, lin_w = weights
    x = scale_layer(torch.stack([img0, img1]), dtype)
    out = {"layer_in": [], "pre_relu": [], "pooled": [], "per_tap": []}
    k = 0
    for (ci, co, pool_before, tap), w, b in zip(layers, conv_w, conv_b):
        if pool_before:
            x = pool(x)
            out["pooled"].append(x)
        out["layer_in"].append(x)
        y = conv(x, w, b, dtype)
        out["pre_relu"].append(y)
        x = torch.relu(y)
        if tap:
            out["per_tap"].append(tap_value(x, lin_w[k]))
            k += 1
    out["per_tap"] = torch.stack(out["per_tap"])
    v = out["per_tap"][0]
    for t in out["per_tap"][1:]:
        v = v + t
    out["value"] = v
    return out


def conv_bound(x, w, b):
    """(K + 2) 2^-24 (sum |w x| + |b|) for a layer's fp32 input x: the bound of a K-term fmaf chain plus the bias addition"""
    K = 9 * int(w.shape[1])
    return (K + 2) * 2.0 ** -24 * conv_magnitude(x, w, b)


def save_image_bytes(x):
    """what torchvision.utils.save_image stores for a (3,H,W) tensor: floor(255 x + 0.5) clamped to [0, 255], in fp32 as torchvision
    computes it, as (H,W,3) uint8"""
    v = x.float().numpy() * np.float32(255) + np.float32(0.5)
    return np.floor(np.clip(v, np.float32(0), np.float32(255))).astype(np.uint8).transpose(1, 2, 0)
