"""The shapes, inputs and expectations the scene-image tests share (tests/test_scene_images_host.py through the emulator,
tests/test_scene_images_gpu.py on the device, tests/golden/make_golden_scene_images.py for Pillow's side), and the resampler restated in
numpy from DESIGN.md §3.15: independent of the product's code.  numpy only: no torch, no Pillow, no product module."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_scene_images_golden.npz")

# (tag, input W, H, output w, h, channels): the smallest shapes at which each mechanism can go wrong
SHAPES = (
    ("clip", 37, 23, 9, 6, 3),             # scale ~ 4, windows clipped at both borders
    ("half", 64, 48, 32, 24, 3),           # exact / 2
    ("odd", 101, 67, 50, 34, 3),           # odd sizes
    ("frac", 123, 77, 77, 48, 3),          # non-integer scale < 2
    ("one", 33, 17, 1, 1, 3),              # one output pixel, window = whole image
    ("noh", 40, 30, 40, 15, 3),            # horizontal pass skipped
    ("nov", 40, 30, 20, 30, 1),            # vertical pass skipped, mode L
    ("same", 50, 40, 50, 40, 3),           # both skipped: conversion only
    ("wide", 1100, 8, 275, 2, 3),          # a row wider than any workgroup tile
    ("tall", 9, 700, 3, 233, 3),           # a column taller than any tile
    ("taps33", 250, 3, 31, 1, 3),          # 33 taps
    ("rgba", 101, 67, 51, 33, 4),          # four L bands resized separately (never Pillow's premultiplying RGBA resize)
    ("up", 20, 10, 30, 15, 3),             # upscale: filterscale clamped to 1
    ("taps257", 1300, 70, 20, 1, 3),       # -r 64-like: 257 taps
)
KINDS = ("random", "steps", "white")


def shape(tag):
    for s in SHAPES:
        if s[0] == tag:
            return s
    raise KeyError(tag)


def golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def make_input(tag, kind):
    """the (H, W, C) uint8 input of a case, regenerated from a seed (never stored).  random: uniform bytes; steps: 0 / 255 steps of
    several widths and single-pixel impulses of both signs -- the negative lobes drive the sums below 0 and above 255, so both ends of
    the clamp are hit; white: constant 255, which must come back as exactly 1.0"""
    i, (_, W, H, _, _, C) = [(i, s) for i, s in enumerate(SHAPES) if s[0] == tag][0]
    rng = np.random.default_rng(7000 + 10 * i + KINDS.index(kind))
    if kind == "random":
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if kind == "white":
        return np.full((H, W, C), 255, np.uint8)
    a = np.zeros((H, W, C), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for c in range(C):
        p = 2 + c
        a[..., c] = np.where(((xx // p) + (yy // (p + 1))) % 2 == 0, 255, 0)
    n = max(4, H * W // 20)
    ys, xs, cs = rng.integers(0, H, n), rng.integers(0, W, n), rng.integers(0, C, n)
    a[ys, xs, cs] = np.where(rng.integers(0, 2, n) == 0, 0, 255).astype(np.uint8)
    a[:, : W // 3] = np.where(a[:, : W // 3] > 127, 0, 255)            # (a long edge through the whole height as well)
    return a


def inputs():
    for s in SHAPES:
        for kind in KINDS:
            yield s, kind, make_input(s[0], kind)


# ---- the resampler restated -----------------------------------------------------------------------------------------
def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(n_in, n_out):
    """-> (taps per output, bounds (n_out, 2) int32 = first input index and count, coefficients (n_out, taps) int32 with 22 fractional
    bits, zero behind the count).  Python floats are IEEE doubles and nothing here is fused."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    taps = int(np.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, taps), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        cnt = min(n_in, int(center + support + 0.5)) - xmin
        w = [bicubic((x + xmin - center + 0.5) * inv) for x in range(cnt)]
        total = 0.0
        for v in w:
            total += v
        for x, v in enumerate(w):
            v = v / total if total != 0.0 else v
            coeffs[xx, x] = int(0.5 + v * (1 << 22)) if v >= 0 else int(-0.5 + v * (1 << 22))
        bounds[xx] = (xmin, cnt)
    return taps, bounds, coeffs


def _pass(img, n_out, axis):
    """one pass over `axis` of an (H, W, C) uint8 image, rounded to 8 bits"""
    n_in = img.shape[axis]
    if n_in == n_out:
        return img
    _, bounds, coeffs = coefficients(n_in, n_out)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for xx in range(n_out):
        lo, cnt = bounds[xx]
        k = coeffs[xx, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (src.ndim - 1))
        s = (1 << 21) + (src[lo:lo + cnt] * k).sum(axis=0)
        assert np.abs(s).max() < 2 ** 31
        out[xx] = np.clip(s >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_bytes(img, w, h):
    """(H, W, C) uint8 -> (h, w, C) uint8: horizontal pass, rounded to 8 bits, then the vertical one"""
    return np.ascontiguousarray(_pass(_pass(img, w, 1), h, 0))


def planar(bytes_hwc):
    """(h, w, C) uint8 -> (C, h, w) float32, each value the correctly rounded float32 quotient byte / 255"""
    return np.ascontiguousarray((bytes_hwc.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the loader's scene: seven small PNG files of different sizes and modes ----------------------------------------------------------------
# (name, mode, W, H); "P" must take the reference's own loadCam
LOADER_FILES = (("a_rgb", "RGB", 64, 48), ("b_rgba", "RGBA", 53, 31), ("c_l", "L", 40, 30), ("d_rgb", "RGB", 101, 67), ("e_p", "P", 32, 24),
                ("f_rgba", "RGBA", 20, 10), ("g_l", "L", 77, 19))


def loader_pixels(i):
    name, mode, W, H = LOADER_FILES[i]
    C = {"RGB": 3, "RGBA": 4, "L": 1, "P": 1}[mode]
    a = np.random.default_rng(9100 + i).integers(0, 256, (H, W, C), dtype=np.uint8)
    return a[..., 0] if C == 1 else a


def resolution_of(orig_w, orig_h, resolution, resolution_scale):
    """the output size loadCam's arithmetic gives (utils/camera_utils.py:20-39), restated"""
    if resolution in (1, 2, 4, 8, 16, 32, 64):
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        down = orig_w / resolution
    s = float(down) * float(resolution_scale)
    return int(orig_w / s), int(orig_h / s)
