#!/usr/bin/env python3
"""Time one LPIPS call (full-width VGG, seeded random weights) and each of its convolution layers, next to the same composition in
torch on the same GPU (what the pip package runs).  Recorded in DESIGN.md §5 and profiles/; nothing is gated on it.

    python tests/devtools/dev_lpips_time.py [--width 1600 --height 1063 --reps 5 --out profiles/lpips_1600x1063.json]

Per measurement: 2 warm-up runs, `reps` timed runs between device events on the current stream, the median is reported."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-opacity-fields_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import image_metrics as M  # noqa: E402
import lpips_restatement as R  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def torch_lpips(a, b, weights):
    conv_w, conv_b, lin_w = weights
    x = R.scale_layer(torch.stack([a, b]), torch.float32)
    total, k = 0.0, 0
    for (ci, co, pool, tap), w, bias in zip(M.VGG_LAYERS, conv_w, conv_b):
        if pool:
            x = F.max_pool2d(x, 2, 2)
        x = torch.relu(F.conv2d(x, w, bias, padding=1))
        if tap:
            total = total + R.tap_value(x, lin_w[k])
            k += 1
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1063)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H = args.width, args.height
    weights = tuple([t.to(dev) for t in group] for group in R.make_weights(M.VGG_LAYERS, seed=11))
    img0, img1 = (t[0].to(dev) for t in R.make_images(W, H, seed=5))
    rows = []
    w, h = W, H
    g = torch.Generator(device="cpu").manual_seed(3)
    for i, (ci, co, pool, tap) in enumerate(M.VGG_LAYERS):
        if pool:
            w, h = w // 2, h // 2
        x = torch.rand((2, ci, h, w), generator=g).to(dev)
        flop = 2.0 * 2 * h * w * co * 9 * ci
        ms_hip = timed(lambda: M.conv3x3(x, weights[0][i], weights[1][i], relu=True), args.reps)
        ms_torch = timed(lambda: torch.relu(F.conv2d(x, weights[0][i], weights[1][i], padding=1)), args.reps)
        rows.append({"layer": i, "c_in": ci, "c_out": co, "width": w, "height": h, "gflop": flop / 1e9, "hip_ms": ms_hip, "hip_tflops": flop / ms_hip / 1e9,
                     "torch_ms": ms_torch, "torch_tflops": flop / ms_torch / 1e9})
        print("layer %2d %3d->%3d %4dx%-4d %7.1f GFLOP  hip %8.3f ms %6.1f TF/s | torch %8.3f ms %6.1f TF/s" % (i, ci, co, w, h, flop / 1e9, ms_hip,
              flop / ms_hip / 1e9, ms_torch, flop / ms_torch / 1e9), flush=True)
        del x
    ms_call = timed(lambda: M.network_distance(img0, img1, M.VGG_LAYERS, *weights), args.reps)
    ms_torch_call = timed(lambda: torch_lpips(img0, img1, weights), args.reps)
    v_hip = M.network_distance(img0, img1, M.VGG_LAYERS, *weights)[0].item()
    v_torch = float(torch_lpips(img0, img1, weights))
    total = sum(r["gflop"] for r in rows)
    print("one call at %dx%d (%.0f GFLOP of convolutions): hip %.2f ms (%.1f TF/s), torch %.2f ms (%.1f TF/s); values %.9g / %.9g" % (
        W, H, total, ms_call, total / ms_call, ms_torch_call, total / ms_torch_call, v_hip, v_torch))
    result = {"width": W, "height": H, "reps": args.reps, "device": torch.cuda.get_device_name(0), "layers": rows, "call_hip_ms": ms_call,
              "call_torch_ms": ms_torch_call, "conv_gflop": total, "value_hip": v_hip, "value_torch": v_torch}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
