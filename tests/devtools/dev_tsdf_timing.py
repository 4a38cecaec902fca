#!/usr/bin/env python3
"""Timing of the TSDF fusion (csrc/tsdf.hip) with HIP events: per-view touch + integrate and one extraction, at DTU's training shape
(800x600, 49 views) and at 1600x1200, on analytic depth maps of a sphere (radius 0.5, ring of cameras at 1.6, voxel 0.002 as
extract_mesh_tsdf.py).  Integrate's rate counts 2 x 20 B per voxel of the frame's blocks plus the depth and colour bytes.

    python tests/devtools/dev_tsdf_timing.py [--out profiles/tsdf_timing.md]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-opacity-fields_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsdf_restatement as T  # noqa: E402
import tsdf_fusion as F  # noqa: E402


def views(W, H, n, radius=1.6):
    K = T.intrinsic(W, H, 45.0)
    dev = "cuda"
    u, v = torch.meshgrid(torch.arange(W, dtype=torch.float64, device=dev), torch.arange(H, dtype=torch.float64, device=dev), indexing="xy")
    out = []
    for i in range(n):
        a = 2 * math.pi * i / n
        E = T.look_at((radius * math.cos(a), radius * math.sin(a), 0.4 * math.sin(2.0 * i)))
        Et = torch.from_numpy(E).to(dev)
        R, t = Et[:3, :3], Et[:3, 3]
        C = -R.T @ t
        dc = torch.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], torch.ones_like(u)], -1)
        d = dc @ R
        b = 2 * (d @ C)
        aa = (d * d).sum(-1)
        q = b * b - 4 * aa * (C @ C - 0.25)
        tt = (-b - torch.sqrt(q.clamp_min(0))) / (2 * aa)
        depth = torch.where((q > 0) & (tt > 0), tt, torch.zeros_like(tt)).float().contiguous()
        col = torch.stack([0.5 + 0.5 * torch.sin(0.02 * u), v / H, torch.full_like(u, 0.3)], 0).float().contiguous()
        out.append((depth, col, torch.from_numpy(K).float().cuda(), Et.float()))
    return out


def run(W, H, n, v=0.002):
    vs = views(W, H, n)
    for warm in range(2):
        vol = F.TSDFVolume(v, block_count=50000)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        torch.cuda.synchronize()
        ev[0].record()
        for i, (d, c, K, E) in enumerate(vs):
            vol.integrate(d, c, K, E)
            ev[i + 1].record()
        torch.cuda.synchronize()
        per_view = [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = vol.extract_triangle_mesh()
        e1.record()
        torch.cuda.synchronize()
    ext_ms = e0.elapsed_time(e1)
    # frame block counts (for the byte count): one more pass with the counts read back from a fresh volume per view
    nb = []
    for d, c, K, E in vs:
        one = F.TSDFVolume(v, block_count=1024)
        one.integrate(d, c, K, E)
        nb.append(one.num_blocks)
    ms = sorted(per_view)[len(per_view) // 2]
    mean_nb = sum(nb) / len(nb)
    bytes_view = 2 * 20 * 4096 * mean_nb + W * H * 16
    return dict(shape="%dx%d" % (W, H), views=n, median_view_ms=ms, mean_view_ms=sum(per_view) / n, frame_blocks=mean_nb,
                gbs=bytes_view / (ms * 1e-3) / 1e9, active=vol.num_blocks, extract_ms=ext_ms, us_per_block=1e3 * ext_ms / vol.num_blocks,
                V=m.vertices.shape[0], F=m.triangles.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run(800, 600, 49), run(1600, 1200, 49)]
    lines = ["| shape | views | touch+integrate per view, median (mean) ms | frame blocks | integrate GB/s (of ~6300) | active blocks | extraction ms | us per active block | V | F |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %d | %.3f (%.3f) | %.0f | %.0f | %d | %.2f | %.3f | %d | %d |" % (
            r["shape"], r["views"], r["median_view_ms"], r["mean_view_ms"], r["frame_blocks"], r["gbs"], r["active"], r["extract_ms"],
            r["us_per_block"], r["V"], r["F"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
