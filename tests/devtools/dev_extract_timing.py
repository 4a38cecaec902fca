#!/usr/bin/env python3
"""Times the mesh extraction's own steps (mesh_extraction, csrc/extract.hip) with HIP events and writes profiles/extract_timing.md.

    python tests/devtools/dev_extract_timing.py [--out profiles/extract_timing.md] [--gaussians 5e6] [--views 300] [--edges 20e6] [--size 1600x1063]

The three entry points on the device (median of --repeat runs after one warm-up, events around each call, so allocation and the calls'
own read-backs are inside) against a torch route on the same device.  The torch route is a port of tests/extract_restatement.py
(candidates / seen / bisect_step / edge_filter) to torch tensor operations, one launch per operation: the frustum test one view at a
time in fp64, the bisection round with elementwise selects.  It is not the reference's own code: the reference's two einsums over all
views at once need views x points x 16 bytes, which does not fit at this size, and its boolean-mask assignments synchronise with the
host; the report says what the comparison route is.  Nothing here is asserted anywhere."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "gaussian-opacity-fields_amd")):
    sys.path.insert(0, p)

import extract_restatement as R  # noqa: E402
import mesh_extraction as ME  # noqa: E402


def timed(fn, repeat):
    fn()
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), out


def torch_candidates(xyz, scaling, rotation):
    """extract_restatement.candidates in torch: the rotation entry by entry, one corner at a time, then the centres"""
    q = rotation / torch.sqrt(((rotation[:, 0] * rotation[:, 0] + rotation[:, 1] * rotation[:, 1]) + rotation[:, 2] * rotation[:, 2])
                              + rotation[:, 3] * rotation[:, 3])[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
            [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
            [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]]
    s = scaling * 3.0
    corners = torch.empty((len(xyz), 8, 3), dtype=torch.float32, device=xyz.device)
    for c in range(8):
        a = [s[:, j] if (c >> (2 - j)) & 1 else -s[:, j] for j in range(3)]
        for k in range(3):
            corners[:, c, k] = ((rows[k][0] * a[0] + rows[k][1] * a[1]) + rows[k][2] * a[2]) + xyz[:, k]
    m = torch.maximum(torch.maximum(s[:, 0], s[:, 1]), s[:, 2])
    return torch.cat([corners.reshape(-1, 3), xyz]), torch.cat([m.repeat_interleave(8), m])


def torch_tetra_points(xyz, scaling, rotation, rec, W, H, near, far):
    """extract_restatement.tetra_points in torch on the device: candidates, then extract_restatement.seen one view at a time in fp64"""
    pts, scales = torch_candidates(xyz, scaling, rotation)
    p = pts.double()
    cx, cy = float(np.float32(W / 2.0)), float(np.float32(H / 2.0))
    keep = torch.zeros(len(pts), dtype=torch.bool, device=xyz.device)
    for v in rec:
        m, fx, fy = [float(t) for t in v["m"]], float(v["fx"]), float(v["fy"])
        X = ((m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]) + m[3]
        Y = ((m[4] * p[:, 0] + m[5] * p[:, 1]) + m[6] * p[:, 2]) + m[7]
        Z = ((m[8] * p[:, 0] + m[9] * p[:, 1]) + m[10] * p[:, 2]) + m[11]
        u, w = (fx * X + cx * Z) / Z, (fy * Y + cy * Z) / Z
        keep |= (Z >= near) & (Z <= far) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1)
    return pts[keep], scales[keep]


def torch_bisect_step(l, r, ls, rs, value):
    """extract_restatement.bisect_step (mode FINAL_ALPHA) in torch: elementwise selects, in place -> the next query points"""
    mid = (l + r) / 2
    sdf = (1 - value) - 0.5
    low = ((sdf < 0) & (ls < 0)) | ((sdf > 0) & (ls > 0))
    ls.copy_(torch.where(low, sdf, ls))
    rs.copy_(torch.where(low, rs, sdf))
    l.copy_(torch.where(low[:, None], mid, l))
    r.copy_(torch.where(low[:, None], r, mid))
    return (l + r) / 2


def torch_edge_filter(e, es):
    d = e[:, 0] - e[:, 1]
    return torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= es[:, 0, 0] + es[:, 1, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_timing.md"))
    ap.add_argument("--gaussians", type=float, default=5e6)
    ap.add_argument("--views", type=int, default=300)
    ap.add_argument("--edges", type=float, default=20e6)
    ap.add_argument("--size", default="1600x1063")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    W, H = (int(v) for v in args.size.split("x"))
    P, E = int(args.gaussians), int(args.edges)
    xyz, sc, rot = (torch.from_numpy(a).to(dev) for a in R.gaussians(P))
    cams = R.ring_cameras(args.views, sizes=((W, H),))
    for cam in cams:
        cam.focal_x, cam.focal_y = cam.focal_x * W / 161.0, cam.focal_y * W / 161.0
    rec, _, _ = ME.frustum_records(cams)
    t_tp, (pts, _) = timed(lambda: ME.tetra_points(xyz, sc, rot, rec, W, H, 0.02, 1e6), args.repeat)
    st = ME.last_stats()["tetra_points"]
    rng = np.random.default_rng(5)
    e = torch.from_numpy(rng.uniform(-1, 1, (E, 2, 3)).astype(np.float32)).to(dev)
    es = torch.from_numpy(rng.uniform(0.1, 1.5, (E, 2, 1)).astype(np.float32)).to(dev)
    sdf = torch.from_numpy(rng.uniform(-0.5, 0.5, (E, 2, 1)).astype(np.float32)).to(dev)
    value = torch.from_numpy(rng.uniform(0, 1, E).astype(np.float32)).to(dev)
    l, r, ls, rs = e[:, 0].contiguous(), e[:, 1].contiguous(), sdf[:, 0, 0].contiguous(), sdf[:, 1, 0].contiguous()
    mid = torch.empty((E, 3), dtype=torch.float32, device=dev)
    t_bs, _ = timed(lambda: ME.bisect_step(l, r, ls, rs, value, ME.BISECT_FINAL_ALPHA, mid_out=mid), args.repeat)
    t_ef, keep = timed(lambda: ME.edge_filter(e, es), args.repeat)
    tt = {}
    if not args.no_torch:
        tt["tetra"], (tpts, _) = timed(lambda: torch_tetra_points(xyz, sc, rot, rec, W, H, 0.02, 1e6), 1)
        tl, tr, tls, trs = e[:, 0].clone(), e[:, 1].clone(), sdf[:, 0, 0].clone(), sdf[:, 1, 0].clone()
        tt["bisect"], _ = timed(lambda: torch_bisect_step(tl, tr, tls, trs, value), args.repeat)
        tt["filter"], _ = timed(lambda: torch_edge_filter(e, es), args.repeat)

    def c(k):
        return "%.2f" % tt[k] if k in tt else "not run"
    lines = ["# Mesh extraction steps: first measured times", "",
             "Written by `tests/devtools/dev_extract_timing.py` on %s (%s), torch %s." % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d"), torch.__version__),
             "Workload: %.1f M Gaussians (%.1f M candidates, %d kept) against %d views of %d x %d; %.1f M edges." % (P / 1e6, 9 * P / 1e6, st["kept"], len(cams), W, H, E / 1e6),
             "Times: HIP events around each call, median of %d after one warm-up; allocations and the calls' own read-backs included." % args.repeat,
             "torch route: tests/extract_restatement.py ported to torch tensor operations on the same device (one launch per operation; the frustum",
             "test one view at a time in fp64, the round with elementwise selects) -- not the reference's code, whose einsums over all views at once",
             "would need %.0f GB for their first tensor alone." % (len(cams) * 9 * P * 16 / 1e9), "",
             "| step | HIP ms | torch ms |", "|---|---|---|",
             "| tetra_points (count + emit) | %.2f | %s |" % (t_tp, c("tetra")),
             "| bisect_step, one round | %.2f | %s |" % (t_bs, c("bisect")),
             "| edge_filter | %.2f | %s |" % (t_ef, c("filter")), "",
             "Workspace of tetra_points: %.2f B per candidate." % (st["workspace_bytes"] / (9 * P)), ""]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
