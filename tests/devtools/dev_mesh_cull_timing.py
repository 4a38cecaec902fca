#!/usr/bin/env python3
"""Times the mesh culling (mesh_cull, csrc/mesh_cull.hip) with HIP events and writes profiles/mesh_cull_timing.md.

    python tests/devtools/dev_mesh_cull_timing.py [--out profiles/mesh_cull_timing.md] [--vertices 5e6] [--faces 10e6] [--views 64] [--size 1600x1200]

The three stages on the device (median of --repeat runs after one warm-up, events around each call, so allocation and the calls' own
read-backs are inside), the library's per-entry-point split (gof_profile_*), and the same stages through the restatement's route on the
CPU of the same machine (SciPy dilation; the projection with torch on the CPU in fp64; numpy compaction), for reference.  Nothing here
is asserted anywhere."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "gaussian-opacity-fields_amd")):
    sys.path.insert(0, p)

import mesh_cull as M  # noqa: E402
import mesh_cull_cases as K  # noqa: E402
import mesh_cull_restatement as R  # noqa: E402


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


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def cpu_cull(V32, views, dil):
    """the projection of the contract with torch on the CPU (fp64), view by view"""
    v = torch.from_numpy(V32).double()
    keep = torch.ones(len(V32), dtype=torch.bool)
    for (m, W, H, _), d in zip(views, dil):
        mt = torch.from_numpy(np.asarray(m, np.float64).reshape(3, 4))
        x, y, z = (((mt[r, 0] * v[:, 0] + mt[r, 1] * v[:, 1]) + mt[r, 2] * v[:, 2]) + mt[r, 3] for r in range(3))
        dd = z + 1e-6
        px, py = ((x / dd) / (W - 1) - 0.5) * 2, ((y / dd) / (H - 1) - 0.5) * 2
        valid = (px > -1) & (px < 1) & (py > -1) & (py < 1)
        ix = torch.round((px + 1) / 2 * (W - 1)).clamp(0, W - 1).nan_to_num(0).long()
        iy = torch.round((py + 1) / 2 * (H - 1)).clamp(0, H - 1).nan_to_num(0).long()
        keep &= ~valid | torch.from_numpy(d)[iy, ix]
    return keep.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cull_timing.md"))
    ap.add_argument("--vertices", type=float, default=5e6)
    ap.add_argument("--faces", type=float, default=10e6)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    W, H = (int(v) for v in args.size.split("x"))
    nv, nf = int(args.vertices), int(args.faces)
    rng = np.random.default_rng(3)
    V32 = rng.uniform(-1.2, 1.2, (nv, 3)).astype(np.float32)
    V32 = V32[np.argsort(V32[:, 0], kind="stable")]
    F = np.minimum(rng.integers(0, nv, (nf, 1)) + rng.integers(0, 40, (nf, 3)), nv - 1).astype(np.int32)
    views = K.ring_views(args.views, ((W, H),), 9)
    masks_d = [torch.from_numpy(v[3]).to(dev) for v in views]
    words = H * M.mask_row_words(W)
    buf = torch.empty(len(views) * words, dtype=torch.int64, device=dev)

    def dilate_all():
        return [M.dilate_mask(m, 6, out=buf[i * words:(i + 1) * words]) for i, m in enumerate(masks_d)]
    t_dil, packed = timed(dilate_all, args.repeat)
    vd, fd = torch.from_numpy(V32).to(dev), torch.from_numpy(F).to(dev)
    dviews = [(v[0], W, H, p) for v, p in zip(views, packed)]
    t_cull, keep = timed(lambda: M.cull_vertices(vd, dviews), args.repeat)
    v64 = vd.double()
    t_comp, out = timed(lambda: M.compact_mesh(keep, fd, [v64]), args.repeat)
    st = M.last_stats()
    M.lib.gof_profile_enable(1)
    dilate_all()
    M.compact_mesh(M.cull_vertices(vd, dviews), fd, [v64])
    torch.cuda.synchronize()
    rep = C.create_string_buffer(1 << 16)
    M.lib.gof_profile_report(rep, len(rep))
    M.lib.gof_profile_enable(0)
    lines = ["# Mesh culling: first measured times", "",
             "Written by `tests/devtools/dev_mesh_cull_timing.py` on %s (%s), torch %s; CPU side: %d threads."
             % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d"), torch.__version__, torch.get_num_threads()),
             "Workload: %.1f M vertices, %.1f M faces, %d views of %d x %d, disk radius 6; %d vertices and %d faces survive."
             % (nv / 1e6, nf / 1e6, len(views), W, H, st["compact"]["kept_vertices"], st["compact"]["kept_faces"]),
             "Device times: HIP events around each call, median of %d after one warm-up; allocations and the calls' own read-backs included." % args.repeat,
             "CPU times: one run, wall clock: SciPy `binary_dilation` with the disk as structure, the contract's projection with torch (fp64) view by view, numpy indexing.", ""]
    cpu = {}
    if not args.no_cpu:
        cpu["dilate"], dil = wall(lambda: [R.dilate(v[3], 6) for v in views])
        cpu["cull"], keep_cpu = wall(lambda: cpu_cull(V32, views, dil))
        cpu["compact"], _ = wall(lambda: R.compact(keep_cpu, F, attrs=(V32.astype(np.float64),)))
        lines.append("The CPU route's keep mask equals the device's: %s." % bool(np.array_equal(keep_cpu, keep.cpu().numpy())))
        lines.append("")

    def c(k):
        return "%.0f" % cpu[k] if k in cpu else "not run"
    lines += ["| stage | MI355X ms | CPU ms |", "|---|---|---|",
              "| dilate_mask, %d masks | %.2f | %s |" % (len(views), t_dil, c("dilate")),
              "| cull_vertices, one launch over all views | %.2f | %s |" % (t_cull, c("cull")),
              "| compact_mesh (+ gather of the fp64 vertices) | %.2f | %s |" % (t_comp, c("compact")), "",
              "Workspace: %d B (culling), %.1f B per vertex + face (compaction); packed masks %.1f MB."
              % (st["cull"]["workspace_bytes"], st["compact"]["workspace_bytes"] / (nv + nf), len(views) * words * 8 / 1e6), "",
              "Per entry point over one pass of the three stages (the library's own event timers):", "", "```", rep.value.decode(errors="replace").strip(), "```", ""]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
