#!/usr/bin/env python3
"""Times the mesh simplification (mesh_simplify, csrc/mesh_simplify.hip) with HIP events and writes profiles/mesh_simplify_timing.md.

    python tests/devtools/dev_mesh_simplify_timing.py [--out profiles/mesh_simplify_timing.md] [--faces 1e6,1e7] [--grid 256]

The workload of tests/devtools/dev_mesh_components_timing.py (one grid component and floaters, the faces shuffled) at each face count.
Per stage on the device (median, smallest and largest of --repeat runs after one warm-up, events around each call, so allocation and
the calls' own read-backs are inside): the count-only probe, cluster, cluster + solve + faces (mesh_simplify.simplify), DeviceMesh.simplify with its
compactions, the library's per-entry-point split (gof_profile_*) -- and, as the yardstick, mesh_components on the same mesh: both run
the same sorts.  Nothing here is asserted anywhere."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "gaussian-opacity-fields_amd"), HERE):
    sys.path.insert(0, p)

import mesh_cull as M  # noqa: E402
import mesh_components as MC  # noqa: E402
import mesh_simplify as MS  # noqa: E402
from dev_mesh_components_timing import workload  # noqa: E402


def timed(fn, repeat):
    """-> ((median, smallest, largest) ms over `repeat` runs after one warm-up, the last result)"""
    fn()
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return (float(np.median(ts)), float(min(ts)), float(max(ts))), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify_timing.md"))
    ap.add_argument("--faces", default="1e6,1e7")
    ap.add_argument("--grid", type=float, default=256.0)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = ["# Mesh simplification: first measured times", "",
             "Written by `tests/devtools/dev_mesh_simplify_timing.py` on %s (%s), torch %s." % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d"), torch.__version__),
             "One run of the tool in one process. Device times: HIP events around each call, one warm-up, then %d runs: their median and, in "
             "brackets, the smallest and the largest; allocations and the calls' own read-backs included." % args.repeat, ""]
    name = torch.cuda.get_device_name(0)
    for nf in (int(float(x)) for x in args.faces.split(",")):
        V, F = workload(nf, nf // 200)
        vd, fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
        h, _ = MS.choose_cell(vd, grid=args.grid)
        rows = []
        t, nc = timed(lambda: MS.count_clusters(vd, h), args.repeat)
        rows.append(("count_clusters (one probe of the target search)", t))
        t, _ = timed(lambda: MS.cluster(vd, h), args.repeat)
        rows.append(("cluster", t))
        t, _ = timed(lambda: MS.simplify(vd, fd, cell=h), args.repeat)
        rows.append(("simplify: cluster + solve + faces", t))
        st = {}

        def whole():
            st.update(M.DeviceMesh.from_device(vd, fd).simplify(cell=h))
        t, _ = timed(whole, args.repeat)
        rows.append(("DeviceMesh.simplify(cell=h): the above + both compactions", t))
        t, _ = timed(lambda: M.DeviceMesh.from_device(vd, fd).simplify(target_vertices=max(nc, 1)), args.repeat)
        rows.append(("DeviceMesh.simplify(target_vertices=%d): up to 24 probes first" % max(nc, 1), t))
        t, _ = timed(lambda: MC.components(vd, fd), args.repeat)
        rows.append(("yardstick: mesh_components.components (edge mode, labels + stats)", t))
        MS.lib.gof_profile_enable(1)
        whole()
        torch.cuda.synchronize()
        rep = C.create_string_buffer(1 << 16)
        MS.lib.gof_profile_report(rep, len(rep))
        MS.lib.gof_profile_enable(0)
        lines += ["## %.1f M faces, %.1f M vertices, grid %g (h = %.6g): %d clusters, %d -> %d faces, used_mean in %d cells"
                  % (len(F) / 1e6, len(V) / 1e6, args.grid, h, st["clusters"], st["faces_before"], st["faces_after"], st["used_mean"]), "",
                  "| stage | %s, ms |" % name, "|---|---|"] + ["| %s | %.2f (%.2f – %.2f) |" % ((n,) + t) for n, t in rows]
        lines += ["", "Per entry point over one DeviceMesh.simplify (the library's own event timers):", "", "```", rep.value.decode(errors="replace").strip(), "```", ""]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
