#!/usr/bin/env python3
"""Times the mesh connected components (mesh_components, csrc/mesh_components.hip) with HIP events and writes
profiles/mesh_components_timing.md.

    python tests/devtools/dev_mesh_components_timing.py [--out profiles/mesh_components_timing.md] [--faces 20e6] [--floaters 1e5]

One object of nearly all faces (a triangulated grid, the faces shuffled) next to --floaters components of 1..7 faces: the shape a
marching-tetrahedra mesh has.  Per entry point on the device (median of --repeat runs after one warm-up, events around each call, so
allocation and the calls' own read-backs are inside), the library's per-entry-point split (gof_profile_*), and the same labels through
SciPy's connected_components on the CPU of the same machine, for reference.  Nothing here is asserted anywhere."""
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
import mesh_components as MC  # noqa: E402
import mesh_components_cases as K  # noqa: E402
import mesh_components_restatement as R  # noqa: E402


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


def workload(nf, floaters, seed=1):
    """a grid of quads cut into two triangles each (one component) + `floaters` strips of 1..7 faces, the faces shuffled"""
    rng = np.random.default_rng(seed)
    side = int(np.sqrt(nf / 2))
    i, j = np.meshgrid(np.arange(side, dtype=np.int64), np.arange(side, dtype=np.int64), indexing="ij")
    a = (i * (side + 1) + j).reshape(-1)
    grid = np.concatenate([np.stack([a, a + 1, a + side + 2], -1), np.stack([a, a + side + 2, a + side + 1], -1)])
    gx, gy = np.meshgrid(np.arange(side + 1.0), np.arange(side + 1.0), indexing="ij")
    verts = [np.stack([gx.reshape(-1), gy.reshape(-1), rng.uniform(-0.2, 0.2, gx.size)], -1)]
    lengths = rng.integers(1, 8, floaters)
    starts = (side + 1) ** 2 + np.concatenate([[0], np.cumsum(lengths + 2)])
    small = np.concatenate([K.strip(int(n), int(s)) for n, s in zip(lengths, starts[:-1])]) if floaters else np.zeros((0, 3), np.int32)
    verts.append(rng.uniform(-50, side + 50, (int(starts[-1]) - (side + 1) ** 2, 3)))
    F = np.concatenate([grid, small.astype(np.int64)])
    return np.concatenate(verts), F[rng.permutation(len(F))].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_components_timing.md"))
    ap.add_argument("--faces", type=float, default=20e6)
    ap.add_argument("--floaters", type=float, default=1e5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda")
    V, F = workload(int(args.faces), int(args.floaters))
    vd, fd = torch.from_numpy(V).to(dev), torch.from_numpy(F).to(dev)
    rows, comps = [], None
    for mode in K.MODES:
        t, (comp, count) = timed(lambda: MC.face_components(fd, len(V), mode), args.repeat)
        rows.append(("face_components, %s (%d components)" % (mode, int(count)), t, MC.last_stats()["components"]["workspace_bytes"]))
        if mode == "edge":
            comps = (comp, int(count))
    t, table = timed(lambda: MC.component_stats(vd, fd, comps[0], comps[1]), args.repeat)
    rows.append(("component_stats", t, MC.last_stats()["stats"]["workspace_bytes"]))
    keep = MC.select(table[0], table[2], largest=1)
    t, mask = timed(lambda: MC.component_mask(comps[0], keep), args.repeat)
    rows.append(("component_mask", t, 0))
    t, _ = timed(lambda: MC.referenced_vertices(fd, len(V), mask), args.repeat)
    rows.append(("referenced_vertices", t, 0))

    def whole():
        mesh = M.DeviceMesh.from_device(vd, fd)
        return mesh.keep_components(largest=1)
    t, counts = timed(whole, args.repeat)
    rows.append(("DeviceMesh.keep_components(largest=1), all of the above + both compactions", t, 0))
    MC.lib.gof_profile_enable(1)
    whole()
    torch.cuda.synchronize()
    rep = C.create_string_buffer(1 << 16)
    MC.lib.gof_profile_report(rep, len(rep))
    MC.lib.gof_profile_enable(0)
    lines = ["# Mesh connected components: first measured times", "",
             "Written by `tests/devtools/dev_mesh_components_timing.py` on %s (%s), torch %s; CPU side: %d threads."
             % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d"), torch.__version__, torch.get_num_threads()),
             "Workload: %.1f M faces over %.1f M vertices: one grid component and %d floaters of 1..7 faces, the faces shuffled; "
             "keep_components(largest=1) keeps %d of %d components." % (len(F) / 1e6, len(V) / 1e6, int(args.floaters), counts[0], sum(counts)),
             "Device times: HIP events around each call, median of %d after one warm-up; allocations and the calls' own read-backs included." % args.repeat, ""]
    if not args.no_cpu:
        t_cpu, lab = wall(lambda: R.scipy_labels(F, "edge"))
        same = bool(np.array_equal(R.numbering(lab)[0], comps[0].cpu().numpy()))
        lines += ["SciPy on the CPU (np.unique over the sorted edges, a sparse adjacency matrix, `connected_components`), edge mode, one run, wall "
                  "clock: %.0f ms; its labels equal the device's: %s." % (t_cpu, same), ""]
    lines += ["| entry point | MI355X ms | workspace MB |", "|---|---|---|"] + ["| %s | %.2f | %.0f |" % (n, t, w / 1e6) for n, t, w in rows]
    lines += ["", "Per entry point over one keep_components (the library's own event timers):", "", "```", rep.value.decode(errors="replace").strip(), "```", ""]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
