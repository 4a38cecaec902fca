#!/usr/bin/env python3
"""Times the DTU Chamfer evaluation (mesh_eval, csrc/cloud.hip) with HIP events and writes profiles/mesh_eval_timing.md.

    python tests/devtools/dev_mesh_eval_timing.py [--out profiles/mesh_eval_timing.md] [--sizes 5e6,30e6] [--scan 3e6] [--cpu-max 6e6]

Per size (sampled points of a torus mesh, scan of --scan points): the three stages and the whole of dtu_chamfer on the device
(median of --repeat runs after one warm-up, events around each call, so allocation and the calls' own read-backs are inside), the
library's per-entry-point split (gof_profile_*), rounds / distance evaluations / workspace bytes per point of the thinning, boxes
scanned per query of the nearest search -- and the restatement (tests/mesh_eval_restatement.py: numpy + scikit-learn's kd-tree, all
CPUs the process may use) on the same inputs, for sizes up to --cpu-max points.  Nothing here is asserted anywhere."""
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

import mesh_eval as M  # noqa: E402
import mesh_eval_restatement as R  # noqa: E402
import test_mesh_eval_host as H  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_eval_timing.md"))
    ap.add_argument("--sizes", default="5e6,30e6")
    ap.add_argument("--scan", type=float, default=3e6)
    ap.add_argument("--cpu-max", type=float, default=6e6)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda")
    V, T = H.torus(400, 200)
    rng = np.random.default_rng(8)
    ns = int(args.scan)
    u, v = rng.random(ns) * 2 * np.pi, rng.random(ns) * 2 * np.pi
    stl = np.stack([(20 + 6.05 * np.cos(v)) * np.cos(u), (20 + 6.05 * np.cos(v)) * np.sin(u), 6.05 * np.sin(v)], -1).astype(np.float32).astype(np.float64)
    bb = np.array([[-30.0, -30.0, -8.0], [30.0, 30.0, 8.0]])
    obs = np.ones((61, 61, 17), np.uint8)
    plane = np.array([0.0, 0.0, 1.0, 4.5])
    Vd, Td, stl_d = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev), torch.from_numpy(stl).to(dev)
    lines = ["# DTU Chamfer evaluation: first measured times", "",
             "Written by `tests/devtools/dev_mesh_eval_timing.py` on %s (%s), torch %s; CPU side: %d CPUs available to the run."
             % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d"), torch.__version__, __import__("joblib").cpu_count()),
             "Device times: HIP events around each call, median of %d after one warm-up; allocations and the calls' own read-backs included." % args.repeat,
             "CPU times: one run of the restatement (numpy + scikit-learn kd-tree, `n_jobs=-1`), wall clock.", ""]
    for size in [float(s) for s in args.sizes.split(",")]:
        th = 0.0232 * (8.03e6 / size) ** 0.5                   # the torus gives 8.03 M samples at 0.0232; samples scale with 1 / thresh^2
        t_sample, pts = timed(lambda: M.sample_mesh(Vd, Td, th), args.repeat)
        n = int(pts.size(0))
        perm = np.random.default_rng(0).permutation(n)
        shuffled = pts[torch.from_numpy(perm).to(dev)]
        t_thin, keep = timed(lambda: M.thin(shuffled, th), args.repeat)
        st_thin = M.last_stats()["thin"]
        down = shuffled[keep]
        t_d2s, _ = timed(lambda: M.nearest(down, stl_d), args.repeat)
        st_d2s = M.last_stats()["nearest"]
        t_s2d, _ = timed(lambda: M.nearest(stl_d, down), args.repeat)
        st_s2d = M.last_stats()["nearest"]
        M.lib.gof_profile_enable(1)
        t_all, res = timed(lambda: M.dtu_chamfer((Vd, Td), obs, bb, 1.0, plane, stl_d, downsample_density=th, seed=0), 1)
        import ctypes as C
        rep = C.create_string_buffer(1 << 16)
        M.lib.gof_profile_report(rep, len(rep))
        M.lib.gof_profile_enable(0)
        lines += ["## %.1f M sampled points (thresh = r = %.5f), scan of %.1f M" % (n / 1e6, th, ns / 1e6), "",
                  "| stage | MI355X ms | CPU ms |", "|---|---|---|"]
        cpu = {}
        if n <= args.cpu_max:
            cpu["sample"], want = wall(lambda: R.sample_mesh(V, T, th))
            cpu["thin"], wk = wall(lambda: R.thin(want[perm], th))
            wd = want[perm][wk]
            cpu["d2s"], _ = wall(lambda: R.nearest(wd, stl))
            cpu["s2d"], _ = wall(lambda: R.nearest(stl, wd))
            cpu["all"], _ = wall(lambda: R.dtu_chamfer(want, perm, obs, bb, 1.0, plane, stl, thresh=th))
            cpu["all"] += cpu["sample"]

        def c(k):
            return "%.0f" % cpu[k] if k in cpu else "not run (above --cpu-max)"
        lines += ["| sample_mesh | %.2f | %s |" % (t_sample, c("sample")), "| thin (%d -> %d points) | %.2f | %s |" % (n, st_thin["kept"], t_thin, c("thin")),
                  "| nearest, thinned cloud -> scan | %.2f | %s |" % (t_d2s, c("d2s")), "| nearest, scan -> thinned cloud | %.2f | %s |" % (t_s2d, c("s2d")),
                  "| dtu_chamfer, whole | %.2f | %s |" % (t_all, c("all")), "",
                  "Thinning: %d rounds, %d read-backs, %.1f distance evaluations and %.1f range searches per point, workspace %.0f B per point."
                  % (st_thin["rounds"], st_thin["read_backs"], st_thin["distance_evaluations"] / n, st_thin["range_searches"] / n, st_thin["workspace_bytes"] / n),
                  "Nearest: %.2f boxes of 256 scanned per query (cloud -> scan, %.0f distance evaluations per query), %.2f (scan -> cloud, %.0f); index %.0f B per reference point."
                  % (st_d2s["boxes_per_query"], st_d2s["distance_evaluations"] / max(1, st_d2s["queries"]), st_s2d["boxes_per_query"],
                     st_s2d["distance_evaluations"] / max(1, st_s2d["queries"]), st_d2s["index_bytes"] / max(1, st_d2s["ref"])), "",
                  "Result: mean_d2s %.6f, mean_s2d %.6f, overall %.6f." % (res["mean_d2s"], res["mean_s2d"], res["overall"]), "",
                  "Per entry point inside dtu_chamfer (the library's own event timers):", "", "```", rep.value.decode(errors="replace").strip(), "```", ""]
        print("\n".join(lines[-14:]), flush=True)
        del pts, shuffled, keep, down, res
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
