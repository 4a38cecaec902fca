#!/usr/bin/env python3
"""Timing of the Delaunay tetrahedralization (csrc/delaunay.hip): wall time (host clock around a device synchronise), rounds,
exact-path fraction, cells per point and peak device bytes, for 1 M uniform points and the tetra points (9 per Gaussian) of
1 M / 5 M-Gaussian synthetic scenes; SciPy's Qhull on the 1 M input for comparison.  The 45 M-point run is checked for
orientation, face pairing and Euler characteristic on the device.

    python tests/devtools/dev_delaunay_timing.py [--cases uniform_1m,tetra_1m,tetra_5m] [--scipy] [--check] [--json rows.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof -o dt -- python tests/devtools/dev_delaunay_timing.py --cases uniform_1m
    python tests/devtools/dev_delaunay_timing.py --cases "" --merge rows1.json rows2.json --kernel-stats prof/.../dt_kernel_stats.csv \
        --out profiles/delaunay_timing.md

Each case can run in a process of its own (--json), and --out writes the markdown table of every row measured or merged, with the
per-kernel split of a separate rocprofv3 run (--kernel-stats).
"""
import csv
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-opacity-fields_amd"))
import delaunay  # noqa: E402
import synthetic_scenes as S  # noqa: E402


def points(name):
    if name == "uniform_1m":
        return np.random.default_rng(1).random((1_000_000, 3)).astype(np.float32)
    g = {"tetra_1m": 1_000_000, "tetra_5m": 5_000_000}[name]
    return S.tetra_points(S.scene_frustum(g, seed=5))


def device_check(P, T):
    """orientation (fp64; the bound-undecided count is reported), face pairing, Euler characteristic"""
    X = P.double()
    M = T.shape[0]
    und = bad = 0
    for s in range(0, M, 1 << 24):
        t = T[s:s + (1 << 24)].long()
        A = X[t[:, 0]]
        u, v, w = X[t[:, 1]] - A, X[t[:, 2]] - A, X[t[:, 3]] - A
        c = torch.cross(v, w, dim=1)
        det = (u * c).sum(1)
        av, aw = v.abs(), w.abs()
        cperm = torch.stack([av[:, 1] * aw[:, 2] + av[:, 2] * aw[:, 1], av[:, 2] * aw[:, 0] + av[:, 0] * aw[:, 2],
                             av[:, 0] * aw[:, 1] + av[:, 1] * aw[:, 0]], 1)
        perm = (u.abs() * cperm).sum(1)
        ok = det.abs() > 1e-10 * perm
        und += int((~ok).sum())
        bad += int(((det <= 0) & ok).sum())
    n = P.shape[0] + 1
    T = T.long()
    F = torch.sort(T[:, [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]].reshape(-1, 3), dim=1).values
    _, fc = torch.unique(torch.stack([F[:, 0] * n + F[:, 1], F[:, 2]], 1), dim=0, return_counts=True)
    del F
    E = torch.sort(T[:, [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]].reshape(-1, 2), dim=1).values
    nE = torch.unique(E[:, 0] * n + E[:, 1]).numel()
    del E
    nV = torch.unique(T).numel()
    return dict(negative=bad, undecided=und, max_face_use=int(fc.max()), euler=int(nV - nE + fc.numel() - M))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="uniform_1m,tetra_1m,tetra_5m")
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--merge", nargs="*", default=[], help="JSON rows of earlier runs to include in --out")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a separate run")
    ap.add_argument("--out", default=None, help="markdown report")
    args = ap.parse_args()
    rows = []
    for f in args.merge:
        rows += json.load(open(f))
    for name in [c for c in args.cases.split(",") if c]:
        P = points(name)
        Pd = torch.from_numpy(P).cuda()
        delaunay.triangulate(Pd[:20000])            # warm-up (module load, first launches)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        T = delaunay.triangulate(Pd)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = delaunay.last_stats()
        peak = torch.cuda.max_memory_allocated() - base
        r = dict(case=name, points=len(P), seconds=round(dt, 3), cells_per_point=round(T.shape[0] / len(P), 3),
                 peak_bytes=int(peak), bytes_per_point=round(peak / len(P), 1), **{k: int(v) for k, v in st.items()})
        if args.check:
            r.update(device_check(Pd, T))
        print(json.dumps(r), flush=True)
        rows.append(r)
        del T
        if args.scipy and name == "uniform_1m":
            from scipy.spatial import Delaunay
            t0 = time.perf_counter()
            Dl = Delaunay(P.astype(np.float64))
            r2 = dict(case="scipy_" + name, seconds=round(time.perf_counter() - t0, 3), cells=int(len(Dl.simplices)))
            print(json.dumps(r2), flush=True)
            rows.append(r2)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if args.out:
        write_report(args.out, rows, args.kernel_stats)


def write_report(path, rows, kernel_stats):
    L = ["# Delaunay tetrahedralization timing (csrc/delaunay.hip)", "",
         "`tests/devtools/dev_delaunay_timing.py` on one MI355X. Wall time: a host clock around a device synchronise, after a 20 k-point "
         "warm-up call. Peak bytes: `torch.cuda.max_memory_allocated` above what was allocated before the call (workspace and output). "
         "Exact fraction: exact predicate evaluations per cell. `check`: orientation in fp64 on the device (bound-undecided cells "
         "counted), face use, Euler characteristic V - E + F - T. SciPy: `scipy.spatial.Delaunay` (Qhull, single-threaded) on the "
         "same points in float64, in the same run.", "",
         "| input | points | wall time s | rounds | exact evaluations | exact / cell | slow-path insertions | cells / point | peak bytes / point | check |",
         "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["case"].startswith("scipy_"):
            L.append("| %s (SciPy) | | %.2f | | | | | %.3f | | |" % (r["case"][6:], r["seconds"], r["cells"] / 1e6 if "uniform_1m" in r["case"] else 0))
            continue
        chk = ""
        if "euler" in r:
            chk = "negative %d, undecided %d, max face use %d, Euler %d" % (r["negative"], r["undecided"], r["max_face_use"], r["euler"])
        L.append("| %s | %d | %.2f | %d | %d | %.2e | %d | %.3f | %.0f | %s |" % (
            r["case"], r["points"], r["seconds"], r["rounds"], r["exact_evaluations"], r["exact_evaluations"] / max(1, r["cells"]),
            r["slow_insertions"], r["cells_per_point"], r["bytes_per_point"], chk))
    if kernel_stats:
        L += ["", "Per-kernel split (rocprofv3 --kernel-trace --stats, a run of its own on the 1 M uniform input, warm-up included):", "",
              "| kernel | calls | total ms | share |", "|---|---|---|---|"]
        with open(kernel_stats) as f:
            st = list(csv.DictReader(f))
        tot = sum(float(x["TotalDurationNs"]) for x in st)
        for x in sorted(st, key=lambda x: -float(x["TotalDurationNs"]))[:16]:
            L.append("| `%s` | %s | %.1f | %.1f %% |" % (x["Name"].split("(")[0], x["Calls"], float(x["TotalDurationNs"]) / 1e6,
                                                        100 * float(x["TotalDurationNs"]) / tot))
        L.append("| all kernels | | %.1f | |" % (tot / 1e6))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
