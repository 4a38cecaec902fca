#!/usr/bin/env python3
"""Times the Tanks-and-Temples F-score evaluation (tnt_eval, csrc/cloud_reg.hip + cloud.hip's nearest neighbour) with HIP events and
writes profiles/tnt_eval_timing.md.

    python tests/devtools/dev_tnt_eval_timing.py [--out profiles/tnt_eval_timing.md] [--sizes 5e6,20e6] [--cpu-max 6e6]

Per size (target points of the test surface, 0.6 x as many source points): crop, voxel down-sampling, one ICP evaluation split into
transformation / nearest-neighbour query / the two sums (the library's own event timers), and run_evaluation's device sequence
(three registrations and the F-score; the file reads and the host RANSAC are not in it) -- against the restatement
(tests/tnt_eval_restatement.py: numpy + SciPy's cKDTree with 16 workers) on the same inputs for sizes up to --cpu-max.  Device
times: median of --repeat runs after one warm-up, events around each call, so allocations and the calls' own read-backs are
inside.  Nothing here is asserted anywhere."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "gaussian-opacity-fields_amd")):
    sys.path.insert(0, p)

import tnt_eval as M  # noqa: E402
import tnt_eval_restatement as R  # noqa: E402
import test_tnt_eval_host as H  # noqa: E402


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


def sequence(mod, s, t, init, vol, tau):
    T = mod.registration_vol_ds(s, t, init, vol, tau, 80 * tau)[0]
    T = mod.registration_vol_ds(s, t, T, vol, tau / 2, 20 * tau)[0]
    T = mod.registration_unif(s, t, T, vol, 2 * tau)[0]
    return mod.tnt_fscore(s, t, T, vol, tau)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tnt_eval_timing.md"))
    ap.add_argument("--sizes", default="5e6,20e6")
    ap.add_argument("--cpu-max", type=float, default=6e6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--cpu-sequence", type=int, default=1, help="0: leave the restatement's whole sequence out (about 60 kd-tree evaluations)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    tau = 0.05
    vol = H.volume_for(2)
    init = H.KNOWN @ H.similarity_matrix(1.004, 0.4, [0.5, 0.2, 1.0], [0.1, -0.08, 0.05])
    lines = ["# Tanks-and-Temples F-score evaluation: first measured times", "",
             "Written by `tests/devtools/dev_tnt_eval_timing.py` on %s (%s), torch %s." % (torch.cuda.get_device_name(0), time.strftime("%Y-%m-%d"), torch.__version__),
             "Device times: HIP events around each call, median of %d after one warm-up; allocations and the calls' own read-backs included." % args.repeat,
             "CPU times: one run of the restatement (numpy + SciPy cKDTree, %d workers), wall clock, same machine, same run." % R.WORKERS,
             "The sequence = `registration_vol_ds` (tau, 80 tau), (tau / 2, 20 tau), `registration_unif` (2 tau), `tnt_fscore` at tau = %g: what"
             " `run_evaluation` does on the device (its file reads and the host RANSAC over the camera centres are not in it)." % tau, ""]
    for size in [float(x) for x in args.sizes.split(",")]:
        nt, ns = int(size), int(0.6 * size)
        source, target = H.registration_case(nt, ns, seed=31, n_far=300)
        s_d, t_d = torch.from_numpy(source).to(dev), torch.from_numpy(target).to(dev)
        t_crop, (sc, _) = timed(lambda: M.crop(s_d, vol, init), args.repeat)
        t_crop_t, (tc, _) = timed(lambda: M.crop(t_d, vol), args.repeat)
        t_vox, (sv, _) = timed(lambda: M.voxel_down_sample(sc, tau), args.repeat)
        st_vox = M.last_stats()["voxel"]
        t_vox_t, (tv, _) = timed(lambda: M.voxel_down_sample(tc, tau), args.repeat)
        M.icp(sv, tv, 20 * tau, max_iteration=1)
        M.lib.gof_profile_enable(1)
        t_icp, (_, _, _, rec) = timed(lambda: M.icp(sv, tv, 20 * tau, max_iteration=20), 1)
        rep = C.create_string_buffer(1 << 16)
        M.lib.gof_profile_report(rep, len(rep))
        M.lib.gof_profile_enable(0)
        prof = json.loads(rep.value.decode(errors="replace"))
        t_seq, res = timed(lambda: sequence(M, s_d, t_d, init, vol, tau), 1)
        cpu = {}
        if nt <= args.cpu_max:
            cpu["crop"], (rc, _) = wall(lambda: R.crop(source, vol, init))
            cpu["vox"], (rv, _) = wall(lambda: R.voxel_down_sample(rc, tau))
            rt = R.voxel_down_sample(R.crop(target, vol)[0], tau)[0]
            cpu["eval"], _ = wall(lambda: R.icp_evaluate(rv, rt, np.eye(4), 20 * tau))
            if args.cpu_sequence:
                cpu["seq"], want = wall(lambda: sequence(R, source, target, init, vol, tau))

        def c(k):
            return "%.0f" % cpu[k] if k in cpu else "not run"

        def per(name):
            e = prof.get(name, {"calls": 0, "total_ms": 0.0})
            return e["total_ms"] / max(1, e["calls"])
        lines += ["## target %.1f M points, source %.1f M" % (nt / 1e6, ns / 1e6), "", "| stage | MI355X ms | CPU ms |", "|---|---|---|",
                  "| crop, source with transformation (%d -> %d) | %.2f | %s |" % (ns, len(sc), t_crop, c("crop")),
                  "| crop, target (%d -> %d) | %.2f | |" % (nt, len(tc), t_crop_t),
                  "| voxel_down_sample, source (%d -> %d) | %.2f | %s |" % (len(sc), len(sv), t_vox, c("vox")),
                  "| voxel_down_sample, target (%d -> %d) | %.2f | |" % (len(tc), len(tv), t_vox_t),
                  "| one ICP evaluation (transformation + query + sums; CPU: with the tree build) | %.2f | %s |" % (t_icp / len(rec), c("eval")),
                  "| icp, %d evaluations, index build included | %.2f | |" % (len(rec), t_icp),
                  "| the sequence (3 registrations + F-score) | %.2f | %s |" % (t_seq, c("seq")), "",
                  "Per call inside that ICP (the library's event timers, ms): transformation %.3f, nearest-neighbour query %.3f, sums pass 1 %.3f, sums pass 2 %.3f; index build %.2f."
                  % (per("cloud_transform"), per("cloud_nn_query"), per("cloud_icp_sums1"), per("cloud_icp_sums2"), per("cloud_nn_build")),
                  "Voxel workspace %.0f B per point.  Result: precision %.4f, recall %.4f, F-score %.4f%s." %
                  (st_vox["workspace_bytes"] / max(1, st_vox["points"]), res["precision"], res["recall"], res["fscore"],
                   (" (restatement: %.4f)" % want["fscore"]) if "seq" in cpu else ""), ""]
        print("\n".join(lines[-16:]), flush=True)
        del s_d, t_d, sc, tc, sv, tv, res
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
