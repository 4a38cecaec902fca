"""Trips the backward blend's entry merging saves on a full-size workload, WITHOUT a GPU: the instrumented build of the kernels'
source (-DGOF_STATS -DGOF_BW_COUNT_LOOKAHEAD) run on the host (tests/hipemu), as dev_hipemu_structure.py does.  Per scene:
  rule (a), consecutive merge   g_bw_stats[5]:  A pairs with the NEXT visited entry of the mask word when their lanes are disjoint
                                                (greedy; what GOF_BW_MERGE=1 runs -- the build without the look-ahead flag counts the
                                                merged trips it really took in [11], and the two agree);
  rule (b), bounded look-ahead  g_bw_stats[11]: B may be any of the next three unmerged entries whose lanes are disjoint from A's
                                                and from every entry skipped on the way.
    python tests/devtools/dev_hipemu_merge_counts.py [s1m|s1m_clustered|small ...] -> profiles/backward_merge/backward_merge_counts_<scene>.json"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "hipemu"), os.path.join(ROOT, "gaussian-opacity-fields_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import emu_binding as E  # noqa: E402
from dev_hipemu_structure import SCENES  # noqa: E402


def run(which):
    sc = SCENES[which]()
    out = (C.c_ulonglong * 12)()
    rep = {"scene": which, "P": int(sc["means3D"].shape[0]), "W": sc["W"], "H": sc["H"]}
    for label, flags, tag in (("look_ahead_count_build", ("-DGOF_STATS", "-DGOF_BW_COUNT_LOOKAHEAD"), "stats_lookahead"),):
        lib = E.load(extra_flags=flags, tag=tag)
        e = E.EmuScene(sc, lib=lib)
        pc, _ = e.forward()
        lib.gof_debug_bw_stats(out, 1)
        e.backward(np.ones_like(pc))
        lib.gof_debug_bw_stats(out, 1)
        b = list(out)
        rep["R"] = e.R
        rep[label] = {"visited_wave_entries": b[0], "contributing_lane_pairs": b[2], "lanes_per_visit": b[2] / b[0],
                      "rule_a_trips_saved": b[5], "rule_a_fraction_of_visits": b[5] / b[0],
                      "rule_b_trips_saved": b[11], "rule_b_fraction_of_visits": b[11] / b[0], "rule_b_over_rule_a": b[11] / max(b[5], 1)}
    return rep


if __name__ == "__main__":
    out_dir = os.path.join(ROOT, "profiles", "backward_merge")
    os.makedirs(out_dir, exist_ok=True)
    for w in (sys.argv[1:] or ["s1m"]):
        rep = run(w)
        with open(os.path.join(out_dir, "backward_merge_counts_%s.json" % w), "w") as f:
            json.dump({"tool": "tests/devtools/dev_hipemu_merge_counts.py", "scene": rep}, f, indent=1)
        print(json.dumps(rep, indent=1), flush=True)
