#!/usr/bin/env python3
"""Times model_io.save_ply / load_ply on the device at 1 M and 6 M Gaussians of SH degree 3 (a record, not a gate), the
parts of a save on their own (the pack kernel, the pinned device-to-host copy, the file write) and, beside them, a numpy restatement of
the reference's host path (scene/gaussian_model.py:390-408: eight .cpu() copies, np.concatenate, list(map(tuple, ...)) into the
structured array; the write of the array is timed with it).  Reads nothing of the reference.

    python tests/devtools/dev_model_io_timing.py [--sizes 1000000,6000000] [--out profiles/model_io_timing.md] [--limit 900]

Every figure is the median of `--repeats` timed runs after `--warmup` untimed ones, with the spread (min .. max) beside it; the kernel
is timed with events on its stream, everything that touches the host with a wall clock between synchronisations.  The restatement is run
once on at most `--restate-rows` rows and scaled linearly where the model is larger (said so in the table).  The script ends itself
after --limit seconds."""
import argparse
import os
import signal
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gaussian-opacity-fields_amd"))
HBM_PEAK_GBS = 8000.0           # MI355X: 8 TB/s HBM3E


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def fmt(t):
    return "%.1f (%.1f .. %.1f)" % tuple(1e3 * v for v in t)


class Model:
    max_sh_degree, active_sh_degree = 3, 0


def make_model(P, torch):
    g = torch.Generator(device="cuda").manual_seed(P)
    m = Model()

    def rnd(*shape):
        return torch.randn(shape, generator=g, device="cuda", dtype=torch.float32)
    m._xyz, m._features_dc, m._features_rest = rnd(P, 3) * 3, rnd(P, 1, 3), rnd(P, 15, 3) * 0.2
    m._opacity, m._scaling, m._rotation = rnd(P, 1) * 3, torch.log(torch.rand((P, 3), generator=g, device="cuda") * 0.045 + 0.005), rnd(P, 4)
    m.filter_3D = torch.rand((P, 1), generator=g, device="cuda") * 0.045 + 0.005
    return m


def wall(fn, torch, warmup, repeats):
    out = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(time.perf_counter() - t0)
    return stats(out)


def restatement(m, path, rows):
    """the reference's save_ply in numpy, on the first `rows` Gaussians -> seconds (copies + concatenate + tuples + write)"""
    t0 = time.perf_counter()
    xyz = m._xyz[:rows].detach().cpu().numpy()
    normals = np.zeros_like(xyz)
    f_dc = m._features_dc[:rows].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    f_rest = m._features_rest[:rows].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    parts = [xyz, normals, f_dc, f_rest] + [t[:rows].detach().cpu().numpy() for t in (m._opacity, m._scaling, m._rotation, m.filter_3D)]
    elements = np.empty(rows, dtype=[("c%d" % i, "f4") for i in range(63)])
    attributes = np.concatenate(parts, axis=1)
    t1 = time.perf_counter()
    elements[:] = list(map(tuple, attributes))
    t2 = time.perf_counter()
    with open(path, "wb") as fh:
        fh.write(elements.tobytes())
    t3 = time.perf_counter()
    return t1 - t0, t2 - t1, t3 - t2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,6000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_io_timing.md"))
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--restate-rows", type=int, default=1000000)
    ap.add_argument("--limit", type=int, default=900)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("dev_model_io_timing: time limit of %d s reached" % a.limit))
    signal.alarm(a.limit)
    import torch
    import model_io as MIO
    assert torch.cuda.is_available(), "needs a ROCm device"
    lines = ["# model_io timing (tests/devtools/dev_model_io_timing.py)", "",
             "Device: %s.  SH degree 3 (63 floats = 252 bytes per row), chunks of %d rows.  Milliseconds: median (min .. max) of %d runs after %d "
             "warm-up run(s).  The kernel is timed with events on its stream, the rest with a wall clock between synchronisations."
             % (torch.cuda.get_device_name(0), MIO.chunk_rows(), a.repeats, a.warmup), ""]
    tmp = a.dir or tempfile.mkdtemp(prefix="gof_model_io_")
    os.makedirs(tmp, exist_ok=True)
    for P in [int(s) for s in a.sizes.split(",")]:
        print("P = %d: building the model" % P, flush=True)
        m = make_model(P, torch)
        ts = [getattr(m, f) for f in MIO._FIELDS]
        nbytes = P * 252
        # the pack kernel alone, over the whole model, into device memory
        out = torch.empty(P * 63, dtype=torch.float32, device="cuda")
        ev = []
        for i in range(a.warmup + a.repeats + 2):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            MIO.pack_rows(ts, out=out)
            e.record()
            e.synchronize()
            if i >= a.warmup:
                ev.append(s.elapsed_time(e) * 1e-3)
        pack = stats(ev)
        rows = out.view(torch.uint8)
        dests = [torch.empty_like(t) for t in ts]
        ev = []
        for i in range(a.warmup + a.repeats + 2):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            MIO.unpack_rows(rows, 252, [(4 * c, 0) for c in list(range(3)) + list(range(6, 63))], dests)
            e.record()
            e.synchronize()
            if i >= a.warmup:
                ev.append(s.elapsed_time(e) * 1e-3)
        unpack = stats(ev)
        assert all(torch.equal(d, t) for d, t in zip(dests, ts))
        del dests
        print("  pack %s ms, unpack %s ms" % (fmt(pack), fmt(unpack)), flush=True)
        # one chunk's pinned copy and file write
        n = min(MIO.chunk_rows(), P) * 63
        host = torch.empty(n, dtype=torch.float32, pin_memory=True)
        d2h = wall(lambda: host.copy_(out[:n], non_blocking=True), torch, a.warmup, a.repeats)
        path = os.path.join(tmp, "chunk.bin")

        def write_chunk():
            with open(path, "wb") as fh:
                fh.write(host.numpy())
        wr = wall(write_chunk, torch, a.warmup, a.repeats)
        del out, rows
        chunk_gb = n * 4 / 1e9
        print("  chunk of %.1f MB: D2H %s ms, write %s ms" % (chunk_gb * 1e3, fmt(d2h), fmt(wr)), flush=True)
        ply = os.path.join(tmp, "point_cloud.ply")
        save = wall(lambda: MIO.save_ply(m, ply), torch, a.warmup, a.repeats)
        print("  save_ply %s ms" % fmt(save), flush=True)
        h = Model()
        load = wall(lambda: MIO.load_ply(h, ply), torch, a.warmup, a.repeats)
        assert all(torch.equal(getattr(h, f).detach(), getattr(m, f)) for f in MIO._FIELDS)
        print("  load_ply %s ms" % fmt(load), flush=True)
        fused = wall(lambda: MIO.save_fused_ply(m, ply), torch, a.warmup, a.repeats)
        r = min(P, a.restate_rows)
        print("  the reference's host path restated in numpy, on %d rows" % r, flush=True)
        rs = restatement(m, os.path.join(tmp, "restated.bin"), r)
        scale = P / r
        lines += ["## P = %d (%.2f GB file)" % (P, nbytes / 1e9), "", "| step | ms | rate |", "|---|---|---|",
                  "| `gof_model_pack`, whole model, device to device | %s | %.0f GB/s read + written (%.0f %% of the %.0f GB/s HBM peak) |"
                  % (fmt(pack), 2 * nbytes / pack[0] / 1e9, 100 * 2 * nbytes / pack[0] / 1e9 / HBM_PEAK_GBS, HBM_PEAK_GBS),
                  "| `gof_model_unpack`, whole model, device to device | %s | %.0f GB/s read + written |" % (fmt(unpack), 2 * nbytes / unpack[0] / 1e9),
                  "| pinned device-to-host copy of one chunk (%.1f MB) | %s | %.1f GB/s |" % (chunk_gb * 1e3, fmt(d2h), chunk_gb / d2h[0]),
                  "| file write of one chunk | %s | %.1f GB/s |" % (fmt(wr), chunk_gb / wr[0]),
                  "| `save_ply` (header, %d chunks, pack + copy overlapped with the write) | %s | %.2f GB/s |"
                  % (MIO.last_stats()["save"]["chunks"], fmt(save), nbytes / save[0] / 1e9),
                  "| `save_fused_ply` | %s | |" % fmt(fused),
                  "| `load_ply` (read, copy, unpack) | %s | %.2f GB/s |" % (fmt(load), nbytes / load[0] / 1e9),
                  "| reference's host path restated in numpy: copies + concatenate / tuples into the structured array / write; ONE run on %d rows%s | %.0f / %.0f / %.0f, sum %.0f | |"
                  % (r, "" if r == P else ", SCALED by %.1f to this size" % scale, 1e3 * rs[0] * scale, 1e3 * rs[1] * scale, 1e3 * rs[2] * scale, 1e3 * sum(rs) * scale),
                  "", "save_ply against the restated host path: %.0fx." % (sum(rs) * scale / save[0]), ""]
        del m, h, host
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    signal.alarm(0)


if __name__ == "__main__":
    main()
