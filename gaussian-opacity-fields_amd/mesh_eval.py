"""DTU Chamfer evaluation on the GPU: the reference's dtu_eval/eval.py without Open3D and scikit-learn.

    points = sample_mesh(vertices, triangles, thresh)      # eval.py:50-71   (vertices first, then the lattice samples)
    keep = thin(points, r)                                   # eval.py:86-94   (greedy radius thinning in the given order)
    dist, index = nearest(query, ref)                        # eval.py:119-134 (exact nearest neighbour, fp64)
    result = dtu_chamfer(data, obs_mask, bb, res, plane, stl, mode="mesh")
    python -m mesh_eval --data mesh.ply --scan 24 --dataset_dir <DTU> --vis_out_dir <out>     # eval.py's command line + --seed

The kernels are ``gof_cloud_*`` of libgof_hip.so (csrc/cloud.hip, include/gof_cloud_hip.h); the contract is DESIGN.md §3.8: fp64
[N,3] tensors on a ROCm device in and out, results bit-equal to numpy's.  There is no host fallback: host tensors are refused.
One stated deviation: eval.py shuffles the cloud with an unseeded generator; here the permutation comes from
``numpy.random.default_rng(seed)`` and a run is bit-reproducible.
"""
import contextlib
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["sample_mesh", "thin", "nearest", "last_stats", "dtu_chamfer", "read_ply", "read_ply_elements", "write_vis_ply", "main"]

lib = B.lib
_vp, _sz, _i64, _f64 = C.c_void_p, C.c_size_t, C.c_int64, C.c_double
_P64 = C.POINTER(C.c_int64)
gn.bind(lib, {_name: [_i64] for _name in ("gof_cloud_sample_ws_bytes", "gof_cloud_thin_ws_bytes", "gof_cloud_nn_index_bytes", "gof_cloud_nn_query_ws_bytes")}, {
        "gof_cloud_sample_count": [_i64, _vp, _i64, _vp, _f64, _vp, _sz, _P64, _vp],
        "gof_cloud_sample_emit": [_i64, _vp, _i64, _vp, _f64, _vp, _sz, _i64, _vp, _vp],
        "gof_cloud_thin": [_i64, _vp, _f64, _vp, _vp, _sz, _P64, _vp],
        "gof_cloud_thin_stats": [_vp, _vp, _vp],
        "gof_cloud_nn_build": [_i64, _vp, _vp, _sz, _vp],
        "gof_cloud_nn_query": [_i64, _vp, _sz, _i64, _vp, _vp, _vp, _vp, _sz, _vp],
        "gof_cloud_nn_stats": [_vp, _vp, _vp]})

_last = {}


def last_stats():
    """Statistics of the last sample_mesh / thin / nearest calls (one sub-dictionary each): counts, rounds, distance evaluations,
    boxes visited, workspace bytes."""
    return {k: dict(v) for k, v in _last.items()}


# the device seams, by the names the host tests replace per module (tests/test_mesh_eval_host.py); one definition each: gof_native
# (tsdf_fusion and delaunay bind them the same way)
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr
_device = functools.partial(gn.current_device, "mesh_eval")


def _cloud(t, who, what="points", dtype=torch.float64):
    return gn.rows(t, who, what, dtype, on_device=_on_device)


def sample_mesh(vertices, triangles, thresh):
    """eval.py:50-71: the mesh's vertices followed by the lattice samples of every triangle of non-zero area, in triangle order.
    vertices (NV,3) float64, triangles (NT,3) int32, on a ROCm device -> (NV + samples, 3) float64 there."""
    v = _cloud(vertices, "sample_mesh", "vertices")
    t = _cloud(triangles, "sample_mesh", "triangles", torch.int32)
    if t.device != v.device:
        raise RuntimeError("sample_mesh: vertices and triangles are on different devices")
    nv, nt = int(v.size(0)), int(t.size(0))
    with _device_of(v):
        nb = lib.gof_cloud_sample_ws_bytes(nt)
        ws = torch.empty(nb, dtype=torch.uint8, device=v.device)
        m = C.c_int64()
        B._check(lib.gof_cloud_sample_count(nv, _ptr(v), nt, _ptr(t), float(thresh), ws.data_ptr(), nb, C.byref(m), _stream()))
        out = torch.empty((nv + m.value, 3), dtype=torch.float64, device=v.device)
        out[:nv] = v
        B._check(lib.gof_cloud_sample_emit(nv, _ptr(v), nt, _ptr(t), float(thresh), ws.data_ptr(), nb, m.value,
                                           out[nv:].data_ptr() if m.value else None, _stream()))
    _last["sample"] = {"vertices": nv, "triangles": nt, "samples": int(m.value), "workspace_bytes": int(nb)}
    return out


def thin(points, r):
    """eval.py:86-94: keep[i] iff no kept j < i lies within r of point i -> (N,) bool on points.device"""
    p = _cloud(points, "thin")
    n = int(p.size(0))
    with _device_of(p):
        nb = lib.gof_cloud_thin_ws_bytes(n)
        ws = torch.empty(nb, dtype=torch.uint8, device=p.device)
        keep = torch.empty(n, dtype=torch.uint8, device=p.device)
        kept = C.c_int64()
        B._check(lib.gof_cloud_thin(n, _ptr(p), float(r), _ptr(keep), ws.data_ptr(), nb, C.byref(kept), _stream()))
        st = (C.c_int64 * 4)()
        B._check(lib.gof_cloud_thin_stats(ws.data_ptr(), st, _stream()))
    _last["thin"] = {"points": n, "kept": int(kept.value), "rounds": int(st[0]), "distance_evaluations": int(st[1]), "read_backs": int(st[2]),
                     "range_searches": int(st[3]), "workspace_bytes": int(nb)}
    return keep.bool()


def nearest(query, ref):
    """eval.py:119-120, 132-133: for every query point the distance to the nearest point of `ref` and its index (the smallest on a
    tie) -> ((NQ,) float64, (NQ,) int64).  An empty `ref` gives +inf and -1."""
    q = _cloud(query, "nearest", "query")
    s = _cloud(ref, "nearest", "ref")
    if q.device != s.device:
        raise RuntimeError("nearest: query and ref are on different devices")
    nq, ns = int(q.size(0)), int(s.size(0))
    with _device_of(q):
        ib = lib.gof_cloud_nn_index_bytes(ns)
        index = torch.empty(ib, dtype=torch.uint8, device=q.device)
        B._check(lib.gof_cloud_nn_build(ns, _ptr(s), index.data_ptr(), ib, _stream()))
        nb = lib.gof_cloud_nn_query_ws_bytes(nq)
        ws = torch.empty(nb, dtype=torch.uint8, device=q.device)
        dist = torch.empty(nq, dtype=torch.float64, device=q.device)
        idx = torch.empty(nq, dtype=torch.int32, device=q.device)
        B._check(lib.gof_cloud_nn_query(ns, index.data_ptr(), ib, nq, _ptr(q), _ptr(dist), _ptr(idx), ws.data_ptr(), nb, _stream()))
        st = (C.c_int64 * 4)()
        B._check(lib.gof_cloud_nn_stats(ws.data_ptr(), st, _stream()))
    _last["nearest"] = {"queries": nq, "ref": ns, "boxes_scanned": int(st[0]), "boxes_staged": int(st[1]), "distance_evaluations": int(st[2]),
                        "boxes_per_query": (int(st[0]) / nq if nq else 0.0), "index_bytes": int(ib), "workspace_bytes": int(nb)}
    return dist, idx.long()


def dtu_chamfer(data, obs_mask, bb, res, plane, stl, *, mode="mesh", downsample_density=0.2, patch_size=60, max_dist=20, seed=0):
    """eval.py:43-134, 157 between the file reads and the three numbers, on the device.

    data: (vertices (NV,3) float64, triangles (NT,3) int32) in "mesh" mode, points (N,3) float64 in "pcd" mode; obs_mask (X,Y,Z);
    bb (2,3); res scalar; plane (4,); stl (S,3) float64 -- all on one ROCm device.  Returns mean_d2s, mean_s2d, overall (floats) and
    the tensors the visualisation needs: data_down, dist_d2s + idx_d2s + d2s_index (rows of data_down that were measured),
    dist_s2d + idx_s2d + s2d_index (rows of stl above the ground plane)."""
    thresh = float(downsample_density)
    if mode == "mesh":
        vertices, triangles = data
        pcd = sample_mesh(vertices, triangles, thresh)
    elif mode == "pcd":
        pcd = _cloud(data, "dtu_chamfer", "data")
    else:
        raise ValueError("dtu_chamfer: mode must be 'mesh' or 'pcd'")
    stl = _cloud(stl, "dtu_chamfer", "stl")
    dev = pcd.device
    # eval.py:81-82 (the stated deviation: seeded)
    perm = torch.from_numpy(np.random.default_rng(seed).permutation(int(pcd.size(0)))).to(dev)
    pcd = pcd[perm]
    data_down = pcd[thin(pcd, thresh)]
    # eval.py:99-110: BB is rounded to float32 and the patch is added in float32
    bb32 = torch.as_tensor(bb, device=dev).to(torch.float32).reshape(2, 3)
    lo = (bb32[:1] - float(patch_size)).double()
    hi = (bb32[1:] + float(patch_size) * 2).double()
    inbound = ((data_down >= lo) & (data_down < hi)).sum(dim=-1) == 3
    data_in = data_down[inbound]
    obs = torch.as_tensor(obs_mask, device=dev)
    grid = torch.round((data_in - bb32[:1].double()) / float(res)).to(torch.int32)         # np.around: round half to even
    shape = torch.tensor(list(obs.shape), dtype=torch.int32, device=dev).reshape(1, 3)
    grid_inbound = ((grid >= 0) & (grid < shape)).sum(dim=-1) == 3
    g = grid[grid_inbound].long()
    in_obs = obs[g[:, 0], g[:, 1], g[:, 2]].bool()
    d2s_index = torch.nonzero(inbound).reshape(-1)[grid_inbound][in_obs]
    data_in_obs = data_in[grid_inbound][in_obs]
    dist_d2s, idx_d2s = nearest(data_in_obs, stl)
    mean_d2s = dist_d2s[dist_d2s < max_dist].mean().item()
    # eval.py:126-130: ((x a + y b) + z c) + d
    P = torch.as_tensor(plane, device=dev).double().reshape(4)
    above = ((stl[:, 0] * P[0] + stl[:, 1] * P[1]) + stl[:, 2] * P[2]) + P[3] > 0
    s2d_index = torch.nonzero(above).reshape(-1)
    dist_s2d, idx_s2d = nearest(stl[above], data_in)
    mean_s2d = dist_s2d[dist_s2d < max_dist].mean().item()
    return {"mean_d2s": mean_d2s, "mean_s2d": mean_s2d, "overall": (mean_d2s + mean_s2d) / 2,
            "data_down": data_down, "dist_d2s": dist_d2s, "idx_d2s": idx_d2s, "d2s_index": d2s_index,
            "dist_s2d": dist_s2d, "idx_s2d": idx_s2d, "s2d_index": s2d_index}


# ---- files --------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_elements(path):
    """The parser behind read_ply (and mesh_cull.load): -> {element name: numpy record array}, one field per property; the list
    property of a face element becomes the fields "_n" (the counts) and "_i" ((M,3) indices: faces must be triangles)."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    body = raw.find(b"\n", end) + 1
    fmt, elements = None, []
    for line in raw[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property":
            elements[-1][2].append((w[-1], w[1:-1]))
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError("%s: PLY format %r is not supported (binary_little_endian, ascii)" % (path, fmt))
    tokens = raw[body:].split() if fmt == "ascii" else None
    pos = 0 if fmt == "ascii" else body
    out = {}
    for name, count, props in elements:
        lists = [p for p in props if p[1][0] == "list"]
        fields = []
        for pname, ptype in props:
            if ptype[0] == "list":
                if name != "face" or len(lists) != 1:
                    raise ValueError("%s: list property %r outside a face element" % (path, pname))
                fields.append(("_n", "<" + _PLY_TYPES[ptype[1]]))
                fields.append(("_i", "<" + _PLY_TYPES[ptype[2]], (3,)))
            else:
                fields.append((pname, "<" + _PLY_TYPES[ptype[0]]))
        dt = np.dtype(fields)
        width = sum(3 if f[0] == "_i" else 1 for f in fields)
        if fmt == "ascii":
            if name == "face" and count and tokens[pos] != b"3":
                raise ValueError("%s: only triangles are supported" % path)
            flat = np.array(tokens[pos:pos + count * width], dtype=np.float64).reshape(count, width)
            pos += count * width
            rec = np.zeros(count, dt)
            col = 0
            for f in fields:
                k = 3 if f[0] == "_i" else 1
                rec[f[0]] = flat[:, col:col + k].reshape((count, 3) if k == 3 else (count,))
                col += k
        else:
            rec = np.frombuffer(raw, dtype=dt, count=count, offset=pos)
            pos += count * dt.itemsize
        if name == "face" and lists and count and not (rec["_n"] == 3).all():
            raise ValueError("%s: only triangles are supported" % path)
        out[name] = rec
    if "vertex" not in out:
        raise ValueError("%s: no vertex element" % path)
    return out


def read_ply(path):
    """A small PLY reader (binary little-endian and ASCII): -> (vertices (N,3) float64, triangles (M,3) int32 or None).  float / double
    coordinates; other vertex properties (colours, normals) are skipped; faces must be triangles."""
    el = read_ply_elements(path)
    rec = el["vertex"]
    vertices = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1).astype(np.float64)
    triangles = None
    if "face" in el and "_i" in (el["face"].dtype.names or ()):
        triangles = np.ascontiguousarray(el["face"]["_i"].astype(np.int32)).reshape(-1, 3)
    return np.ascontiguousarray(vertices), triangles


def write_vis_ply(path, points, colors):
    """The coloured point cloud of eval.py:21-25 as binary little-endian PLY: x y z (double), red green blue (uchar = colour * 255,
    truncated).  (tsdf_fusion.write_ply writes float vertices with normals and faces: a mesh, not this cloud.)"""
    p = np.ascontiguousarray(torch.as_tensor(points).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3)
    c = np.asarray(torch.as_tensor(colors).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 3)
    rec = np.empty(len(p), dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for i, k in enumerate("xyz"):
        rec[k] = p[:, i]
    for i, k in enumerate(("red", "green", "blue")):
        rec[k] = np.clip(c[:, i] * 255.0, 0.0, 255.0).astype(np.uint8)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(p))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def _vis_colors(n, index, dist, vis_dist, max_dist, device):
    """eval.py:139-151: blue where nothing was measured, white -> red with the distance, green beyond max_dist"""
    color = torch.zeros((n, 3), dtype=torch.float64, device=device)
    color[:, 2] = 1.0
    alpha = (dist.clamp(max=vis_dist) / vis_dist).reshape(-1, 1)
    R = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64, device=device)
    W = torch.ones((1, 3), dtype=torch.float64, device=device)
    color[index] = R * alpha + W * (1 - alpha)
    color[index[dist >= max_dist]] = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device=device)
    return color


def main(argv=None):
    """eval.py's command line (same argument names and defaults) plus --seed; prints the three numbers, writes results.json and the
    two visualisation clouds into --vis_out_dir.  Returns the result dictionary of dtu_chamfer."""
    import argparse
    from scipy.io import loadmat
    parser = argparse.ArgumentParser(prog="mesh_eval")
    parser.add_argument("--data", type=str, default="data_in.ply")
    parser.add_argument("--scan", type=int, default=1)
    parser.add_argument("--mode", type=str, default="mesh", choices=["mesh", "pcd"])
    parser.add_argument("--dataset_dir", type=str, default=".")
    parser.add_argument("--vis_out_dir", type=str, default=".")
    parser.add_argument("--downsample_density", type=float, default=0.2)
    parser.add_argument("--patch_size", type=float, default=60)
    parser.add_argument("--max_dist", type=float, default=20)
    parser.add_argument("--visualize_threshold", type=float, default=10)
    parser.add_argument("--seed", type=int, default=0)
    args = parser.parse_args(argv)
    dev = _device()
    vertices, triangles = read_ply(args.data)
    if args.mode == "mesh":
        if triangles is None:
            raise ValueError("%s has no faces (use --mode pcd for a point cloud)" % args.data)
        data = (torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev))
    else:
        data = torch.from_numpy(vertices).to(dev)
    obs_file = loadmat("%s/ObsMask/ObsMask%d_10.mat" % (args.dataset_dir, args.scan))
    plane = loadmat("%s/ObsMask/Plane%d.mat" % (args.dataset_dir, args.scan))["P"]
    stl_np, _ = read_ply("%s/Points/stl/stl%03d_total.ply" % (args.dataset_dir, args.scan))
    stl = torch.from_numpy(stl_np).to(dev)
    res = dtu_chamfer(data, np.ascontiguousarray(obs_file["ObsMask"]), np.asarray(obs_file["BB"]), float(np.asarray(obs_file["Res"]).reshape(-1)[0]),
                      np.asarray(plane, dtype=np.float64).reshape(-1), stl, mode=args.mode, downsample_density=args.downsample_density,
                      patch_size=args.patch_size, max_dist=args.max_dist, seed=args.seed)
    os.makedirs(args.vis_out_dir, exist_ok=True)
    down = res["data_down"]
    write_vis_ply("%s/vis_%03d_d2s.ply" % (args.vis_out_dir, args.scan), down,
                  _vis_colors(len(down), res["d2s_index"], res["dist_d2s"], args.visualize_threshold, args.max_dist, down.device))
    write_vis_ply("%s/vis_%03d_s2d.ply" % (args.vis_out_dir, args.scan), stl,
                  _vis_colors(len(stl), res["s2d_index"], res["dist_s2d"], args.visualize_threshold, args.max_dist, stl.device))
    print(res["mean_d2s"], res["mean_s2d"], res["overall"])
    with open("%s/results.json" % args.vis_out_dir, "w") as fp:
        json.dump({"mean_d2s": res["mean_d2s"], "mean_s2d": res["mean_s2d"], "overall": res["overall"]}, fp, indent=True)
    return res


if __name__ == "__main__":
    with contextlib.suppress(BrokenPipeError):
        main(sys.argv[1:])
