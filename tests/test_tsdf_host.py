"""CPU tests of the TSDF fusion (DESIGN.md "TSDF fusion"): the kernels of csrc/tsdf.hip through the host emulator (tests/hipemu)
behind tsdf_fusion.TSDFVolume itself, against the float64 restatement (tests/tsdf_restatement.py), the PLY writer, the marching-cubes
tables, and the launcher's binding of extract_mesh_tsdf.py's tsdf_fusion.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context are the host stand-ins of tests/hipemu/host_child.py, and tsdf_fusion._buffer, through which a TSDFVolume
allocates every buffer by role, applies the fill policy below."""
import ast
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import host_child  # noqa: E402
from host_child import PKG  # noqa: E402
import tsdf_restatement as T  # noqa: E402

REF_SCRIPT = "/root/reference/extract_mesh_tsdf.py"

# scene name -> (W, H, views, voxel size)
EMU_SCENES = {"plane": (64, 48, 3, 0.05), "sphere": (96, 72, 5, 0.03), "boxes": (160, 120, 4, 0.02)}
# the DTU-like shape (device test): thousands of keys per frame set
LARGE_SCENES = {"plane_large": (800, 600, 20, 0.004), "boxes_large": (800, 600, 20, 0.004)}
TAU = 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# the child: tsdf_fusion.TSDFVolume over the emulated library
# ---------------------------------------------------------------------------------------------------------------------------
# ---- what a buffer holds when the library receives it (include/gof_hip.h: "workspaces may hold anything on entry unless stated") ------
# TSDFVolume allocates the volume's arrays and both workspaces with torch.empty: recycled memory.  GOF_TSDF_FILL (read by
# the child process) is "zero" (the default), "0xA5", "0xFF" (all-ones keys, counts and cursors, NaN voxels) or "stale": every buffer
# holds what the buffer of the same role held when a LARGER volume (STALE_DONOR: more views, finer voxels, hence more blocks, a larger
# table and larger frame sets) had been fused and extracted -- cut to the new size, or extended with 0xA5
FILLS = ("zero", "0xA5", "0xFF", "stale")
STALE_DONOR = ("boxes", 0.016)          # (scene, voxel size): finer than every EMU_SCENES entry
_fill = "zero"
_left = {}             # role -> the bytes the donor volume's last buffer of that role holds
_recording = False


WRITTEN = ("block_coords", "vertices", "triangles", "colors", "normals")      # outputs the header documents as fully written


def _buf(role, shape, dtype, device):
    """tsdf_fusion._buffer on the host: a workspace or volume array under the fill policy; a fully written output as NaN / 0x7fffffff
    under a poison policy (zero otherwise)"""
    import torch
    a = torch.zeros(shape, dtype=dtype)
    if role in WRITTEN:
        return a if _fill == "zero" else a.fill_(float("nan") if a.is_floating_point() else 0x7fffffff)
    raw = a.view(torch.uint8)
    if _fill == "0xFF":
        raw[:] = 0xFF
    elif _fill != "zero":
        raw[:] = 0xA5
        if _fill == "stale" and role in _left:
            n = min(raw.numel(), _left[role].numel())
            raw[:n] = _left[role].view(torch.uint8)[:n]
    if _recording:
        _left[role] = a          # (the live tensor: what it holds when the donor is done)
    return a


def _fuse(F, views, v, block_count=4):
    """a TSDFVolume of `views` that starts small enough to grow its blocks and to redo a frame whose block set did not fit"""
    vol = F.TSDFVolume(v, block_count=block_count)
    vol._set_cap = 64
    for d, c, K, E in views:
        vol._frame_ws = None          # every frame workspace a fresh buffer under the fill policy
        vol.integrate(F.torch.from_numpy(d), F.torch.from_numpy(np.ascontiguousarray(c)), K, E)
    return vol


def scene_inputs(name, voxel=None):
    W, H, nv, v = EMU_SCENES[name] if name in EMU_SCENES else LARGE_SCENES[name]
    v = voxel or v
    K = T.intrinsic(W, H)
    views = []
    for E in T.ring_views(nv, seed=len(name)):
        d, c = T.render_scene(name.split("_")[0], K, E, H, W)
        views.append((d, c, K, E))
    return views, v


def run_emulated(name, out):
    """child process: every frame's block set (a one-frame volume each), the fused volume and its mesh -> npz"""
    global _fill, _recording
    import tsdf_fusion as F
    host_child.install_seams(F, buffers=None)
    F._buffer = _buf
    touch, redone = F.B.lib.gof_tsdf_touch, []

    def counted_touch(*args):          # (a frame redone with twice the slots: the touch returns GOF_E_CAPACITY)
        rc = touch(*args)
        redone.append(rc == -5)
        return rc
    F.B.lib.gof_tsdf_touch = counted_touch
    _fill = os.environ.get("GOF_TSDF_FILL", "zero")
    assert _fill in FILLS, _fill
    if _fill == "stale":          # the larger volume first: fused and extracted on 0xA5 buffers, which then are what it left behind
        _fill, _recording = "0xA5", True
        donor = _fuse(F, *scene_inputs(*STALE_DONOR))
        donor.extract_triangle_mesh(TAU)
        _left.update({k: a.clone() for k, a in _left.items()})
        _fill, _recording = "stale", False
    views, v = scene_inputs(name)
    res = {}
    for i, view in enumerate(views):
        res["frame%d" % i] = _fuse(F, [view], v, block_count=1).block_coords().numpy()
    vol = _fuse(F, views, v)
    assert vol.block_capacity > 4 and vol._set_cap > 64, "the scene no longer reaches the block growth and the redone frame"
    assert any(redone) or name != "boxes", "no frame of boxes (the scene whose frame sets exceed 64 slots) was redone"
    res["coords"], res["data"] = vol.block_coords().numpy(), vol.block_data().numpy().copy()
    res["V"], res["F"], res["C"], res["N"] = (t.numpy() for t in vol.extract_triangle_mesh(TAU))
    if _fill == "stale":
        assert donor.num_blocks > vol.num_blocks and donor._vol.table_capacity >= vol._vol.table_capacity, "the stale policy's donor volume is not the larger one"
    np.savez(out, **res)


def _emulate(name, tmp_path, order=None, fill="zero"):
    return host_child.run_child(__file__, name, tmp_path, order=order, env={"GOF_TSDF_FILL": fill}, tag=fill, timeout=900)


def check_against_restatement(name, res):
    views, v = scene_inputs(name)
    ref = T.Volume(v)
    amb = {}
    for i, (d, c, K, E) in enumerate(views):
        nf = set()
        fr = T.touch(d, K, E, v, near_face=nf)
        got = {tuple(b) for b in res["frame%d" % i]}
        assert len(got) == len(res["frame%d" % i]), "a frame's block set holds a block twice"
        diff = got ^ fr
        assert diff <= nf, "frame %d: blocks %s differ from the restatement away from block faces" % (i, sorted(diff - nf)[:5])
        # the update over the kernels' own frame set (equal up to near-face blocks, checked above): every block is comparable
        ref.integrate(d, c, K, E, ambiguous=amb, frame=got)
    # volume: the same blocks, every one compared, away from ambiguous voxels
    coords = {tuple(b): k for k, b in enumerate(res["coords"])}
    assert len(coords) == len(res["coords"])
    assert set(coords) == set(ref.blocks)
    # tsdf is (depth - camera z) / trunc: the float32 camera z of a voxel some metres away carries ~5e-7 m, which at a small trunc
    # exceeds 1e-5 of it (trunc = 0.032 at v = 0.004)
    tol_tsdf = max(1e-5, 1e-6 / ref.trunc)
    compared = 0
    for b, arr in ref.blocks.items():
        got = res["data"][coords[b]].astype(np.float64)
        ok = ~amb.get(b, np.zeros((16, 16, 16), bool))
        assert np.array_equal(got[1][ok], arr[1][ok]), "block %s: weights differ" % (b,)
        err = np.abs(got[0][ok] - arr[0][ok]).max()
        assert err <= tol_tsdf, "block %s: tsdf differs by %g" % (b, err)
        err = np.abs(got[2:][:, ok] - arr[2:][:, ok]).max()
        assert err <= 1e-5, "block %s: colour differs by %g" % (b, err)
        compared += int(ok.sum())
    assert compared > 0.9 * 4096 * len(coords) and compared > 50000
    # extraction: the restatement's marching cubes over the emulated volume's own values
    blocks = {tuple(b): res["data"][k].astype(np.float64) for k, b in enumerate(res["coords"])}
    V, F, Cc, N = T.extract(blocks, v, TAU)
    assert len(V) > 1000 and len(F) > 1000
    assert res["V"].shape == V.shape and res["F"].shape == F.shape
    assert np.array_equal(res["F"], F)
    # 1e-5 v, or the float32 spacing of the coordinates (2^-22 relative) where that is coarser (v = 0.004, |x| ~ 1)
    assert (np.abs(res["V"] - V) <= 1e-5 * v + 2.0 ** -22 * np.abs(V)).all(), np.abs(res["V"] - V).max() / v
    assert np.abs(res["C"] - Cc).max() <= 1e-5
    assert np.abs(res["N"] - N).max() <= 1e-4


@pytest.mark.parametrize("name", sorted(EMU_SCENES))
def test_emulated_kernels_match_restatement(name, tmp_path):
    check_against_restatement(name, _emulate(name, tmp_path))


_zero_filled = {}


@pytest.mark.parametrize("fill", FILLS[1:])
@pytest.mark.parametrize("name", sorted(EMU_SCENES))
def test_emulated_kernels_do_not_depend_on_what_their_buffers_held(name, fill, tmp_path):
    """the volume's arrays (gof_tsdf_grow's destination), the frame and the extract workspace filled with 0xA5, with 0xFF, or left over
    from a larger volume: the same comparison with the restatement, and every bit of the run on cleared buffers (blocks in key order)"""
    got = _emulate(name, tmp_path, fill=fill)
    check_against_restatement(name, got)
    if name not in _zero_filled:
        _zero_filled[name] = _emulate(name, tmp_path)
    want = _zero_filled[name]
    assert sorted(got) == sorted(want)
    for k in want:
        if k.startswith("frame"):          # (a frame's block set: its storage order is the order the allocating lanes arrived in)
            assert np.array_equal(np.sort(T.pack(got[k])), np.sort(T.pack(want[k]))), k
        elif k not in ("coords", "data"):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    kg, kw = T.pack(got["coords"]), T.pack(want["coords"])
    assert np.array_equal(np.sort(kg), np.sort(kw))
    assert got["data"][np.argsort(kg)].tobytes() == want["data"][np.argsort(kw)].tobytes()


@pytest.mark.parametrize("order", ["reverse", "random:7"])
def test_emulated_kernels_independent_of_lane_order(order, tmp_path):
    """the mesh is bit-identical, and the volume (in key order) equal, whatever order the emulator runs lanes and waves in"""
    a = _emulate("sphere", tmp_path)
    b = _emulate("sphere", tmp_path, order)
    for k in ("V", "F", "C", "N"):
        assert np.array_equal(a[k], b[k]), k
    ka, kb = T.pack(a["coords"]), T.pack(b["coords"])
    assert np.array_equal(np.sort(ka), np.sort(kb))
    assert np.array_equal(a["data"][np.argsort(ka)], b["data"][np.argsort(kb)])


# ---------------------------------------------------------------------------------------------------------------------------
# tables, PLY, restatement self-checks
# ---------------------------------------------------------------------------------------------------------------------------
def test_tables_header_is_generated():
    """csrc/tsdf_tables.h (compiled into the product) holds what gen_tsdf_tables.py constructs"""
    with open(os.path.join(PKG, "csrc", "tsdf_tables.h")) as f:
        assert f.read() == T.tables_header()


def _face_of(e0, e1):
    """the cube face both edges lie on, or None"""
    for f in T.FACES:
        fe = {frozenset((f[k], f[(k + 1) % 4])) for k in range(4)}
        if frozenset(T.EDGES[e0]) in fe and frozenset(T.EDGES[e1]) in fe:
            return f
    return None


def test_tables_close_a_surface():
    """every cube case: the used edges are the edge mask's; within the cube every triangle side is shared by exactly one other triangle
    in the opposite direction, or it lies on a cube face -- one segment per face between two crossing edges, the segments of a face
    being what the face's corner signs alone decide (so the cube on the other side of the face closes them)"""
    em, tris = T.mc_tables()
    assert em[0] == 0 and em[255] == 0 and em[1] == 0x109 and em[0x80] == 0x8C0      # Lorensen-Cline / Bourke edge table entries
    for case in range(256):
        used = set(e for t in tris[case] for e in t)
        assert used == {e for e in range(12) if (em[case] >> e) & 1}
        assert em[case] == em[255 - case]
        sides = {}
        for t in tris[case]:
            for k in range(3):
                sides[(t[k], t[(k + 1) % 3])] = sides.get((t[k], t[(k + 1) % 3]), 0) + 1
        assert all(n == 1 for n in sides.values()), case
        boundary = [(a, b) for (a, b) in sides if (b, a) not in sides]
        inside = [c for c in range(8) if (case >> c) & 1]
        per_face = {}
        for a, b in boundary:
            f = _face_of(a, b)
            assert f is not None, "case %d: side %s is inside the cube but has no twin" % (case, (a, b))
            per_face.setdefault(f, []).append(frozenset((a, b)))
        for f in T.FACES:
            cut = [k for k in range(4) if ((f[k] in inside) != (f[(k + 1) % 4] in inside))]
            assert len(per_face.get(f, [])) == len(cut) // 2, (case, f)
        # every crossing edge is an end of exactly two boundary sides (it lies on two faces)
        ends = [e for s in boundary for e in s]
        assert all(ends.count(e) == 2 for e in used), case


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode().split("\n")
    assert head[1] == "format binary_little_endian 1.0"
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    props = [l.split()[-1] for l in head if l.startswith("property ") and "list" not in l]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert "property list uchar int vertex_indices" in head
    vd = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    fd = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(data) == end + nv * vd.itemsize + nf * fd.itemsize
    v = np.frombuffer(data, vd, nv, end)
    f = np.frombuffer(data, fd, nf, end + nv * vd.itemsize)
    assert (f["n"] == 3).all()
    return v, f["i"]


def test_write_ply_round_trip(tmp_path):
    import torch
    from tsdf_fusion import write_ply
    rng = np.random.default_rng(3)
    V = rng.standard_normal((57, 3)).astype(np.float32)
    N = rng.standard_normal((57, 3)).astype(np.float32)
    Cc = rng.uniform(-0.1, 1.1, (57, 3)).astype(np.float32)
    F = rng.integers(0, 57, (91, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    write_ply(p, torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(Cc), torch.from_numpy(N))
    v, f = _read_ply(p)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), V)
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), N)
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), np.round(np.clip(Cc.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    assert np.array_equal(f, F)
    write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 3)), np.zeros((0, 3)))
    v, f = _read_ply(str(tmp_path / "e.ply"))
    assert len(v) == 0 and len(f) == 0


def test_restatement_tables_give_a_closed_sphere():
    """an analytic signed distance of a sphere on fully weighted blocks: a closed 2-manifold (every directed edge once, its reverse
    once), Euler characteristic 2, no orphan vertex, triangles wound toward positive tsdf, normals radial"""
    v, c0, r0 = 0.05, np.array([0.013, -0.021, 0.007]), 0.9
    zz, yy, xx = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    blocks = {}
    for b in np.ndindex(4, 4, 4):
        b = tuple(int(q) - 2 for q in b)
        p = v * np.stack([b[0] * 16 + xx, b[1] * 16 + yy, b[2] * 16 + zz], -1)
        a = np.zeros((5, 16, 16, 16))
        a[0] = np.clip((np.linalg.norm(p - c0, axis=-1) - r0) / (8 * v), -1, 1)
        a[1] = 3.0
        blocks[b] = a
    V, F, _, N = T.extract(blocks, v, 3.0)
    edges = {}
    for f in F:
        for i in range(3):
            edges[(f[i], f[(i + 1) % 3])] = edges.get((f[i], f[(i + 1) % 3]), 0) + 1
    assert all(n == 1 and edges.get((b, a)) == 1 for (a, b), n in edges.items())
    assert len(V) - len(edges) // 2 + len(F) == 2
    assert len(np.unique(F)) == len(V)
    radial = (V - c0) / np.linalg.norm(V - c0, axis=1, keepdims=True)
    g = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    assert (np.sum(g * radial[F[:, 0]], 1) > 0).all()
    assert np.sum(N * radial, 1).min() > np.cos(np.radians(10))
    assert np.abs(np.linalg.norm(V - c0, axis=1) - r0).max() < 0.1 * v


# ---------------------------------------------------------------------------------------------------------------------------
# launcher
# ---------------------------------------------------------------------------------------------------------------------------
def _launcher():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_run_reference_script", os.path.join(PKG, "launch", "run_reference_script.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_launcher_rebinds_tsdf_fusion():
    if not os.path.exists(REF_SCRIPT):
        pytest.skip("the reference's extract_mesh_tsdf.py is not present")
    L = _launcher()
    src = open(REF_SCRIPT).read()
    tree = ast.parse(src)
    defined = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    fn = [n for n in defined if n.name == "tsdf_fusion"]
    assert fn, "the script defines tsdf_fusion itself"
    guards = [i for i, n in enumerate(tree.body) if L._is_main_guard(n)]
    assert guards and guards == list(range(len(tree.body) - len(guards), len(tree.body))), "the main guard comes last (run_script splits there)"
    import tsdf_fusion
    assert [a.arg for a in fn[0].args.args] == list(inspect.signature(tsdf_fusion.tsdf_fusion).parameters)
    launcher_src = open(os.path.join(PKG, "launch", "run_reference_script.py")).read()
    assert 'rebind["tsdf_fusion"] = tsdf_fusion.tsdf_fusion' in launcher_src


def test_run_script_replaces_a_defined_tsdf_fusion(tmp_path):
    """run_script's split on a script shaped like extract_mesh_tsdf.py: the product function is what the main block calls"""
    L = _launcher()
    script = tmp_path / "s.py"
    script.write_text("import json, sys\ndef tsdf_fusion(model_path, name, iteration, views, gaussians, pipeline, background, kernel_size):\n"
                      "    raise SystemExit('script function ran')\n"
                      "if __name__ == '__main__':\n    tsdf_fusion('m', 'test', 7, [], None, None, None, 0.0)\n")
    seen = []
    L.run_script(str(script), {"tsdf_fusion": lambda *a: seen.append(a)})
    assert seen == [("m", "test", 7, [], None, None, None, 0.0)]


def test_open3d_imports_resolve_to_the_product_stand_in(tmp_path):
    """`import open3d; import open3d.core as o3c` (extract_mesh_tsdf.py:12-13) in a script run by the launcher: with open3d absent
    they resolve to shims/open3d, whose attributes raise when called"""
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    probe = subprocess.run([sys.executable, "-c", "import open3d"], env=env, capture_output=True, text=True, timeout=120)
    if probe.returncode == 0:
        pytest.skip("a real open3d is installed: the launcher leaves it in place")
    script = tmp_path / "uses_open3d.py"
    script.write_text("import open3d as o3d\nimport open3d.core as o3c\nprint('FILE', o3d.__file__)\n"
                      "try:\n    o3c.Device('CUDA:0')\nexcept RuntimeError:\n    print('RAISES')\n")
    env.update(GOF_TORCH_EPILOGUE="1", GOF_INTEGRATE_CACHE_GB="0")
    r = subprocess.run([sys.executable, os.path.join(PKG, "launch", "run_reference_script.py"), str(script)], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.split("\n")
    assert any(l.startswith("FILE " + os.path.join(PKG, "shims", "open3d")) for l in out), r.stdout
    assert "RAISES" in out


if __name__ == "__main__":
    run_emulated(sys.argv[1], sys.argv[2])
