"""CPU-only, needs the reference's Python scripts as __graft_entry__.build() stages them (oracle/_ref/refpy, byte-identical copies;
skipped where they were not staged): item 13 of launch/run_reference_script.py -- GaussianModel.save_ply / save_fused_ply / load_ply
become model_io's, `import plyfile` and `import cv2` resolve to the stand-ins where nothing else provides them, and the reference's own
file functions run on the plyfile stand-in.

Every case runs in a child process with the launcher's own path set-up (what main() does before it runs the script): the cases change
sys.path and import the reference's packages, which must not leak into the session."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "refpy")
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
OPTIONAL = ("plyfile", "cv2", "open3d", "trimesh", "torchvision")
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="oracle/_ref/refpy not staged (build() stages it where the reference exists)")


def _launcher():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher", os.path.join(PKG, "launch", "run_reference_script.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _set_up_paths(L, first=()):
    """what main() does in front of the script"""
    sys.path.insert(0, REF)
    sys.path.insert(0, PKG)
    for p in first:
        sys.path.insert(0, p)
    L.add_import_stand_ins()
    L.add_dtu_shims(os.path.join(REF, "train.py"))
    L.add_trimesh_stand_in()
    L.add_cv2_stand_in()


def _cpu_model(GaussianModel, m, degree):
    import torch
    g = GaussianModel.__new__(GaussianModel)          # (__init__ builds the appearance network on the device)
    g.max_sh_degree, g.active_sh_degree = degree, 0
    g.setup_functions()
    for attr, key in (("_xyz", "xyz"), ("_features_dc", "f_dc"), ("_features_rest", "f_rest"), ("_opacity", "opacity"),
                      ("_scaling", "scaling"), ("_rotation", "rotation")):
        setattr(g, attr, torch.nn.Parameter(torch.from_numpy(m[key].copy())))
    g.filter_3D = torch.from_numpy(m["filter_3D"].copy())
    return g


def _child(case, tmp):
    import importlib.util
    import inspect
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import model_io_cases as K
    L = _launcher()
    out = {}
    if case in ("rebound", "torch_ply"):
        _set_up_paths(L)
        from scene.gaussian_model import GaussianModel
        orig = {n: getattr(GaussianModel, n) for n in ("save_ply", "save_fused_ply", "load_ply")}
        L.rebind_model_io()
        now = {n: getattr(GaussianModel, n) for n in orig}
        out["rebound"] = {n: now[n] is not orig[n] for n in orig}
        out["to_launcher"] = {n: now[n] is getattr(L, "_" + n) for n in orig}
        out["kept"] = {n: L._REFERENCE_PLY.get(n) is orig[n] for n in orig}
        out["signatures"] = {n: list(inspect.signature(now[n]).parameters) == list(inspect.signature(orig[n]).parameters) for n in orig}
        if case == "rebound":
            import plyfile
            out["plyfile"] = os.path.relpath(plyfile.__file__, PKG)
            m = K.golden_model("d1")
            g = _cpu_model(GaussianModel, m, 1)
            raw, fused = os.path.join(tmp, "a", "raw.ply"), os.path.join(tmp, "a", "fused.ply")
            g.save_ply(raw)                          # a host model: model_io hands it to the reference's own method
            g.save_fused_ply(fused)
            import model_io
            out["reference_is_the_launchers"] = model_io.reference is L._REFERENCE_PLY
            out["nothing_saved_here"] = "save" not in model_io.last_stats()
            gold = K.golden()
            out["raw_bytes_equal"] = open(raw, "rb").read() == K.header(5, K.names(3)) + gold["d1_raw"].tobytes()
            # (the fused file's log columns are torch's vectorised math, whose last bit may follow the CPU: compared as numbers)
            data = open(fused, "rb").read()
            head = K.header(5, K.names(3, fused=True))
            got = np.frombuffer(data[len(head):], np.float32).reshape(5, 26)
            ref = np.frombuffer(gold["d1_fused"].tobytes(), np.float32).reshape(5, 26)
            moved = [c for c in range(26) if not 18 <= c < 22]
            out["fused_bytes_equal"] = bool(data.startswith(head) and got[:, moved].tobytes() == ref[:, moved].tobytes()
                                            and np.allclose(got, ref, rtol=1e-5, atol=0))
    elif case == "plyfile_wins":
        fake = os.path.join(tmp, "site")
        os.makedirs(os.path.join(fake, "plyfile"))
        with open(os.path.join(fake, "plyfile", "__init__.py"), "w") as fh:
            fh.write("INSTALLED = True\n")
        _set_up_paths(L, first=[fake])
        import plyfile
        out["installed_wins"] = bool(getattr(plyfile, "INSTALLED", False))
        out["shims_last"] = sys.path.index(os.path.join(PKG, "shims")) > sys.path.index(REF)
    elif case == "store_fetch":
        _set_up_paths(L)
        import plyfile
        out["plyfile"] = os.path.relpath(plyfile.__file__, PKG)
        from scene.dataset_readers import fetchPly, storePly
        rng = np.random.default_rng(4)
        xyz = rng.normal(0, 2, (37, 3)).astype(np.float32)
        rgb = rng.integers(0, 256, (37, 3)).astype(np.uint8)
        path = os.path.join(tmp, "points3D.ply")
        storePly(path, xyz, rgb)
        head = open(path, "rb").read(400)
        out["header"] = head[:head.index(b"end_header\n") + 11].decode()
        out["size"] = os.path.getsize(path)
        pc = fetchPly(path)
        out["points_equal"] = bool(np.array_equal(pc.points, xyz))
        out["colors_equal"] = bool(np.array_equal(pc.colors, rgb / 255.0))
        out["normals_zero"] = bool((pc.normals == 0).all() and pc.normals.shape == (37, 3))
    elif case == "train_imports":
        import ast
        out["installed"] = [n for n in OPTIONAL if importlib.util.find_spec(n) is not None]
        _set_up_paths(L)
        tree = ast.parse(open(os.path.join(REF, "train.py")).read())
        imports = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
        out["statements"] = len(imports)
        ns = {"__name__": "train_imports"}
        exec(compile(ast.Module(body=imports, type_ignores=[]), "train.py", "exec"), ns)
        out["names"] = sorted(k for k in ns if k in ("cv2", "GaussianModel", "Scene", "render", "l1_loss", "ssim"))
        out["origins"] = {n: os.path.relpath(sys.modules[n].__file__, PKG) for n in OPTIONAL if n in sys.modules and n not in out["installed"]}
    else:
        raise KeyError(case)
    print("RESULT " + json.dumps(out))


def _run(case, tmp_path, env=None):
    e = dict(os.environ, **(env or {}))
    e.pop("GOF_HIP_LIB", None)
    if "GOF_TORCH_PLY" not in (env or {}):
        e.pop("GOF_TORCH_PLY", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, str(tmp_path)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "%s failed (rc %d):\n%s\n%s" % (case, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0][7:])


def test_the_three_methods_are_rebound_and_a_host_model_falls_through(tmp_path):
    out = _run("rebound", tmp_path)
    for key in ("rebound", "to_launcher", "kept", "signatures"):
        assert out[key] == {"save_ply": True, "save_fused_ply": True, "load_ply": True}, (key, out[key])
    assert out["plyfile"] == os.path.join("shims", "plyfile", "__init__.py")
    assert out["reference_is_the_launchers"] and out["nothing_saved_here"]
    # the reference's own methods, running on the plyfile stand-in, write the golden's bytes behind the header this project writes
    assert out["raw_bytes_equal"] and out["fused_bytes_equal"]


def test_gof_torch_ply_leaves_the_reference_alone(tmp_path):
    out = _run("torch_ply", tmp_path, env={"GOF_TORCH_PLY": "1"})
    assert out["rebound"] == {"save_ply": False, "save_fused_ply": False, "load_ply": False}
    assert out["kept"] == {"save_ply": False, "save_fused_ply": False, "load_ply": False}


def test_an_installed_plyfile_wins(tmp_path):
    out = _run("plyfile_wins", tmp_path)
    assert out["installed_wins"] and out["shims_last"]


def test_store_and_fetch_ply_of_the_reference_on_the_stand_in(tmp_path):
    out = _run("store_fetch", tmp_path)
    if out["plyfile"] != os.path.join("shims", "plyfile", "__init__.py"):
        pytest.skip("a plyfile package is installed: the stand-in is not what the reference imports")
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex 37\n" + "".join("property float %s\n" % n for n in ("x", "y", "z", "nx", "ny", "nz"))
            + "".join("property uchar %s\n" % n for n in ("red", "green", "blue")) + "end_header\n")
    assert out["header"] == want and out["size"] == len(want) + 37 * 27
    assert out["points_equal"] and out["colors_equal"] and out["normals_zero"]


def test_train_py_imports_with_no_optional_package(tmp_path):
    out = _run("train_imports", tmp_path)
    assert out["statements"] >= 10 and {"cv2", "GaussianModel", "Scene", "render"} <= set(out["names"])
    for n in ("plyfile", "cv2", "trimesh"):             # imported at module top on train.py's way; open3d and torchvision are not
        if n not in out["installed"]:
            assert out["origins"][n].split(os.sep)[0] in ("shims", "shims_dtu"), out["origins"]


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
