"""The launcher's binding of eval_tnt/cull_mesh.py (run_reference_script.py 18.): for a script that defines `Mesher` and
`extract_depth_from_mesh` exactly those two names are replaced; the import stand-ins the script needs import and raise only when
called; and, where the reference tree is present, the unchanged script's __main__ reaches the bound Mesher with the script's own
intrinsics and the trajectory its get_traj loaded.  The Mesher bound here is a recording stand-in: nothing is rendered."""
import importlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
from host_child import PKG  # noqa: E402

REFERENCE_SCRIPT = "/root/reference/eval_tnt/cull_mesh.py"
SCRIPT = ("import os\n"
          "def extract_depth_from_mesh(mesh, c2w_list, H, W, fx, fy, cx, cy, far=20.0):\n"
          "    raise SystemExit('the script\\'s own render ran')\n"
          "class Mesher(object):\n"
          "    def __init__(self, *a, **k):\n"
          "        raise SystemExit('the script\\'s own Mesher ran')\n"
          "def get_traj(path):\n"
          "    return ['traj of ' + path]\n"
          "if __name__ == '__main__':\n"
          "    import sys\n"
          "    Mesher(1080, 1920, 1.0, 2.0, 3.0, 4.0, 20.0, points_batch_size=5e5)(sys.argv[1], get_traj(sys.argv[2]))\n")


def launcher():
    spec = importlib.util.spec_from_file_location("gof_launcher_raster", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L


def test_exactly_the_two_names_are_rebound(tmp_path, monkeypatch):
    L = launcher()
    monkeypatch.delenv("GOF_TNT_CULL_TORCH", raising=False)
    script = tmp_path / "cull_mesh.py"
    script.write_text(SCRIPT)
    table = L.tnt_cull_rebinding(str(script))
    assert set(table) == {"Mesher", "extract_depth_from_mesh"}
    only_one = tmp_path / "other.py"
    only_one.write_text(SCRIPT.replace("class Mesher", "class Mesher2").replace("    Mesher(", "    Mesher2("))
    assert L.tnt_cull_rebinding(str(only_one)) == {} and L.tnt_cull_rebinding(str(tmp_path / "missing.py")) == {}
    monkeypatch.setenv("GOF_TNT_CULL_TORCH", "1")
    assert L.tnt_cull_rebinding(str(script)) == {}
    src = open(os.path.join(PKG, "launch", "run_reference_script.py")).read()
    assert src.index("rebind.update(tnt_cull_rebinding(script))") < src.index("        run_script(script, rebind)") and " 18. eval_tnt/cull_mesh.py" in src


def test_run_script_replaces_the_class_and_the_function(tmp_path):
    L = launcher()
    script = tmp_path / "cull_mesh.py"
    script.write_text(SCRIPT)
    seen = []

    class Recorder:
        def __init__(self, *a, **k):
            seen.append(("init", a, k))

        def __call__(self, *a):
            seen.append(("call", a))
    argv = sys.argv
    sys.argv = [str(script), "mesh.ply", "traj.npy"]
    try:
        L.run_script(str(script), {"Mesher": Recorder, "extract_depth_from_mesh": len})
    finally:
        sys.argv = argv
    assert seen == [("init", (1080, 1920, 1.0, 2.0, 3.0, 4.0, 20.0), {"points_batch_size": 5e5}), ("call", ("mesh.ply", ["traj of traj.npy"]))]
    assert L.SCRIPT_OWN["Mesher"].__name__ == "Mesher" and L.SCRIPT_OWN["extract_depth_from_mesh"].__name__ == "extract_depth_from_mesh"


def test_the_stand_ins_import_and_raise_only_when_called():
    code = ("import sys; sys.path.append(%r); sys.path.append(%r); sys.path.append(%r)\n"
            "import pyrender\n"
            "cam = pyrender.IntrinsicsCamera; flags = pyrender.RenderFlags.OFFSCREEN; other = pyrender.anything.at.all\n"
            "try:\n"
            "    pyrender.Scene()\n"
            "except RuntimeError as e:\n"
            "    assert 'render_depth' in str(e) and 'pyrender.Scene' in str(e)\n"
            "else:\n"
            "    raise SystemExit('calling the stand-in did not raise')\n"
            "print('ok', pyrender.__file__)\n") % (os.path.join(PKG, "shims"), os.path.join(PKG, "shims_dtu", "trimesh"), os.path.join(PKG, "shims_dtu", "cv2"))
    have = importlib.util.find_spec("pyrender")
    if have is not None and not (have.origin or "").startswith(PKG):
        pytest.skip("a real pyrender is installed: it wins over the stand-in")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok") and os.path.join("shims", "pyrender") in r.stdout, r.stdout + r.stderr


def _child(traj, ply, out):
    """the unchanged reference script under the launcher's path set-up and rebinding, its Mesher a recorder"""
    L = launcher()
    script = REFERENCE_SCRIPT
    sys.path.insert(0, os.path.dirname(script))
    sys.path.insert(0, PKG)
    L.add_import_stand_ins()
    L.add_trimesh_stand_in()
    L.add_cv2_stand_in()
    table = L.tnt_cull_rebinding(script)
    seen = {}

    class Recorder:
        def __init__(self, *a, **k):
            seen["init"] = [list(a), {k2: v for k2, v in k.items()}]

        def __call__(self, path, traj):
            seen["call"] = [path, [np.asarray(t).tolist() for t in traj]]
    rebind = dict(table, Mesher=Recorder)
    sys.argv = [script, "--traj-path", traj, "--ply-path", ply]
    L.run_script(script, rebind)
    seen["names"] = sorted(table)
    seen["bound"] = [table["Mesher"].__name__, table["extract_depth_from_mesh"].__name__]
    with open(out, "w") as fh:
        json.dump(seen, fh)


@pytest.mark.skipif(not os.path.exists(REFERENCE_SCRIPT), reason="the reference tree is not present")
def test_the_unchanged_script_reaches_the_bound_mesher_with_its_intrinsics(tmp_path):
    poses = np.stack([np.eye(4, dtype=np.float32)[:3] + k for k in range(3)])
    np.save(tmp_path / "traj.npy", poses)
    out = tmp_path / "seen.json"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path / "traj.npy"), str(tmp_path / "mesh.ply"), str(out)], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, GOF_TNT_CULL_TORCH="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    seen = json.loads(out.read_text())
    assert seen["names"] == ["Mesher", "extract_depth_from_mesh"] and seen["bound"] == ["_tnt_mesher", "_tnt_render_depth"]
    import mesh_cull
    t = mesh_cull.TNT_INTRINSICS
    assert seen["init"] == [[t["height"], t["width"], t["fx"], t["fy"], t["cx"], t["cy"], 20.0], {"points_batch_size": 5e5}]
    assert seen["call"][0] == str(tmp_path / "mesh.ply") and len(seen["call"][1]) == 3
    want = [np.concatenate([p, [[0, 0, 0, 1]]]).tolist() for p in poses]
    assert seen["call"][1] == want and [m.numpy().tolist() for m in mesh_cull.get_traj(str(tmp_path / "traj.npy"))] == want


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2], sys.argv[3])
