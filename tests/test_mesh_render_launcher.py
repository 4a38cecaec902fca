"""Item 19 of launch/run_reference_script.py: `mesh_viewer.py PATH` becomes mesh_render's command line over a
turntable of 8 shaded views, written to PATH_views/; GOF_MESH_VIEWER_WINDOW=1 leaves the script alone.  Open3D is never imported."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")
LAUNCHER = os.path.join(PKG, "launch", "run_reference_script.py")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "hipemu"))

# a viewer that, like the reference's, imports open3d first: a marker file tells that its own __main__ ran
STUB = """import sys
open(sys.argv[1] + ".own_main", "w").write("ran")
"""
DRIVER = """import runpy, sys
sys.argv = [%r, %r, %r]
try:
    runpy.run_path(%r, run_name="__main__")
except SystemExit as e:
    assert not e.code, e.code
assert "open3d" not in sys.modules
print("NO_OPEN3D")
"""


def _launch(tmp_path, mesh, env):
    script = tmp_path / "mesh_viewer.py"
    script.write_text(STUB)
    code = DRIVER % (LAUNCHER, str(script), mesh, LAUNCHER)
    return subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)


def test_the_rebinding_is_for_mesh_viewer_alone(monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "launch"))
    import run_reference_script as L
    monkeypatch.delenv("GOF_MESH_VIEWER_WINDOW", raising=False)
    assert list(L.mesh_viewer_rebinding("/somewhere/mesh_viewer.py")) == ["main"] and L.mesh_viewer_rebinding("/somewhere/render.py") == {}
    monkeypatch.setenv("GOF_MESH_VIEWER_WINDOW", "1")
    assert L.mesh_viewer_rebinding("/somewhere/mesh_viewer.py") == {}
    assert "19. mesh_viewer.py" in L.__doc__


def test_the_window_switch_runs_the_scripts_own_main(tmp_path):
    import host_child
    mesh = str(tmp_path / "mesh.ply")
    r = _launch(tmp_path, mesh, {"GOF_MESH_VIEWER_WINDOW": "1", "GOF_HIP_LIB": host_child.emulated_library()})
    assert r.returncode == 0 and "NO_OPEN3D" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(mesh + ".own_main") and not os.path.exists(mesh + "_views")


@pytest.mark.gpu
def test_mesh_viewer_writes_eight_views(tmp_path):
    from PIL import Image
    import mesh_cull as M
    import mesh_render_cases as KR
    V, F, col = KR.closed_mesh()
    mesh = str(tmp_path / "mesh.ply")
    M.DeviceMesh(V, F, colors=col).export(mesh)
    r = _launch(tmp_path, mesh, {"GOF_MESH_VIEWER_WINDOW": "0"})
    assert r.returncode == 0 and "NO_OPEN3D" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(mesh + "_views")) == ["0000%d.png" % k for k in range(8)] and not os.path.exists(mesh + ".own_main")
    img = np.asarray(Image.open(os.path.join(mesh + "_views", "00003.png")).convert("RGB"))
    assert img.shape == (600, 800, 3) and (img != 255).any(axis=2).mean() > 0.05 and (img[0, 0] == 255).all()      # the mesh on a white ground
