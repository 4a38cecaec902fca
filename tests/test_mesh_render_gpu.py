"""GPU tests of the mesh renderer: the cases and checks of tests/test_mesh_render_host.py on the device: normals,
depth, face, barycentrics and the image of every mode equal to tests/mesh_render_restatement.py bit for bit; the depth equals
gof_mesh_render_depth's; the order of the faces, repetition and the contents of workspaces and outputs do not matter; refused input
writes nothing; the command line's PNG files hold the planes."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mesh_raster_cases as K  # noqa: E402
import mesh_render_cases as KR  # noqa: E402
import test_mesh_render_host as T  # noqa: E402
from test_mesh_raster_gpu import _up, _down, _alloc  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")


@pytest.fixture(scope="module")
def M():
    import mesh_cull
    return mesh_cull


@pytest.fixture(scope="module")
def MR():
    import mesh_render
    return mesh_render


@pytest.mark.parametrize("size", ["%dx%d_" % s for s in K.SIZES])
def test_every_case_equals_the_restatement(M, MR, size):
    tiling = M.raster_tiling()
    S = KR.scenes(tiling)
    T.check_scenes(lambda tag: KR.run(MR, M, _up, S[tag], _down), T.old_names(size, tiling), tiling)


def test_the_new_scenes_equal_the_restatement(M, MR):
    tiling = M.raster_tiling()
    S = KR.scenes(tiling)
    T.check_new(lambda tag: KR.run(MR, M, _up, S[tag], _down), tiling)


def test_face_order_and_repetition(M, MR):
    tiling = M.raster_tiling()
    T.check_order(T.order_runs(MR, M, _up, _down, KR.scenes(tiling)), tiling)


def test_workspace_and_output_contents_do_not_matter(M, MR):
    tiling = M.raster_tiling()
    S = KR.scenes(tiling)
    got = {}
    for tag in T.FILL_SCENES:
        for fill in T.FILLS:
            cfg = T.FILL_CONFIG if S[tag][3] is not None else ("shaded", "shaded", False, False)
            got.update({"%s_%02x_%s" % (tag, fill, k): v for k, v in T.run_abi(M, MR, _alloc, _down, S[tag], fill, cfg).items()})
    T.check_fills(got, tiling)


def test_bad_input_is_refused_with_nothing_written(M, MR):
    scene = KR.scenes(M.raster_tiling())["closed"]
    got = {}
    for tag, sc, cfg, mutate, params, drop, _, _ in T.bad_inputs(scene):
        got.update({"%s_%s" % (tag, k): v for k, v in T.run_abi(M, MR, _alloc, _down, sc, 0x5C, cfg, mutate, params, drop).items()})
    T.check_errors(got, scene)


def test_python_layer(M, MR, tmp_path):
    T.check_python(T.python_runs(MR, M, _up, _down, str(tmp_path), device=True))


def test_versions(M, MR):
    L = M.lib
    assert L.gof_mesh_render_abi_version() == 4 and L.gof_mesh_raster_abi_version() == 3 and L.gof_mesh_abi_version() == 2 and L.gof_abi_version() == 12


def test_command_line_writes_the_planes(M, MR, tmp_path):
    """python -m mesh_render over a turntable: N PNG files whose pixels are floor(255 x + 0.5) of the planes render() returns"""
    from PIL import Image
    V, F, col = KR.closed_mesh()
    ply = str(tmp_path / "closed.ply")
    M.DeviceMesh(V, F, colors=col).export(ply)
    out = str(tmp_path / "views")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, "-m", "mesh_render", ply, "--turntable", "3", "--mode", "normal_world", "--out", out, "--size", "70x33"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["00000.png", "00001.png", "00002.png"]
    mesh = M.load(ply)
    t = MR.turntable(mesh, 3, 33, 70)
    img = _down(MR.render(mesh, t["c2w"], 33, 70, t["fx"], t["fy"], t["cx"], t["cy"], mode="normal_world", zfar=4.0 * t["radius"] + 1.0))
    assert (img != 1.0).any()
    for k in range(3):
        png = np.asarray(Image.open(os.path.join(out, "%05d.png" % k)).convert("RGB"))
        assert np.array_equal(png, np.floor(255.0 * img[k].astype(np.float64).transpose(1, 2, 0) + 0.5).astype(np.uint8)), k
