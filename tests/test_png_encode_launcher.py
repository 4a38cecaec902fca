"""Item 15 of launch/run_reference_script.py: with GOF_HIP_PNG=1 torchvision.utils.save_image becomes
image_writer.save_image, GOF_PIL_PNG=1 leaves it alone, by default nothing changes (CPU, in child processes: the cases change sys.path);
and on the GPU the reference's unchanged render.py on the end-to-end fixture scene writes the same file names with the same pixels as
the default path.  Needs the reference's scripts as build() stages them (oracle/_ref/refpy) for the render.py run only."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
REFPY = os.path.join(ROOT, "oracle", "_ref", "refpy")
SHIMS = os.path.join(ROOT, "tests", "e2e_shims")
LAUNCHER = os.path.join(PKG, "launch", "run_reference_script.py")


def _launcher():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher", LAUNCHER)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _child(case):
    L = _launcher()
    sys.path.insert(0, PKG)
    L.add_import_stand_ins()
    import torchvision.utils as tvu
    before = tvu.save_image
    L.rebind_png_writer()
    rebound = tvu.save_image is not before
    if case == "rebound":
        assert rebound and tvu.save_image is L._save_image
        L.rebind_png_writer()                                   # a second call keeps the first function as the previous one
        assert L._PREVIOUS_SAVE_IMAGE["save_image"] is before
        import torch
        L._PREVIOUS_SAVE_IMAGE["save_image"] = lambda tensor, fp, format=None, **kw: print("PREVIOUS", fp)
        tvu.save_image(torch.zeros(3, 2, 2), "x.jpg")           # not a PNG: the function bound before, through image_writer
        import image_writer
        assert image_writer.previous is L._PREVIOUS_SAVE_IMAGE["save_image"]
        L.flush_png_writer()
    else:
        assert not rebound and "image_writer" not in sys.modules
        L.flush_png_writer()
    print("RESULT ok")


def _run_child(case, **env):
    e = dict(os.environ)
    for k in ("GOF_HIP_PNG", "GOF_PIL_PNG"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, "rc %d:\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_gof_hip_png_rebinds_save_image():
    assert "PREVIOUS x.jpg" in _run_child("rebound", GOF_HIP_PNG="1")


def test_gof_pil_png_leaves_save_image_alone():
    _run_child("alone", GOF_HIP_PNG="1", GOF_PIL_PNG="1")


def test_the_default_leaves_save_image_alone():
    _run_child("alone")


# ---- render.py on the fixture scene -------------------------------------------------------------------------------------------------------
def _env(**extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([SHIMS] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    env.update(extra)
    return env


def _run(cmd, env, timeout=600):
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, "command failed: %s\n--- stdout\n%s\n--- stderr\n%s" % (" ".join(cmd), r.stdout[-4000:], r.stderr[-6000:])
    return r.stdout


def _files(base):
    out = {}
    for d, _, names in os.walk(base):
        for n in names:
            if n.endswith(".png"):
                p = os.path.join(d, n)
                out[os.path.relpath(p, base)] = open(p, "rb").read()
    return out


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REFPY), reason="oracle/_ref/refpy not staged (build() stages it where the reference exists)")
def test_render_py_writes_the_same_files_with_the_same_pixels(tmp_path):
    """a model trained for 30 iterations on the fixture scene, render.py --skip_train twice: the default path, then GOF_HIP_PNG=1"""
    import io
    from PIL import Image
    scene, model = str(tmp_path / "scene"), str(tmp_path / "model")
    _run([sys.executable, os.path.join(ROOT, "tests", "fixtures", "make_blender_scene.py"), scene], _env())
    _run([sys.executable, LAUNCHER, os.path.join(REFPY, "train.py"), "-s", scene, "-m", model, "--iterations", "30", "--save_iterations", "30",
          "--test_iterations", "-1", "--eval", "--quiet"], _env())
    render = [sys.executable, LAUNCHER, os.path.join(REFPY, "render.py"), "-m", model, "--iteration", "30", "--skip_train", "--quiet"]
    base = os.path.join(model, "test", "ours_30")
    _run(render, _env())
    default = _files(base)
    assert len(default) == 8, sorted(default)
    for rel in default:
        os.remove(os.path.join(base, rel))
    _run(render, _env(GOF_HIP_PNG="1"))
    ours = _files(base)
    assert sorted(ours) == sorted(default)
    differ = 0
    for rel, data in ours.items():
        a, b = Image.open(io.BytesIO(data)), Image.open(io.BytesIO(default[rel]))
        assert a.mode == b.mode == "RGB" and a.size == b.size == (160, 120), rel
        assert np.array_equal(np.array(a), np.array(b)), "%s: the pixels differ from the default path's file" % rel
        differ += data != default[rel]
        print("%-32s ours %7d bytes  default %7d bytes (%.4f)" % (rel, len(data), len(default[rel]), len(data) / len(default[rel])))
    assert differ == len(ours), "the files are byte-identical to Pillow's: the device path did not run"


if __name__ == "__main__":
    _child(sys.argv[1])
