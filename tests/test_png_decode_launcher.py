"""Item 16 of launch/run_reference_script.py: with GOF_HIP_PNG_READ=1 a script's `readImages` becomes
png_reader.read_images_for_metrics, GOF_PIL_PNG_READ=1 leaves it alone whatever else is set, by default nothing changes; the rebinding
keeps the script's own function, and the files the unit does not take -- and only they -- go through it (CPU: the kernels run through the
host emulator, in child processes).  Where the reference checkout exists, the lines of metrics.py the replacement restates are
confirmed on its source."""
import ast
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
LAUNCHER = os.path.join(PKG, "launch", "run_reference_script.py")
REF = "/root/reference"

# a script shaped like metrics.py: it defines readImages itself and calls it from its __main__ block
SCRIPT = '''
import os
def readImages(renders_dir, gt_dir):
    print("OWN readImages", os.path.basename(str(renders_dir)))
    return ["own"], ["own"], ["own"]
def other():
    return readImages
if __name__ == "__main__":
    import sys
    print("BOUND", readImages.__module__, readImages.__name__)
'''


def _launcher():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher", LAUNCHER)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _pillow_read_images(renders_dir, gt_dir):
    """metrics.py's readImages, restated without .cuda() and for every mode Pillow opens: what the not-taken files are compared with"""
    import torch
    from PIL import Image
    calls.append(sorted(os.listdir(renders_dir)))

    def one(path):
        a = np.asarray(Image.open(path).convert("RGB"))
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255).unsqueeze(0)[:, :3, :, :]
    names = list(os.listdir(renders_dir))
    return [one(renders_dir / n) for n in names], [one(gt_dir / n) for n in names], names


calls = []


def _child(case, tmp):
    L = _launcher()
    sys.path.insert(0, PKG)
    if case in ("rebound", "alone"):
        script = os.path.join(tmp, "script.py")
        with open(script, "w") as f:
            f.write(SCRIPT)
        rebind = L.png_reader_rebinding(script)
        assert (case == "rebound") == ("readImages" in rebind) and "png_reader" not in sys.modules
        L.run_script(script, rebind)
        if case == "rebound":
            assert L.SCRIPT_OWN["readImages"].__name__ == "readImages" and L.SCRIPT_OWN["readImages"] is not L._read_images_for_metrics
        else:
            assert not L.SCRIPT_OWN
        print("RESULT ok")
        return
    # "files": the replacement on a renders / gt pair through the emulator, the previous function a Pillow restatement
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import png_decode_cases as K
    import png_reader as R
    import test_png_decode_host as TH
    check = TH.host_seams(R)
    renders, gt = os.path.join(tmp, "renders"), os.path.join(tmp, "gt")
    os.makedirs(renders)
    os.makedirs(gt)
    taken = {"00000.png": ("grid_65x129", "pillow_1"), "00001.png": ("pillow_6", "pillow_6"), "00002.png": ("pillow_9", "c1"), "00003.png": ("c2", "pillow_la")}
    for n, (a, b) in taken.items():
        open(os.path.join(renders, n), "wb").write(K.build(a))
        open(os.path.join(gt, n), "wb").write(K.build(b))
    other = K.not_taken_files()
    for k, (n, (data, _)) in enumerate(sorted(other.items())):
        # the refused file once as the render, once as the ground truth
        open(os.path.join(renders, "x_%s.png" % n), "wb").write(data if k % 2 == 0 else K.build("mix"))
        open(os.path.join(gt, "x_%s.png" % n), "wb").write(data if k % 2 == 1 else K.build("mix"))
    L.SCRIPT_OWN["readImages"] = _pillow_read_images
    from pathlib import Path
    r, g, names = L._read_images_for_metrics(Path(renders), Path(gt))
    assert R.previous is _pillow_read_images
    assert names == list(os.listdir(renders)) and len(r) == len(g) == len(names) == len(taken) + len(other)
    assert calls == [sorted("x_%s.png" % n for n in other)], "the function bound before is given the refused files, once, and only them"
    want_r, want_g, want_names = _pillow_read_images(Path(renders), Path(gt))
    assert want_names == names
    import torch
    for n, a, b, wa, wb in zip(names, r, g, want_r, want_g):
        for got, want, d in ((a, wa, renders), (b, wb, gt)):
            f = open(os.path.join(d, n), "rb").read()
            c = min(3, K.header(f)[2]) if n in taken else 3
            assert got.dtype == torch.float32 and got.dim() == 4 and got.shape[:2] == (1, c), (n, got.shape)
            if c == 3:
                assert torch.equal(got, want), n
            else:                                   # a 1- or 2-channel file keeps the channels it has: [:, :3] of to_tensor's
                w, h, cc = K.header(f)
                assert torch.equal(got[0], K.to_tensor(K.pillow_pixels(f))[:3]), n
    assert R.stats["previous"] == len(other) and check() > 0
    print("RESULT ok")


def _run_child(case, tmp_path, **env):
    sys.path.insert(0, os.path.join(ROOT, "tests", "hipemu"))
    import host_child
    e = dict(os.environ, GOF_HIP_LIB=host_child.emulated_library())
    for k in ("GOF_HIP_PNG_READ", "GOF_PIL_PNG_READ"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, str(tmp_path)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RESULT ok" in r.stdout, "rc %d:\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


def test_gof_hip_png_read_rebinds_read_images(tmp_path):
    assert "BOUND gof_launcher _read_images_for_metrics" in _run_child("rebound", tmp_path, GOF_HIP_PNG_READ="1")


def test_gof_pil_png_read_leaves_the_script_alone(tmp_path):
    assert "BOUND __main__ readImages" in _run_child("alone", tmp_path, GOF_HIP_PNG_READ="1", GOF_PIL_PNG_READ="1")
    assert "BOUND __main__ readImages" in _run_child("alone", tmp_path, GOF_PIL_PNG_READ="1")


def test_the_default_leaves_the_script_alone(tmp_path):
    assert "BOUND __main__ readImages" in _run_child("alone", tmp_path)
    assert _launcher().PNG_READER_BY_DEFAULT is False


def test_refused_files_go_through_the_function_bound_before_and_the_rest_is_bit_identical(tmp_path):
    pytest.importorskip("PIL")
    _run_child("files", tmp_path)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "metrics.py")), reason="the reference checkout is not present")
def test_metrics_py_reads_its_images_the_way_the_replacement_restates():
    tree = ast.parse(open(os.path.join(REF, "metrics.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "readImages"]
    assert len(fn) == 1 and [a.arg for a in fn[0].args.args] == ["renders_dir", "gt_dir"]
    src = ast.unparse(fn[0])
    assert "for fname in os.listdir(renders_dir)" in src
    assert "Image.open(renders_dir / fname)" in src and "Image.open(gt_dir / fname)" in src
    assert src.count("tf.to_tensor(") == 2 and src.count(".unsqueeze(0)[:, :3, :, :].cuda()") == 2
    assert "return (renders, gts, image_names)" in src
    guards = [n for n in tree.body if isinstance(n, ast.If)]
    assert guards and tree.body[-1] is guards[-1], "the __main__ block is the last statement: run_script can split the script there"


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
