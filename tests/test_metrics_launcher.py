"""CPU-only: under the launcher's sys.path arrangement `import lpips` and `import torchvision` resolve (to an installed package, or to
the stand-ins of shims/), with everything render.py and metrics.py use of them; the stand-ins' two functions have torchvision's
arithmetic.  The tests that parse the reference's scripts need the reference checkout and skip without it."""
import ast
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import lpips_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
SHIMS = os.path.join(PKG, "shims")
REF = "/root/reference"
PACKAGES = ("torchvision", "lpips", "PIL")


def _launcher():
    spec = importlib.util.spec_from_file_location("gof_launcher_metrics", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L


@pytest.fixture
def arranged():
    """the launcher's arrangement of the import stand-ins, undone afterwards"""
    path, mods = list(sys.path), set(sys.modules)
    L = _launcher()
    L.add_import_stand_ins()
    try:
        yield L
    finally:
        sys.path[:] = path
        for k in set(sys.modules) - mods:
            if k.split(".")[0] in ("torchvision", "lpips", "open3d", "tetranerf", "utils", "scene"):
                del sys.modules[k]


def test_import_lpips_and_torchvision_resolve_under_the_launcher(arranged):
    missing = [m for m in ("lpips", "torchvision") if not any(os.path.isdir(os.path.join(p, m)) or os.path.isfile(os.path.join(p, m + ".py"))
                                                                for p in sys.path if p != SHIMS)]
    if missing:
        assert sys.path[-1] == SHIMS                       # last: an installed package wins
    import lpips
    import torchvision
    import torchvision.transforms.functional as tf
    import image_metrics
    assert callable(lpips.LPIPS) and callable(torchvision.utils.save_image) and callable(tf.to_tensor)
    if "lpips" in missing:
        assert lpips.LPIPS is image_metrics.LPIPS
        with pytest.raises(RuntimeError, match="not installed"):
            lpips.im2tensor(None)
    if "torchvision" in missing and os.path.abspath(torchvision.__file__).startswith(SHIMS):
        with pytest.raises(RuntimeError, match="not installed"):
            torchvision.models.vgg16()
        with pytest.raises(RuntimeError, match="not installed"):
            torchvision.utils.make_grid(None)


def _stand_in(name):
    """a module of the torchvision stand-in, loaded by path (whatever is installed)"""
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] == "torchvision"}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, SHIMS)
    try:
        return importlib.import_module(name)
    finally:
        sys.path.remove(SHIMS)
        for k in [k for k in sys.modules if k.split(".")[0] == "torchvision"]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_save_image_and_to_tensor_have_torchvisions_arithmetic(tmp_path):
    from PIL import Image
    utils, tf = _stand_in("torchvision.utils"), _stand_in("torchvision.transforms.functional")
    g = torch.Generator().manual_seed(2)
    x = torch.rand((3, 21, 34), generator=g) * 1.2 - 0.1              # values below 0 and above 1 are clamped
    x[0, 0, :6] = torch.tensor([0.0, 1.0, 0.5 / 255, 1.5 / 255, 254.5 / 255, 0.49999 / 255])
    utils.save_image(x, str(tmp_path / "a.png"))
    pic = Image.open(str(tmp_path / "a.png"))
    want = R.save_image_bytes(x)
    assert pic.mode == "RGB" and pic.size == (34, 21) and np.array_equal(np.asarray(pic), want)
    t = tf.to_tensor(pic)
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 21, 34)
    assert torch.equal(t, torch.from_numpy(want.transpose(2, 0, 1).copy()).to(torch.float32).div(255))
    utils.save_image(x[None], str(tmp_path / "b.png"))              # render.py passes (3,H,W); a batch of one is the same image
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "b.png"))), want)
    rgba = Image.fromarray(np.dstack([want, np.full(want.shape[:2], 200, np.uint8)]), "RGBA")
    assert tuple(tf.to_tensor(rgba).shape) == (4, 21, 34) and torch.equal(tf.to_tensor(rgba)[:3], t)      # metrics.py:33 slices [:3]
    with pytest.raises(RuntimeError, match="make_grid"):
        utils.save_image(torch.zeros((2, 3, 4, 4)), str(tmp_path / "c.png"))


def _used_names(tree):
    """{local name: dotted module path} for the imports of PACKAGES, and every attribute chain the script uses on those names"""
    names = {}
    for n in ast.walk(tree):
        if isinstance(n, ast.Import):
            for a in n.names:
                if a.name.split(".")[0] in PACKAGES:
                    names[a.asname or a.name.split(".")[0]] = a.name if a.asname else a.name.split(".")[0]
        elif isinstance(n, ast.ImportFrom) and n.module and n.module.split(".")[0] in PACKAGES:
            for a in n.names:
                names[a.asname or a.name] = n.module + "." + a.name
    chains = set()
    for n in ast.walk(tree):
        if isinstance(n, ast.Attribute):
            parts, cur = [], n
            while isinstance(cur, ast.Attribute):
                parts.append(cur.attr)
                cur = cur.value
            if isinstance(cur, ast.Name) and cur.id in names:
                chains.add(names[cur.id] + "." + ".".join(reversed(parts)))
    return names, chains


def _resolve(dotted):
    parts = dotted.split(".")
    obj = importlib.import_module(parts[0])
    for i, p in enumerate(parts[1:], 1):
        try:
            obj = getattr(obj, p)
        except AttributeError:
            obj = importlib.import_module(".".join(parts[:i + 1]))
    return obj


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not present")
@pytest.mark.parametrize("script", ["metrics.py", "render.py"])
def test_every_name_the_scripts_use_of_the_packages_resolves(script, arranged):
    tree = ast.parse(open(os.path.join(REF, script)).read())
    names, chains = _used_names(tree)
    assert "torchvision" in " ".join(names.values())
    if script == "metrics.py":
        assert {"torchvision.transforms.functional.to_tensor", "lpips.LPIPS", "PIL.Image.open"} <= chains
    else:
        assert "torchvision.utils.save_image" in chains
    for dotted in sorted(set(names.values()) | chains):
        obj = _resolve(dotted)
        assert type(obj).__name__ != "Missing", "%s uses %s, which the stand-in does not provide" % (script, dotted)
        if dotted in chains and not isinstance(obj, type(os)):
            assert callable(obj), dotted


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference checkout is not present")
def test_metrics_py_gets_the_hip_ssim(arranged):
    from train_epilogue import deferred
    sys.path.insert(0, REF)
    try:
        arranged.rebind_train_epilogue()
        import utils.loss_utils as ref_loss
        assert ref_loss.ssim is deferred.ssim
    finally:
        deferred.enable(False)                              # (the launcher switches deferred evaluation on for the process)
    tree = ast.parse(open(os.path.join(REF, "metrics.py")).read())
    assert any(isinstance(n, ast.ImportFrom) and n.module == "utils.loss_utils" and any(a.name == "ssim" for a in n.names) for n in tree.body)
