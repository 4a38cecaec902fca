"""CPU-only: the launcher rebinds `L1_loss_appearance` by name in a script that defines it (train.py:67), as it rebinds
`evaluage_alpha`; GOF_TORCH_APPEARANCE=1 keeps the script's own function; a script that does not define the name runs untouched.
While the HIP path is not the default (launch/run_reference_script.py: APPEARANCE_BY_DEFAULT) GOF_HIP_APPEARANCE=1 asks for it."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")

DEFINES = """
import sys
def L1_loss_appearance(image, gt_image, gaussians, view_idx, return_transformed_image=False):
    return "the script's own"
def other():
    return L1_loss_appearance
if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        f.write(L1_loss_appearance.__module__ + ":" + L1_loss_appearance.__name__ + ":" + other().__name__)
"""
DOES_NOT = """
import sys
def l1(image, gt_image):
    return 0
if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        f.write(__name__ + ":" + l1.__name__ + ":" + str("L1_loss_appearance" in globals()))
"""


@pytest.fixture
def launcher():
    spec = importlib.util.spec_from_file_location("gof_launcher_appearance", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L


def _run(L, text, tmp_path, monkeypatch):
    script, out = tmp_path / "script.py", tmp_path / "out.txt"
    script.write_text(text)
    monkeypatch.setattr("sys.argv", [str(script), str(out)])
    L.run_script(str(script), L.appearance_rebinding(str(script)))
    return out.read_text()


def _env(monkeypatch, **values):
    for k in ("GOF_TORCH_APPEARANCE", "GOF_HIP_APPEARANCE", "GOF_TORCH_EPILOGUE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in values.items():
        monkeypatch.setenv(k, v)


def test_the_name_is_rebound_in_a_script_that_defines_it(launcher, tmp_path, monkeypatch):
    _env(monkeypatch, GOF_HIP_APPEARANCE="1")
    rebind = launcher.appearance_rebinding("train.py")
    assert list(rebind) == ["L1_loss_appearance"] and rebind["L1_loss_appearance"] is launcher._l1_loss_appearance
    # every use of the name inside the script sees the replacement (the script's functions look it up in the script's namespace)
    assert _run(launcher, DEFINES, tmp_path, monkeypatch) == "gof_launcher_appearance:_l1_loss_appearance:_l1_loss_appearance"


def test_the_default_follows_the_measured_decision(launcher, tmp_path, monkeypatch):
    _env(monkeypatch)
    rebind = launcher.appearance_rebinding("train.py")
    assert bool(rebind) == bool(launcher.APPEARANCE_BY_DEFAULT)
    want = "gof_launcher_appearance:_l1_loss_appearance:_l1_loss_appearance" if launcher.APPEARANCE_BY_DEFAULT else "__main__:L1_loss_appearance:L1_loss_appearance"
    assert _run(launcher, DEFINES, tmp_path, monkeypatch) == want


@pytest.mark.parametrize("env", [{"GOF_TORCH_APPEARANCE": "1"}, {"GOF_TORCH_APPEARANCE": "1", "GOF_HIP_APPEARANCE": "1"}, {"GOF_TORCH_EPILOGUE": "1", "GOF_HIP_APPEARANCE": "1"}],
                         ids=lambda e: "+".join(sorted(e)))
def test_the_switch_keeps_the_scripts_own_function(env, launcher, tmp_path, monkeypatch):
    _env(monkeypatch, **env)
    assert launcher.appearance_rebinding("train.py") == {}
    assert _run(launcher, DEFINES, tmp_path, monkeypatch) == "__main__:L1_loss_appearance:L1_loss_appearance"


def test_a_script_that_does_not_define_the_name_is_untouched(launcher, tmp_path, monkeypatch):
    _env(monkeypatch, GOF_HIP_APPEARANCE="1")
    assert _run(launcher, DOES_NOT, tmp_path, monkeypatch) == "__main__:l1:False"


def test_the_replacement_has_the_references_signature_and_reaches_the_hip_unit(launcher, monkeypatch):
    import inspect
    import sys
    assert list(inspect.signature(launcher._l1_loss_appearance).parameters) == ["image", "gt_image", "gaussians", "view_idx", "return_transformed_image"]
    assert inspect.signature(launcher._l1_loss_appearance).parameters["return_transformed_image"].default is False
    if PKG not in sys.path:
        monkeypatch.syspath_prepend(PKG)
    import train_epilogue.appearance as A
    real = inspect.signature(A.L1_loss_appearance)          # the unit's own function, before it is replaced below
    assert list(real.parameters) == ["image", "gt_image", "gaussians", "view_idx", "return_transformed_image"]
    assert real.parameters["return_transformed_image"].default is False
    seen = []
    monkeypatch.setattr(A, "L1_loss_appearance", lambda *a: seen.append(a) or "hip")
    assert launcher._l1_loss_appearance(1, 2, 3, 4) == "hip" and seen == [(1, 2, 3, 4, False)]
