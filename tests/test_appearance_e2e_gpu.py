"""GPU, end to end: the reference's UNCHANGED train.py (oracle/_ref/refpy) with `--use_decoupled_appearance` through the launcher with
GOF_HIP_APPEARANCE=1: the script's `L1_loss_appearance` is train_epilogue.appearance's, fed with the rasterizer's own channel slice.
Every iteration's appearance L1 runs on the HIP unit (forward and backward counted), the carried 0-dim term leaves the rest of the loss
ONE fused call (no helper eager), the network and the embeddings train, the scene is learnt."""
import json
import os
import sys

import pytest

import test_e2e_scripts_gpu as E

pytestmark = pytest.mark.gpu
ITERS = 60


def test_train_py_with_the_hip_appearance_l1_keeps_the_rest_of_the_loss_fused(tmp_path):
    scene, model = str(tmp_path / "scene"), str(tmp_path / "model")
    E._run([sys.executable, os.path.join(E.ROOT, "tests", "fixtures", "make_blender_scene.py"), scene], E._env())
    args = ["--iterations", str(ITERS), "--densify_from_iter", "30", "--densification_interval", "20", "--distortion_from_iter", "30",
            "--depth_normal_from_iter", "30", "--test_iterations", "1", str(ITERS), "--save_iterations", str(ITERS), "--eval", "--use_decoupled_appearance"]
    cmd = [sys.executable, os.path.join(E.PKG, "launch", "run_reference_script.py"), os.path.join(E.REFPY, "train.py"), "-s", scene, "-m", model] + args
    env = E._env(GOF_STATS_JSON=os.path.join(model, "binding_stats.json"), GOF_HIP_APPEARANCE="1")
    env.pop("GOF_TORCH_APPEARANCE", None)
    out = E._run(cmd, env)
    assert "Training complete." in out
    ps = E._psnr(out)
    assert ps[ITERS] > ps[1] + 1.0, ps
    st = json.load(open(os.path.join(model, "binding_stats.json")))
    assert st["appearance"] == {"forwards": ITERS, "backwards": ITERS}, st.get("appearance")
    d = st["deferred_loss"]
    assert d["fused_backwards"] == ITERS and d["eager_terms"] == 0 and d["eager_tensors"] == 0, d
