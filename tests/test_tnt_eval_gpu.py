"""GPU tests of the Tanks-and-Temples F-score evaluation: the cases of tests/test_tnt_eval_host.py on the device
with the same equalities, and one large case (a 5 M-point target, a 3 M-point source, one registration_vol_ds and the F-score)
against tests/tnt_eval_restatement.py on SciPy's cKDTree: the sums of every ICP evaluation bit-equal (teacher-forced), the F-score
integers equal."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tnt_eval_restatement as R  # noqa: E402
import test_tnt_eval_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
bits = H.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(case, tmp_path=None):
    import tnt_eval as M
    return H.run_case(M, case, str(tmp_path) if tmp_path is not None else None, dev)


@pytest.mark.parametrize("name", H.CROP_CASES)
def test_crop_is_bit_equal(name):
    H.check_crop(name, run("crop:" + name))


@pytest.mark.parametrize("name", H.VOXEL_CASES)
def test_voxel_means_are_bit_equal(name):
    H.check_voxel(name, run("voxel:" + name))


@pytest.mark.parametrize("name", H.SUMS_CASES)
def test_correspondence_sums_are_the_tree(name):
    s, t, thr = H.sums_case(name)
    res = run("sums:" + name)
    assert not np.isnan(res["rec_s2"][0]).any()
    assert H.check_record(res, s, t, thr) == 1


@pytest.mark.parametrize("threshold", ["10.0", "1.0"])
def test_icp_teacher_forced(threshold):
    s, t = H.registration_case()
    s = R.transform(s, H.KNOWN @ H.similarity_matrix(1.02, 2.0, [0.5, 0.2, 1.0], [0.4, -0.3, 0.2]))
    res = run("icp:" + threshold)
    assert H.check_record(res, s[:20000], t[:25000], float(threshold)) == 7


def test_icp_three_stages_free_running():
    s, t = H.registration_case()
    want = H.restated_stages(s, t)
    got = run("stages:run")["T"]
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, got[k], want[k])


def test_fscore_equals_the_restatement():
    s, t = H.registration_case()
    want = R.tnt_fscore(s, t, H.KNOWN @ H.similarity_matrix(1.0, 0.2, [0, 1, 0], [0.05, 0.0, 0.1]), H.volume_for(2), H.TAU)
    H.check_fscore(run("fscore:run"), want)


def test_command_line_on_a_synthetic_scene(tmp_path):
    res = run("cli:barn", tmp_path)
    H.check_cli(str(res["root"]), str(res["error"]))


def test_large_registration_and_fscore():
    """a 5 M-point target, a 3 M-point source: one registration_vol_ds (voxel tau, threshold 20 tau) and the F-score at tau.  The far
    patch is 300 points: the restatement's kd-tree visits most of the target for each of them (50 000 of them cost it two minutes per
    evaluation); the points lifted off the surface by 0.3 .. 14 keep the mask biting at 20 tau = 1.  Nearly all of the test's time is
    the restatement's: one kd-tree build and query per evaluation, up to 21 of them."""
    import tnt_eval as M
    tau = 0.05
    source, target = H.registration_case(5_000_000, 3_000_000, seed=31, n_far=300)
    vol = H.volume_for(2)
    init = H.KNOWN @ H.similarity_matrix(1.004, 0.4, [0.5, 0.2, 1.0], [0.1, -0.08, 0.05])
    s_d, t_d = dev(source), dev(target)
    T, fit, rmse, rec = M.registration_vol_ds(s_d, t_d, init, vol, tau, 20 * tau, 20)
    print("icp:", M.last_stats()["icp"], "fitness", fit, "rmse", rmse)
    s = R.voxel_down_sample(R.crop(source, vol, init)[0], tau)[0]
    t = R.voxel_down_sample(R.crop(target, vol)[0], tau)[0]
    assert len(s) > 1_000_000 and len(t) > 1_000_000, (len(s), len(t))
    res = H.pack_record(rec)
    assert H.check_record(res, s, t, 20 * tau) == len(rec) >= 3
    assert 0 < rec[-1]["n"] < len(s)
    got = M.tnt_fscore(s_d, t_d, T, vol, tau)
    want = R.tnt_fscore(source, target, T, vol, tau)
    print("fscore:", {k: want[k] for k in ("precision", "recall", "fscore")})
    H.check_fscore({k: (v.cpu().numpy() if hasattr(v, "cpu") else np.array(v)) for k, v in got.items()}, want)
