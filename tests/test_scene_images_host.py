"""CPU tests of the scene images: the kernels of csrc/scene_images.hip through the host emulator (tests/hipemu) behind
scene_images' own Python layer, each group of cases in a child process (an emulator abort fails one test, not the session), held to
Pillow and the reference's PILtoTorch through the committed golden (tests/golden/ref_scene_images_golden.npz, written by
tests/golden/make_golden_scene_images.py) and to the resampler restated in tests/scene_images_cases.py.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context / pinned allocation / side stream / events are replaced by host stand-ins, and EVERY buffer scene_images
allocates (workspaces, raw images, outputs) is filled with 0xA5 and followed by guard bytes that are checked after the run.  The runs and
checks are tests/scene_images_runs.py's: tests/test_scene_images_gpu.py performs the same ones on the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import scene_images_cases as K  # noqa: E402
import scene_images_runs as R  # noqa: E402


def host_seams(SI):
    """the stand-ins for scene_images' device seams -> check() of the guards"""
    check = host_child.install_transfer_seams(SI)
    SI._side_stream = lambda: None
    SI._side_waits_for_caller = lambda side: None
    SI._copy_on = lambda side, dst, src: dst.copy_(src)
    SI._record_on = lambda side: None
    SI._wait = lambda e: None
    SI._caller_waits_for = lambda e: None
    return check


def _child(case, out):
    import torch
    import scene_images as SI
    check = host_seams(SI)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).copy())
    alloc, down = host_child.host_buffers(SI)
    tmp = os.path.join(os.path.dirname(out), "files_" + case)
    os.makedirs(tmp, exist_ok=True)
    if case.startswith("shapes:"):
        res = R.run_shapes(SI, up, alloc, down, tmp, tags=case.split(":")[1].split(","))
    else:
        res = R.RUNS[case](SI, up, alloc, down, tmp)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=600)
    assert int(res["buffers"]) > 0
    return res


GROUPS = (("clip", "half", "odd", "frac", "one"), ("noh", "nov", "same", "wide", "tall"), ("taps33", "rgba", "up", "taps257"))


@pytest.mark.parametrize("tags", GROUPS, ids=lambda t: t[0])
def test_shapes_are_the_references_bits(tmp_path, tags):
    """every shape of the table x {random bytes, 0/255 steps and impulses, constant 255}, and five of them with a row pitch that is no
    multiple of 4: bit for bit the reference's PILtoTorch of Pillow's resize"""
    assert R.check_shapes(_emulate("shapes:" + ",".join(tags), tmp_path), K.golden(), tags=tags) == 3 * len(tags)


def test_every_shape_is_in_a_group():
    assert sorted(t for g in GROUPS for t in g) == sorted(s[0] for s in K.SHAPES)


def test_all_256_byte_values(tmp_path):
    R.check_bytes(_emulate("bytes", tmp_path))


def test_workspace_contents_and_argument_errors(tmp_path):
    R.check_entry(_emulate("entry", tmp_path), K.golden())


def test_loader_pool_equals_serial(tmp_path):
    pytest.importorskip("PIL")
    R.check_loader(_emulate("loader", tmp_path))


def test_coefficient_tables_equal_the_restatement():
    """gof_image_coeffs (host only) against the numpy restatement for every axis of the table, and the tap counts the issue names"""
    import scene_images as SI
    axes = {(s[1], s[3]) for s in K.SHAPES} | {(s[2], s[4]) for s in K.SHAPES} | {(4946, 1237), (1920, 960), (65535, 1), (1, 7)}
    for n_in, n_out in sorted(axes):
        if n_in * n_out > 4e6 and n_out > 1:
            continue
        taps, bounds, coeffs = SI.coefficients(n_in, n_out)
        t2, b2, c2 = K.coefficients(n_in, n_out)
        assert taps == t2 and np.array_equal(bounds, b2) and np.array_equal(coeffs, c2), (n_in, n_out)
        assert (np.abs(coeffs.astype(np.int64)).sum(axis=1) * 255 < 2 ** 31).all()
    assert SI.coefficients(400, 100)[0] == 17 and SI.coefficients(800, 100)[0] == 33 and SI.coefficients(6400, 100)[0] == 257
    assert SI.lib.gof_image_taps(0, 5) == -1 and SI.lib.gof_image_taps(5, 65536) == -1 and SI.lib.gof_image_abi_version() == 1
    assert SI.lib.gof_abi_version() == 12


def test_live_pillow_agrees_with_the_golden():
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    g = K.golden()
    for (tag, W, H, w, h, C), kind, a in K.inputs():
        if C == 4:
            live = np.stack([np.array(b.resize((w, h))) for b in Image.fromarray(a, "RGBA").split()], axis=-1)
        else:
            live = np.array((Image.fromarray(a[..., 0], "L") if C == 1 else Image.fromarray(a, "RGB")).resize((w, h))).reshape(h, w, C)
        assert K.same_bits(live, g["bytes_%s_%s" % (tag, kind)]), "Pillow %s differs from the golden's %s at %s %s" % (PIL.__version__, g["pillow_version"], tag, kind)


def test_resolution_arithmetic():
    import scene_images as SI
    for res in (1, 2, 4, 8, 16, 64, -1, 37, 800.5):
        for scale in (1.0, 2.0):
            for W, H in ((1604, 5), (101, 67), (4946, 3286), (1600, 900)):
                assert SI.resolution_of(R.Args(res), W, H, scale) == K.resolution_of(W, H, res, scale), (res, scale, W, H)


def test_host_images_are_refused_without_a_reference_function():
    import scene_images as SI
    info = R.CamInfo(1, None, None, 0.5, 0.5, type("Im", (), {"mode": "RGB", "size": (4, 4)})(), "", "x", 4, 4)
    assert not SI.reference
    with pytest.raises(RuntimeError, match="ROCm device"):
        SI.load_cam(R.Args(1), 0, info, 1.0)


def test_golden_is_small_and_complete():
    assert os.path.getsize(K.GOLDEN) < 400 * 1024
    g = K.golden()
    assert str(g["pillow_version"])
    for (tag, W, H, w, h, C) in K.SHAPES:
        for kind in K.KINDS:
            assert g["bytes_%s_%s" % (tag, kind)].shape == (h, w, C) and g["planar_%s_%s" % (tag, kind)].shape == (C, h, w)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
