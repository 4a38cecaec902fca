"""GPU tests of the scene images: the runs and checks of tests/scene_images_runs.py -- the ones
tests/test_scene_images_host.py performs over the emulator -- through the real library at the same small shapes, every source lying inside
a larger poisoned allocation (every second one at an ODD address: the byte-assembling loads), a non-default stream, the staging buffers
forced small, and the loader against the reference's own loadCam with the real Camera where the reference's scripts are staged.  Reads
the committed golden only."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import scene_images_cases as K  # noqa: E402
import scene_images_runs as R  # noqa: E402
from gpu_poison import Poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
REF = os.path.join(ROOT, "oracle", "_ref", "refpy")
_mem = Poisoned()
alloc, down, guards_intact = _mem.alloc, _mem.down, _mem.guards_intact
_count = [0]


def up(a):
    import torch
    _count[0] += 1
    return _mem.up(torch.from_numpy(np.ascontiguousarray(a)), offset=_count[0] & 1)       # (every second source at an odd address)


@pytest.fixture(scope="module")
def golden():
    return K.golden()


def _run(case, tmp_path, guarded=True):
    import torch
    import scene_images as SI
    _mem.clear()
    res = R.RUNS[case](SI, up, alloc, down, str(tmp_path))
    torch.cuda.synchronize()
    assert guards_intact() > 0 or not guarded          # (the loader's run allocates everything itself)
    return res


def test_shapes_are_the_references_bits(tmp_path, golden):
    assert R.check_shapes(_run("shapes", tmp_path), golden) == 3 * len(K.SHAPES)


def test_all_256_byte_values(tmp_path):
    R.check_bytes(_run("bytes", tmp_path))


def test_workspace_contents_and_argument_errors(tmp_path, golden):
    R.check_entry(_run("entry", tmp_path), golden)


def test_a_side_stream_gives_the_same_bits(tmp_path, golden):
    import torch
    import scene_images as SI
    tags = ("odd", "wide", "rgba", "same")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _mem.clear()
    with torch.cuda.stream(side):
        res = R.run_shapes(SI, up, alloc, down, str(tmp_path), tags=tags)
    side.synchronize()
    assert guards_intact() > 0
    assert R.check_shapes(res, golden, tags=tags) == 3 * len(tags)


def test_loader_pool_equals_serial(tmp_path):
    pytest.importorskip("PIL")
    import scene_images as SI
    keep = (SI._camera_class, SI.reference)
    try:
        R.check_loader(_run("loader", tmp_path, guarded=False))
    finally:
        SI._camera_class, SI.reference = keep


def test_small_staging_buffers_are_reused(tmp_path):
    """five 300 x 200 RGB images through staging buffers of 50 000 bytes: 4 chunks per image, both buffers written ten times"""
    pytest.importorskip("PIL")
    import scene_images as SI
    rng = np.random.default_rng(5)
    px = [rng.integers(0, 256, (200, 300, 3), dtype=np.uint8) for _ in range(5)]
    infos = R.write_scene(str(tmp_path / "five"), files=[("im%d" % i, "RGB", p) for i, p in enumerate(px)])
    keep = (SI._camera_class, SI.STAGE_BYTES)
    SI._camera_class, SI.STAGE_BYTES = (lambda: R.RecordingCamera), 50000
    try:
        cams = SI.camera_list_from_cam_infos(infos, 1.0, R.Args(2))
    finally:
        SI._camera_class, SI.STAGE_BYTES = keep
    st = SI.last_stats()
    assert st["chunks"] == 20 and st["bytes"] == 5 * 180000 and st["native"] == 5
    for i, c in enumerate(cams):
        assert c.fields["uid"] == i and c.gt_alpha_mask is None and c.image.is_cuda
        assert K.same_bits(down(c.image), K.planar(K.resize_bytes(px[i], 150, 100))), i


@pytest.mark.skipif(not os.path.isdir(REF), reason="oracle/_ref/refpy not staged (build() stages it where the reference exists)")
def test_cameras_equal_the_references_with_the_real_camera(tmp_path):
    """the reference's loadCam and load_cam, both with the reference's own Camera: original_image, gt_alpha_mask and the sizes bit for bit"""
    pytest.importorskip("PIL")
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(HERE, "test_scene_images_launcher.py"), "real_camera", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "rc %d:\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "RESULT ok" in r.stdout, r.stdout[-2000:]
