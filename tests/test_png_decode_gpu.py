"""GPU tests of the PNG decoder: the runs and checks of tests/png_decode_cases.py -- the ones
tests/test_png_decode_host.py performs over the emulator -- through the real library; a batch of mixed sizes against the files read one
by one; two streams; the round trip through image_writer's device encoder, at 1600 x 1063 too; and read_images_for_metrics on a
renders / gt pair against Pillow + to_tensor."""
import io
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_decode_cases as K  # noqa: E402
import png_encode_cases as E  # noqa: E402
from gpu_poison import Poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
_mem = Poisoned()
alloc, down, guards_intact = _mem.alloc, _mem.down, _mem.guards_intact


def up_bytes(b):
    import torch
    v = alloc(max(len(b), 1))
    v[:len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return v


@pytest.mark.parametrize("names", K.GROUPS, ids=lambda g: g[0])
def test_files_decode_to_the_restated_bytes_and_to_tensors_planes(names):
    import torch
    import image_writer as IW
    import png_reader as R
    res = K.run_cases(R, IW, lambda t: t.cuda(), down, names)
    torch.cuda.synchronize()
    K.check_cases(res, names)


def test_corrupt_streams_fail_their_own_image_only():
    import png_reader as R
    K.check_corrupt(K.run_corrupt(R, down))


def test_workspace_contents_and_argument_errors():
    import torch
    import png_reader as R
    _mem.clear()
    res = K.run_entry(R, up_bytes, alloc, down)
    torch.cuda.synchronize()
    assert guards_intact() > 0
    K.check_entry(res)


MIXED = ("1x1", "c2", "grid_65x129", "pillow_6", "stored_65535", "300x1", "c4", "dist32768", "1x300", "fib15")


def test_a_mixed_batch_equals_the_files_read_one_by_one_on_two_streams():
    import torch
    import png_reader as R
    files = [K.build(n) for n in MIXED]
    batch = R.read_images(files)
    single = [R.read_image(f) for f in files]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = R.read_images(files)
    side.synchronize()
    for n, f, a, b, c in zip(MIXED, files, batch, single, other):
        w, h, ch = K.header(f)
        assert tuple(a.shape) == (ch, h, w) and a.dtype == torch.float32 and a.is_cuda, n
        assert torch.equal(a, b) and torch.equal(a, c), n


def test_a_small_group_budget_gives_the_same_tensors(monkeypatch):
    import torch
    import png_reader as R
    files = [K.build(n) for n in MIXED]
    whole = R.read_images(files)
    before = R.stats["groups"]
    monkeypatch.setattr(R, "GROUP_BYTES", 200000)
    parts = R.read_images(files)
    assert R.stats["groups"] - before > 2
    assert all(torch.equal(a, b) for a, b in zip(whole, parts))


@pytest.mark.parametrize("name", ["photo", "gray", "values", "block_plus_1", "workload"])
def test_round_trip_through_the_device_encoder(name):
    """image_writer.encode_png -> this decoder: the quantised bytes the encoder's tests restate; `workload` is 1600 x 1063 (a stream of
    megabytes, 17 bands)"""
    import torch
    import image_writer as IW
    import png_reader as R
    t = E._smooth(1600, 1063, 99) if name == "workload" else E.view(name, E.tensor(name))
    png = IW.encode_png(t.cuda())
    px = E.quantised(t)
    got = R.read_images([png], planes=False)[0]
    assert np.array_equal(got.cpu().numpy(), px)
    planes = R.read_image(png)
    assert torch.equal(planes.cpu(), K.to_tensor(px))
    if name != "workload":
        assert np.array_equal(K.unfilter(zlib.decompress(K.idat_of(png)), *px.shape[:2], 3), px)


def test_read_images_for_metrics_equals_pillow_and_to_tensor(tmp_path):
    """six small files in renders/ and gt/: the same names in os.listdir's order, every tensor (1, 3, H, W) on the device and bit-equal to
    to_tensor(Image.open(...)).unsqueeze(0)[:, :3]"""
    import torch
    from PIL import Image
    import png_reader as R
    renders, gt = tmp_path / "renders", tmp_path / "gt"
    renders.mkdir()
    gt.mkdir()
    for k, (a, b) in enumerate((("grid_63x63", "pillow_1"), ("pillow_6", "pillow_optimize"), ("mix", "grid_64x65"), ("pillow_1", "pillow_1"), ("c4", "pillow_6"),
                                ("grid_65x129", "band_f4"))):
        (renders / ("%05d.png" % k)).write_bytes(K.build(a))
        (gt / ("%05d.png" % k)).write_bytes(K.build(b))
    r, g, names = R.read_images_for_metrics(renders, gt)
    assert names == list(os.listdir(renders)) and len(r) == len(g) == 6
    for n, a, b in zip(names, r, g):
        for got, d in ((a, renders), (b, gt)):
            pic = Image.open(io.BytesIO((d / n).read_bytes()))
            want = K.to_tensor(np.asarray(pic)).unsqueeze(0)[:, :3, :, :]
            assert got.is_cuda and got.shape[1] == 3 and torch.equal(got.cpu(), want), n
