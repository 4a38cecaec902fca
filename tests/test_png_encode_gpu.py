"""GPU tests of the PNG encoder: the runs and checks of tests/png_encode_cases.py -- the ones
tests/test_png_encode_host.py performs over the emulator -- through the real library, every input lying inside a larger poisoned
allocation, on the default stream and on a side stream; and image_writer's pipeline: more files than pinned buffers, a host tensor, what
goes to the function bound before, and a writer-thread error that surfaces from flush()."""
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_encode_cases as K  # noqa: E402
from gpu_poison import Poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
_mem = Poisoned()
up, alloc, down, guards_intact = _mem.up, _mem.alloc, _mem.down, _mem.guards_intact


@pytest.mark.parametrize("names", K.GROUPS, ids=lambda g: g[0])
def test_files_decode_to_torchs_bytes_and_streams_to_the_restated_scanlines(names):
    """every check of the emulated run, the pinned bytes (tests/golden/png_encode_pins.json) included: the device writes the emulator's file"""
    import torch
    import image_writer as IW
    _mem.clear()
    res = K.run_cases(IW, up, alloc, down, names)
    torch.cuda.synchronize()
    assert guards_intact() > 0
    assert len(K.check_cases(res, names)) == len(names)


def test_workspace_contents_and_argument_errors():
    import torch
    import image_writer as IW
    _mem.clear()
    res = K.run_entry(IW, up, alloc, down)
    torch.cuda.synchronize()
    assert guards_intact() > 0
    K.check_entry(res)


def test_a_side_stream_gives_the_same_bytes():
    import torch
    import image_writer as IW
    names = ("photo", "black", "random", "mono", "strided")
    first = K.run_cases(IW, up, alloc, down, names)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = K.run_cases(IW, up, alloc, down, names)
    side.synchronize()
    assert guards_intact() > 0
    for n in names:
        assert first["png_" + n].tobytes() == second["png_" + n].tobytes(), n
        K.check_pin(n, first["png_" + n].tobytes())


def test_save_image_pipelines_more_files_than_buffers(tmp_path):
    """ten files through RING = 3 pinned buffers, device and host tensors, shapes (3,H,W), (1,H,W), (H,W), (1,3,H,W): every file equals
    encode_png's bytes; jpg and a file object go to the function bound before"""
    import torch
    import image_writer as IW
    names = ["photo", "black", "mono", "w6", "random", "gray", "values", "mono2d", "strided", "1x1"]
    before = dict(IW.stats)
    want = {}
    for i, n in enumerate(names):
        t = K.tensor(n)
        want[n] = IW.encode_png(K.view(n, t.cuda()))
        src = K.view(n, t if i % 3 == 2 else t.cuda())          # every third one from the host (--data_device cpu)
        if n == "photo":
            src = src[None]
        IW.save_image(src, str(tmp_path / (n + ".png")) if i % 2 else tmp_path / (n + ".png"))
    calls = []
    keep = IW.previous
    IW.previous = lambda tensor, fp, format=None, **kw: calls.append(fp)
    try:
        IW.save_image(K.tensor("w6").cuda(), str(tmp_path / "x.jpg"))
        IW.save_image(K.tensor("w6").cuda(), io.BytesIO(), format="png")
    finally:
        IW.previous = keep
    IW.flush()
    assert len(calls) == 2 and IW.stats["device"] - before["device"] == len(names)
    for n in names:
        assert (tmp_path / (n + ".png")).read_bytes() == want[n], n
    assert torch.cuda.is_available()


def test_a_writer_error_surfaces_from_flush(tmp_path):
    import image_writer as IW
    IW.flush()
    IW.save_image(K.tensor("w6").cuda(), str(tmp_path / "no_such_directory" / "a.png"))
    IW.save_image(K.tensor("w5").cuda(), str(tmp_path / "b.png"))
    with pytest.raises(OSError):
        IW.flush()
    assert (tmp_path / "b.png").read_bytes() == IW.encode_png(K.tensor("w5").cuda())     # the thread went on with the next file
    IW.flush()                                                                           # the error was reported once
