"""CPU tests of the PNG encoder: the kernels of csrc/png_encode.hip through the host emulator (tests/hipemu) behind
image_writer's own encode_png, each group of cases in a child process (an emulator abort fails one test, not the session).  The oracles
need no tolerance: Pillow decodes the file to the bytes torch computes on the CPU, zlib inflates the IDAT payload to the scanline stream
restated in tests/png_encode_cases.py (filter choice included), two encodes agree, and the stream is no longer than zlib's own Z_RLE
stream plus the derived allowance.  tests/test_png_encode_gpu.py performs the same runs on the device.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context / upload are host stand-ins, and EVERY buffer image_writer allocates (workspace, output, size word) is filled with
0xA5 and followed by guard bytes that are checked after the run."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import png_encode_cases as K  # noqa: E402


host_seams = host_child.install_transfer_seams


def _child(case, out):
    import image_writer as IW
    check = host_seams(IW)

    def up(t):
        return t.clone()
    alloc, down = host_child.host_buffers(IW)
    kind, _, names = case.partition(":")
    res = {"cases": K.run_cases, "entry": K.run_entry}[kind](IW, up, alloc, down, names.split(",") if names else None)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=600)
    assert int(res["buffers"]) > 0
    return res


@pytest.mark.parametrize("names", K.GROUPS, ids=lambda g: g[0])
def test_files_decode_to_torchs_bytes_and_streams_to_the_restated_scanlines(tmp_path, names):
    """every case: Pillow's decode equals torch's CPU arithmetic, the inflated IDAT payload equals the restated scanline stream, two
    encodes are identical, the stream is within the stored bound and (compressible cases of at least one block) within the derived
    allowance over zlib's Z_RLE stream, and the file is byte for byte the pinned one (tests/golden/png_encode_pins.json); the sizes are
    printed"""
    pytest.importorskip("PIL")
    assert len(K.check_cases(_emulate("cases:" + ",".join(names), tmp_path), names)) == len(names)


def test_every_case_is_in_a_group_and_serves_its_purpose():
    assert sorted(n for g in K.GROUPS for n in g) == sorted(K.CASES)
    K.check_purposes()
    # excluded from the size assertion: the random image and the images smaller than one block, nothing else
    for n in K.EXCLUDED:
        t = K.view(n, K.tensor(n))
        H, W = t.shape[-2:]
        assert n == "random" or H * (3 * W + 1) < K.BLOCK, n


def test_workspace_contents_and_argument_errors(tmp_path):
    K.check_entry(_emulate("entry", tmp_path))


def test_restated_scanlines_are_what_pillow_inflates_to():
    """the restatement itself: a file framed around zlib's own stream of the restated scanlines decodes to the pixels"""
    PIL = pytest.importorskip("PIL")  # noqa: F841
    import io
    import zlib
    from PIL import Image
    import image_writer as IW
    for n in ("w6", "photo", "values", "fibonacci"):
        px = K.quantised(K.tensor(n))
        png = IW.frame(px.shape[1], px.shape[0], zlib.compress(K.scanlines(px)))
        assert np.array_equal(np.array(Image.open(io.BytesIO(png))), px), n


def test_framing_splits_idat_chunks(monkeypatch):
    import zlib
    import image_writer as IW
    monkeypatch.setattr(IW, "IDAT_BYTES", 1000)
    px = K.quantised(K.tensor("photo"))
    stream = zlib.compress(K.scanlines(px), 1)
    png = IW.frame(160, 120, stream)
    kinds = [k for k, _ in K.chunks(png)]
    assert kinds.count(b"IDAT") == -(-len(stream) // 1000) > 3 and IW.stream_of(png) == stream


def test_save_image_keeps_the_stand_ins_shape_rules_and_goes_elsewhere_without_a_device(tmp_path, monkeypatch):
    import torch
    import image_writer as IW
    calls = []
    monkeypatch.setattr(IW, "previous", lambda tensor, fp, format=None, **kw: calls.append((tuple(tensor.shape), fp, format)))
    monkeypatch.setattr(IW, "_have_device", lambda: False)
    with pytest.raises(RuntimeError, match="a batch of 2 images would need make_grid"):
        IW.save_image(torch.zeros(2, 3, 4, 4), str(tmp_path / "a.png"))
    with pytest.raises(RuntimeError, match=r"expected \(C,H,W\) with C in \(1, 3, 4\), got \(2, 4, 4\)"):
        IW.save_image(torch.zeros(2, 4, 4), str(tmp_path / "a.png"))
    IW.save_image(torch.zeros(3, 4, 4), str(tmp_path / "a.png"))
    assert calls == [((3, 4, 4), str(tmp_path / "a.png"), None)]
    # with a device: jpg, a file object, four channels, another dtype and extra arguments still go to the function bound before
    monkeypatch.setattr(IW, "_have_device", lambda: True)
    import io
    IW.save_image(torch.zeros(3, 4, 4), str(tmp_path / "a.jpg"))
    IW.save_image(torch.zeros(3, 4, 4), io.BytesIO(), format="png")
    IW.save_image(torch.zeros(4, 4, 4), str(tmp_path / "b.png"))
    IW.save_image(torch.zeros(3, 4, 4, dtype=torch.float64), str(tmp_path / "c.png"))
    IW.save_image(torch.zeros(3, 4, 4), str(tmp_path / "d.png"), quality=3)
    assert len(calls) == 6
    IW.flush()


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
