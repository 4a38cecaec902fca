"""CPU tests of the PNG decoder: the kernels of csrc/png_decode.hip through the host emulator (tests/hipemu) behind
png_reader's own functions, each group of cases in a child process (an emulator abort fails one test, not the session).  The oracles
need no tolerance (tests/png_decode_cases.py): scanlines == zlib.decompress, bytes == the numpy unfilter == Pillow, planes bit-equal to
to_tensor's.  tests/test_png_decode_gpu.py performs the same runs on the device.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context / pinned buffer / upload / download are host stand-ins, and EVERY buffer png_reader allocates (workspace,
outputs, status words) is filled with 0xA5 and followed by guard bytes that are checked after the run; the corrupt streams run with
those guards around every buffer."""
import io
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import png_decode_cases as K  # noqa: E402


host_seams = host_child.install_transfer_seams


def _child(case, out):
    import torch
    import image_writer as IW
    import png_reader as R
    check = host_seams(R, IW)
    alloc, down = host_child.host_buffers(R)

    def up_bytes(b):
        t = alloc(max(len(b), 1))
        t[:len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
        return t
    kind, _, names = case.partition(":")
    if kind == "cases":
        res = K.run_cases(R, IW, lambda t: t.clone(), down, names.split(","))
    elif kind == "corrupt":
        res = K.run_corrupt(R, down)
    else:
        res = K.run_entry(R, up_bytes, alloc, down)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path, **kw):
    res = host_child.run_child(__file__, case, tmp_path, timeout=600, **kw)
    assert int(res["buffers"]) > 0
    return res


_files = {}


@pytest.mark.parametrize("names", K.GROUPS, ids=lambda g: g[0])
def test_files_decode_to_the_restated_bytes_and_to_tensors_planes(tmp_path, names):
    """every case: Pillow's decode equals the numpy unfilter of zlib's scanlines equals the decoder's bytes; the planes are bit-equal to
    to_tensor's; two decodes are identical"""
    pytest.importorskip("PIL")
    _files.update(K.check_cases(_emulate("cases:" + ",".join(names), tmp_path), names))


@pytest.mark.parametrize("order", ["reverse", "random:7"])
def test_results_do_not_depend_on_the_fiber_order(tmp_path, order):
    pytest.importorskip("PIL")
    K.check_cases(_emulate("cases:" + ",".join(K.ORDER_GROUP), tmp_path, order=order), K.ORDER_GROUP)


def test_every_case_is_in_a_group_and_serves_its_purpose(tmp_path):
    assert sorted(n for g in K.GROUPS for n in g) == sorted(K.CASES)
    files = {n: K.build(n) for n in K.CASES if not K.needs_encoder(n)}
    own = [n for n in K.CASES if K.needs_encoder(n)]
    if not all(n in _files for n in own):           # (run alone: the encoder's files come from a run of their group)
        _files.update(K.check_cases(_emulate("cases:" + ",".join(own), tmp_path), own))
    files.update({n: _files[n] for n in own})
    K.check_purposes(files)


def test_corrupt_streams_fail_their_own_image_only(tmp_path):
    """every corrupt stream between good images in one batch: its status on its own image, the neighbours bit-exact, every guard intact;
    read_images raises ValueError naming the file and the reason"""
    K.check_corrupt(_emulate("corrupt", tmp_path))


def test_workspace_contents_and_argument_errors(tmp_path):
    K.check_entry(_emulate("entry", tmp_path))


def test_restated_unfilter_is_pillows_on_pillows_own_files():
    pytest.importorskip("PIL")
    for c, seed in ((1, 1), (2, 2), (3, 3), (4, 4)):
        for kw in (dict(compress_level=1), dict(optimize=True)):
            px = K._noisy(37, 41, c, seed) if seed % 2 else K._random(37, 41, c, seed)
            f = K.pillow_file(px, **kw)
            w, h, cc = K.header(f)
            assert (w, h, cc) == (41, 37, c)
            assert np.array_equal(K.unfilter(zlib.decompress(K.idat_of(f)), h, w, cc), px)


def test_parse_walks_the_chunks_and_names_what_it_does_not_take():
    import png_reader as R
    f = K.build("ancillary")
    p = R.parse(f)
    assert (p.width, p.height, p.channels, p.bit_depth, p.color_type, p.interlace, p.not_taken) == (14, 12, 3, 8, 2, 0, None)
    assert len(p.payloads) > 3 and p.stream == K.idat_of(f) and p.stream_bytes == len(p.stream)
    one = R.parse(K.build("idat_1byte"))
    assert len(one.payloads) == one.stream_bytes and one.stream == R.parse(K.build("idat_one")).stream
    for name, (data, why) in K.not_taken_files().items():
        assert R.parse(data).not_taken == why, name
    wide = K.frame(65536, 1, 1, zlib.compress(bytes(65537)))
    assert R.parse(wide).not_taken == "65536 x 1 pixels"


def test_parse_raises_for_a_corrupt_file(tmp_path):
    import png_reader as R
    f = K.build("idat_one")
    path = tmp_path / "x.png"
    crc = bytearray(f)
    crc[40] ^= 1                                    # a byte of the IDAT data
    cases = {"signature": b"\x88" + f[1:], "CRC-32": bytes(crc), "file ends": f[:-20], "cut off": f[:-3], "no IHDR or no IEND": f[:-12],
             "not IHDR": f[:8] + f[33:], "no IDAT": f[:33] + f[-12:],
             "IHDR": f[:8] + K.chunk(b"IHDR", struct.pack(">IIBBBBB", 14, 12, 8, 5, 0, 0, 0)) + f[33:]}
    for text, data in cases.items():
        path.write_bytes(data)
        with pytest.raises(ValueError, match=text) as e:
            R.parse(path)
        assert str(path) in str(e.value)
    assert io.BytesIO(f).read(8) == R.SIGNATURE


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
