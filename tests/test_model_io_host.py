"""CPU tests of the model file: the kernels of csrc/model_io.hip through the host emulator (tests/hipemu) behind
model_io's own Python layer, each group of cases in a child process (an emulator abort fails one test, not the session), held to the
reference through the committed golden (tests/golden/ref_model_ply_golden.npz, written by tests/golden/make_golden_ply.py from the
reference's own save_ply / save_fused_ply / load_ply) and to the layout restated in tests/model_io_cases.py.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context / pinned allocation / events are replaced by host stand-ins, and EVERY buffer model_io allocates (staging
buffers, outputs, destinations) is filled with 0xA5 and followed by guard bytes that are checked after the run.  The runs and checks are
tests/model_io_runs.py's: tests/test_model_io_gpu.py performs the same ones on the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import model_io_cases as K  # noqa: E402
import model_io_runs as R  # noqa: E402


def _child(case, out):
    import torch
    import model_io as MIO
    check = host_child.install_seams(MIO, buffers="all")
    MIO._have_device = lambda: True
    MIO._pinned = lambda n, dtype: MIO.torch.empty(n, dtype=dtype)
    MIO._record = lambda: None
    MIO._wait = lambda e: None

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).copy())

    def alloc(shape):
        return MIO.torch.empty(tuple(shape), dtype=torch.float32)

    def down(t):
        return t.detach().numpy().copy()
    tmp = os.path.join(os.path.dirname(out), "files_" + case)
    os.makedirs(tmp, exist_ok=True)
    res = R.RUNS[case](MIO, up, alloc, down, tmp)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=600)
    assert int(res["buffers"]) > 0
    return res


def test_raw_rows_are_the_references_bytes(tmp_path):
    """save_ply's rows for the golden's five models, P in {0, 1, 63, 64, 65, 129}, sub-ranges, three chunk lengths -> one file; the
    normals written as +0.0 over poison; nothing written behind the rows"""
    R.check_raw(_emulate("raw", tmp_path), K.golden())


def test_unpack_gives_the_references_tensors(tmp_path):
    """load_ply's tensors bit for bit: the plain file, float64 opacity and scale, a shuffled property order behind an extra uchar (every
    offset odd, the pitch no multiple of 4, the last row ending the buffer), a sub-range"""
    R.check_unpack(_emulate("unpack", tmp_path), K.golden())


def test_files_round_trip_bit_for_bit(tmp_path):
    """load_ply(save_ply(model)) for every golden model and one with -0.0, denormals, infinities and NaN payloads; files exchanged with
    tests/e2e_shims/plyfile.py in both directions; an ASCII file"""
    R.check_files(_emulate("files", tmp_path), K.golden())


def test_fused_rows(tmp_path):
    """save_fused_ply: moved columns byte-equal to the golden; sigmoid64(opacity) and exp64(scale) within 3e-6 + roundtrip_rel (relative) of
    the golden's activated tensors; two runs and two chunk lengths identical"""
    R.check_fused(_emulate("fused", tmp_path), K.golden())


def test_bad_files_and_arguments_are_refused(tmp_path):
    R.check_errors(_emulate("errors", tmp_path))


def test_header_text():
    """character for character what plyfile emits for one element of float32 properties"""
    import model_io
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\n" + "".join("property float %s\n" % n for n in
            ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "f_rest_0", "f_rest_1", "f_rest_2", "f_rest_3", "f_rest_4", "f_rest_5",
             "f_rest_6", "f_rest_7", "f_rest_8", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3", "filter_3D"])
            + "end_header\n")
    assert model_io.header_bytes(7, model_io.attribute_names(3)).decode("ascii") == want
    assert model_io.attribute_names(3, fused=True) == model_io.attribute_names(3)[:-1]
    assert len(model_io.attribute_names(15)) == 63 and len(model_io.attribute_names(0)) == 18
    assert model_io.channel_names(15) == [n for n in K.names(15) if n[0] != "n"]


def test_header_parser(tmp_path):
    import model_io
    p = str(tmp_path / "h.ply")
    with open(p, "wb") as fh:
        fh.write(b"ply\r\nformat binary_little_endian 1.0\r\ncomment a\r\nobj_info b\r\nelement vertex 2\r\nproperty uchar flag\r\n"
                 b"property float64 x\r\nproperty ushort s\r\nelement face 0\r\nproperty list uchar int vertex_indices\r\nend_header\r\nBODY")
    h = model_io.read_header(p)
    assert h["format"] == "binary_little_endian" and h["data_offset"] == os.path.getsize(p) - 4
    assert h["elements"] == [("vertex", 2, [("flag", "uchar"), ("x", "float64"), ("s", "ushort")]), ("face", 0, [("vertex_indices", "list")])]
    with open(p, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\n")
    with pytest.raises(ValueError, match="end_header"):
        model_io.read_header(p)
    with open(p, "wb") as fh:
        fh.write(b"plx\nend_header\n")
    with pytest.raises(ValueError, match="not a PLY file"):
        model_io.read_header(p)
    # the reference's name rules: suffix order, not file order
    props = [(n, "float") for n in reversed(K.names(3))]
    Kc, pitch, cols = model_io.model_columns(props, 1)
    assert (Kc, pitch) == (3, 108) and cols[0] == (4 * 26, 0) and cols[6] == (4 * (26 - 9), 0) and cols[-1] == (0, 0)


def test_size_queries_and_argument_checks():
    import model_io
    L = model_io.lib
    assert L.gof_model_row_floats(15, 0) == 63 and L.gof_model_row_floats(15, 1) == 62 and L.gof_model_row_floats(0, 0) == 18
    assert L.gof_model_row_floats(25, 0) == -1 and L.gof_model_row_floats(-1, 0) == -1 and L.gof_model_row_floats(3, 2) == -1
    assert L.gof_model_channels(15) == 60 and L.gof_model_channels(24) == 87 and L.gof_model_channels(25) == -1
    none7 = [None] * 7
    assert L.gof_model_pack(0, 15, 0, 0, *none7, 0, None, None) == 0
    assert L.gof_model_pack(10, 15, 0, 10, *none7, 0, None, None) < 0 and b"NULL" in L.gof_last_error()
    assert L.gof_model_pack(10, 15, 4, 7, *none7, 0, None, None) < 0 and b"do not lie inside" in L.gof_last_error()
    assert L.gof_model_pack(2 ** 31, 15, 0, 0, *none7, 0, None, None) < 0
    tab = model_io.column_table(K.channel_offsets(15))
    assert L.gof_model_unpack(0, 15, 0, 0, None, 252, tab, *none7, None) == 0
    assert L.gof_model_unpack(5, 15, 0, 5, None, 252, tab, *none7, None) < 0 and b"NULL" in L.gof_last_error()
    assert L.gof_model_unpack(5, 15, 0, 5, None, 0, tab, *none7, None) < 0 and b"pitch" in L.gof_last_error()
    assert L.gof_model_unpack(5, 15, 0, 5, None, 251, tab, *none7, None) < 0 and b"does not lie inside a row" in L.gof_last_error()
    assert L.gof_model_unpack(5, 15, 0, 5, None, 252, None, *none7, None) < 0 and b"column table" in L.gof_last_error()


def test_host_models_are_refused_without_a_reference_method(tmp_path):
    import torch
    import model_io
    g = R.model_of(K.golden_model("d1"), lambda a: torch.from_numpy(a.copy()))
    assert not model_io.reference
    with pytest.raises(RuntimeError, match="ROCm device"):
        model_io.save_ply(g, str(tmp_path / "x.ply"))
    with pytest.raises(RuntimeError, match="ROCm device"):
        model_io.pack_rows(R.tensors_of(K.golden_model("d1"), lambda a: torch.from_numpy(a.copy())))
    assert not os.path.exists(str(tmp_path / "x.ply"))


def test_golden_is_small_and_complete():
    assert os.path.getsize(K.GOLDEN) < 200 * 1024
    g = K.golden()
    for tag, d, P in K.GOLDEN_MODELS:
        Kc = (d + 1) ** 2 - 1
        assert g[tag + "_raw"].size == P * 4 * (18 + 3 * Kc) and g[tag + "_fused"].size == P * 4 * (17 + 3 * Kc)
        assert 0 < float(g[tag + "_roundtrip_rel"]) < 1e-6
        # raw opacities reach both ends without saturating: the activated opacity spans orders of magnitude and stays inside (0, 1)
        assert 0 < g[tag + "_act_opacity"].min() and g[tag + "_act_opacity"].max() < 1
    assert g["big_act_opacity"].min() < 1e-3 and g["big_act_opacity"].max() > 0.8


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
