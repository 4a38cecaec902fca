"""GPU tests of the model file: the runs and checks of tests/model_io_runs.py -- the ones tests/test_model_io_host.py
performs over the emulator -- through the real library at the same small shapes, every tensor lying inside a larger poisoned allocation
(sources of the unpack at an ODD byte offset: the byte-assembling loads), and one model of 100 003 Gaussians through many chunks, the
two staging buffers and a stream that is not the default one.  Reads the committed golden only; no reference code runs here."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_io_cases as K  # noqa: E402
import model_io_runs as R  # noqa: E402
from gpu_poison import Poisoned  # noqa: E402

pytestmark = pytest.mark.gpu
_mem = Poisoned()
down, guards_intact = _mem.down, _mem.guards_intact


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    return _mem.up(torch.from_numpy(a), offset=1 if a.dtype == np.uint8 else 0)          # (file bytes: an odd address)


def alloc(shape):
    import torch
    return _mem.alloc(int(np.prod(shape)) * 4).view(torch.float32).reshape(tuple(shape))


@pytest.fixture(scope="module")
def golden():
    return K.golden()


def _run(case, tmp_path):
    import torch
    import model_io as MIO
    _mem.clear()
    res = R.RUNS[case](MIO, up, alloc, down, str(tmp_path))
    torch.cuda.synchronize()
    assert guards_intact() > 0
    return res


def test_raw_rows_are_the_references_bytes(tmp_path, golden):
    R.check_raw(_run("raw", tmp_path), golden)


def test_unpack_gives_the_references_tensors(tmp_path, golden):
    R.check_unpack(_run("unpack", tmp_path), golden)


def test_files_round_trip_bit_for_bit(tmp_path, golden):
    R.check_files(_run("files", tmp_path), golden)


def test_fused_rows(tmp_path, golden):
    R.check_fused(_run("fused", tmp_path), golden)


def test_bad_files_and_arguments_are_refused(tmp_path):
    R.check_errors(_run("errors", tmp_path))


def test_fused_columns_are_the_activations_own_bits():
    """o and s of the fused file come from the device functions behind gof_act_opacity / gof_act_scaling: log(o / (1 - o)) and log(s)
    of what train_epilogue.activations returns, rounded once more by logf, lie within 2 ulp of the file's columns"""
    import torch
    import model_io as MIO
    from train_epilogue import activations as A
    m = K.make_model(3, 1000, 31)
    ts = [torch.from_numpy(m[f]).cuda() for f in K.FIELDS]
    rows = MIO.pack_rows(ts, mode=MIO.FUSED)
    g = R.Model(3)
    g._opacity, g._scaling, g.filter_3D = ts[3], ts[4], ts[6]
    with torch.no_grad():
        o = A.get_opacity_with_3D_filter(g)
        s = A.get_scaling_with_3D_filter(g)
    want_o, want_s = torch.log(o / (1.0 - o)), torch.log(s)
    got_o, got_s = rows[:, 54:55], rows[:, 55:58]
    ulp = lambda a, b: ((a.view(torch.int32) - b.view(torch.int32)).abs().max().item())        # noqa: E731  (same sign, finite)
    assert ulp(got_o.contiguous(), want_o.contiguous()) <= 2 and ulp(got_s.contiguous(), want_s.contiguous()) <= 2


def test_many_chunks_on_a_side_stream(tmp_path):
    """P = 100 003 in chunks of 4 099 rows (25 chunks, the last one short, neither a multiple of the tile) on a non-default stream:
    the file is the layout's bytes, and loads back bit for bit"""
    import torch
    import model_io as MIO
    P = 100003
    m = K.make_model(3, P, 9)
    m["xyz"].view(np.uint32)[:5, 0] = [0x80000000, 0x7FC12345, 0x00000001, 0xFF800000, 0x7F800001]
    want = K.header(P, K.names(15)) + K.raw_rows(m).tobytes()
    g = R.model_of(m, lambda a: torch.from_numpy(a).cuda())
    path = str(tmp_path / "iteration_7000" / "point_cloud.ply")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with R.chunk_rows(4099), torch.cuda.stream(side):
        MIO.save_ply(g, path)
        assert MIO.last_stats()["save"]["chunks"] == 25
        with open(path, "rb") as fh:
            assert fh.read() == want
        h = R.Model(3)
        MIO.load_ply(h, path)
        assert MIO.last_stats()["load"]["chunks"] == 25
    side.synchronize()
    got = R.arrays_of(h, down)
    for f in K.FIELDS:
        assert K.same_bits(got[f], m[f]), f
    assert h._xyz.requires_grad and isinstance(h._features_rest, torch.nn.Parameter) and h.active_sh_degree == 3 and h._xyz.is_cuda
