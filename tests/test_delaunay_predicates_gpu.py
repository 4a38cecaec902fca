"""GPU tests of the Delaunay predicates: the classes, the integer reference and the checks of
tests/test_delaunay_predicates_host.py on the device code of libgof_hip.so -- gfx950's f64 fma, its denormals, and what the compiler
made of the error-free transformations -- one launch of gof_debug_delaunay_predicates per (class, variant, op)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "gaussian-opacity-fields_amd")
for _p in (HERE, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_delaunay_predicates_host as H  # noqa: E402

pytestmark = pytest.mark.gpu


def _lib():
    from diff_gaussian_rasterization import _backend as B
    f = B.lib.gof_debug_delaunay_predicates
    f.restype = C.c_int
    f.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return B


def gpu_probe(P, idx, op):
    B = _lib()
    Pd = torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda()
    Id = torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda()
    out = torch.full((3, len(idx)), -0x5A5A5A5B, dtype=torch.int32, device="cuda")          # 0xA5A5A5A5
    rc = B.lib.gof_debug_delaunay_predicates(len(P), Pd.data_ptr(), len(idx), Id.data_ptr(), op, out[0].data_ptr(), out[1].data_ptr(),
                                             out[2].data_ptr(), B._stream())
    o = out.cpu().numpy()
    return rc, o[0], o[1].view(np.uint32), o[2].view(np.uint32)


@pytest.mark.parametrize("name", H.CLASSES)
def test_signs_equal_exact_arithmetic(name):
    H.check_class(name, H.run_class(gpu_probe, name))


def test_argument_errors():
    B = _lib()
    P, idx = H.case("A2")
    bad = idx[:10].copy()
    bad[7, 2] = len(P)
    rc, _, _, _ = gpu_probe(P, bad, 0)
    assert rc == H.GOF_E_INVALID and b"index" in B.lib.gof_last_error()
    assert gpu_probe(P, idx[:10], 7)[0] == H.GOF_E_INVALID
    assert gpu_probe(P, idx[:10], 0)[0] == 0
