"""GPU tests of the shared device-wide scan and radix sort (csrc/radix.hip) through the debug entries of libgof_hip.so: every group of
tests/prim_cases.py on the device -- those of tests/test_primitives_host.py, and the regimes that begin at 2 M / 8 M words: the sort's
histogram / scan / scatter launches against its single-kernel passes (first_hist_done with them), the scan's big tiles and its
three-launch form.  Every comparison is exact against numpy."""
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

import prim_cases as PC  # noqa: E402

pytestmark = pytest.mark.gpu


class DeviceMem:
    def __init__(self, backend):
        self.stream = backend._stream()

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()

    def down(self, h):
        return h.cpu().numpy().view(np.uint32)

    def ptr(self, h, word):
        return h.data_ptr() + 4 * word

    def sync(self):
        torch.cuda.synchronize()


@pytest.mark.parametrize("group", list(PC.GPU_GROUPS))
def test_group_equals_numpy(group):
    from diff_gaussian_rasterization import _backend as B
    assert PC.GPU_GROUPS[group](PC.bind(B.lib), DeviceMem(B)) > 0
