"""GPU tests of the mesh depth rasteriser and visibility cull: the cases and checks of tests/test_mesh_raster_host.py on
the device: every depth image, count, culled mesh and exported byte equal to tests/mesh_raster_restatement.py bit for bit; the order
of the faces, repetition and the contents of workspaces and outputs do not matter; refused input writes nothing."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mesh_raster_cases as K  # noqa: E402
import test_mesh_raster_host as T  # noqa: E402

pytestmark = pytest.mark.gpu


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _down(t):
    return t.detach().cpu().numpy()


def _alloc(nbytes):
    import torch
    return torch.empty(int(nbytes), dtype=torch.uint8, device="cuda:0")


@pytest.fixture(scope="module")
def M():
    import mesh_cull
    return mesh_cull


@pytest.mark.parametrize("size", ["%dx%d_" % s for s in K.SIZES])
def test_every_case_equals_the_restatement(M, size):
    tiling = M.raster_tiling()
    S = K.scenes(tiling)
    T.check_cases(lambda tag: K.run(M, _up, S[tag], _down), size, tiling)


def test_face_order_and_repetition_do_not_matter(M):
    V, F, views = K.scenes(M.raster_tiling())["64x48_views"]
    first = K.run(M, _up, (V, F, views), _down)
    assert K.same(first, K.want("64x48_views", M.raster_tiling())) == []
    perm = np.random.default_rng(1).permutation(len(F))
    for f in (F, F[perm], F[::-1]):
        again = K.run(M, _up, (V, f, views), _down)
        assert all(np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)) for k in first)


def test_workspace_and_output_contents_do_not_matter(M):
    tiling = M.raster_tiling()
    S = K.scenes(tiling)
    for tag in ("64x48_views", "70x33_threshold", "70x33_near_fan"):
        for fill in T.FILLS:
            got = T.run_abi(M, _alloc, _down, *S[tag], fill)
            assert got["rc"].tolist() == [0, 0, 0] and bool(got["guards"]), (tag, fill)
            assert K.same(got, K.want(tag, tiling)) == [], (tag, fill)


def test_bad_input_is_refused_with_nothing_written(M):
    V, F, views = K.scenes(M.raster_tiling())["70x33_views"]
    got = {}
    for tag, v, f, mutate, _ in T.bad_inputs(V, F):
        got.update({"%s_%s" % (tag, k): x for k, x in T.run_abi(M, _alloc, _down, v, f, views, 0x5C, mutate=mutate).items()})
    T.check_errors(got, V, F)


def test_cull_by_visibility_and_the_exported_bytes(M, tmp_path):
    T.check_cull(T.cull_runs(M, _up, _down, str(tmp_path)))


def test_statistics_count_the_two_paths(M):
    """the threshold case: two triangles are drawn by their own thread, four walk the list; nothing is refused"""
    V, F, views = K.scenes(M.raster_tiling())["64x48_threshold"]
    M.render_depth(M.DeviceMesh.from_device(_up(V), _up(F)), views["c2w"], stats=True, **K._kw(views))
    st = M.last_stats()["render_depth"]
    assert st["triangles"] == 6 and st["listed"] == 4 and st["refused_by_full_list"] == 0 and st["pixels"] == st["atomics"] == 265
