"""The visibility cull against the reference's own code: tests/golden/tnt_cull_scene.npz holds what the unchanged
Mesher.point_masks of eval_tnt/cull_mesh.py answered on the CPU for 24 views at 64 x 48 of a mesh of 2 000 vertices
(tests/golden/make_golden_tnt_cull.py), fed the restatement's depth images.  The product renders the same images bit for bit, counts
what the fp64 restatement counts, and keeps exactly what the reference kept on every vertex the generator found decided: those whose
fp64 margins exceed the float32 rounding of the reference's own arithmetic.  At most 2 % of the vertices may be undecided."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "tnt_cull_scene.npz")


def run(M, up, down):
    g = np.load(FIXTURE)
    kw = dict(H=int(g["H"]), W=int(g["W"]), fx=float(g["fx"]), fy=float(g["fy"]), cx=float(g["cx"]), cy=float(g["cy"]))
    mesh = M.DeviceMesh.from_device(up(g["vertices"]), up(g["faces"]))
    c2w = list(g["c2w"])
    depth = M.render_depth(mesh, c2w, **kw)
    count, keep = M.visibility(mesh, c2w, eps=float(g["eps"]), min_views=int(g["min_views"]), **kw)
    against = M.visible_count(up(g["vertices"]), c2w, depth=up(g["depth"]), eps=float(g["eps"]), **kw)
    return {"depth": down(depth), "count": down(count), "keep": down(keep), "count_on_fixture_depth": down(against)}


def check(res):
    g = np.load(FIXTURE)
    assert np.array_equal(res["depth"].view(np.uint32), g["depth"].view(np.uint32))                 # the restatement's images, bit for bit
    assert np.array_equal(res["count"], g["count"]) and np.array_equal(res["count_on_fixture_depth"], g["count"])
    decided, mask = g["decided"], g["mask"]
    assert 1.0 - decided.mean() <= 0.02 and min(mask.sum(), (~mask).sum()) >= 100
    assert np.array_equal(res["keep"][decided], mask[decided])                                      # the reference's own answer
    assert np.array_equal(res["keep"], g["count"] >= int(g["min_views"]))


def _child(case, out):
    import torch
    import mesh_cull as M
    chk = host_child.install_seams(M, buffers="all")
    res = run(M, lambda a: torch.from_numpy(np.ascontiguousarray(a)), lambda t: t.detach().numpy().copy())
    res["buffers"] = np.array(chk())
    np.savez(out, **res)


def test_the_fixture_holds_data_only():
    g = np.load(FIXTURE, allow_pickle=False)
    assert os.path.getsize(FIXTURE) < 1 << 20 and all(g[k].dtype.kind in "fiub" for k in g.files)
    assert g["vertices"].shape == (2000, 3) and g["depth"].shape == (24, 48, 64) and g["mask"].shape == (2000,)


def test_the_emulated_kernels_keep_what_the_reference_kept(tmp_path):
    check(host_child.run_child(__file__, "golden", tmp_path, timeout=900))


@pytest.mark.gpu
def test_the_device_keeps_what_the_reference_kept():
    import torch
    import mesh_cull as M
    check(run(M, lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0"), lambda t: t.detach().cpu().numpy()))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
