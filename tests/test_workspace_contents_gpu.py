"""include/gof_hip.h: "workspaces may hold anything on entry unless stated" -- on the GPU, through the product binding.  The binding
allocates every workspace and every fully-written output with torch.empty: the caching allocator's recycled memory, so a kernel that
read a word before anything of this frame wrote it would show as a rare, non-reproducible mismatch.  Here the allocations of ONE call
are replaced (monkeypatched _View.bytes_tensor and torch.empty) by buffers filled with 0xA5 or 0xFF, or by buffers that just served a
complete frame of a larger scene at another resolution, and forward (two-stage and sync-free), backward and the opacity-field query
must give the bits of the same calls on zero-filled buffers -- the backward is bit-reproducible (no atomics), so equality is the bar.
Ordinary calls on initialised memory; nothing is measured.  The CPU counterpart with every entry point: tests/test_workspace_contents.py."""
import numpy as np
import pytest
import torch

import synthetic_scenes as S
import test_parity_gpu as TP
from gpu_common import fetch, product_forward_raw, to_dev

pytestmark = pytest.mark.gpu

TABLES = ["ranges", "point_list", "point_list_keys", "final_T", "n_contrib", "contrib_hash", "tile_cost"]


class contents:
    """with contents(policy): every workspace (_View.bytes_tensor) and every torch.empty of the binding's calls inside the block holds
    `policy`: "zero", "0xA5", "0xFF", or "stale" -- a workspace is then the front of a buffer the donor frame used (recycled, not
    copied; the largest first), other tensors are 0xA5"""

    def __init__(self, policy, donor_buffers=()):
        self.policy = policy
        self.value = {"zero": 0, "0xA5": 0xA5, "0xFF": 0xFF, "stale": 0xA5}[policy]
        self.free = sorted(donor_buffers, key=lambda t: -t.numel())

    def __enter__(self):
        from diff_gaussian_rasterization import _backend as B
        self.B, self.real_empty, self.real_bytes = B, torch.empty, B._View.bytes_tensor
        real_empty, value, ctx = self.real_empty, self.value, self

        def empty(*a, **k):
            t = real_empty(*a, **k)
            if t.is_cuda and t.numel():
                t.view(-1).view(torch.uint8).fill_(value)
            return t

        def bytes_tensor(view, n):
            n = int(n)
            if ctx.policy == "stale" and ctx.free and ctx.free[0].numel() >= n > 0:
                return ctx.free.pop(0)[:n]
            return empty(n, dtype=torch.uint8, device=view.device)

        torch.empty = empty
        B._View.bytes_tensor = bytes_tensor
        return self

    def __exit__(self, *exc):
        torch.empty = self.real_empty
        self.B._View.bytes_tensor = self.real_bytes
        return False


class recorded:
    """with recorded() as r: the workspaces the binding allocates inside the block are kept in r.buffers (the donor frame of `stale`)"""

    def __enter__(self):
        from diff_gaussian_rasterization import _backend as B
        self.B, self.real_bytes, self.buffers = B, B._View.bytes_tensor, []
        real, keep = self.real_bytes, self.buffers

        def bytes_tensor(view, n):
            t = real(view, n)
            keep.append(t)
            return t

        B._View.bytes_tensor = bytes_tensor
        return self

    def __exit__(self, *exc):
        self.B._View.bytes_tensor = self.real_bytes
        return False


def _forget_learnt_sizes():
    """the binding sizes its pools from earlier frames of a shape: every run starts from the same (empty) knowledge"""
    from diff_gaussian_rasterization import _backend as B
    for d in (B._capacity, B._mask_need, B._staged_need, B._recent_P):
        d.clear()


def _frame(sd, pts, out=None, tag=""):
    """two frames of one view -- the first runs the two-stage forward, the second the sync-free one on the capacity the first taught --
    each with its backward, then the opacity-field query; -> {name: numpy array}"""
    from diff_gaussian_rasterization import _backend as B
    out = {} if out is None else out
    _forget_learnt_sizes()
    g = torch.Generator(device="cpu").manual_seed(3)
    dL = torch.randn((9, sd["H"], sd["W"]), generator=g).to(sd["means3D"].device)
    for frame in ("two-stage", "sync-free"):
        res = product_forward_raw(sd, fused=True)
        a = res["args"]
        out["%s %s color" % (tag, frame)] = res["color"].cpu().numpy()
        out["%s %s radii" % (tag, frame)] = res["radii"].cpu().numpy()
        R = int(res["R"])
        for name in TABLES:
            t = fetch(res, name)
            out["%s %s table:%s" % (tag, frame, name)] = t[:R] if name.startswith("point_list") else t
        grads = B.rasterize_gaussians_backward(a[0], a[1], res["radii"], a[2], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], dL,
                                               a[17], a[18], a[19], res["geom"], res["R"], res["binning"], res["img"], False)
        names = ("means2D", "colors", "opacity", "means3D", "cov3D", "sh", "scales", "rotations", "view2gaussian")
        for k, v in zip(names, grads):
            out["%s %s grad:%s" % (tag, frame, k)] = v.cpu().numpy().copy()
    assert B._stats["two_stage_frames"] >= 1
    q = B.integrate_gaussians_to_points(a[0], pts, a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13], a[14], a[15], a[16],
                                        a[17], a[18], a[19], False, False)
    for k, v in zip(("image", "alpha", "color at points", "radii"), q[1:5]):
        out["%s query %s" % (tag, k)] = v.cpu().numpy().copy()
    torch.cuda.synchronize()
    return out


def _points(sc, most):
    pts = np.ascontiguousarray(S.tetra_points(sc), dtype=np.float32)
    if len(pts) > most:
        pts = pts[np.random.default_rng(3).choice(len(pts), most, replace=False)]
    return torch.from_numpy(pts).cuda()


def _assert_same_bits(got, want, what):
    assert list(got) == list(want)
    bad = [k for k in want if got[k].shape != want[k].shape or not np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8))]
    assert not bad, (what, "differ from the run on zero-filled buffers", bad)


def _donor_buffers():
    """a complete frame (forward, backward, query) of a scene with more Gaussians and instances than the table's, at another resolution"""
    sc = S.scene_frustum(200_000, W=1008, H=624, focal=700.0, seed=8, sigma_px=4.0)
    with recorded() as r:
        _frame(to_dev(sc), _points(sc, 100_000))
    return r.buffers


def _check(sc, policies, most_points):
    sd, pts = to_dev(sc), _points(sc, most_points)
    with contents("zero"):
        want = _frame(sd, pts)
    assert (want[" sync-free radii"] > 0).any() and np.isfinite(want[" sync-free color"]).all()
    for policy in policies:
        donor = _donor_buffers() if policy == "stale" else ()
        with contents(policy, donor):
            got = _frame(sd, pts)
        _assert_same_bits(got, want, policy)


@pytest.mark.parametrize("name", ["ragged", "long_lists", "posed_mod2", "clustered150k"])
def test_forward_backward_and_query_do_not_depend_on_what_their_buffers_held(name):
    _check(TP.SCENES[name](), ("0xA5", "0xFF", "stale"), 200_000)


def test_forward_backward_and_query_do_not_depend_on_what_their_buffers_held_at_1m_gaussians():
    """BASELINE config 2's scene (1M Gaussians, 1600x1063, 8.8 M instances: the tile sort as histogram / scan / scatter launches), once"""
    _check(S.scene_frustum(1_000_000, seed=0), ("0xA5",), 500_000)
