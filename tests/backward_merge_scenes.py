"""Hand-built scenes for the backward blend's entry merging (csrc/blend_backward.hip, GOF_BW_MERGE), shared by
tests/test_backward_merge_gpu.py and tests/test_backward_merge_hipemu.py.

A wave of the backward is an 8x8 pixel quadrant of a 16x16 tile and walks the tile list back to front; two consecutive visited
entries of a mask word (32 list positions, aligned to the list start) ride in one trip when no lane contributes to both.  The
scenes put isotropic splats of sigma = 1 px at chosen pixels and depths of ONE tile: with an opacity of 0.02 a splat reaches
alpha >= 1/255 only within 1.8 px of its centre (0.02 exp(-r^2 / 2) >= 1/255), a 3x3 block of pixels, so which lanes an entry has is
known by construction; the list position of a splat is the number of nearer splats of the tile (fillers, all on one spot of another
quadrant: they share every lane, none of them merges).  At 70x50 the tile is the image's last column of tiles, where pixels 70 .. 79
do not exist: part of every wave is outside the image."""
import numpy as np

import synthetic_scenes as S

FOCAL = 400.0          # (long: the splats sit up to 35 px off the axis, and a footprint stretches radially by 1 / cos^2 of that angle)
SIZES = ((64, 48), (70, 50))
NAMES = ("pair", "share_pixel", "word_boundary", "batch_boundary", "chain3", "depth_branch", "two_waves", "long_list")
# merged trips of one backward call (counter [11] of the -DGOF_STATS build) where the construction fixes them
MERGED_TRIPS = {"pair": 1, "chain3": 1, "share_pixel": 0, "word_boundary": 0, "batch_boundary": 0}


def _build(W, H, splats):
    """splats: (u, v, z, sigma_px, opacity) -- image position of the centre in pixels (pixel i spans [i, i + 1)), depth"""
    P = len(splats)
    sc = S.scene_frustum(P, W=W, H=H, focal=FOCAL, seed=77)
    a = np.asarray(splats, np.float64)
    u, v, z, sig, op = a.T
    sc["means3D"] = np.stack([(u - W / 2) / FOCAL * z, (v - H / 2) / FOCAL * z, z], 1).astype(np.float32)
    sc["scales"] = np.repeat((sig * z / FOCAL)[:, None], 3, 1).astype(np.float32)
    sc["rotations"] = np.tile(np.asarray([1.0, 0.0, 0.0, 0.0], np.float32), (P, 1))
    sc["opacities"] = op[:, None].astype(np.float32)
    return sc


def _fillers(n, ox, oy):
    return [(ox + 1.5, oy + 12.5, 2.0 + 0.01 * i, 1.0, 0.02) for i in range(n)]


def scene(name, W, H):
    ox, oy = (16, 16) if W == 64 else (64, 16)            # the quadrant the entries under test lie in (wave 0 of its tile)
    bx = 5.5 if W == 64 else 4.5                          # (70 wide: columns 64 .. 69 exist)
    A = (ox + 1.5, oy + 1.5, 6.0, 1.0, 0.02)              # the farther one: walked first
    B = (ox + bx, oy + 5.5, 5.0, 1.0, 0.02)
    if name == "pair":                                    # opposite corners of the quadrant, different depths: one merged trip
        return _build(W, H, [A, B])
    if name == "share_pixel":                             # the same pair moved to share pixels: two trips
        return _build(W, H, [A, (ox + 2.5, oy + 2.5, 5.0, 1.0, 0.02)])
    if name == "word_boundary":                           # list positions 32 and 31: two mask words
        return _build(W, H, _fillers(31, ox, oy) + [A, B])
    if name == "batch_boundary":                          # list positions 64 and 63: two batches
        return _build(W, H, _fillers(63, ox, oy) + [A, B])
    if name == "chain3":                                  # three mutually disjoint entries: the first two merge, the third walks alone
        return _build(W, H, [(ox + 1.5, oy + 1.5, 7.0, 1.0, 0.02), (ox + bx, oy + 1.5, 6.0, 1.0, 0.02), (ox + 1.5, oy + 5.5, 5.0, 1.0, 0.02)])
    if name == "depth_branch":                            # B opaque enough to be the median-depth contributor of its pixels
        return _build(W, H, [A, (ox + bx, oy + 5.5, 5.0, 1.0, 0.6)])
    if name == "two_waves":                               # B reaches into the quadrant below: wave 0 merges it with A, wave 2 visits it alone
        return _build(W, H, [A, (ox + bx, oy + 7.5, 5.0, 1.0, 0.02)])
    if name == "long_list":                               # 262 entries: a pair at positions 101 / 102, one at 260 / 261 (second mask chunk of the forward)
        # (the fillers cycle over four spots of the quadrant below -- 65 deep per pixel, the depth the oracle bars were measured at --
        # so neighbours in the list are disjoint too: merged trips all along the walk)
        spots = [(ox + 1.5, oy + 9.5), (ox + 4.5, oy + 13.5), (ox + 4.5, oy + 9.5), (ox + 1.5, oy + 13.5)]
        fill = [(spots[i % 4][0], spots[i % 4][1], 2.0 + 0.01 * i, 1.0, 0.02) for i in range(258)]
        return _build(W, H, fill + [(A[0], A[1], 3.006, 1.0, 0.02), (B[0], B[1], 3.003, 1.0, 0.02), A, B])
    raise KeyError(name)


def fuzz_scene(seed):
    return S.scene_frustum(2000, W=128, H=96, focal=100.0, seed=1000 + seed, sigma_px=1.5, kernel_size=0.1 if seed % 2 else 0.0,
                           pose_seed=(seed if seed % 3 == 0 else None))
