"""Densification on the host: the plain numpy restatement (tests/densify_restatement.py) against the results the reference's own
GaussianModel.densify_and_prune gave on CPU tensors (tests/golden/ref_densify_golden.npz, written by tests/golden/make_golden_densify.py).
The GPU tests (tests/test_densify_gpu.py) hold the kernels to the restatement and the method to the same fixture."""
import os

import numpy as np
import pytest

import densify_restatement as DR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_densify_golden.npz")
CASES = ("p1_clone", "p1_split", "p1_pruned", "p2", "p257", "p600_ms20", "p600_msneg", "p300_nonorm", "p300_ties")
_golden = {}


def golden():
    if not _golden:
        _golden.update(DR.load_golden(GOLDEN))
    return _golden


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_the_fixture_holds_the_cases_the_tests_name_and_stays_within_the_size_limit():
    assert tuple(golden()) == CASES
    largest = max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN)) if f != os.path.basename(GOLDEN))
    assert os.path.getsize(GOLDEN) <= largest
    g = golden()
    assert g["p1_clone"]["ret"] == (1, 0, 0) and g["p1_split"]["ret"] == (0, 1, 0) and g["p1_pruned"]["after"]["xyz"].shape[0] == 0
    assert g["p257"]["max_screen_size"] is None and min(g["p257"]["ret"]) > 0                     # clones, splits and prunes all occur
    assert g["p600_ms20"]["max_screen_size"] == 20 and g["p600_msneg"]["max_screen_size"] == -1 and g["p600_msneg"]["after"]["xyz"].shape[0] == 0


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_equals_the_references_result(case):
    """Return triple, the order and shapes of the draws, and every tensor bit for bit -- except the sampled positions R(q) (std z) + x, a
    three-term float32 dot product behind a normalised quaternion: those lie within 8 ulp of |x| + sum_j |R_ij| |std_j z_j| around their
    float64 evaluation (the fixture records that the reference's own CPU result does: its worst case is 2.66 ulp), and so does the
    reference's recorded result."""
    c = golden()[case]
    out, ret, shapes, info = DR.densify_and_prune(c["before"], c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"], c["z"])
    assert ret == c["ret"]
    assert shapes == c["draw_shapes"] and sum(s[0] for s in shapes) == c["z"].shape[0]             # clones first, then splits; every draw used
    assert shapes == [(ret[0], 3), (2 * ret[1], 3)]
    assert info["clone_idx"].dtype == info["split_idx"].dtype == info["keep_idx"].dtype == np.int32
    assert (len(info["clone_idx"]), len(info["split_idx"]), len(info["keep_idx"])) == (ret[0], ret[1], c["before"]["xyz"].shape[0] - ret[1])
    s = info["sampled"]
    assert c["worst_ulp"] <= c["bound_ulp"]
    for name, want in c["after"].items():
        got = out[name]
        assert got.shape == want.shape and got.dtype == want.dtype, name
        if name == "xyz":
            assert np.array_equal(bits(got[~s]), bits(want[~s]))
            tol = c["bound_ulp"] * 2.0 ** -23 * info["mag"][s]
            for which, v in (("restatement", got), ("reference", want)):
                err = np.abs(v[s].astype(np.float64) - c["xyz_f64"][s])
                assert (err <= tol).all(), "%s: sampled positions up to %.2f ulp away" % (which, (err / (2.0 ** -23 * info["mag"][s])).max())
        else:
            assert np.array_equal(bits(got), bits(want)), name


def test_the_tie_case_holds_every_constructed_category():
    """a later edit of the generator cannot quietly lose an edge: at least one Gaussian in each of the eight categories, and each
    category decides the way the rule says (>= against >, <= against <, NaN -> 0, inf, magnitude against raw value)"""
    c = golden()["p300_ties"]
    cat = DR.tie_categories(c["before"], c["max_grad"], c["extent"])
    assert len(cat) == 8
    for name, rows in cat.items():
        assert len(rows) >= 1, name
    _, _, _, info = DR.densify_and_prune(c["before"], c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"], c["z"])
    role = info["role"]
    smax = DR.exp32(c["before"]["scaling"]).max(axis=1)
    small = smax <= np.float32(float(c["before"]["percent_dense"]) * c["extent"])
    ga = DR.quotient(c["before"]["xyz_gradient_accum_abs"], c["before"]["denom"])
    below_q = ga < info["Q"]
    assert set(role[cat["quotient == max_grad"]]) == {1, 2}                                          # >= : selected, small and large
    assert set(role[cat["quotient one ulp below max_grad"]][below_q[cat["quotient one ulp below max_grad"]]]) == {0}
    assert set(role[cat["grads_abs == Q"]]) == {1, 2}
    assert set(role[cat["scale_max == threshold"]]) == {1} and set(role[cat["scale_max one ulp above threshold"]]) == {2}
    assert set(role[cat["0 / 0 (NaN)"]]) == {0} and set(role[cat["x / 0 (inf)"]]) == {1, 2}
    neg = cat["negative accum past max_grad"]
    assert set(role[neg][small[neg]]) == {1} and set(role[neg][~small[neg] & below_q[neg]]) == {0} and (~small[neg]).any() and small[neg].any()
    q = np.concatenate([DR.quotient(c["before"][k], c["before"]["denom"]) for k in ("xyz_gradient_accum", "xyz_gradient_accum_abs")])
    assert (np.abs(q[q != 0]) >= 1e-12).all()                      # below ~1e-19 sqrt(g * g) underflows where fabsf does not: kept out on purpose


def test_the_no_norm_case_selects_exactly_the_maximal_rows():
    c = golden()["p300_nonorm"]
    _, _, _, info = DR.densify_and_prune(c["before"], c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"], c["z"])
    g, ga = (DR.quotient(c["before"][k], c["before"]["denom"]) for k in ("xyz_gradient_accum", "xyz_gradient_accum_abs"))
    assert (np.abs(g) < np.float32(c["max_grad"])).all() and info["Q"] == ga.max()
    top = np.nonzero(ga == ga.max())[0]
    assert len(top) > 1 and np.array_equal(np.nonzero(info["role"])[0], top) and {1, 2} == set(info["role"][top])


def test_the_primitives_of_the_restatement_on_hand_written_examples():
    role, keep, clone, split = DR.select(np.float32([4, 4, -4, -4, 0, 1, 1]), np.float32([0, 0, 0, 0, 0, 9, 1]), np.float32([2, 2, 2, 2, 0, 1, 0]),
                                         np.float32([1, 2, 1, 2, 2, 1, 2]), 2.0, 9.0, 1.0)
    assert role.tolist() == [1, 2, 1, 0, 0, 1, 2] and keep.tolist() == [0, 2, 3, 4, 5] and clone.tolist() == [0, 2, 5] and split.tolist() == [1, 6]
    assert DR.compact_rows(np.uint8([0, 2, 255, 0, 1])).tolist() == [1, 2, 4]
    assert DR.compact_rows(np.uint8([1, 0, 1]), np.int32([7, -1, -3])).tolist() == [7, -3]
    src, extra = np.float32([[1, 2], [3, 4]]), np.float32([[9, 8], [7, 6]])
    assert DR.rows_gather(np.int32([1, -2, 1, 0, -1]), src, extra).tolist() == [[3, 4], [7, 6], [3, 4], [1, 2], [9, 8]]
    assert DR.rows_gather(np.int32([1, -2]), src, None).tolist() == [[3, 4], [0, 0]]
    assert DR.quantile(np.float32([3, 1, 2, 4]), 0.5) == 2.5 and DR.quantile(np.float32([3, 1, 2, 4]), 1.0) == 4.0
