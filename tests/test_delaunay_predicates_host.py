"""CPU tests of the Delaunay predicates (csrc/delaunay_predicates.h and collinear / insphere_perturbed / incircle_perturbed of
csrc/delaunay.hip) through gof_debug_delaunay_predicates of the emulated library (tests/hipemu), each class in a child
process: every sign equals exact integer arithmetic (tests/delaunay_exact.py) on the classes of tests/delaunay_predicate_cases.py --
general position over every float32 magnitude, exact degeneracies, one ulp off them, coordinate differences that round in fp64,
ties of the symbolic perturbation.  Every assertion is an integer equality.  tests/test_delaunay_predicates_gpu.py runs the same
classes and checks (run_class, check_class) on the device.

The issue behind these tests asked for at least 50 ties of class E decided by the THIRD epsilon coefficient.  There are none: for
five distinct cospherical points around a non-flat cell, the coefficient of a point is the orientation of the other four, and two of
them cannot vanish (two coplanar quadruples share three points of a sphere, which are not collinear and fix the plane: all five
would be coplanar, the cell flat); for the in-circle form a vanishing coefficient needs three collinear points of a circle.  So the
third candidate of either loop is reachable only through a wrong earlier sign; test_class_conditions asserts the first and the
second coefficient, the largest-query case, and that the reference finds no third."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu"))
import host_child  # noqa: E402
import delaunay_exact as X  # noqa: E402
import delaunay_predicate_cases as G  # noqa: E402

GOF_E_INVALID = -1
CLASSES = list(G.CASES)
SIGN_OPS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def case(name):
    P, idx = G.CASES[name][0]()
    assert len(idx) == G.COUNT[name] and len(P) == 5 * len(idx)
    P.setflags(write=False)
    idx.setflags(write=False)
    return P, idx


@functools.lru_cache(maxsize=None)
def reference(name):
    """op -> the exact signs of the class (ops 2 and 3 are ops 0 and 1); 'term' / 'row' for the perturbed ops"""
    P, idx = case(name)
    ops = G.CASES[name][1]
    ref = {}
    if 0 in ops or 2 in ops:
        ref[0] = ref[2] = X.orient(P, idx)
    if 1 in ops or 3 in ops:
        ref[1] = ref[3] = X.insphere(P, idx)
    if 4 in ops:
        ref[4] = X.collinear(P, idx)
    if 5 in ops:
        ref[5], ref["term"], ref["row"] = X.insphere_perturbed(P, idx)
    if 6 in ops:
        ref[6], ref["term"], ref["row"] = X.incircle_perturbed(P, idx)
    return ref


@functools.lru_cache(maxsize=None)
def scaling(name):
    P, idx = case(name)
    ks = G.scale_exponents(P, idx)
    return ks, G.scaled(P, idx, ks)


def runs(name):
    """the launches of a class: (tag, points, idx, op).  Classes A and C also run with two cell vertices swapped, with an even
    permutation of the cell, and with every query multiplied by a power of two."""
    P, idx = case(name)
    ops = G.CASES[name][1]
    out = [("base:%d" % op, P, idx, op) for op in ops]
    if name[0] in "AC":
        swap, even = idx[:, [1, 0, 2, 3, 4, 5]], idx[:, [1, 2, 0, 3, 4, 5]]
        for op in ops:
            if op in SIGN_OPS:
                out += [("swap:%d" % op, P, np.ascontiguousarray(swap), op), ("even:%d" % op, P, np.ascontiguousarray(even), op)]
            out.append(("scaled:%d" % op, scaling(name)[1], idx, op))
    return out


def run_class(probe, name):
    """probe(points, idx, op) -> (rc, sign, exact, err); -> {tag: [3][Q] int64}"""
    res = {}
    for tag, P, idx, op in runs(name):
        rc, s, ex, er = probe(P, idx, op)
        assert rc == 0, (tag, rc)
        res[tag] = np.stack([np.asarray(s, np.int64), np.asarray(ex, np.int64), np.asarray(er, np.int64)])
    return res


def _same(got, want, what):
    got = np.asarray(got)
    want = np.broadcast_to(np.asarray(want), got.shape)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "%s: %d queries differ, first %s (got %s, expected %s)" % (what, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def check_class(name, res):
    ref = reference(name)
    ops = G.CASES[name][1]
    assert set(res) == {r[0] for r in runs(name)}
    for tag, (s, ex, er) in res.items():
        kind, op = tag.split(":")
        op = int(op)
        assert len(s) == G.COUNT[name]
        _same(er, 0, "%s %s: error bits" % (name, tag))
        _same(s, -ref[op] if kind == "swap" else ref[op], "%s %s: sign against exact arithmetic" % (name, tag))
        if op in (5, 6):
            assert (s != 0).all()
        assert ((ex >= 0) & (ex <= 4)).all(), "%s %s: exact evaluations (at most the in-sphere test and three orientations)" % (name, tag)     # (and not the 0xA5 the outputs are handed over with)
        if op in (2, 3):
            _same(ex, 1, "%s %s: exact evaluations of one exact call" % (name, tag))
        if name[0] == "B" and op in (0, 1, 4):
            assert (ex >= 1).all(), "%s %s: the filter decided a true zero" % (name, tag)
    if name[0] == "A":
        for kind in ("base", "swap", "even", "scaled"):
            _same(res["%s:2" % kind][0], res["%s:0" % kind][0], "%s %s: orient_exact against orient" % (name, kind))
            _same(res["%s:3" % kind][0], res["%s:1" % kind][0], "%s %s: insphere_exact against insphere" % (name, kind))
    assert ops


# ---------------------------------------------------------------------------------------------------------------------------
# the emulated library, driven from a child process
# ---------------------------------------------------------------------------------------------------------------------------
def _emu_lib():
    lib = C.CDLL(os.environ["GOF_HIP_LIB"])
    lib.gof_last_error.restype = C.c_char_p
    lib.gof_debug_delaunay_predicates.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def emu_probe(lib):
    def probe(P, idx, op):
        P, idx = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(idx, np.int32)
        out = np.full((3, len(idx)), 0xA5A5A5A5, np.uint32)              # (as uninitialised as a device allocation)
        rc = lib.gof_debug_delaunay_predicates(len(P), P.ctypes.data, len(idx), idx.ctypes.data, op, out[0].ctypes.data, out[1].ctypes.data,
                                               out[2].ctypes.data, None)
        return rc, out[0].view(np.int32), out[1], out[2]
    return probe


def _child(name, out):
    lib = _emu_lib()
    if name != "arguments":
        np.savez(out, **run_class(emu_probe(lib), name))
        return
    P, idx = case("A2")
    P, idx = P[:50], np.ascontiguousarray(idx[:10])
    o = np.zeros((3, 10), np.uint32)
    f = lib.gof_debug_delaunay_predicates

    def call(n=50, p=P.ctypes.data, q=10, i=idx, op=0, s=o[0].ctypes.data, ex=o[1].ctypes.data, er=o[2].ctypes.data):
        rc = f(n, p, q, i.ctypes.data if i is not None else None, op, s, ex, er, None)
        return rc, len(lib.gof_last_error() or b"") > 0 if rc else True

    def with_index(col, v):
        j = idx.copy()
        j[7, col] = v
        return j
    rcs = {"ok": call(), "empty": call(q=0), "op -1": call(op=-1), "op 7": call(op=7), "points NULL": call(p=None), "idx NULL": call(i=None),
           "sign NULL": call(s=None), "exact NULL": call(ex=None), "err NULL": call(er=None), "index 50": call(i=with_index(3, 50)),
           "index -1": call(i=with_index(0, -1)), "e 50 unread by op 0": call(i=with_index(4, 50)), "e 50 read by op 1": call(i=with_index(4, 50), op=1),
           "d 50 unread by op 4": call(i=with_index(3, 50), op=4), "aux 4 op 6": call(i=with_index(5, 4), op=6), "aux 4 unread by op 5": call(i=with_index(5, 4), op=5),
           "negative n": call(n=-1), "negative q": call(q=-1)}
    np.savez(out, names=np.array(list(rcs)), rc=np.array([v[0] for v in rcs.values()]), msg=np.array([v[1] for v in rcs.values()]))


def _emulate(name, tmp_path):
    return host_child.run_child(__file__, name, tmp_path, timeout=1200)


# ---------------------------------------------------------------------------------------------------------------------------
def test_reference_conventions():
    """the integer reference on answers that are obvious"""
    tet = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert X.orient_rows(*tet) == 1 and X.orient_rows(tet[1], tet[0], tet[2], tet[3]) == -1
    assert X.insphere_rows(*tet, [1, 1, 1]) == 0 and X.insphere_rows(*tet, [1, 1, 0]) == 0          # the unit cube's corners
    assert X.insphere_rows(*[[4 * v for v in p] for p in tet], [1, 1, 1]) == 1 and X.insphere_rows(*tet, [2, 2, 2]) == -1
    assert X.collinear_rows([0, 0, 0], [1, 2, 3], [-2, -4, -6]) == 1 and X.collinear_rows([0, 0, 0], [1, 2, 3], [-2, -4, -5]) == 0
    assert X.det([[2, 0, 0, 0, 0], [0, 3, 0, 0, 0], [0, 0, 0, 5, 0], [0, 0, 7, 0, 0], [0, 0, 0, 0, 1]]) == -210
    # no tie: the perturbation does not matter
    assert X.perturbed_rows(tet + [[2, 2, 2]], (1, 1, 1, 1, 1)) == (-1, 0, -1)
    # a tie whose query is the largest point: its epsilon lifts it off the sphere
    assert X.perturbed_rows(tet + [[1, 1, 1]], (1, 1, 1, 1, 1)) == (-1, 1, 4)
    # the same five points with the largest in the cell: (1, 1, 1) lifted, the sphere through it grows and takes in the query (0, 0, 1)
    cell = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1]]
    assert X.orient_rows(*cell) == 1 and X.perturbed_rows(cell + [[0, 0, 1]], (1, 1, 1, 1, 1))[0] == 1


def test_class_conditions():
    """what the classes promise, from the reference alone"""
    total = sum(G.COUNT.values())
    assert total <= 30000 and all(len(case(n)[1]) == G.COUNT[n] for n in CLASSES)
    for n in ("B_coplanar", "B_cospherical"):
        assert all((reference(n)[op] == 0).all() for op in G.CASES[n][1])
    assert (reference("B_collinear")[4] == 1).all()
    near = np.concatenate([reference(n)[G.CASES[n][1][0]] for n in CLASSES if n[0] in "CD" and G.CASES[n][1][0] in (0, 1)])
    assert (near == 1).mean() >= 0.2 and (near == -1).mean() >= 0.2
    for n in ("E_sphere", "E_circle"):
        P, idx = case(n)
        assert (X.orient(P, idx) == 1).all() and (X.insphere(P, idx) == 0).all()                   # positive cells, true ties
        assert (reference(n)["term"] >= 1).all()
    term = np.concatenate([reference(n)["term"] for n in ("E_sphere", "E_circle")])
    row = np.concatenate([reference(n)["row"] for n in ("E_sphere", "E_circle")])
    assert (term == 1).sum() >= 50 and (term == 2).sum() >= 50 and ((term == 1) & (row == 4)).sum() >= 50
    assert (term >= 3).sum() == 0                       # (no third coefficient exists: the module's docstring)
    assert sorted(np.unique(case("E_circle")[1][:, 5]).tolist()) == [0, 1, 2, 3]
    for n in CLASSES:
        if n[0] in "AC":
            assert (scaling(n)[0] != 0).mean() >= 0.5, n


@pytest.mark.parametrize("name", CLASSES)
def test_signs_equal_exact_arithmetic(name, tmp_path):
    check_class(name, _emulate(name, tmp_path))


def test_argument_errors_and_fully_written_outputs(tmp_path):
    r = _emulate("arguments", tmp_path)
    got = dict(zip(r["names"].tolist(), zip(r["rc"].tolist(), r["msg"].tolist())))
    valid = {"ok", "empty", "e 50 unread by op 0", "d 50 unread by op 4", "aux 4 unread by op 5"}
    for k, (rc, msg) in got.items():
        assert rc == (0 if k in valid else GOF_E_INVALID) and msg, (k, rc, msg)
    # (outputs handed over as 0xA5 come back fully written: emu_probe prefills them, and check_class holds every word of the three)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
