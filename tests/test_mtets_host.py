"""CPU: marching tetrahedra (csrc/mtets.hip compiled for the host, tests/hipemu) on UNORDERED, Delaunay-style tets -- the inputs of
tests/mtets_cases.py -- bit for bit against the golden output of the reference's utils/tetmesh.py (tests/golden/ref_mtets_golden.npz),
against the oracle where there is no golden (`sizes`, the chunk layouts), and against the geometry alone (mtets_cases.check_surface).
Then the one input the library refuses: a vertex id outside [0, V).  The GPU twin is tests/test_mtets_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "hipemu"),):
    if p not in sys.path:
        sys.path.insert(0, p)
import mtets_cases as MC  # noqa: E402
import oracle_binding as ob  # noqa: E402

build_emu = pytest.importorskip("build_emu")
if not os.path.exists(build_emu.CXX):
    pytest.skip("no host clang++ (%s) to build the emulated library" % build_emu.CXX, allow_module_level=True)
import emu_binding as E  # noqa: E402
from test_hipemu_epilogue import _mtets  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ref_mtets_golden.npz"))
GOF_E_INVALID = -1


def _lib():
    lib = E.load()
    lib.gof_debug_mtets_chunk.restype = C.c_int64
    lib.gof_debug_mtets_chunk.argtypes = [C.c_int64]
    return lib


def _golden_class(cls, oriented=False):
    lib = _lib()
    for name in MC.CASES[cls]:
        inputs = MC.case(name)
        got = _mtets(lib, *inputs)
        MC.assert_matches_golden(GOLD, name, inputs, got)
        MC.check_surface(inputs, got, oriented=oriented)
    assert not E.guards_intact()          # (emu_binding's helper returns the list of BROKEN guards: empty = nothing wrote past a workspace)


def test_single_all_every_sign_case_in_every_vertex_order():
    _golden_class("single_all")


def test_shuffled_grid_matches_the_reference_and_faces_its_inside():
    _golden_class("shuffled_grid", oriented=True)


def test_special_sdf_values_classify_as_in_the_reference():
    """+0, -0, NaN, +-inf, denormals: `sdf > 0` and nothing else (NaN is outside); NaN / inf scales are payload, copied bit for bit"""
    _golden_class("special_sdf")
    ids = _mtets(_lib(), *MC.case("special_7_6_5"))[0]
    sdf, scales = MC.case("special_7_6_5")[2:]
    bits = set(sdf[ids].view(np.uint32).ravel().tolist())
    assert set(MC.SPECIAL_BITS) <= bits, "a special sdf value is on no crossing edge: the case does not test it"
    assert np.isnan(scales[ids]).any() and np.isinf(scales[ids]).any()


def test_degenerate_duplicated_and_collapsed_tets():
    _golden_class("degenerate")


def test_vertex_bits_around_powers_of_two():
    _golden_class("vertex_bits")


@pytest.mark.parametrize("name", MC.CASES["sizes"])
def test_sizes_on_the_kernels_boundaries_match_the_oracle(name):
    inputs = MC.case(name)
    got = _mtets(_lib(), *inputs)
    MC.assert_same(got, ob.marching_tets(*inputs), name)
    MC.check_surface(inputs, got)


@pytest.mark.parametrize("fill", ["0xA5", "0xFF"])
def test_unordered_tets_do_not_depend_on_what_the_workspaces_held(fill):
    lib = _lib()
    with E.fill(fill):
        for name in ["shuffled_7_6_5"] + MC.CASES["single_all"]:
            inputs = MC.case(name)
            MC.assert_matches_golden(GOLD, name, inputs, _mtets(lib, *inputs))


# ---- chunk boundaries at small sizes (gof_debug_mtets_chunk) --------------------------------------------------------------------------
@pytest.mark.parametrize("label,chunk", [(label, chunk) for label, _, chunk in MC.chunk_cases()])
def test_face_order_follows_the_chunking_at_small_chunk_sizes(label, chunk):
    inputs = [c for lab, c, _ in MC.chunk_cases() if lab == label][0]
    lib = _lib()
    want = ob.marching_tets(*inputs, chunk_size=chunk)
    prev = lib.gof_debug_mtets_chunk(chunk)
    try:
        assert prev == 32 * 1024 * 1024
        got = _mtets(lib, *inputs)
    finally:
        assert lib.gof_debug_mtets_chunk(0) == chunk
    MC.assert_same(got, want, label)
    if chunk < len(inputs[1]):
        assert not np.array_equal(got[4], ob.marching_tets(*inputs)[4]), "the chunk size did not change the face order: the case tests nothing"
    assert lib.gof_debug_mtets_chunk(0) == 32 * 1024 * 1024


def test_more_chunks_than_the_table_holds_is_refused():
    verts, tets, sdf, scales = MC.case("shuffled_14_12_10")
    lib = _lib()
    want = ob.marching_tets(verts, tets, sdf, scales)
    lib.gof_debug_mtets_chunk(MC.TOO_MANY_CHUNKS)
    try:
        rc, out = _emit_with_sentinels(lib, verts, tets, sdf, scales, len(want[0]), len(want[4]))
    finally:
        lib.gof_debug_mtets_chunk(0)
    assert rc == GOF_E_INVALID and b"too many chunks" in lib.gof_last_error()
    assert all(_untouched(a) for a in out)
    MC.assert_same(_mtets(lib, verts, tets, sdf, scales), want, "after the refusal")


# ---- vertex ids outside [0, V) --------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def _untouched(a):
    return (a.view(np.uint8) == SENTINEL).all()


def _emit_with_sentinels(lib, verts, tets, sdf, scales, Ec, F, classify_rc=0, count_rc=0):
    """classify + count + emit with every output pre-filled -> (emit's return code, the outputs)"""
    V, Tt = len(verts), len(tets)
    t64 = np.ascontiguousarray(tets, np.int64); v32 = np.ascontiguousarray(verts, np.float32).reshape(-1)
    s32 = np.ascontiguousarray(sdf, np.float32); sc32 = np.ascontiguousarray(scales, np.float32)
    tws = E._aligned(lib.gof_mtets_tet_ws_bytes(Tt))
    nv = C.c_int64(77)
    assert lib.gof_mtets_classify(V, Tt, E._p(t64), E._p(s32), E._p(tws), tws.size, C.byref(nv), None) == classify_rc
    if classify_rc:
        assert nv.value == 0
    ews = E._aligned(lib.gof_mtets_edge_ws_bytes(max(int(nv.value), Tt if classify_rc else 0)))
    ne, nf = C.c_int64(77), C.c_int64(77)
    assert lib.gof_mtets_count(V, Tt, E._p(t64), E._p(s32), E._p(tws), tws.size, E._p(ews), ews.size, C.byref(ne), C.byref(nf), None) == count_rc
    if count_rc:
        assert ne.value == 0 and nf.value == 0
    out = [np.full((Ec, 2), 0, np.int64), np.zeros((Ec, 2, 3), np.float32), np.zeros((Ec, 2), np.float32), np.zeros((Ec, 2), np.float32),
           np.zeros((F, 3), np.int64)]
    for a in out:
        a.view(np.uint8)[...] = SENTINEL
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    rc = lib.gof_mtets_emit(V, Tt, E._p(t64), p(v32), p(s32), p(sc32), E._p(tws), tws.size, E._p(ews), ews.size, Ec, F, *[p(a) for a in out], None)
    return rc, out


@pytest.mark.parametrize("label,t,corner,val", MC.bad_id_cases(300, 8193))
def test_a_vertex_id_outside_the_vertices_is_refused_not_read(label, t, corner, val):
    verts, tets, sdf, scales = MC.case("size_8193")
    assert len(verts) == 300 and len(tets) == 8193
    bad = tets.copy()
    bad[t, corner] = val
    lib = _lib()
    rc, out = _emit_with_sentinels(lib, verts, bad, sdf, scales, 5, 7, classify_rc=GOF_E_INVALID, count_rc=GOF_E_INVALID)
    msg = lib.gof_last_error().decode()
    assert rc == GOF_E_INVALID and "refused" in msg, msg
    assert all(_untouched(a) for a in out)
    # ... and with nothing to write
    assert _emit_with_sentinels(lib, verts, bad, sdf, scales, 0, 0, classify_rc=GOF_E_INVALID, count_rc=GOF_E_INVALID)[0] == GOF_E_INVALID
    # the message of classify itself names the first offending tet, the id and the count
    tws = E._aligned(lib.gof_mtets_tet_ws_bytes(len(bad)))
    nv = C.c_int64(5)
    assert lib.gof_mtets_classify(len(verts), len(bad), E._p(bad), E._p(sdf), E._p(tws), tws.size, C.byref(nv), None) == GOF_E_INVALID
    msg = lib.gof_last_error().decode()
    assert "vertex id %d (tet %d, corner %d)" % (val, t, corner) in msg and "[0, 300)" in msg and "1 of 8193 tets" in msg, msg
    assert not E.guards_intact()
    # the library is not left in a refusing state
    MC.assert_same(_mtets(lib, verts, tets, sdf, scales), ob.marching_tets(verts, tets, sdf, scales), "after the refusal")


def test_several_bad_ids_name_the_first_tet_and_the_count():
    verts, tets, sdf, scales = MC.case("size_8193")
    bad = tets.copy()
    bad[[17, 4095, 4096, 8000], [0, 1, 2, 3]] = [300, -5, 1 << 40, 301]
    lib = _lib()
    tws = E._aligned(lib.gof_mtets_tet_ws_bytes(len(bad)))
    nv = C.c_int64(5)
    assert lib.gof_mtets_classify(300, len(bad), E._p(bad), E._p(sdf), E._p(tws), tws.size, C.byref(nv), None) == GOF_E_INVALID
    msg = lib.gof_last_error().decode()
    assert "vertex id 300 (tet 17, corner 0)" in msg and "4 of 8193 tets" in msg, msg


def test_tets_without_vertices_are_refused():
    lib = _lib()
    tets = np.zeros((3, 4), np.int64)
    tws = E._aligned(lib.gof_mtets_tet_ws_bytes(3))
    nv = C.c_int64(5)
    assert lib.gof_mtets_classify(0, 3, E._p(tets), None, E._p(tws), tws.size, C.byref(nv), None) == GOF_E_INVALID
    assert nv.value == 0 and b"no vertices" in lib.gof_last_error()


@pytest.mark.parametrize("reclassify", [False, True])
def test_count_and_emit_refuse_on_their_own_what_classify_would_refuse(reclassify):
    """count and emit read sdf / vertices / scales through the ids, so they refuse -- before any launch, outputs untouched -- tets
    without vertices and a number of vertices other than the one the ids were compared with, also on a workspace that holds a valid
    classification of the same tets (reclassify: after gof_mtets_classify itself refused V = 0 on that workspace)"""
    verts, tets, sdf, scales = MC.case("size_17")
    V, Tt = len(verts), len(tets)
    v32 = np.ascontiguousarray(verts).reshape(-1)
    lib = _lib()
    tws = E._aligned(lib.gof_mtets_tet_ws_bytes(Tt))
    nv, ne, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731

    def count(nverts):
        ne.value = nf.value = 77
        return lib.gof_mtets_count(nverts, Tt, p(tets), p(sdf), p(tws), tws.size, p(ews), ews.size, C.byref(ne), C.byref(nf), None)

    def emit(nverts, Ec, F, ws=None, ws_size=None):
        out = [np.zeros((5, 2), np.int64), np.zeros((5, 2, 3), np.float32), np.zeros((5, 2), np.float32), np.zeros((5, 2), np.float32), np.zeros((7, 3), np.int64)]
        for a in out:
            a.view(np.uint8)[...] = SENTINEL
        rc = lib.gof_mtets_emit(nverts, Tt, p(tets), p(v32), p(sdf), p(scales), p(tws) if ws is None else ws, tws.size if ws_size is None else ws_size,
                                p(ews), ews.size, Ec, F, *[p(a) for a in out], None)
        assert all(_untouched(a) for a in out)
        return rc

    assert lib.gof_mtets_classify(V, Tt, p(tets), p(sdf), p(tws), tws.size, C.byref(nv), None) == 0 and nv.value > 0
    ews = E._aligned(lib.gof_mtets_edge_ws_bytes(nv.value))
    assert count(V) == 0 and ne.value > 0 and nf.value > 0
    if reclassify:
        assert lib.gof_mtets_classify(0, Tt, p(tets), None, p(tws), tws.size, C.byref(nv), None) == GOF_E_INVALID and nv.value == 0
        assert b"no vertices" in lib.gof_last_error()
    for nverts, text in ((0, b"no vertices"), (V - 1, b"refused" if reclassify else b"classified for 300 vertices, not 299"),
                         (V + 1, b"refused" if reclassify else b"classified for 300 vertices, not 301")):
        assert count(nverts) == GOF_E_INVALID and ne.value == 0 and nf.value == 0 and text in lib.gof_last_error(), lib.gof_last_error()
        for Ec, F in ((5, 7), (0, 0)):
            assert emit(nverts, Ec, F) == GOF_E_INVALID and text in lib.gof_last_error(), lib.gof_last_error()
    if reclassify:
        # the refusal voided the classification the workspace held: not even the right V gets through
        assert count(V) == GOF_E_INVALID and emit(V, 5, 7) == GOF_E_INVALID and emit(V, 0, 0) == GOF_E_INVALID
    else:
        # emit needs the tet workspace to tell, also with nothing to write
        assert emit(V, 0, 0, ws=None) == 0
        assert emit(V, 0, 0, ws=C.c_void_p(None)) == GOF_E_INVALID
        assert emit(V, 0, 0, ws_size=16) == -2
    # nothing of this left the library or the inputs in a refusing state
    MC.assert_same(_mtets(lib, verts, tets, sdf, scales), ob.marching_tets(verts, tets, sdf, scales), "after the refusals")
