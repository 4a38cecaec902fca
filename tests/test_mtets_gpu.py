"""GPU: marching tetrahedra (csrc/mtets.hip) against the golden output of the reference's
utils/tetmesh.py (tests/golden/ref_python_golden.npz) and against the oracle restatement -- integer
results, bit-exact."""
import os

import numpy as np
import pytest
import torch

import mtets_cases as MC
import oracle_binding as ob
import synthetic_scenes as S

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_python_golden.npz"))
MT_GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_mtets_golden.npz"))


def run(verts, tets, sdf, scales):
    from tetmesh import marching_tetrahedra
    d = "cuda"
    v = torch.from_numpy(verts).to(d)[None]
    out = marching_tetrahedra(v, torch.from_numpy(tets).to(d), torch.from_numpy(sdf).to(d)[None], torch.from_numpy(scales).to(d)[None, :, None])
    (pos, esdf), esc, faces, ids = [o[0] for o in out]
    torch.cuda.synchronize()
    return ids.cpu().numpy(), pos.cpu().numpy(), esdf.cpu().numpy(), esc.cpu().numpy(), faces.cpu().numpy()


def test_matches_reference_golden():
    ids, pos, esdf, esc, faces = run(GOLD["mt_verts"], GOLD["mt_tets"], GOLD["mt_sdf"], GOLD["mt_scales"])
    assert np.array_equal(ids, GOLD["mt_edge_ids"])
    assert np.array_equal(faces, GOLD["mt_faces"])
    assert np.array_equal(pos, GOLD["mt_edge_pos"])
    assert np.array_equal(esdf, GOLD["mt_edge_sdf"])
    assert np.array_equal(esc, GOLD["mt_edge_scales"])


def test_docstring_example():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    ids, pos, esdf, esc, faces = run(v, np.array([[0, 1, 2, 3]], np.int64), np.array([-1, -1, 0.5, 0.5], np.float32), np.ones(4, np.float32))
    assert np.array_equal(faces, np.array([[3, 0, 1], [3, 2, 0]]))
    assert np.array_equal(ids, GOLD["mt_doc_edge_ids"])


@pytest.mark.parametrize("n", [(3, 3, 3), (24, 20, 16)])
def test_matches_oracle_on_grids_and_degenerate_fields(n):
    verts, tets = S.freudenthal_tets(*n)
    rng = np.random.default_rng(7)
    centre = np.array(n, np.float32) / 2
    sdf = (0.4 * min(n) - np.linalg.norm(verts - centre, axis=1) + rng.normal(0, 0.3, len(verts))).astype(np.float32)
    scales = rng.uniform(0.1, 1, len(verts)).astype(np.float32)
    got = run(verts, tets, sdf, scales)
    want = ob.marching_tets(verts, tets, sdf, scales)
    for a, b in zip(got, [want[0], want[1], want[2][..., None], want[3][..., None], want[4]]):
        assert np.array_equal(a, b)
    assert got[4].min() >= 0 and got[4].max() < len(got[0])
    # all-outside and all-inside fields: no surface
    for const in (-1.0, 1.0):
        ids, pos, esdf, esc, faces = run(verts, tets, np.full(len(verts), const, np.float32), scales)
        assert len(ids) == 0 and len(faces) == 0
    # sdf exactly 0 counts as outside (sdf > 0 test, tetmesh.py:98)
    z = sdf.copy(); z[::3] = 0.0
    got = run(verts, tets, z, scales); want = ob.marching_tets(verts, tets, z, scales)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[4], want[4])


def test_more_than_32Mi_tets_face_order_follows_the_references_chunking():
    """utils/tetmesh.py:55-95 processes more than 32 Mi tets in torch.chunk pieces, which fixes the ORDER of the faces (chunk by
    chunk, inside a chunk the 1-triangle tets first).  47M tets = 2 chunks whose boundary is not a multiple of the kernels' 4096-tet
    blocks; bit-exact against the oracle (which restates the chunk loop) -- edges, positions and every face."""
    n = (200, 199, 201)
    # 6 tets per cell of an n0 x n1 x n2 vertex grid, built on the GPU (the numpy helper takes 25 s at this size)
    ax = [torch.arange(k, device="cuda", dtype=torch.float32) for k in n]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    verts = torch.stack([X, Y, Z], -1).reshape(-1, 3).cpu().numpy()
    idx = torch.arange(n[0] * n[1] * n[2], device="cuda").reshape(n)
    c = [idx[i:n[0] - 1 + i, j:n[1] - 1 + j, k:n[2] - 1 + k].reshape(-1) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    v000, v001, v010, v011, v100, v101, v110, v111 = c
    tets = torch.stack([torch.stack(t, 1) for t in ((v000, v100, v110, v111), (v000, v100, v101, v111), (v000, v010, v110, v111),
                                                     (v000, v010, v011, v111), (v000, v001, v101, v111), (v000, v001, v011, v111))], 1)
    tets = tets.reshape(-1, 4).cpu().numpy()
    del X, Y, Z, idx, c
    torch.cuda.empty_cache()
    assert len(tets) > 32 * 1024 * 1024
    rng = np.random.default_rng(11)
    centre = np.array(n, np.float32) / 2
    sdf = (0.37 * min(n) - np.linalg.norm(verts - centre, axis=1) + rng.normal(0, 0.2, len(verts)).astype(np.float32)).astype(np.float32)
    scales = rng.uniform(0.1, 1, len(verts)).astype(np.float32)
    got = run(verts, tets, sdf, scales)
    want = ob.marching_tets(verts, tets, sdf, scales)
    assert len(want[4]) > 100_000
    for a, b in zip(got, [want[0], want[1], want[2][..., None], want[3][..., None], want[4]]):
        assert np.array_equal(a, b)


# ---- unordered, Delaunay-style tets (tests/mtets_cases.py; the host twin is tests/test_mtets_host.py) ---------------------------------
def _golden_class(cls, oriented=False):
    for name in MC.CASES[cls]:
        inputs = MC.case(name)
        got = run(*inputs)
        MC.assert_matches_golden(MT_GOLD, name, inputs, got)
        MC.check_surface(inputs, got, oriented=oriented)


def test_single_all_every_sign_case_in_every_vertex_order():
    _golden_class("single_all")


def test_shuffled_grid_matches_the_reference_and_faces_its_inside():
    _golden_class("shuffled_grid", oriented=True)


def test_special_sdf_values_classify_as_in_the_reference():
    """+0, -0, NaN, +-inf, denormals: `sdf > 0` and nothing else (NaN is outside); NaN / inf scales are payload, copied bit for bit"""
    _golden_class("special_sdf")


def test_degenerate_duplicated_and_collapsed_tets():
    _golden_class("degenerate")


def test_vertex_bits_around_powers_of_two():
    _golden_class("vertex_bits")


def test_sizes_on_the_kernels_boundaries_match_the_oracle():
    for name in MC.CASES["sizes"]:
        inputs = MC.case(name)
        got = run(*inputs)
        MC.assert_same(got, ob.marching_tets(*inputs), name)
        MC.check_surface(inputs, got)


def _chunk_override():
    import ctypes as C
    from diff_gaussian_rasterization import _backend as B
    f = B.lib.gof_debug_mtets_chunk
    f.restype, f.argtypes = C.c_int64, [C.c_int64]
    return f


def test_face_order_follows_the_chunking_at_small_chunk_sizes():
    """per_chunk_of, mt_chunk_table and the fidx arithmetic of mt_write_faces with the chunk size overridden (gof_debug_mtets_chunk):
    boundaries that split a thread's 16 tets, a chunk without a valid tet, a last chunk of one tet -- against the oracle at the same
    chunk size"""
    override = _chunk_override()
    for label, inputs, chunk in MC.chunk_cases():
        want = ob.marching_tets(*inputs, chunk_size=chunk)
        assert override(chunk) == 32 * 1024 * 1024
        try:
            got = run(*inputs)
        finally:
            assert override(0) == chunk
        MC.assert_same(got, want, label)


def test_more_chunks_than_the_table_holds_is_refused():
    from diff_gaussian_rasterization import _backend as B
    override = _chunk_override()
    inputs = MC.case("shuffled_14_12_10")
    override(MC.TOO_MANY_CHUNKS)
    try:
        with pytest.raises(B.GofError, match="too many chunks"):
            run(*inputs)
    finally:
        override(0)
    MC.assert_matches_golden(MT_GOLD, "shuffled_14_12_10", inputs, run(*inputs))


def test_a_vertex_id_outside_the_vertices_is_refused_not_read():
    """ids V, V + 2^32, -1 and INT64_MIN in the first tet, the last tet and the middle of a 4096-block, and tets without vertices:
    gof_mtets_classify compares every id with V before anything is read through it and returns GOF_E_INVALID; count and emit refuse the
    workspace and write nothing (tests/test_mtets_host.py runs the same cases on the host first)"""
    import ctypes as C
    from diff_gaussian_rasterization import _backend as B
    verts, tets, sdf, scales = MC.case("size_8193")
    for label, t, corner, val in MC.bad_id_cases(len(verts), len(tets)):
        bad = tets.copy()
        bad[t, corner] = val
        with pytest.raises(B.GofError, match=r"vertex id %d \(tet %d, corner %d\) is outside \[0, 300\); 1 of 8193 tets" % (val, t, corner)):
            run(verts, bad, sdf, scales)
    with pytest.raises(B.GofError, match="no vertices"):
        run(verts[:0], tets[:3], sdf[:0], scales[:0])
    # the three calls one by one on the last of these inputs: count and emit refuse the workspace, the outputs stay as they were
    d = "cuda"
    V, Tt = len(verts), len(bad)
    t64, s32 = torch.from_numpy(bad).to(d), torch.from_numpy(sdf).to(d)
    v32, sc32 = torch.from_numpy(verts).to(d), torch.from_numpy(scales).to(d)
    tws = torch.empty(int(B.lib.gof_mtets_tet_ws_bytes(Tt)), dtype=torch.uint8, device=d)
    ews = torch.empty(int(B.lib.gof_mtets_edge_ws_bytes(Tt)), dtype=torch.uint8, device=d)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nv, ne, nf = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    assert B.lib.gof_mtets_classify(V, Tt, B._ptr(t64), B._ptr(s32), B._ptr(tws), tws.numel(), C.byref(nv), stream) == -1 and nv.value == 0
    assert B.lib.gof_mtets_count(V, Tt, B._ptr(t64), B._ptr(s32), B._ptr(tws), tws.numel(), B._ptr(ews), ews.numel(), C.byref(ne), C.byref(nf), stream) == -1
    assert ne.value == 0 and nf.value == 0 and b"refused" in B.lib.gof_last_error()
    outs = [torch.full(shape, 0x5A, dtype=torch.uint8, device=d) for shape in ((5 * 2 * 8,), (5 * 6 * 4,), (5 * 2 * 4,), (5 * 2 * 4,), (7 * 3 * 8,))]
    for E, F in ((5, 7), (0, 0)):
        assert B.lib.gof_mtets_emit(V, Tt, B._ptr(t64), B._ptr(v32), B._ptr(s32), B._ptr(sc32), B._ptr(tws), tws.numel(), B._ptr(ews), ews.numel(), E, F,
                                    *[B._ptr(o) for o in outs], stream) == -1
        assert b"refused" in B.lib.gof_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == 0x5A).all()) for o in outs)
    # the library is not left in a refusing state
    MC.assert_same(run(verts, tets, sdf, scales), ob.marching_tets(verts, tets, sdf, scales), "after the refusal")


def test_count_and_emit_refuse_on_their_own_what_classify_would_refuse():
    """tets without vertices and a number of vertices other than the classified one, on a workspace that holds a valid classification
    of the same tets: count and emit return GOF_E_INVALID before any launch, outputs untouched; then the same after classify itself
    refused V = 0 on that workspace (the host twin in tests/test_mtets_host.py runs first)"""
    import ctypes as C
    from diff_gaussian_rasterization import _backend as B
    verts, tets, sdf, scales = MC.case("size_17")
    d = "cuda"
    V, Tt = len(verts), len(tets)
    t64, s32 = torch.from_numpy(tets.copy()).to(d), torch.from_numpy(sdf.copy()).to(d)
    v32, sc32 = torch.from_numpy(verts.copy()).to(d), torch.from_numpy(scales.copy()).to(d)
    tws = torch.empty(int(B.lib.gof_mtets_tet_ws_bytes(Tt)), dtype=torch.uint8, device=d)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nv, ne, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    outs = [torch.full(shape, 0x5A, dtype=torch.uint8, device=d) for shape in ((5 * 2 * 8,), (5 * 6 * 4,), (5 * 2 * 4,), (5 * 2 * 4,), (7 * 3 * 8,))]

    def count(nverts):
        ne.value = nf.value = 77
        return B.lib.gof_mtets_count(nverts, Tt, B._ptr(t64), B._ptr(s32), B._ptr(tws), tws.numel(), B._ptr(ews), ews.numel(), C.byref(ne), C.byref(nf), stream)

    def emit(nverts, E, F):
        return B.lib.gof_mtets_emit(nverts, Tt, B._ptr(t64), B._ptr(v32), B._ptr(s32), B._ptr(sc32), B._ptr(tws), tws.numel(), B._ptr(ews), ews.numel(), E, F,
                                    *[B._ptr(o) for o in outs], stream)

    assert B.lib.gof_mtets_classify(V, Tt, B._ptr(t64), B._ptr(s32), B._ptr(tws), tws.numel(), C.byref(nv), stream) == 0 and nv.value > 0
    ews = torch.empty(int(B.lib.gof_mtets_edge_ws_bytes(nv.value)), dtype=torch.uint8, device=d)
    assert count(V) == 0 and ne.value > 0 and nf.value > 0
    for reclassified in (False, True):
        if reclassified:
            assert B.lib.gof_mtets_classify(0, Tt, B._ptr(t64), None, B._ptr(tws), tws.numel(), C.byref(nv), stream) == -1 and nv.value == 0
        for nverts in (0, V - 1, V + 1) + ((V,) if reclassified else ()):
            assert count(nverts) == -1 and ne.value == 0 and nf.value == 0, (reclassified, nverts)
            assert emit(nverts, 5, 7) == -1 and emit(nverts, 0, 0) == -1, (reclassified, nverts)
    torch.cuda.synchronize()
    assert all(bool((o == 0x5A).all()) for o in outs)
    MC.assert_same(run(verts, tets, sdf, scales), ob.marching_tets(verts, tets, sdf, scales), "after the refusals")
