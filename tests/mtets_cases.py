"""Deterministic inputs of the marching-tetrahedra tests on UNORDERED, Delaunay-style tets (csrc/mtets.hip), shared by the golden script
(tests/golden/make_golden_mtets.py: the reference's utils/tetmesh.py run on them), the oracle pin (test_oracle_pins.py), the host
suite (test_mtets_host.py: the kernels through the host emulator) and the GPU suite (test_mtets_gpu.py).  numpy only, seeded.

CASES maps a class to its case names; case(name) -> (verts f32 [V,3], tets i64 [T,4], sdf f32 [V], scales f32 [V]).  Inputs are never
stored: the golden keeps a sha256 of each case's inputs (digest), so a drifting generator fails loudly.  check_surface() is a check of
the OUTPUT that needs neither golden nor oracle.  Test infrastructure only."""
import hashlib
import itertools

import numpy as np

import synthetic_scenes as S

PERMS = list(itertools.permutations(range(4)))          # the 24 vertex orders
SIZES = (1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193)      # the uint4 / byte-loop split, 256, MT_BLOCK = 4096
VBITS = (2, 255, 256, 257, 65535, 65536, 65537, (1 << 24) + 1)                  # V - 1 around a power of two: bits_for(V - 1) changes
# chunk sizes walked on the (14,12,10) grid, T = 10 080 -> tets per chunk: 1000 -> 917; 4096, 4097, 5039, 5040 -> 3360 (3 chunks); 10079 -> 5040;
# 10080 -> one chunk; and two whose chunks split a thread's 16 tets in mt_chunk_table at other offsets: 630 -> 17 chunks of 593 (= 16 k + 1),
# 325 -> exactly MT_MAX_CHUNKS = 32 chunks of 315 (= 16 k + 11)
CHUNKS = (1000, 4096, 4097, 5039, 5040, 10079, 10080, 630, 325)
PER_CHUNK = {1000: 917, 4096: 3360, 4097: 3360, 5039: 3360, 5040: 3360, 10079: 5040, 10080: 10080, 630: 593, 325: 315}

# bit patterns of the special sdf values: +0, -0, two NaNs with payloads, +inf, -inf, the smallest positive and the largest negative denormal
SPECIAL_BITS = (0x00000000, 0x80000000, 0x7FC12345, 0xFFC54321, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001)

CASES = {
    "single_all": ["single_own", "single_own_shuffled", "single_pool8"],
    "shuffled_grid": ["shuffled_7_6_5", "shuffled_14_12_10"],
    "special_sdf": ["special_7_6_5"],
    "degenerate": ["degenerate"],
    "sizes": ["size_%d" % t for t in SIZES] + ["size_hole_12288"],
    "vertex_bits": ["vbits_%d" % v for v in VBITS],
}
GOLDEN_CLASSES = ("single_all", "shuffled_grid", "special_sdf", "degenerate", "vertex_bits")      # `sizes` is compared with the oracle


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def inside(sdf):
    """the classification rule of the reference (utils/tetmesh.py:98), for the generators' own assertions and check_surface"""
    return sdf > 0


# ---- single_all ----------------------------------------------------------------------------------------------------------------------
def _single(name):
    rng = np.random.default_rng(_seed(name))
    combos = [(c, p) for c in range(16) for p in PERMS]                              # 384 tets
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    if name == "single_pool8":
        # one pool of 8 vertices, 4 inside and 4 outside: the tet of (case, order) takes an inside vertex where the case has a bit
        verts = np.concatenate([base, base + np.float32(0.37) + rng.random((4, 3), dtype=np.float32)]).astype(np.float32)
        sdf = np.array([0.5, -0.25, 1.5, -2.0, -0.75, 3.0, -1.25, 0.125], np.float32)
        pos_ids, neg_ids = np.flatnonzero(sdf > 0), np.flatnonzero(~(sdf > 0))
        tets = np.zeros((len(combos), 4), np.int64)
        for k, (c, p) in enumerate(combos):
            pi, ni = list(rng.permutation(pos_ids)), list(rng.permutation(neg_ids))
            by_corner = [pi.pop() if (c >> j) & 1 else ni.pop() for j in range(4)]
            tets[k] = [by_corner[j] for j in p]
        scales = rng.uniform(0.1, 1.0, 8).astype(np.float32)
        return verts, tets, sdf, scales
    T = len(combos)
    verts = (base[None] + 3.0 * np.arange(T, dtype=np.float32)[:, None, None] * np.array([1, 0, 0], np.float32)).reshape(-1, 3).astype(np.float32)
    sdf = np.zeros(4 * T, np.float32)
    tets = np.zeros((T, 4), np.int64)
    for k, (c, p) in enumerate(combos):
        mag = rng.uniform(0.1, 2.0, 4)
        sdf[4 * k:4 * k + 4] = [mag[j] if (c >> j) & 1 else -mag[j] for j in range(4)]
        tets[k] = [4 * k + j for j in p]
    scales = rng.uniform(0.1, 1.0, 4 * T).astype(np.float32)
    if name == "single_own_shuffled":
        tets = tets[rng.permutation(T)]
    return verts, np.ascontiguousarray(tets), sdf, scales


# ---- shuffled_grid, special_sdf ------------------------------------------------------------------------------------------------------
def _shuffled_grid(n, seed):
    """a Freudenthal grid as a Delaunay triangulation hands it over: vertices relabelled by a random permutation, the four ids of every
    tet permuted at random, the tets shuffled; sdf = a noisy sphere (as tests/test_mtets_gpu.py)"""
    rng = np.random.default_rng(seed)
    verts0, tets0 = S.freudenthal_tets(*n)
    V, T = len(verts0), len(tets0)
    centre = np.array(n, np.float32) / 2
    sdf0 = (0.4 * min(n) - np.linalg.norm(verts0 - centre, axis=1) + rng.normal(0, 0.3, V)).astype(np.float32)
    scales0 = rng.uniform(0.1, 1, V).astype(np.float32)
    relabel = rng.permutation(V)                                   # old id -> new id
    verts = np.empty_like(verts0); sdf = np.empty_like(sdf0); scales = np.empty_like(scales0)
    verts[relabel], sdf[relabel], scales[relabel] = verts0, sdf0, scales0
    tets = relabel[tets0]
    order = np.argsort(rng.random((T, 4)), axis=1)
    tets = np.take_along_axis(tets, order, axis=1)[rng.permutation(T)]
    descending = (np.diff(tets, axis=1) < 0).any(axis=1)
    assert descending.mean() > 0.9, descending.mean()
    assert (sdf != 0).all()
    return verts, np.ascontiguousarray(tets.astype(np.int64)), sdf, scales


def _special(name):
    verts, tets, sdf, scales = _shuffled_grid((7, 6, 5), _seed(name))
    sdf, scales = sdf.copy(), scales.copy()
    for k, bits in enumerate(SPECIAL_BITS):
        sdf[2 + k::13] = np.array([bits], np.uint32).view(np.float32)[0]
    sc = scales.view(np.uint32)
    sc[0::11] = 0x7FC0BEEF          # NaN with a payload
    sc[4::11] = 0x7F800000          # +inf
    sc[7::11] = 0xFFFFFFFF          # -NaN, all payload bits
    return verts, tets, sdf, scales


# ---- random tets over a small pool ---------------------------------------------------------------------------------------------------
def _random_tets(rng, ids, T):
    """T tets of four distinct ids of `ids` (with repeats where fewer than four ids exist)"""
    ids = np.asarray(ids, np.int64)
    if len(ids) < 4:
        return ids[rng.integers(0, len(ids), (T, 4))]
    return ids[np.argsort(rng.random((T, len(ids))), axis=1)[:, :4]]


def _degenerate(name):
    rng = np.random.default_rng(_seed(name))
    pool, V = 300, 350                                            # 50 vertices referenced by no tet
    base = _random_tets(rng, np.arange(pool), 5000)
    dup = base[rng.integers(0, 5000, 200)]
    dup_perm = np.take_along_axis(base[rng.integers(0, 5000, 200)], np.argsort(rng.random((200, 4)), axis=1), axis=1)
    rep = base[rng.integers(0, 5000, 200)].copy()
    src, dst = rng.integers(0, 4, 200), rng.integers(1, 4, 200)
    rep[np.arange(200), (src + dst) % 4] = rep[np.arange(200), src]          # a repeated vertex: edges with a == b
    tets = np.concatenate([base, dup, dup_perm, rep])
    tets = tets[rng.permutation(len(tets))]
    verts = rng.random((V, 3), dtype=np.float32)
    sdf = rng.standard_normal(V, dtype=np.float32)
    scales = rng.uniform(0.1, 1, V).astype(np.float32)
    return verts, np.ascontiguousarray(tets), sdf, scales


def _size(name):
    rng = np.random.default_rng(_seed(name))
    V = 300
    verts = rng.random((V, 3), dtype=np.float32)
    sdf = rng.standard_normal(V, dtype=np.float32)
    scales = rng.uniform(0.1, 1, V).astype(np.float32)
    if name == "size_hole_12288":
        tets = _random_tets(rng, np.arange(V), 12288)
        tets[4096:8192] = _random_tets(rng, np.flatnonzero(inside(sdf)), 4096)      # no valid tet inside a whole 4096-block
        occ = inside(sdf)[tets].sum(1)
        assert (occ[4096:8192] == 4).all() and ((occ[:4096] % 4) != 0).any() and ((occ[8192:] % 4) != 0).any()
    else:
        tets = _random_tets(rng, np.arange(V), int(name.split("_")[1]))
    return verts, np.ascontiguousarray(tets), sdf, scales


def _vbits(name):
    V = int(name.split("_")[1])
    rng = np.random.default_rng(_seed(name))
    ids = np.unique(np.concatenate([np.array([0, 1, V - 2, V - 1]), rng.integers(0, V, 64)]))     # the top bit of bits_for(V - 1) decides the order
    tets = _random_tets(rng, ids, 2000)
    verts = rng.random((V, 3), dtype=np.float32)
    sdf = rng.standard_normal(V, dtype=np.float32)
    sdf[0], sdf[V - 1] = abs(sdf[0]) + np.float32(0.1), -abs(sdf[V - 1]) - np.float32(0.1)      # (a surface even where V = 2)
    scales = rng.random(V, dtype=np.float32) + np.float32(0.1)
    return verts, np.ascontiguousarray(tets), sdf, scales


_cache = {}


def case(name):
    """-> (verts, tets, sdf, scales); built once per process, read-only"""
    if name not in _cache:
        if name.startswith("single_"):
            c = _single(name)
        elif name.startswith("shuffled_"):
            c = _shuffled_grid(tuple(int(x) for x in name.split("_")[1:]), _seed(name))
        elif name.startswith("special_"):
            c = _special(name)
        elif name == "degenerate":
            c = _degenerate(name)
        elif name.startswith("size_"):
            c = _size(name)
        elif name.startswith("vbits_"):
            c = _vbits(name)
        else:
            raise KeyError(name)
        assert c[0].dtype == np.float32 and c[1].dtype == np.int64 and c[2].dtype == np.float32 and c[3].dtype == np.float32
        assert c[1].min() >= 0 and c[1].max() < len(c[0]) and len(c[2]) == len(c[3]) == len(c[0])
        for a in c:
            a.setflags(write=False)
        if c[0].nbytes > (64 << 20):
            return c                                               # (the 2^24 + 1 vertex case is not kept: 330 MB)
        _cache[name] = c
    return _cache[name]


# ---- chunk layouts on the (14,12,10) grid (the chunk size is overridden: gof_debug_mtets_chunk, oracle_binding.marching_tets) ---------
def chunk_cases():
    """-> [(label, (verts, tets, sdf, scales), chunk_size)]"""
    verts, tets, sdf, scales = case("shuffled_14_12_10")
    assert len(tets) == 10080
    for c in CHUNKS:                                               # torch.chunk(tets, T // c + 1): ceil(T / n) tets per chunk
        n = 10080 // c + 1 if 10080 > c else 1
        assert -(-10080 // n) == PER_CHUNK[c] and -(-10080 // PER_CHUNK[c]) <= 32, c
    out = [("chunk_%d" % c, (verts, tets, sdf, scales), c) for c in CHUNKS]
    # a chunk without a valid tet: 3 chunks of 3360 tets, the middle one made of tets the surface does not cross
    occ = inside(sdf)[tets].sum(1)
    invalid = np.flatnonzero((occ == 0) | (occ == 4))
    assert len(invalid) >= 3360
    mid = invalid[:3360]
    rest = np.setdiff1d(np.arange(len(tets)), mid)
    order = np.concatenate([rest[:3360], mid, rest[3360:]])
    t2 = np.ascontiguousarray(tets[order])
    occ2 = inside(sdf)[t2].sum(1) % 4
    assert (occ2[3360:6720] == 0).all() and (occ2[:3360] != 0).any() and (occ2[6720:] != 0).any()
    out.append(("chunk_empty_middle", (verts, t2, sdf, scales), 5040))
    # the last chunk is a single tet: 993 tets in chunks of 32 -> torch.chunk(., 32) -> 31 chunks of 32 and one of 1
    t3 = np.ascontiguousarray(tets[:993])
    n = 993 // 32 + 1
    per = -(-993 // n)
    assert n == 32 and per == 32 and 993 - 31 * per == 1
    out.append(("chunk_last_single", (verts, t3, sdf, scales), 32))
    return out


def big_chunked_case():
    """32 Mi + 17 random tets over 2^20 vertices of which 0.3 % are inside (about 1 % of the tets are crossed): the one input on which
    the REFERENCE's own chunk loop (utils/tetmesh.py:55-95) runs; 1 GB of tets, built on demand, not cached"""
    rng = np.random.default_rng(_seed("big_chunked"))
    V, T = 1 << 20, 32 * 1024 * 1024 + 17
    tets = rng.integers(0, V, (T, 4), dtype=np.int64)
    verts = rng.random((V, 3), dtype=np.float32)
    sdf = rng.standard_normal(V, dtype=np.float32) - np.float32(2.75)
    scales = rng.random(V, dtype=np.float32) + np.float32(0.1)
    return verts, tets, sdf, scales


TOO_MANY_CHUNKS = 300          # on 10 080 tets: 34 chunks of 297, more than the product's table holds (MT_MAX_CHUNKS = 32)


# ---- vertex ids outside [0, V): refused by gof_mtets_classify ----------------------------------------------------------------------------
def bad_id_cases(V, T):
    """(label, tet, corner, id): V, V + 2^32 (the low word of a legal id), -1 and INT64_MIN in the first tet, the last tet and the middle of
    a 4096-block"""
    out = []
    for vi, (vname, val) in enumerate((("V", V), ("V+2^32", V + (1 << 32)), ("-1", -1), ("INT64_MIN", -(1 << 63)))):
        for ti, (tname, t) in enumerate((("first", 0), ("last", T - 1), ("mid_block", 4096 + 2048))):
            out.append(("%s_%s" % (vname, tname), t, (vi + ti) % 4, val))
    return out


# ---- digests and comparisons ---------------------------------------------------------------------------------------------------------
def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def canonical(out):
    """(ids, pos, esdf, esc, faces) of any of the runners -> dict of arrays with the floats as bit patterns (NaN payloads count)"""
    ids, pos, esdf, esc, faces = out
    E = len(ids)
    u32 = lambda a, shape: np.ascontiguousarray(a, np.float32).reshape(shape).view(np.uint32)      # noqa: E731
    return {"ids": np.ascontiguousarray(ids, np.int64).reshape(E, 2), "faces": np.ascontiguousarray(faces, np.int64).reshape(-1, 3),
            "pos": u32(pos, (E, 2, 3)), "sdf": u32(esdf, (E, 2)), "scales": u32(esc, (E, 2))}


FIELDS = ("ids", "faces", "pos", "sdf", "scales")
INLINE_BYTES = 160 << 10         # a golden case larger than this keeps sha256 digests of its arrays instead of the arrays


def assert_same(got, want, what):
    g, w = canonical(got), canonical(want)
    for f in FIELDS:
        assert g[f].shape == w[f].shape, (what, f, g[f].shape, w[f].shape)
        assert np.array_equal(g[f], w[f]), (what, f, int((g[f] != w[f]).sum()))


def assert_matches_golden(G, name, inputs, got):
    """G: the loaded ref_mtets_golden.npz"""
    assert str(G[name + "__in"]) == digest(*inputs), "the generator of %s drifted from the golden's inputs" % name
    g = canonical(got)
    E, F = [int(x) for x in G[name + "__EF"]]
    assert (len(g["ids"]), len(g["faces"])) == (E, F), (name, len(g["ids"]), len(g["faces"]), E, F)
    for f in FIELDS:
        key = "%s__%s" % (name, f)
        if key in G.files:
            assert np.array_equal(g[f], G[key].astype(g[f].dtype)), (name, f, int((g[f] != G[key]).sum()))
        else:
            assert digest(g[f]) == str(G[key + "_sha"]), (name, f)


# ---- a check of the output alone -----------------------------------------------------------------------------------------------------
def check_surface(inputs, out, oriented=False):
    """What any correct marching tetrahedra must produce, from the geometry alone:
      * the edge rows are strictly ascending in (min, max) with min <= max, and carry their end points' position, sdf and scale;
      * every edge row has exactly one end with sdf > 0; every face index lies in [0, E);
      * oriented (tets with four distinct vertices, distinct vertex sets, finite non-zero sdf: the shuffled grids): every face lies
        in exactly one tet -- its three edges span the tet's four vertices -- and, with the crossing points interpolated at the sdf's
        zero, its normal points towards the tet's sdf > 0 vertices if the tet is positively oriented, away from them if negatively."""
    verts, tets, sdf, scales = inputs
    ids, pos, esdf, esc, faces = out
    ids = np.asarray(ids).reshape(-1, 2); faces = np.asarray(faces).reshape(-1, 3)
    E = len(ids)
    assert (ids[:, 0] <= ids[:, 1]).all()
    key = ids[:, 0] * (1 << 32) + ids[:, 1]
    assert (np.diff(key) > 0).all(), "edge rows not strictly ascending in (min, max)"
    assert (inside(sdf)[ids].sum(1) == 1).all(), "an edge row without exactly one end inside"
    assert np.array_equal(np.asarray(pos, np.float32).reshape(E, 2, 3).view(np.uint32), verts[ids].view(np.uint32))
    assert np.array_equal(np.asarray(esdf, np.float32).reshape(E, 2).view(np.uint32), sdf[ids].view(np.uint32))
    assert np.array_equal(np.asarray(esc, np.float32).reshape(E, 2).view(np.uint32), scales[ids].view(np.uint32))
    if len(faces):
        assert faces.min() >= 0 and faces.max() < E
    occ = inside(sdf)[tets]
    ntri = np.array([0, 1, 2, 1, 0])[occ.sum(1)]
    assert len(faces) == ntri.sum()
    if not oriented:
        return
    tet_of = {tuple(sorted(t)): i for i, t in enumerate(tets.tolist())}
    assert len(tet_of) == len(tets)
    P = verts.astype(np.float64); s = sdf.astype(np.float64)
    a, b = ids[:, 0], ids[:, 1]
    w = (s[a] / (s[a] - s[b]))[:, None]
    cross = P[a] + (P[b] - P[a]) * w                                # the crossing point of every edge row
    seen = np.zeros(len(tets), np.int64)
    for f in faces:
        t = tet_of[tuple(sorted(set(ids[f].reshape(-1).tolist())))]      # KeyError: the face's edges do not span one tet
        seen[t] += 1
        q = P[tets[t]]
        vol = np.linalg.det(q[1:] - q[0])
        assert vol != 0
        towards = q[occ[t]].mean(0) - q[~occ[t]].mean(0)
        c = cross[f]
        d = np.dot(np.cross(c[1] - c[0], c[2] - c[0]), towards)
        assert d * vol > 0, (t, d, vol)
    assert np.array_equal(seen, ntri), "a tet without its 1 or 2 triangles"
