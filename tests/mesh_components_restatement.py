"""The contract of the mesh connected components restated in plain Python / numpy, for the tests: a sequential
union-find over the faces, the numbering, the per-face areas and the written summation order, the selection and the compaction by
boolean indexing; and, independently of the union-find, the labels through scipy.sparse.csgraph.connected_components.
Test infrastructure only."""
import math

import numpy as np

from mesh_cull_restatement import ply_bytes  # noqa: F401  (the exported file's bytes: the culling unit's restatement of DeviceMesh.export)

SUM_TILE, SUM_BLOCK = 256, 65536


# ---- labels --------------------------------------------------------------------------------------------------------------------------
def _edges(F):
    """(3 NF, 2) the faces' unordered index pairs (0,1), (1,2), (2,0), smaller index first; row 3 f + k belongs to face f"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    e = np.stack([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]], axis=1).reshape(-1, 2)
    return np.sort(e, axis=1)


def labels(F, connectivity="edge"):
    """face_label (NF,) int32: the smallest face index of the face's component -- a sequential union-find"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    nf = len(F)
    parent = list(range(nf))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    first = {}
    if connectivity == "edge":
        for i, (lo, hi) in enumerate(_edges(F).tolist()):
            f = i // 3
            g = first.setdefault((lo, hi), f)
            if g != f:
                union(f, g)
    elif connectivity == "vertex":
        for f, tri in enumerate(F.tolist()):
            for v in tri:
                g = first.setdefault(v, f)
                if g != f:
                    union(f, g)
    else:
        raise KeyError(connectivity)
    return np.array([find(f) for f in range(nf)], np.int32).reshape(nf)


def numbering(label):
    """-> (face_comp (NF,) int32: the rank of the face's label among all roots, C)"""
    label = np.asarray(label, np.int64)
    roots = np.flatnonzero(label == np.arange(len(label)))
    return np.searchsorted(roots, label).astype(np.int32), len(roots)


def scipy_labels(F, connectivity="edge"):
    """the same labels by another road: an adjacency matrix over the faces from np.unique over the sorted edges (vertices), SciPy's
    connected components, and SciPy's labels mapped to the smallest face index of each"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    F = np.asarray(F, np.int64).reshape(-1, 3)
    nf = len(F)
    if nf == 0:
        return np.zeros(0, np.int32)
    if connectivity == "edge":
        e = _edges(F)
        _, group = np.unique(e[:, 0] * (2 ** 31) + e[:, 1], return_inverse=True)
        owner = np.repeat(np.arange(nf), 3)
    else:
        _, group = np.unique(F.reshape(-1), return_inverse=True)
        owner = np.repeat(np.arange(nf), 3)
    group = group.reshape(-1)
    # every face of a group is joined to the group's smallest face: a star per group connects what the group connects
    smallest = np.full(group.max() + 1, nf, np.int64)
    np.minimum.at(smallest, group, owner)
    adj = coo_matrix((np.ones(len(owner), np.int8), (owner, smallest[group])), shape=(nf, nf))
    _, lab = connected_components(adj, directed=False)
    root = np.full(lab.max() + 1, nf, np.int64)
    np.minimum.at(root, lab, np.arange(nf))
    return root[lab].astype(np.int32)


# ---- measures ------------------------------------------------------------------------------------------------------------------------
def face_areas(V, F):
    """fp64, in the contract's order (numpy performs every operation on its own: nothing is contracted)"""
    V = np.asarray(V, np.float64).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        v0, v1, v2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        e1, e2 = v1 - v0, v2 - v0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def _left_to_right(values):
    s = values[0]
    for x in values[1:]:
        s = s + x
    return s


def segment_sum(a, s, e):
    """a: the areas in sorted order (a list of Python floats), [s, e) one component's positions, s < e: tiles of 256 aligned positions
    from left to right, the tile sums of a block of 65536 aligned positions from left to right, the block sums from left to right"""
    blocks = []
    p = s
    while p < e:
        block_end = min(e, (p // SUM_BLOCK + 1) * SUM_BLOCK)
        tiles = []
        q = p
        while q < block_end:
            tile_end = min(block_end, (q // SUM_TILE + 1) * SUM_TILE)
            tiles.append(_left_to_right(a[q:tile_end]))
            q = tile_end
        blocks.append(_left_to_right(tiles))
        p = block_end
    return _left_to_right(blocks)


def stats(V, F, face_comp, C):
    """-> (faces (C,) int64, first_face (C,) int32, area (C,) float64)"""
    face_comp = np.asarray(face_comp, np.int64)
    order = np.argsort(face_comp, kind="stable")
    a = face_areas(V, F)[order].tolist()
    start = np.searchsorted(face_comp[order], np.arange(C + 1))
    cf = np.diff(start).astype(np.int64)
    first = np.array([order[start[c]] if cf[c] else -1 for c in range(C)], np.int32).reshape(C)
    area = np.array([segment_sum(a, int(start[c]), int(start[c + 1])) if cf[c] else 0.0 for c in range(C)], np.float64).reshape(C)
    return cf, first, area


def total_area(area):
    total = 0.0
    for i, x in enumerate(np.asarray(area, np.float64).tolist()):
        total = x if i == 0 else total + x
    return total


# ---- selection and compaction --------------------------------------------------------------------------------------------------------
def select(cf, area, largest=None, by="faces", min_faces=None, min_area_ratio=None):
    C = len(cf)
    keep = [True] * C
    if largest is not None:
        def rank(c):
            if by == "faces":
                return (0, -int(cf[c]), c)
            x = float(area[c])
            return (1, 0.0, c) if math.isnan(x) else (0, -x, c)
        chosen = set(sorted(range(C), key=rank)[:largest])
        keep = [k and c in chosen for c, k in enumerate(keep)]
    if min_faces is not None:
        keep = [k and int(cf[c]) >= min_faces for c, k in enumerate(keep)]
    if min_area_ratio is not None:
        bound = min_area_ratio * total_area(area)
        keep = [k and bool(float(area[c]) > bound) for c, k in enumerate(keep)]
    return np.array(keep, bool).reshape(C)


def keep_faces(face_mask, V, F, N=None, Col=None):
    """boolean indexing: the kept faces, the vertices they refer to, both in their original order -> (V, F, N, Col)"""
    F2 = np.asarray(F)[np.asarray(face_mask, bool)]
    ref = np.zeros(len(V), bool)
    ref[F2.reshape(-1)] = True
    new = np.cumsum(ref) - 1
    return (np.asarray(V)[ref], new[F2].astype(np.int32).reshape(-1, 3), None if N is None else np.asarray(N)[ref],
            None if Col is None else np.asarray(Col)[ref])


def keep_components(V, F, N=None, Col=None, connectivity="edge", **criteria):
    """-> (V, F, N, Col, kept, dropped)"""
    comp, C = numbering(labels(F, connectivity))
    cf, _, area = stats(V, F, comp, C)
    keep = select(cf, area, **criteria)
    mask = keep[comp] if len(comp) else np.zeros(0, bool)
    return keep_faces(mask, V, F, N, Col) + (int(keep.sum()), int(C - keep.sum()))
