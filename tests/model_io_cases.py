"""The models, files and expectations the model-file tests share (tests/test_model_io_host.py through the emulator, tests/test_model_io_gpu.py
on the device, tests/golden/make_golden_ply.py for the reference's side).  numpy only: no torch, no product module."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ref_model_ply_golden.npz")
f32 = np.float32

# (tag, sh degree, P): the golden's five models
GOLDEN_MODELS = (("d0", 0, 5), ("d1", 1, 5), ("d2", 2, 5), ("d3", 3, 5), ("big", 3, 130))
FIELDS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "filter_3D")
# the issue's bar for the fused columns: the project's bar for these activations (tests/test_train_epilogue_gpu.py) on top of what the
# reference's own log-then-exp loses (roundtrip_rel, recorded in the golden)
ACT_REL = 3e-6


def golden():
    return dict(np.load(GOLDEN))


def shapes(P, K):
    return dict(zip(FIELDS, [(P, 3), (P, 1, 3), (P, K, 3), (P, 1), (P, 3), (P, 4), (P, 1)]))


def make_model(degree, P, seed):
    """A seeded model as float32 arrays in the model's own layouts.  Raw opacities in [-6, 6], filter_3D comparable to the scales: the
    inverse sigmoid of the fused file is exercised near both ends without saturating."""
    K = (degree + 1) ** 2 - 1
    rng = np.random.default_rng(1000 + seed)
    m = {"xyz": rng.normal(0, 3, (P, 3)), "f_dc": rng.normal(0, 1, (P, 1, 3)), "f_rest": rng.normal(0, 0.2, (P, K, 3)),
         "opacity": rng.uniform(-6, 6, (P, 1)), "scaling": np.log(rng.uniform(0.005, 0.05, (P, 3))),
         "rotation": rng.normal(0, 1, (P, 4)), "filter_3D": rng.uniform(0.005, 0.05, (P, 1))}
    return {k: np.ascontiguousarray(v, f32) for k, v in m.items()}


def golden_model(tag):
    for i, (t, d, P) in enumerate(GOLDEN_MODELS):
        if t == tag:
            return make_model(d, P, i)
    raise KeyError(tag)


def special_model(P=70, degree=1):
    """a model whose _xyz holds -0.0, denormals, +-inf and NaNs with payloads (a pure-movement path must carry every bit)"""
    m = make_model(degree, P, 77)
    bits = m["xyz"].view(np.uint32).reshape(-1)
    bits[:12] = [0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFBFFFFF,
                 0x00400000, 0x7FFFFFFF]
    bits[-3:] = [0x7FA5A5A5, 0x80000000, 0xFF800000]
    return m


def names(K, fused=False):
    n = ["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(3 * K)]
    n += ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]
    return n if fused else n + ["filter_3D"]


def header(P, nm, types=None, fmt="binary_little_endian", extra=""):
    types = types or ["float"] * len(nm)
    return ("ply\nformat %s 1.0\n%selement vertex %d\n" % (fmt, extra, P) + "".join("property %s %s\n" % (t, n) for t, n in zip(types, nm))
            + "end_header\n").encode("ascii")


def raw_rows(m):
    """the RAW rows of a model, restated from the layout the issue states (float32 (P, 18 + 3K)): independent of the product's code"""
    P, K = m["f_rest"].shape[0], m["f_rest"].shape[1]
    cols = [m["xyz"], np.zeros((P, 3), f32), m["f_dc"].transpose(0, 2, 1).reshape(P, 3), m["f_rest"].transpose(0, 2, 1).reshape(P, 3 * K),
            m["opacity"], m["scaling"], m["rotation"], m["filter_3D"]]
    return np.ascontiguousarray(np.concatenate(cols, axis=1), f32)


def from_rows(rows, K):
    """(P, 18 + 3K) float32 rows -> the seven arrays in the model's layouts (the inverse of raw_rows)"""
    P = rows.shape[0]
    r = np.ascontiguousarray(rows, f32)
    o = 9 + 3 * K
    return {"xyz": r[:, 0:3].copy(), "f_dc": r[:, 6:9].reshape(P, 3, 1).transpose(0, 2, 1).copy(),
            "f_rest": r[:, 9:o].reshape(P, 3, K).transpose(0, 2, 1).copy(), "opacity": r[:, o:o + 1].copy(),
            "scaling": r[:, o + 1:o + 4].copy(), "rotation": r[:, o + 4:o + 8].copy(), "filter_3D": r[:, o + 8:o + 9].copy()}


def channel_offsets(K):
    """[(byte offset, type code 0 = float32)] of the model's channels inside a RAW row, in the column table's order"""
    return [(4 * c, 0) for c in list(range(3)) + list(range(6, 18 + 3 * K))]


def f64_values(col):
    """what the float64-typed variant of a file holds for a float32 column: values BETWEEN float32s (so the rounding is exercised),
    a deterministic function of the column"""
    v = np.asarray(col, np.float64)
    i = np.arange(v.size, dtype=np.float64).reshape(v.shape)
    return v * (1.0 + (np.mod(i, 7.0) - 3.0) * 2.0 ** -25)     # up to 1.5 float32 ulp away: some round back, some to a neighbour


def f64_variant(m):
    """A structured array of the model with `double` opacity and scale_* columns -> (array, names, types)"""
    P, K = m["f_rest"].shape[0], m["f_rest"].shape[1]
    nm = names(K)
    dbl = {"opacity", "scale_0", "scale_1", "scale_2"}
    types = ["double" if n in dbl else "float" for n in nm]
    arr = np.zeros(P, [(n, "<f8" if n in dbl else "<f4") for n in nm])
    rows = raw_rows(m)
    for j, n in enumerate(nm):
        arr[n] = f64_values(rows[:, j]) if n in dbl else rows[:, j]
    return arr, nm, types


def shuffled_variant(m, seed=3, lead_uchar=True):
    """The model's file with the properties in a shuffled order, behind an extra `uchar` property: every offset odd, the pitch (253 + ...)
    no multiple of 4 -> (array, names, types)"""
    P, K = m["f_rest"].shape[0], m["f_rest"].shape[1]
    nm = names(K)
    order = list(np.random.default_rng(seed).permutation(len(nm)))
    rows = raw_rows(m)
    fields = ([("flag", "u1")] if lead_uchar else []) + [(nm[j], "<f4") for j in order]
    arr = np.zeros(P, fields)
    if lead_uchar:
        arr["flag"] = np.arange(P) % 251
    for j in order:
        arr[nm[j]] = rows[:, j]
    return arr, [f[0] for f in fields], [("uchar" if f[1] == "u1" else "float") for f in fields]


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def fused_errors(rows_fused, K, act_opacity, act_scaling):
    """largest relative difference between sigmoid64 / exp64 of a fused file's opacity / scale columns and the activated tensors"""
    o = 9 + 3 * K
    op = sigmoid64(rows_fused[:, o:o + 1])
    sc = np.exp(np.asarray(rows_fused[:, o + 1:o + 4], np.float64))
    a, s = np.asarray(act_opacity, np.float64), np.asarray(act_scaling, np.float64)
    return float(np.abs(op / a - 1.0).max()), float(np.abs(sc / s - 1.0).max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
