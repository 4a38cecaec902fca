"""The runs and the checks the two model-file test files share: tests/test_model_io_host.py performs the runs in a child process over the
emulated library (every buffer the product allocates poisoned and guarded), tests/test_model_io_gpu.py on the device with tensors that
lie inside larger poisoned allocations.  A run takes the product module and three helpers and returns arrays; a check takes what a run
returned and asserts against the committed golden (the reference's side) and the layout restated in model_io_cases.

    up(array) -> a tensor holding it, where the library can read it       alloc(shape) -> a poisoned float32 tensor to write into
    down(tensor) -> numpy array
"""
import importlib.util
import os

import numpy as np

import model_io_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
EDGE_P = (0, 1, 63, 64, 65, 129)                    # tile (64 rows) and chunk edges
SUB_RANGES = ((0, 0), (1, 1), (3, 64), (60, 70), (129, 1), (130, 0), (64, 64))
CHUNKS = (1, 64, 100)
POISON_F32 = np.frombuffer(b"\xA5" * 4, np.float32)[0]


def e2e_plyfile():
    """tests/e2e_shims/plyfile.py under a name of its own (it is not on the path, and must not shadow anything)"""
    spec = importlib.util.spec_from_file_location("e2e_shims_plyfile", os.path.join(HERE, "e2e_shims", "plyfile.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Model:
    """what save_ply / load_ply touch of a GaussianModel"""

    def __init__(self, degree):
        self.max_sh_degree, self.active_sh_degree = degree, 0


def model_of(m, up):
    K_ = m["f_rest"].shape[1]
    g = Model(int(round((K_ + 1) ** 0.5)) - 1)
    for attr, key in (("_xyz", "xyz"), ("_features_dc", "f_dc"), ("_features_rest", "f_rest"), ("_opacity", "opacity"),
                      ("_scaling", "scaling"), ("_rotation", "rotation"), ("filter_3D", "filter_3D")):
        setattr(g, attr, up(m[key]))
    return g


def tensors_of(m, up):
    return [up(m[f]) for f in K.FIELDS]


def arrays_of(g, down):
    return {"xyz": down(g._xyz), "f_dc": down(g._features_dc), "f_rest": down(g._features_rest), "opacity": down(g._opacity),
            "scaling": down(g._scaling), "rotation": down(g._rotation), "filter_3D": down(g.filter_3D)}


def u8(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


class chunk_rows:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get("GOF_PLY_CHUNK_ROWS")
        os.environ["GOF_PLY_CHUNK_ROWS"] = str(self.n)

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["GOF_PLY_CHUNK_ROWS"]
        else:
            os.environ["GOF_PLY_CHUNK_ROWS"] = self.old


def prefix(m, P):
    return {k: np.ascontiguousarray(v[:P]) for k, v in m.items()}


# ---- RAW pack ------------------------------------------------------------------------------------------------------------------------
def run_raw(MIO, up, alloc, down, tmp):
    res = {}
    for tag, _, _ in K.GOLDEN_MODELS:
        res["raw_" + tag] = u8(down(MIO.pack_rows(tensors_of(K.golden_model(tag), up))))
    big = K.golden_model("big")
    for P in EDGE_P:
        m = prefix(big, P)
        out = alloc((P * 63 + 5,))                  # (5 words behind the rows: they must keep their poison)
        rows = MIO.pack_rows(tensors_of(m, up), out=out)
        res["raw_P%d" % P] = u8(down(rows))
        res["raw_P%d_tail" % P] = u8(down(out)[P * 63:])
    ts = tensors_of(big, up)
    for first, count in SUB_RANGES:
        res["raw_sub_%d_%d" % (first, count)] = u8(down(MIO.pack_rows(ts, first=first, count=count)))
    for n in CHUNKS:
        path = os.path.join(tmp, "raw_chunk%d.ply" % n)
        with chunk_rows(n):
            MIO.save_ply(model_of(big, up), path)
        res["raw_file_%d" % n] = np.fromfile(path, np.uint8)
        res["raw_file_%d_chunks" % n] = np.array(MIO.last_stats()["save"]["chunks"])
    path = os.path.join(tmp, "deep", "er", "empty.ply")             # mkdir_p, and a header-only file
    MIO.save_ply(model_of(prefix(big, 0), up), path)
    res["raw_file_empty"] = np.fromfile(path, np.uint8)
    return res


def check_raw(res, g):
    for tag, d, P in K.GOLDEN_MODELS:
        m = K.golden_model(tag)
        assert K.raw_rows(m).tobytes() == g[tag + "_raw"].tobytes(), "the cases' models are not the golden's"
        assert res["raw_" + tag].tobytes() == g[tag + "_raw"].tobytes(), tag
    big = K.golden_model("big")
    ref = np.frombuffer(g["big_raw"].tobytes(), np.float32).reshape(130, 63)
    assert not np.signbit(ref[:, 3:6]).any() and (ref[:, 3:6] == 0).all()
    for P in EDGE_P:
        assert res["raw_P%d" % P].tobytes() == ref[:P].tobytes(), P
        assert (res["raw_P%d_tail" % P] == 0xA5).all(), "pack wrote behind its %d rows" % P
    for first, count in SUB_RANGES:
        assert res["raw_sub_%d_%d" % (first, count)].tobytes() == ref[first:first + count].tobytes(), (first, count)
    want = K.header(130, K.names(15)) + ref.tobytes()
    for n in CHUNKS:
        assert res["raw_file_%d" % n].tobytes() == want, n
        assert int(res["raw_file_%d_chunks" % n]) == -(-130 // n)
    assert res["raw_file_empty"].tobytes() == K.header(0, K.names(15))
    assert big["xyz"].shape == (130, 3)


# ---- unpack --------------------------------------------------------------------------------------------------------------------------
def _dests(alloc, P, Kc):
    return [alloc(s) for s in K.shapes(P, Kc).values()]


def _columns(arr, Kc, dbl=()):
    ch = [n for n in K.names(Kc) if n not in ("nx", "ny", "nz")]
    return [(arr.dtype.fields[n][1], 1 if n in dbl else 0) for n in ch]


def run_unpack(MIO, up, alloc, down, tmp):
    res = {}
    dbl = ("opacity", "scale_0", "scale_1", "scale_2")
    for tag, _, P in K.GOLDEN_MODELS:
        m = K.golden_model(tag)
        Kc = m["f_rest"].shape[1]
        d = _dests(alloc, P, Kc)
        MIO.unpack_rows(up(u8(K.raw_rows(m))), 4 * (18 + 3 * Kc), K.channel_offsets(Kc), d)
        for f, t in zip(K.FIELDS, d):
            res["unpack_%s_%s" % (tag, f)] = down(t)
        arr, _, _ = K.f64_variant(m)
        d = _dests(alloc, P, Kc)
        MIO.unpack_rows(up(u8(arr)), arr.itemsize, _columns(arr, Kc, dbl), d)
        for f, t in zip(K.FIELDS, d):
            res["f64_%s_%s" % (tag, f)] = down(t)
    big = K.golden_model("big")
    arr, _, _ = K.shuffled_variant(big)
    assert arr.itemsize % 4 == 1 and all(o % 2 == 1 for o, _ in _columns(arr, 15))
    d = _dests(alloc, 130, 15)
    MIO.unpack_rows(up(u8(arr)), arr.itemsize, _columns(arr, 15), d)           # (exactly 130 * pitch bytes: the last row ends the buffer)
    for f, t in zip(K.FIELDS, d):
        res["shuffled_" + f] = down(t)
    # a sub-range: rows 60..129 of the file into rows 60..129 of the model; rows 0..59 keep their poison
    d = _dests(alloc, 130, 15)
    MIO.unpack_rows(up(u8(K.raw_rows(big)[60:])), 252, K.channel_offsets(15), d, first=60, count=70)
    for f, t in zip(K.FIELDS, d):
        res["sub_" + f] = down(t)
    return res


def check_unpack(res, g):
    for tag, _, P in K.GOLDEN_MODELS:
        for f in K.FIELDS:
            assert K.same_bits(res["unpack_%s_%s" % (tag, f)], g["%s_load_%s" % (tag, f)]), (tag, f)
            assert K.same_bits(res["f64_%s_%s" % (tag, f)], g["%s_load64_%s" % (tag, f)]), (tag, f)
        assert not K.same_bits(g[tag + "_load64_opacity"], g[tag + "_load_opacity"])          # (the variant's values differ: it bites)
    big = K.golden_model("big")
    for f in K.FIELDS:
        assert K.same_bits(res["shuffled_" + f], g["big_load_" + f]), f
        assert K.same_bits(res["shuffled_" + f], big[f]), f
        got = res["sub_" + f]
        assert K.same_bits(got[60:], big[f][60:]), f
        assert (u8(got[:60]) == 0xA5).all(), "unpack wrote rows it was not given (%s)" % f


# ---- files: round trips, the other plyfile stand-in, ASCII ------------------------------------------------------------------------------
def _load(MIO, path, degree, down):
    h = Model(degree)
    MIO.load_ply(h, path)
    import torch
    for attr in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        t = getattr(h, attr)
        assert isinstance(t, torch.nn.Parameter) and t.requires_grad and t.dtype == torch.float32 and t.is_contiguous(), attr
    assert not isinstance(h.filter_3D, torch.nn.Parameter) and not h.filter_3D.requires_grad and h.filter_3D.dtype == torch.float32
    assert h.active_sh_degree == degree
    return arrays_of(h, down)


def run_files(MIO, up, alloc, down, tmp):
    res = {}
    models = [(tag, K.golden_model(tag), d) for tag, d, _ in K.GOLDEN_MODELS] + [("special", K.special_model(), 1)]
    for tag, m, d in models:
        path = os.path.join(tmp, "rt_%s.ply" % tag)
        with chunk_rows(64 if tag == "big" else 3):
            MIO.save_ply(model_of(m, up), path)
        with chunk_rows(50 if tag == "big" else 2):
            got = _load(MIO, path, d, down)
        for f in K.FIELDS:
            res["rt_%s_%s" % (tag, f)] = got[f]
    big = K.golden_model("big")
    ply = e2e_plyfile()
    # what save_ply wrote, read by the other stand-in
    el = ply.PlyData.read(os.path.join(tmp, "rt_big.ply")).elements[0]
    res["e2e_read_names"] = np.array(" ".join(p.name for p in el.properties))
    res["e2e_read_rows"] = np.stack([el[n] for n in K.names(15)], axis=1)
    # a file the other stand-in writes (the f64 variant and the shuffled one: foreign layouts), loaded here
    for name, (arr, _, _) in (("f64", K.f64_variant(big)), ("shuffled", K.shuffled_variant(big))):
        path = os.path.join(tmp, "e2e_%s.ply" % name)
        ply.PlyData([ply.PlyElement.describe(arr, "vertex")]).write(path)
        with chunk_rows(33):
            got = _load(MIO, path, 3, down)
        for f in K.FIELDS:
            res["e2e_%s_%s" % (name, f)] = got[f]
    # ASCII, with comment lines, an element behind vertex and a float64 column
    m = K.golden_model("d1")
    arr, nm, types = K.f64_variant(m)
    path = os.path.join(tmp, "ascii.ply")
    with open(path, "wb") as fh:
        fh.write(K.header(5, nm, types, fmt="ascii", extra="comment made by a test\nobj_info nothing\n")
                 .replace(b"end_header\n", b"element face 1\nproperty list uchar int vertex_indices\nend_header\n"))
        for row in arr:
            fh.write((" ".join(repr(float(row[n])) if t == "double" else "%.9g" % row[n] for n, t in zip(nm, types)) + "\n").encode())
        fh.write(b"3 0 1 2\n")
    got = _load(MIO, path, 1, down)
    for f in K.FIELDS:
        res["ascii_" + f] = got[f]
    return res


def check_files(res, g):
    for tag, m, in [(t, K.golden_model(t)) for t, _, _ in K.GOLDEN_MODELS] + [("special", K.special_model())]:
        for f in K.FIELDS:
            assert K.same_bits(res["rt_%s_%s" % (tag, f)], m[f]), (tag, f)
    sp = K.special_model()["xyz"]
    assert np.isnan(sp).sum() >= 6 and np.isinf(sp).sum() >= 3 and (np.abs(sp[np.isfinite(sp)]) < 1e-38).sum() >= 4
    assert str(res["e2e_read_names"]) == " ".join(K.names(15))
    assert res["e2e_read_rows"].tobytes() == g["big_raw"].tobytes()
    for f in K.FIELDS:
        assert K.same_bits(res["e2e_f64_" + f], g["big_load64_" + f]), f
        assert K.same_bits(res["e2e_shuffled_" + f], g["big_load_" + f]), f
        assert K.same_bits(res["ascii_" + f], g["d1_load64_" + f]), f


# ---- FUSED ---------------------------------------------------------------------------------------------------------------------------
def run_fused(MIO, up, alloc, down, tmp):
    res = {}
    for tag, _, P in K.GOLDEN_MODELS:
        ts = tensors_of(K.golden_model(tag), up)
        res["fused_" + tag] = down(MIO.pack_rows(ts, mode=MIO.FUSED))
        res["fused_again_" + tag] = down(MIO.pack_rows(ts, mode=MIO.FUSED))
    big = K.golden_model("big")
    for n in (64, 100):
        path = os.path.join(tmp, "fused_chunk%d.ply" % n)
        with chunk_rows(n):
            MIO.save_fused_ply(model_of(big, up), path)
        res["fused_file_%d" % n] = np.fromfile(path, np.uint8)
    return res


def check_fused(res, g):
    """every column but opacity and scale byte-equal to the golden; those four within ACT_REL + roundtrip_rel of the golden's activated
    tensors after sigmoid64 / exp64; two runs and two chunk lengths identical"""
    for tag, d, P in K.GOLDEN_MODELS:
        Kc = (d + 1) ** 2 - 1
        C = 17 + 3 * Kc
        got = res["fused_" + tag]
        ref = np.frombuffer(g[tag + "_fused"].tobytes(), np.float32).reshape(P, C)
        assert got.shape == (P, C) and got.dtype == np.float32
        o = 9 + 3 * Kc
        moved = [c for c in range(C) if not o <= c < o + 4]
        assert got[:, moved].tobytes() == ref[:, moved].tobytes(), tag
        e_op, e_sc = K.fused_errors(got, Kc, g[tag + "_act_opacity"], g[tag + "_act_scaling"])
        bound = K.ACT_REL + float(g[tag + "_roundtrip_rel"])
        print("fused %s: opacity %.3g, scale %.3g relative (bound %.3g; the reference's own round trip %.3g)" % (tag, e_op, e_sc, bound, float(g[tag + "_roundtrip_rel"])))
        assert e_op <= bound and e_sc <= bound, (tag, e_op, e_sc, bound)
        assert got.tobytes() == res["fused_again_" + tag].tobytes()
    want = K.header(130, K.names(15, fused=True)) + res["fused_big"].tobytes()
    assert res["fused_file_64"].tobytes() == want and res["fused_file_100"].tobytes() == want


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def run_errors(MIO, up, alloc, down, tmp):
    import ctypes as C
    res = {}
    m = K.golden_model("d1")
    rows = K.raw_rows(m)
    nm = K.names(3)

    def attempt(name, data, degree=1):
        path = os.path.join(tmp, "bad_%s.ply" % name)
        with open(path, "wb") as fh:
            fh.write(data)
        h = Model(degree)
        try:
            MIO.load_ply(h, path)
            res["err_" + name] = np.array("no error")
        except Exception as e:      # noqa: BLE001  (the test looks at the kind and the text)
            res["err_" + name] = np.array("%s: %s" % (type(e).__name__, e))
        res["err_%s_untouched" % name] = np.array(not hasattr(h, "_xyz") and h.active_sh_degree == 0)

    attempt("list", K.header(5, nm).replace(b"property float opacity\n", b"property list uchar float opacity\n") + rows.tobytes())
    attempt("big_endian", K.header(5, nm, fmt="binary_big_endian") + rows.astype(">f4").tobytes())
    attempt("truncated", K.header(5, nm) + rows.tobytes()[:-1])
    attempt("no_filter", K.header(5, nm[:-1]) + np.ascontiguousarray(rows[:, :-1]).tobytes())
    attempt("f_rest_count", K.header(5, nm) + rows.tobytes(), degree=2)
    types = ["int" if n == "opacity" else "float" for n in nm]
    attempt("int_opacity", K.header(5, nm, types) + rows.tobytes())
    # the entry point itself: an integer-typed channel -> a return code, a message, and destinations that keep their poison
    d = _dests(alloc, 5, 3)
    cols = K.channel_offsets(3)
    cols[6 + 9] = (cols[6 + 9][0], 6)            # opacity as int32
    src = up(u8(rows))
    tab = MIO.column_table(cols)
    args = [src.data_ptr(), 4 * 27, tab] + [t.data_ptr() for t in d] + [None]
    rc = MIO.lib.gof_model_unpack(5, 3, 0, 5, *args)
    res["rc_int_column"] = np.array("%d %s" % (rc, MIO.lib.gof_last_error().decode()))
    cols = K.channel_offsets(3)
    cols[-1] = (4 * 27 - 3, 0)                   # the last channel would end one byte behind the row
    args[2] = MIO.column_table(cols)
    rc = MIO.lib.gof_model_unpack(5, 3, 0, 5, *args)
    res["rc_column_outside"] = np.array("%d %s" % (rc, MIO.lib.gof_last_error().decode()))
    rc = MIO.lib.gof_model_unpack(5, 3, 3, 3, *args[:2], tab, *args[3:])
    res["rc_range"] = np.array("%d" % rc)
    rc = MIO.lib.gof_model_pack(5, 3, 0, 6, *[t.data_ptr() for t in d], 0, src.data_ptr(), None)
    res["rc_pack_range"] = np.array("%d" % rc)
    rc = MIO.lib.gof_model_pack(5, 25, 0, 5, *[t.data_ptr() for t in d], 0, src.data_ptr(), None)
    res["rc_pack_k"] = np.array("%d" % rc)
    rc = MIO.lib.gof_model_pack(5, 3, 0, 5, *[t.data_ptr() for t in d], 2, src.data_ptr(), None)
    res["rc_pack_mode"] = np.array("%d" % rc)
    res["dests_poison"] = np.array(all((u8(down(t)) == 0xA5).all() for t in d))
    res["src_unchanged"] = np.array(down(src).tobytes() == rows.tobytes())
    assert C.sizeof(MIO.GofModelColumn) == 16
    return res


def check_errors(res):
    def err(name):
        return str(res["err_" + name])
    assert err("list").startswith("ValueError") and "list property" in err("list") and "opacity" in err("list")
    assert err("big_endian").startswith("ValueError") and "binary_big_endian" in err("big_endian")
    assert err("truncated").startswith("ValueError") and "truncated" in err("truncated")
    assert err("no_filter").startswith("ValueError") and "'filter_3D'" in err("no_filter")
    assert err("f_rest_count").startswith("AssertionError")
    assert err("int_opacity").startswith("ValueError") and "'opacity'" in err("int_opacity") and "integer" in err("int_opacity")
    for name in ("list", "big_endian", "truncated", "no_filter", "f_rest_count", "int_opacity"):
        assert bool(res["err_%s_untouched" % name]), name
    assert str(res["rc_int_column"]).startswith("-1 ") and "integer type" in str(res["rc_int_column"])
    assert str(res["rc_column_outside"]).startswith("-1 ") and "does not lie inside a row" in str(res["rc_column_outside"])
    assert str(res["rc_range"]) == "-1" and str(res["rc_pack_range"]) == "-1" and str(res["rc_pack_k"]) == "-1" and str(res["rc_pack_mode"]) == "-1"
    assert bool(res["dests_poison"]) and bool(res["src_unchanged"])


RUNS = {"raw": run_raw, "unpack": run_unpack, "files": run_files, "fused": run_fused, "errors": run_errors}
