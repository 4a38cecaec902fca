"""The model file on the GPU: the reference's GaussianModel.save_ply / save_fused_ply / load_ply (scene/gaussian_model.py:374-430,
486-530) without plyfile and without a Python tuple per Gaussian.

    save_ply(model, path)            # :390-408  the seven tensors -> point_cloud.ply
    save_fused_ply(model, path)      # :410-430  the same with the 3D filter folded into opacity and scale, no filter_3D column
    load_ply(model, path)            # :486-530  a PLY file -> six nn.Parameters + filter_3D on the device
    pack_rows / unpack_rows          # the two kernels on plain tensors

The kernels are ``gof_model_pack`` / ``gof_model_unpack`` of libgof_hip.so (csrc/model_io.hip, include/gof_model_io_hip.h); the contract is
DESIGN.md §3.14.  A file travels in chunks of CHUNK_ROWS rows through two pinned staging buffers: the device packs chunk i and copies it to
the host on the caller's stream while the host writes chunk i - 1 (loading: the host reads chunk i while the device unpacks chunk i - 1).
The file of a model is the same for every chunk length.  RAW files and loading are pure data movement, bit for bit; the fused file's
opacity and scale columns are computed by the activations' own device functions.

A model whose tensors are not float32 on a ROCm device goes to the reference's own method where the launcher kept one (`reference`), and
is refused otherwise: there is no second implementation here.
"""
import ctypes as C
import os

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["save_ply", "save_fused_ply", "load_ply", "pack_rows", "unpack_rows", "read_header", "attribute_names", "last_stats",
           "GofModelColumn", "RAW", "FUSED", "CHUNK_ROWS"]

lib = B.lib
_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32


class GofModelColumn(C.Structure):
    """Mirror of ``GofModelColumn`` in include/gof_model_io_hip.h."""
    _fields_ = [("offset", C.c_int64), ("type", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(GofModelColumn) == 16
for _name in ("gof_model_row_floats", "gof_model_channels"):
    getattr(lib, _name).restype = _i64
lib.gof_model_row_floats.argtypes = [_i32, _i32]
lib.gof_model_channels.argtypes = [_i32]
gn.bind(lib, {}, {"gof_model_pack": [_i64, _i32, _i64, _i64] + [_vp] * 7 + [_i32, _vp, _vp],
                  "gof_model_unpack": [_i64, _i32, _i64, _i64, _vp, _i64, C.POINTER(GofModelColumn)] + [_vp] * 7 + [_vp]})

RAW, FUSED = 0, 1
MAX_K = 24
# rows per chunk: 2^18 rows of 252 bytes are 63 MiB per staging buffer -- long enough that the per-chunk costs (one launch, one copy, one
# event) vanish, short enough that the second buffer's worth of overlap is most of the file.  GOF_PLY_CHUNK_ROWS overrides it.
CHUNK_ROWS = 1 << 18

# PLY scalar types: name -> (GOF_PLY_* code, bytes, numpy dtype)
PLY_TYPES = {"float": (0, 4, "<f4"), "float32": (0, 4, "<f4"), "double": (1, 8, "<f8"), "float64": (1, 8, "<f8"),
             "char": (2, 1, "i1"), "int8": (2, 1, "i1"), "uchar": (3, 1, "u1"), "uint8": (3, 1, "u1"),
             "short": (4, 2, "<i2"), "int16": (4, 2, "<i2"), "ushort": (5, 2, "<u2"), "uint16": (5, 2, "<u2"),
             "int": (6, 4, "<i4"), "int32": (6, 4, "<i4"), "uint": (7, 4, "<u4"), "uint32": (7, 4, "<u4")}

# the launcher keeps the reference's own methods here when it rebinds them ({"save_ply": f, ...}): where a model is not on the device
reference = {}
_last = {}

# the device seams, by the names the host tests replace (tests/test_model_io_host.py); one definition each: gof_native
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr


def _have_device():
    return torch.cuda.is_available()


def _device():
    return gn.current_device("model_io")


def _pinned(n, dtype):
    """a page-locked host buffer of n elements: what an asynchronous copy needs on the host side"""
    return torch.empty(n, dtype=dtype, pin_memory=True)


def _record():
    """an event behind everything queued on the caller's stream so far"""
    e = torch.cuda.Event()
    e.record(torch.cuda.current_stream())
    return e


def _wait(e):
    e.synchronize()


def last_stats():
    """Statistics of the last save / load: rows, floats per row, chunks, bytes."""
    return {k: dict(v) for k, v in _last.items()}


def chunk_rows():
    n = int(os.environ.get("GOF_PLY_CHUNK_ROWS", CHUNK_ROWS))
    if n < 1:
        raise ValueError("GOF_PLY_CHUNK_ROWS must be at least 1, got %d" % n)
    return n


def attribute_names(K, fused=False):
    """construct_list_of_attributes (:374-388) for K higher-order coefficients per channel"""
    names = ["x", "y", "z", "nx", "ny", "nz"] + ["f_dc_%d" % i for i in range(3)] + ["f_rest_%d" % i for i in range(3 * K)]
    names += ["opacity"] + ["scale_%d" % i for i in range(3)] + ["rot_%d" % i for i in range(4)]
    return names if fused else names + ["filter_3D"]


def channel_names(K):
    """the model's channels in the order of gof_model_unpack's column table"""
    return [n for n in attribute_names(K) if n not in ("nx", "ny", "nz")]


def header_bytes(P, names):
    """what plyfile writes for one element of float32 properties"""
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P + "".join("property float %s\n" % n for n in names)
            + "end_header\n").encode("ascii")


# ---- the tensors of a model ----------------------------------------------------------------------------------------------------------
_FIELDS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "filter_3D")


def _shapes(P, K):
    return [(P, 3), (P, 1, 3), (P, K, 3), (P, 1), (P, 3), (P, 4), (P, 1)]


def _model_tensors(model):
    return [getattr(model, f) for f in _FIELDS]


def _is_native(tensors):
    return all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and _on_device(t) for t in tensors)


def _checked(tensors, who):
    """the seven tensors, detached and contiguous, with (P, K) -- or a complaint that names the tensor"""
    ts = [t.detach().contiguous() for t in tensors]
    P = int(ts[0].shape[0])
    K = int(ts[2].shape[1]) if ts[2].dim() == 3 else -1
    if not 0 <= K <= MAX_K:
        raise RuntimeError("%s: _features_rest must have dimensions (P, K, 3) with K <= %d, got %s" % (who, MAX_K, tuple(ts[2].shape)))
    for f, t, want in zip(_FIELDS, ts, _shapes(P, K)):
        if tuple(t.shape) != want:
            raise RuntimeError("%s: %s must have dimensions %s, got %s" % (who, f, want, tuple(t.shape)))
        if t.dtype != torch.float32 or not _on_device(t):
            raise RuntimeError("%s (gfx950 backend) needs %s as float32 on a ROCm device, got %s on %s" % (who, f, t.dtype, t.device))
        if t.device != ts[0].device:
            raise RuntimeError("%s: the model's tensors are on different devices" % who)
    if P >= 2 ** 31:
        raise RuntimeError("%s: at most 2^31 - 1 Gaussians" % who)
    return ts, P, K


# ---- the kernels on plain tensors ----------------------------------------------------------------------------------------------------
def pack_rows(tensors, first=0, count=None, mode=RAW, out=None):
    """rows [first, first + count) of the seven tensors (xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D) -> (count, C) float32
    file rows on their device (C = 18 + 3K, FUSED: 17 + 3K).  `out`: a contiguous float32 tensor of at least count * C elements."""
    ts, P, K = _checked(tensors, "pack_rows")
    count = P - first if count is None else int(count)
    Cf = int(lib.gof_model_row_floats(K, mode))
    if Cf < 0:
        raise ValueError("pack_rows: bad mode %r" % (mode,))
    with _device_of(ts[0]):
        if out is None:
            out = torch.empty(max(count, 0) * Cf, dtype=torch.float32, device=ts[0].device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < count * Cf or out.device != ts[0].device:
            raise RuntimeError("pack_rows: out must be a contiguous float32 tensor of at least %d elements on the model's device" % (count * Cf))
        B._check(lib.gof_model_pack(P, K, int(first), count, *[_ptr(t) for t in ts], int(mode), _ptr(out), _stream()))
    return out.reshape(-1)[:count * Cf].view(count, Cf)


def column_table(columns):
    """[(byte offset, GOF_PLY_* code)] -> the ctypes table gof_model_unpack takes"""
    tab = (GofModelColumn * max(len(columns), 1))()
    for i, (off, code) in enumerate(columns):
        tab[i].offset, tab[i].type, tab[i].reserved = int(off), int(code), 0
    return tab


def unpack_rows(rows, pitch, columns, dests, first=0, count=None):
    """count rows of `pitch` bytes each (a uint8 tensor on the device, as they lie in a file) -> rows [first, first + count) of the seven
    destination tensors; columns: [(byte offset, GOF_PLY_* code)] per model channel (channel_names(K))."""
    ts, P, K = _checked(dests, "unpack_rows")
    pitch = int(pitch)
    if rows.dtype != torch.uint8 or not _on_device(rows):
        raise RuntimeError("unpack_rows: rows must be a uint8 tensor on a ROCm device")
    rows = rows.contiguous()         # (a view that starts anywhere: the kernel assembles unaligned values from bytes)
    count = (int(rows.numel()) // pitch if pitch > 0 else 0) if count is None else int(count)
    if len(columns) != 15 + 3 * K:
        raise ValueError("unpack_rows: %d columns for a model of %d channels" % (len(columns), 15 + 3 * K))
    if count < 0 or count * pitch > rows.numel():
        raise RuntimeError("unpack_rows: %d rows of %d bytes do not fit in %d bytes" % (count, pitch, rows.numel()))
    with _device_of(ts[0]):
        B._check(lib.gof_model_unpack(P, K, int(first), count, _ptr(rows), pitch, column_table(columns), *[_ptr(t) for t in ts], _stream()))


# ---- saving --------------------------------------------------------------------------------------------------------------------------
def _fall_back(name, model, path, why):
    ref = reference.get(name)
    if ref is None:
        raise RuntimeError("%s (gfx950 backend) needs %s; there is no host implementation here" % (name, why))
    return ref(model, path)


def _save(model, path, mode, name):
    tensors = _model_tensors(model)
    if not _is_native(tensors):
        return _fall_back(name, model, path, "the model's tensors as float32 on a ROCm device")
    ts, P, K = _checked(tensors, name)
    names = attribute_names(K, fused=mode == FUSED)
    Cf = len(names)
    folder = os.path.dirname(path)
    if folder:
        os.makedirs(folder, exist_ok=True)              # mkdir_p (utils/system_utils.py)
    per = chunk_rows()
    chunks = (P + per - 1) // per
    with open(path, "wb") as fh, torch.no_grad():
        fh.write(header_bytes(P, names))
        if P:
            with _device_of(ts[0]):
                n = min(per, P) * Cf
                dev = torch.empty(n, dtype=torch.float32, device=ts[0].device)
                host = [_pinned(n, torch.float32) for _ in range(min(2, chunks))]
                pending = None
                for i in range(chunks):
                    first = i * per
                    cnt = min(per, P - first)
                    h = host[i & 1]         # chunk i - 2 left this buffer for the file in the previous round
                    B._check(lib.gof_model_pack(P, K, first, cnt, *[_ptr(t) for t in ts], mode, _ptr(dev), _stream()))
                    h[:cnt * Cf].copy_(dev[:cnt * Cf], non_blocking=True)
                    ev = _record()
                    if pending is not None:
                        _wait(pending[0])
                        fh.write(pending[1].numpy())
                    pending = (ev, h[:cnt * Cf])
                _wait(pending[0])
                fh.write(pending[1].numpy())
    _last["save"] = {"rows": P, "row_floats": Cf, "chunks": chunks, "chunk_rows": per, "bytes": P * Cf * 4, "fused": mode == FUSED}


def save_ply(model, path):
    """GaussianModel.save_ply (:390-408)"""
    return _save(model, path, RAW, "save_ply")


def save_fused_ply(model, path):
    """GaussianModel.save_fused_ply (:410-430)"""
    return _save(model, path, FUSED, "save_fused_ply")


# ---- loading -------------------------------------------------------------------------------------------------------------------------
def read_header(path):
    """The header of a PLY file -> dict(format, elements: [(name, count, [(property, type)])], data_offset).  A list property is
    recorded with the type "list"."""
    with open(path, "rb") as fh:
        head = b""
        while True:
            line = fh.readline()
            if not line:
                raise ValueError("load_ply: %s: the header has no end_header line" % path)
            head += line
            if line.strip() == b"end_header":
                break
            if len(head) > (1 << 22):
                raise ValueError("load_ply: %s: the header is longer than 4 MiB" % path)
        offset = fh.tell()
    lines = [ln.strip() for ln in head.decode("ascii", errors="replace").split("\n")]
    if not lines or lines[0] != "ply":
        raise ValueError("load_ply: %s is not a PLY file" % path)
    fmt, elements = None, []
    for ln in lines[1:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info", "end_header"):
            continue
        if w[0] == "format":
            fmt = w[1] if len(w) > 1 else None
        elif w[0] == "element" and len(w) == 3:
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements and len(w) >= 3:
            if w[1] == "list":
                elements[-1][2].append((w[-1], "list"))
            elif w[1] in PLY_TYPES:
                elements[-1][2].append((w[2], w[1]))
            else:
                raise ValueError("load_ply: %s: property %s has the unknown type %s" % (path, w[2], w[1]))
        else:
            raise ValueError("load_ply: %s: header line not understood: %r" % (path, ln))
    return {"format": fmt, "elements": elements, "data_offset": offset}


def _suffix(name):
    return int(name.split("_")[-1])


def model_columns(props, max_sh_degree, path="the file"):
    """The first element's properties [(name, type)] -> (K, pitch, [(byte offset, GOF_PLY_* code)] per model channel), by the reference's
    rules (:489-520): f_rest_*, scale_* and rot* are taken in the order of their integer suffixes."""
    where, off = {}, 0
    for name, typ in props:
        if typ == "list":
            raise ValueError("load_ply: %s: list property %r in the first element: a Gaussian model has scalar properties only" % (path, name))
        code, size, _ = PLY_TYPES[typ]
        where.setdefault(name, (off, code, typ))
        off += size
    pitch = off
    names = [n for n, _ in props]
    rest = sorted((n for n in names if n.startswith("f_rest_")), key=_suffix)
    assert len(rest) == 3 * (max_sh_degree + 1) ** 2 - 3                        # (:503)
    scales = sorted((n for n in names if n.startswith("scale_")), key=_suffix)
    rots = sorted((n for n in names if n.startswith("rot")), key=_suffix)
    if len(scales) != 3 or len(rots) != 4:
        raise ValueError("load_ply: %s: %d scale_* and %d rot* properties, a Gaussian model has 3 and 4" % (path, len(scales), len(rots)))
    K = len(rest) // 3
    if K > MAX_K:
        raise ValueError("load_ply: at most %d f_rest properties per channel" % MAX_K)
    order = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2"] + rest + ["opacity"] + scales + rots + ["filter_3D"]
    columns = []
    for n in order:
        if n not in where:
            raise ValueError("load_ply: %s has no property %r" % (path, n))
        o, code, typ = where[n]
        if code > 1:
            raise ValueError("load_ply: %s: property %r has the integer type %s, a model channel must be float or double" % (path, n, typ))
        columns.append((o, code))
    return K, pitch, columns


def _ascii_rows(path, hdr, P, props, columns):
    """the model's channels of an ASCII file as (P, channels) float32 rows, and the table that describes them"""
    with open(path, "rb") as fh:
        fh.seek(hdr["data_offset"])
        words = fh.read().split()
    if len(words) < P * len(props):
        raise ValueError("load_ply: %s: the body ends after %d of %d values" % (path, len(words), P * len(props)))
    offsets, off = [], 0
    for _, typ in props:
        offsets.append(off)
        off += PLY_TYPES[typ][1]
    index = [offsets.index(o) for o, _ in columns]
    table = np.array(words[:P * len(props)], dtype=object).reshape(P, len(props))[:, index] if P else np.zeros((0, len(index)), object)
    rows = table.astype(np.float64).astype(np.float32)
    return np.ascontiguousarray(rows), [(4 * i, 0) for i in range(len(index))]


def load_ply(model, path):
    """GaussianModel.load_ply (:486-530)"""
    if not _have_device():
        return _fall_back("load_ply", model, path, "a ROCm device")
    hdr = read_header(path)
    if not hdr["elements"]:
        raise ValueError("load_ply: %s has no element" % path)
    _, P, props = hdr["elements"][0]
    if hdr["format"] not in ("binary_little_endian", "ascii"):
        raise ValueError("load_ply: %s: format %s is not supported (binary_little_endian and ascii are)" % (path, hdr["format"]))
    K, pitch, columns = model_columns(props, int(model.max_sh_degree), path)
    if not 0 <= P < 2 ** 31:
        raise ValueError("load_ply: %s: %d vertices" % (path, P))
    ascii_rows = None
    if hdr["format"] == "ascii":
        ascii_rows, columns = _ascii_rows(path, hdr, P, props, columns)
        pitch = 4 * len(columns)
    elif os.path.getsize(path) - hdr["data_offset"] < P * pitch:
        raise ValueError("load_ply: %s is truncated: %d vertices of %d bytes need %d bytes behind the header, the file has %d"
                         % (path, P, pitch, P * pitch, os.path.getsize(path) - hdr["data_offset"]))
    dev = _device()
    per = chunk_rows()
    chunks = (P + per - 1) // per
    dests = [torch.empty(s, dtype=torch.float32, device=dev) for s in _shapes(P, K)]
    with _device_of(dests[0]), torch.no_grad():
        if P:
            n = min(per, P) * pitch
            stage = torch.empty(n, dtype=torch.uint8, device=dev)
            host = [_pinned(n, torch.uint8) for _ in range(min(2, chunks))]
            free = [None, None]                 # the event behind the last upload out of each host buffer
            tab = column_table(columns)
            with open(path, "rb") as fh:
                fh.seek(hdr["data_offset"])
                for i in range(chunks):
                    first = i * per
                    cnt = min(per, P - first)
                    h = host[i & 1][:cnt * pitch]
                    if free[i & 1] is not None:
                        _wait(free[i & 1])
                    if ascii_rows is not None:
                        h.copy_(torch.from_numpy(ascii_rows[first:first + cnt].reshape(-1).view(np.uint8)))
                    elif fh.readinto(h.numpy()) != cnt * pitch:
                        raise ValueError("load_ply: %s is truncated" % path)
                    stage[:cnt * pitch].copy_(h, non_blocking=True)
                    free[i & 1] = _record()
                    B._check(lib.gof_model_unpack(P, K, first, cnt, _ptr(stage), pitch, tab, *[_ptr(t) for t in dests], _stream()))
                for e in free:
                    if e is not None:
                        _wait(e)
    nn = torch.nn
    model._xyz = nn.Parameter(dests[0].requires_grad_(True))                      # :522-528
    model._features_dc = nn.Parameter(dests[1].requires_grad_(True))
    model._features_rest = nn.Parameter(dests[2].requires_grad_(True))
    model._opacity = nn.Parameter(dests[3].requires_grad_(True))
    model._scaling = nn.Parameter(dests[4].requires_grad_(True))
    model._rotation = nn.Parameter(dests[5].requires_grad_(True))
    model.filter_3D = dests[6]
    model.active_sh_degree = model.max_sh_degree                                   # :530
    _last["load"] = {"rows": P, "row_bytes": pitch, "chunks": chunks, "chunk_rows": per, "bytes": P * pitch, "ascii": ascii_rows is not None}
