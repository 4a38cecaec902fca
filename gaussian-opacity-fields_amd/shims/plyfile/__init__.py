"""Stand-in for the ``plyfile`` pip package, for what the reference's scripts ask of it: scene/dataset_readers.py:112-135 (fetchPly /
storePly: the scene's point cloud, float positions and normals with uchar colours) and scene/gaussian_model.py:390-430, 486-530 (the
model file, where the launcher has left the reference's own methods in place: GOF_TORCH_PLY=1 or a model on the host).

Written against the PLY format (Turk, "The PLY Polygon File Format"): a header of `element <name> <count>` lines each followed by its
`property <type> <name>` lines, then the elements' records in header order.  What is covered: elements of SCALAR properties of any PLY
scalar type as numpy structured arrays; binary little-endian read and write; ASCII read; ``PlyData.read(path)``, ``plydata['vertex']``,
``.elements[0]``, ``element['x']``, ``element.properties``, ``PlyElement.describe(array, name)``, ``PlyData([...]).write(path)``.  An
element with a list property (faces) keeps its header entry; asking for its data is an error, and so is any other format.

launch/run_reference_script.py puts this directory LAST on sys.path and only when no real plyfile is importable, so an installed package
wins."""
import numpy as np

__all__ = ["PlyData", "PlyElement", "PlyProperty", "PlyParseError"]

# PLY scalar type names (both spellings) -> numpy kind + size; numpy -> the short PLY name plyfile writes
_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
          "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float", "f8": "double"}


class PlyParseError(Exception):
    pass


class PlyProperty:
    """a scalar property: its name and its numpy type string without byte order ('f4', 'u1', ...)"""

    def __init__(self, name, val_dtype):
        self.name = str(name)
        self.val_dtype = _TYPES.get(val_dtype, val_dtype)
        if self.val_dtype not in _NAMES:
            raise ValueError("plyfile stand-in: %r is not a PLY scalar type" % (val_dtype,))

    @property
    def dtype(self):
        return self.val_dtype

    def __str__(self):
        return "property %s %s" % (_NAMES[self.val_dtype], self.name)

    __repr__ = __str__


class _ListProperty:
    def __init__(self, name, line):
        self.name, self._line = str(name), line

    def __str__(self):
        return self._line


class PlyElement:
    def __init__(self, name, properties, count, data=None):
        self.name = str(name)
        self.properties = tuple(properties)
        self.count = int(count)
        self._data = data

    @staticmethod
    def describe(data, name, len_types=None, val_types=None, comments=None):
        data = np.asarray(data)
        if data.dtype.names is None or data.ndim != 1:
            raise ValueError("plyfile stand-in: describe() takes a one-dimensional structured array")
        props = []
        for n in data.dtype.names:
            t = data.dtype[n]
            if t.shape or t.kind not in "iuf" or t.str[1:] not in _NAMES:
                raise ValueError("plyfile stand-in: field %r of type %s is not a PLY scalar" % (n, t))
            props.append(PlyProperty(n, t.str[1:]))
        return PlyElement(name, props, len(data), data)

    @property
    def data(self):
        if self._data is None:
            raise PlyParseError("plyfile stand-in: element %r has a list property (or lies behind one): its data is not read" % self.name)
        return self._data

    def dtype(self, byte_order="<"):
        return np.dtype([(p.name, byte_order + p.val_dtype) for p in self.properties])

    def ply_property(self, name):
        for p in self.properties:
            if p.name == name:
                return p
        raise KeyError(name)

    def __getitem__(self, key):
        return self.data[key]

    def __setitem__(self, key, value):
        self.data[key] = value

    def __len__(self):
        return self.count

    @property
    def header(self):
        return "\n".join(["element %s %d" % (self.name, self.count)] + [str(p) for p in self.properties])


class PlyData:
    def __init__(self, elements=(), text=False, byte_order="=", comments=(), obj_info=()):
        self.elements = list(elements)
        self.text = bool(text)
        self.byte_order = byte_order
        self.comments = list(comments)
        self.obj_info = list(obj_info)

    def __getitem__(self, name):
        for e in self.elements:
            if e.name == name:
                return e
        raise KeyError(name)

    def __contains__(self, name):
        return any(e.name == name for e in self.elements)

    def __iter__(self):
        return iter(self.elements)

    def __len__(self):
        return len(self.elements)

    @property
    def header(self):
        lines = ["ply", "format binary_little_endian 1.0"] + ["comment " + c for c in self.comments] + ["obj_info " + c for c in self.obj_info]
        return "\n".join(lines + [e.header for e in self.elements] + ["end_header"])

    def write(self, stream):
        """binary little-endian, whatever `text` / `byte_order` say: the one format every reader of this pipeline takes"""
        if self.text:
            raise NotImplementedError("plyfile stand-in: ASCII files are read, not written")
        own = isinstance(stream, (str, bytes)) or hasattr(stream, "__fspath__")
        fh = open(stream, "wb") if own else stream
        try:
            fh.write((self.header + "\n").encode("ascii"))
            for e in self.elements:
                fh.write(np.ascontiguousarray(e.data.astype(e.dtype("<"), copy=False)).tobytes())
        finally:
            if own:
                fh.close()

    @staticmethod
    def read(stream):
        own = isinstance(stream, (str, bytes)) or hasattr(stream, "__fspath__")
        fh = open(stream, "rb") if own else stream
        try:
            return PlyData._read(fh)
        finally:
            if own:
                fh.close()

    @staticmethod
    def _read(fh):
        if fh.readline().strip() != b"ply":
            raise PlyParseError("plyfile stand-in: not a PLY file (the first line is not 'ply')")
        fmt, comments, obj_info, elements = None, [], [], []
        while True:
            raw = fh.readline()
            if not raw:
                raise PlyParseError("plyfile stand-in: the header has no end_header line")
            line = raw.decode("ascii", errors="replace").strip()
            w = line.split()
            if not w:
                continue
            if w[0] == "end_header":
                break
            if w[0] == "format" and len(w) >= 2:
                fmt = w[1]
            elif w[0] == "comment":
                comments.append(line[len("comment"):].strip())
            elif w[0] == "obj_info":
                obj_info.append(line[len("obj_info"):].strip())
            elif w[0] == "element" and len(w) == 3:
                elements.append([w[1], int(w[2]), []])
            elif w[0] == "property" and elements and len(w) >= 3:
                if w[1] == "list":
                    elements[-1][2].append(_ListProperty(w[-1], line))
                elif w[1] in _TYPES and len(w) == 3:
                    elements[-1][2].append(PlyProperty(w[2], w[1]))
                else:
                    raise PlyParseError("plyfile stand-in: property line not understood: %r" % line)
            else:
                raise PlyParseError("plyfile stand-in: header line not understood: %r" % line)
        if fmt not in ("binary_little_endian", "ascii"):
            raise PlyParseError("plyfile stand-in: format %s is not supported (binary_little_endian and ascii are)" % fmt)
        out, readable = [], True
        words = None
        for name, count, props in elements:
            readable = readable and not any(isinstance(p, _ListProperty) for p in props)
            el = PlyElement(name, props, count)
            if readable:
                dt = el.dtype("<")
                if fmt == "binary_little_endian":
                    buf = fh.read(dt.itemsize * count)
                    if len(buf) != dt.itemsize * count:
                        raise PlyParseError("plyfile stand-in: element %s ends after %d of %d bytes" % (name, len(buf), dt.itemsize * count))
                    el._data = np.frombuffer(buf, dtype=dt, count=count).copy()
                else:
                    if words is None:
                        words = fh.read().split()
                    n = count * len(props)
                    if len(words) < n:
                        raise PlyParseError("plyfile stand-in: element %s ends after %d of %d values" % (name, len(words), n))
                    table = np.array(words[:n], dtype=object).reshape(count, len(props))
                    words = words[n:]
                    data = np.zeros(count, dt)
                    for j, p in enumerate(props):
                        col = table[:, j]
                        data[p.name] = col.astype(np.float64) if p.val_dtype[0] == "f" else np.array([int(v) for v in col], dtype=np.int64)
                    el._data = data
            out.append(el)
        return PlyData(out, text=fmt == "ascii", byte_order="<", comments=comments, obj_info=obj_info)
