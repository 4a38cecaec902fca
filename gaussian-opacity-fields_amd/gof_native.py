"""What the ctypes front ends of libgof_hip.so share (mesh_eval, tnt_eval, mesh_cull, tsdf_fusion, delaunay, simple_knn,
train_epilogue): the signature declarations, the device seams (stream, device context, device check, current device, pointer) and the row
validator.  The evaluation modules, tsdf_fusion and delaunay bind the seams to private names of their own (``_stream = gn.stream``):
those names are what the host tests replace with stand-ins for the emulated library, and a module's workspaces are allocated
through its own ``torch`` for the same reason (the tests put guard bytes behind them); tsdf_fusion allocates through its
``_buffer``, by role."""
import ctypes as C

import torch

from diff_gaussian_rasterization import _backend as B


def bind(lib, sizes, calls):
    """Declare entry points of `lib`: sizes {name: argtypes} return size_t (the *_bytes queries), calls {name: argtypes} an int status."""
    for restype, table in ((C.c_size_t, sizes), (C.c_int, calls)):
        for name, args in table.items():
            f = getattr(lib, name)
            f.restype = restype
            f.argtypes = args
    return lib


def stream():
    return B._stream()


def device_of(t):
    return torch.cuda.device(t.device)


def on_device(t):
    return t.device.type == "cuda"


def current_device(who):
    if not torch.cuda.is_available():
        raise RuntimeError("%s (gfx950 backend) needs a ROCm device" % who)
    return torch.device("cuda", torch.cuda.current_device())


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def rows(t, who, what="points", dtype=torch.float64, cols=3, limit=2 ** 31, shape_first=True, on_device=on_device):
    """A tensor of rows the library can take -> t.contiguous().  dtype: one dtype or a tuple of accepted ones; cols: None = any shape;
    limit: the first row count that is refused.  shape_first: which of two faults is reported, the shape (the cloud modules) or the
    device and dtype (mesh_cull) -- each module keeps the order it has always had.  on_device: the caller's device check (a module's
    own name for it, which the host tests replace)."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("%s: %s must be a torch tensor" % (who, what))

    def shape():
        if cols is not None and (t.dim() != 2 or t.size(1) != cols):
            raise RuntimeError("%s: %s must have dimensions (N, %d)" % (who, what, cols))
    if shape_first:
        shape()
    if not on_device(t):
        raise RuntimeError("%s (gfx950 backend) needs %s on a ROCm device, got %s" % (who, what, t.device))
    if t.dtype not in dtypes:
        raise RuntimeError("%s: %s must be %s, got %s" % (who, what, " or ".join(str(d) for d in dtypes), t.dtype))
    if not shape_first:
        shape()
    if t.size(0) >= limit:
        raise RuntimeError("%s: at most 2^31 - %d rows" % (who, 2 ** 31 - limit + 1))
    return t.contiguous()
