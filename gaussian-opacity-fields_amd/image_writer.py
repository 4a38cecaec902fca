"""PNG files written from the device: torchvision.utils.save_image (render.py:35-36) with the quantisation, the PNG filters, the deflate
stream and its Adler-32 computed by one HIP unit; the host frames the chunks and writes the bytes.

    encode_png(tensor) -> bytes                 # synchronous: the whole file
    save_image(tensor, fp, format=None)         # drop-in for torchvision.utils.save_image; queues the file, returns at once
    flush()                                     # waits for every queued file, re-raises the first error of the writer thread

The kernels are ``gof_png_encode`` of libgof_hip.so (csrc/png_encode.hip, include/gof_png_hip.h); the contract is DESIGN.md §3.16.  The
files are valid 8-bit RGB PNGs with the pixels torchvision's arithmetic gives on the CPU; they are not Pillow's bytes.

save_image takes the device path for a float32 image of 1 or 3 channels that goes to a ``.png`` file name (or ``format="png"``) where a
ROCm device is present; a host tensor is uploaded first.  Everything else -- another format, four channels, a file object, another
dtype, no device -- goes to the function that was bound before (`previous`, set by the launcher; torchvision's own otherwise).

Pipelining: the kernels run on the caller's stream.  A side stream waits for them and copies the size word into a pinned buffer; the
one writer thread waits for that copy, asks for exactly that many bytes on the side stream, frames the file and writes it.  The caller
never synchronises per image; it blocks only while all RING pinned buffers hold files that are not written yet.  flush() runs at exit.
"""
import atexit
import ctypes as C
import os
import queue
import struct
import threading

import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn
from png_chunks import SIGNATURE, chunk as _chunk, walk as _walk

__all__ = ["encode_png", "save_image", "flush", "frame", "stream_of", "GofPngEncode", "BLOCK_BYTES", "RING", "IDAT_BYTES", "stats"]

lib = B.lib
_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32


class GofPngEncode(C.Structure):
    """Mirror of ``GofPngEncode`` in include/gof_png_hip.h."""
    _fields_ = [("width", _i32), ("height", _i32), ("channels", _i32), ("reserved", _i32), ("plane_stride", _i64)]


assert C.sizeof(GofPngEncode) == 24
lib.gof_png_abi_version.restype = C.c_int
lib.gof_png_abi_version.argtypes = []
lib.gof_png_block_bytes.restype = _i32
lib.gof_png_block_bytes.argtypes = []
gn.bind(lib, {"gof_png_ws_bytes": [_i32, _i32], "gof_png_max_bytes": [_i32, _i32]},
        {"gof_png_encode": [C.POINTER(GofPngEncode), _vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, _vp]})
if lib.gof_png_abi_version() != 1:
    raise ImportError("image_writer: libgof_hip.so has PNG ABI %d, this module is written for 1" % lib.gof_png_abi_version())

BLOCK_BYTES = int(lib.gof_png_block_bytes())    # scanline bytes per deflate block
RING = 3                                        # pinned buffers: files in flight between the device and the disk
IDAT_BYTES = 1 << 20                            # bytes of the zlib stream per IDAT chunk

# the function save_image was bound to before the launcher rebound it (None: torchvision's own, looked up when it is needed)
previous = None
stats = {"device": 0, "previous": 0, "waits": 0}

# the device seams, by the names the host tests replace (tests/test_png_encode_host.py); one definition each: gof_native
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr


def _have_device():
    return torch.cuda.is_available()


def _device():
    return gn.current_device("image_writer")


def _to_device(t, dev):
    return t.to(dev)


# ---- shapes: the stand-in's rules and messages (shims/torchvision/utils.py) --------------------------------------------------------------
def _image_of(tensor):
    """-> (C, H, W) view of what save_image is given: (3,H,W), (1,H,W), (H,W) or (1,C,H,W)"""
    t = tensor.detach()
    if t.dim() == 4:
        if t.size(0) != 1:
            raise RuntimeError("torchvision.utils.save_image (stand-in): a batch of %d images would need make_grid, which is not provided" % t.size(0))
        t = t[0]
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.size(0) not in (1, 3, 4):
        raise RuntimeError("torchvision.utils.save_image (stand-in): expected (C,H,W) with C in (1, 3, 4), got %s" % (tuple(tensor.shape),))
    return t


def _planes_of(t):
    """(C, H, W) float32 with C in (1, 3), where the library can read it -> (tensor, C, H, W, plane stride in floats): a copy only where
    the rows are not contiguous (rendering[:3] of a 9-channel image is read in place)"""
    Cn, H, W = int(t.shape[0]), int(t.shape[1]), int(t.shape[2])
    if H < 1 or W < 1:
        raise RuntimeError("image_writer: an image of %d x %d pixels" % (W, H))
    rows = (W == 1 or t.stride(2) == 1) and (H == 1 or t.stride(1) == W)
    if not rows or (Cn == 3 and t.stride(0) < H * W):
        t = t.contiguous()
    return t, Cn, H, W, (int(t.stride(0)) if Cn == 3 else H * W)


def _encode_device(t):
    """t: (C, H, W) float32 on the device, C in (1, 3) -> (out uint8 [capacity], size int64 [1], W, H), queued on the caller's stream"""
    t, Cn, H, W, stride = _planes_of(t)
    with _device_of(t):
        need = int(lib.gof_png_ws_bytes(W, H))
        cap = int(lib.gof_png_max_bytes(W, H))
        if need == 0 or cap == 0:
            raise ValueError("image_writer: %d x %d pixels are outside what the library takes (sizes up to 65535, 2^31 - 1 scanline bytes)" % (W, H))
        ws = torch.empty(need, dtype=torch.uint8, device=t.device)
        out = torch.empty(cap, dtype=torch.uint8, device=t.device)
        size = torch.empty(1, dtype=torch.int64, device=t.device)
        a = GofPngEncode(W, H, Cn, 0, stride)
        B._check(lib.gof_png_encode(C.byref(a), _ptr(t), _ptr(out), cap, _ptr(size), _ptr(ws), need, _stream()))
    return out, size, W, H


def frame(width, height, stream):
    """the file around a zlib stream: signature, IHDR (8-bit RGB, no interlace), IDAT chunks of IDAT_BYTES, IEND; no ancillary chunks"""
    stream = memoryview(stream)
    parts = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))]
    per = max(1, int(IDAT_BYTES))
    for off in range(0, max(1, len(stream)), per):
        parts.append(_chunk(b"IDAT", bytes(stream[off:off + per])))
    parts.append(_chunk(b"IEND", b""))
    return b"".join(parts)


def stream_of(png):
    """the zlib stream of a PNG file's IDAT chunks (what frame() was given); ValueError where a chunk's length or CRC-32 is wrong"""
    return b"".join(bytes(body) for kind, body in _walk(png) if kind == b"IDAT")


def _checked(tensor):
    t = _image_of(tensor)
    if t.size(0) not in (1, 3) or t.dtype != torch.float32:
        raise RuntimeError("image_writer.encode_png: a float32 image of 1 or 3 channels, got %s %s" % (t.dtype, tuple(tensor.shape)))
    if not _on_device(t):
        t = _to_device(t, _device())
    return t


def encode_png(tensor):
    """(3,H,W), (1,H,W), (H,W) or (1,C,H,W) float32 -> the PNG file as bytes.  Synchronous."""
    out, size, W, H = _encode_device(_checked(tensor))
    n = int(size.cpu().item())
    return frame(W, H, out[:n].cpu().numpy().tobytes())


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------
class _Slot:
    def __init__(self):
        self.host = None                        # pinned bytes
        self.word = torch.empty(1, dtype=torch.int64, pin_memory=True)


class _Writer:
    """RING pinned buffers, a side stream and one thread.  A buffer goes back to the ring only after its file is written."""

    def __init__(self, dev):
        self.dev = dev
        self.side = torch.cuda.Stream(device=dev)
        self.free = queue.Queue()
        for _ in range(max(1, int(RING))):
            self.free.put(_Slot())
        self.jobs = queue.Queue()
        self.error = None
        self.lock = threading.Lock()
        self.thread = threading.Thread(target=self._run, name="gof-png-writer", daemon=True)
        self.thread.start()

    def submit(self, out, size, W, H, path):
        try:
            slot = self.free.get_nowait()
        except queue.Empty:
            stats["waits"] += 1
            slot = self.free.get()              # every buffer holds a file that is not written yet
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.side):
            slot.word.copy_(size, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self.side)
        self.jobs.put((slot, out, size, ready, W, H, path))

    def _one(self, slot, out, ready, W, H, path):
        ready.synchronize()
        n = int(slot.word.item())
        if not 6 <= n <= out.numel():
            raise RuntimeError("image_writer: the device reported a stream of %d bytes for %s (capacity %d)" % (n, path, out.numel()))
        if slot.host is None or slot.host.numel() < n:
            slot.host = torch.empty(max(n, out.numel()), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(self.side):
            slot.host[:n].copy_(out[:n], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.side)
        done.synchronize()
        data = frame(W, H, slot.host[:n].numpy())
        with open(path, "wb") as fh:
            fh.write(data)

    def _run(self):
        torch.cuda.set_device(self.dev)
        while True:
            job = self.jobs.get()
            if job is None:
                self.jobs.task_done()
                return
            slot, out, size, ready, W, H, path = job
            try:
                self._one(slot, out, ready, W, H, path)
            except BaseException as e:          # noqa: BLE001  (kept for flush(); the thread goes on with the next file)
                with self.lock:
                    if self.error is None:
                        self.error = e
            finally:
                del out, size, job
                self.free.put(slot)
                self.jobs.task_done()

    def flush(self):
        self.jobs.join()
        with self.lock:
            e, self.error = self.error, None
        if e is not None:
            raise e


_writers = {}
_writers_lock = threading.Lock()


def _writer(dev):
    with _writers_lock:
        w = _writers.get(dev)
        if w is None:
            w = _writers[dev] = _Writer(dev)
        return w


def flush():
    """Wait until every queued file is written; re-raise the first exception of a writer thread."""
    with _writers_lock:
        ws = list(_writers.values())
    first = None
    for w in ws:
        try:
            w.flush()
        except BaseException as e:              # noqa: BLE001
            first = first or e
    if first is not None:
        raise first


atexit.register(flush)


def _is_png_path(fp, format):
    if not isinstance(fp, (str, os.PathLike)):
        return False
    if format is not None:
        return str(format).lower() == "png"
    return os.fspath(fp).lower().endswith(".png")


def _previous():
    if previous is not None:
        return previous
    import torchvision.utils as tvu
    f = tvu.save_image
    if f is save_image:
        raise RuntimeError("image_writer.save_image: this image does not take the device path and no other save_image is bound")
    return f


def save_image(tensor, fp, format=None, **kwargs):
    """torchvision.utils.save_image for one image.  The file exists after flush() (which runs at exit)."""
    t = _image_of(tensor)
    if not (_is_png_path(fp, format) and t.size(0) in (1, 3) and t.dtype == torch.float32 and not kwargs and _have_device()):
        stats["previous"] += 1
        return _previous()(tensor, fp, format=format, **kwargs)
    if not _on_device(t):
        t = _to_device(t, _device())
    out, size, W, H = _encode_device(t)
    _writer(t.device).submit(out, size, W, H, os.fspath(fp))
    stats["device"] += 1
