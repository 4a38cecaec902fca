"""PNG files read onto the device: what metrics.py:25-36 (readImages) does with Pillow and to_tensor, with the inflate, the PNG filters
and the conversion to float planes computed by one HIP unit for a whole batch of files; the host reads the files and walks the chunks.

    read_images(paths, device=None, planes=True) -> a list: per file a (C,H,W) float32 device tensor, or NOT_TAKEN
    read_image(path)                              # one file; raises for a file that is not taken
    parse(path_or_bytes) -> Png                   # header fields + the zlib stream (the concatenated IDAT payloads)
    read_images_for_metrics(renders_dir, gt_dir)  # drop-in for metrics.py's readImages (the launcher's item 16)

The kernels are ``gof_png_decode_batch`` of libgof_hip.so (csrc/png_decode.hip, include/gof_png_read_hip.h); the contract is DESIGN.md
§3.17.  The tensors are bit-identical to ``to_tensor(Image.open(path))``.

Taken: 8 bits per sample, colour types 0, 2, 4, 6 (1, 3, 2, 4 channels), not interlaced, no tRNS chunk, width and height in 1..65535.
Every other valid file -- interlaced, another bit depth, a palette, tRNS -- is NOT_TAKEN for that file: the caller decides what reads
it (read_images_for_metrics: the function that was bound before, `previous`, set by the launcher).  A corrupt file (signature, chunk
length, CRC, IHDR, a missing IDAT or IEND, and whatever the device reports: zlib header, a bad block, Adler-32, a stream shorter or
longer than H (W C + 1) bytes, a filter byte > 4) raises ValueError naming the file and the reason.

Host side: GOF_PNG_READ_THREADS workers (default 8, 1..16) read and parse the files of a group; the IDAT payloads go straight into one
pinned buffer, one upload and one gof_png_decode_batch per group, the status words are read once per group (the only synchronisation).
A group is bounded by GROUP_BYTES of device memory (streams, workspace and outputs), so a scene of hundreds of views does not need all
its scanline buffers at once.
"""
import collections
import ctypes as C
import os
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn
from png_chunks import SIGNATURE, walk as _walk

__all__ = ["read_images", "read_image", "parse", "read_images_for_metrics", "Png", "GofPngImage", "NOT_TAKEN", "STATUS", "GROUP_BYTES", "stats"]

lib = B.lib
_vp, _i32, _u64, _sz = C.c_void_p, C.c_int32, C.c_uint64, C.c_size_t


class GofPngImage(C.Structure):
    """Mirror of ``GofPngImage`` in include/gof_png_read_hip.h."""
    _fields_ = [("width", _i32), ("height", _i32), ("channels", _i32), ("reserved", _i32), ("stream_offset", _u64), ("stream_bytes", _u64),
                ("bytes_offset", _u64), ("planes_offset", _u64)]


assert C.sizeof(GofPngImage) == 48
lib.gof_png_read_abi_version.restype = C.c_int
lib.gof_png_read_abi_version.argtypes = []
gn.bind(lib, {"gof_png_decode_ws_bytes": [_i32, C.POINTER(GofPngImage), _i32]},
        {"gof_png_decode_batch": [_i32, C.POINTER(GofPngImage), _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp]})
if lib.gof_png_read_abi_version() != 1:
    raise ImportError("png_reader: libgof_hip.so has PNG-read ABI %d, this module is written for 1" % lib.gof_png_read_abi_version())

NOT_TAKEN = None                                # what read_images returns for a file the unit does not take
MAX_DIM = 65535
MAX_IMAGES = 65535                              # GOF_PNG_READ_MAX_IMAGES
GROUP_BYTES = 1 << 30                           # device bytes of one group: streams + workspace + outputs
DEFAULT_THREADS, MAX_THREADS = 8, 16
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}             # colour type -> samples per pixel
# the status words of include/gof_png_read_hip.h
STATUS = {1: "the zlib header is not a deflate stream with a window of at most 32 KiB and no dictionary", 2: "the zlib stream is truncated",
          3: "a deflate block of type 3", 4: "a stored block whose NLEN is not ~LEN", 5: "invalid code lengths in a dynamic block",
          6: "bits that are no code of their block", 7: "a match that starts in front of the output", 8: "the stream is longer than H (W C + 1) bytes",
          9: "the stream is shorter than H (W C + 1) bytes", 10: "the Adler-32 of the scanlines is not the stream's", 11: "a filter byte > 4"}

# the function readImages was bound to before the launcher rebound it (None: Pillow and to_tensor, restated below)
previous = None
stats = {"device": 0, "previous": 0, "groups": 0}

# the device seams, by the names the host tests replace (tests/test_png_decode_host.py); one definition each: gof_native
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr


def _device():
    return gn.current_device("png_reader")


def _pinned(n):
    """a page-locked host buffer of n bytes: what an asynchronous copy needs on the host side"""
    return torch.empty(n, dtype=torch.uint8, pin_memory=True)


def _upload(host, dev):
    return host.to(dev, non_blocking=True)


def _download(t):
    return t.cpu()


def read_threads():
    """GOF_PNG_READ_THREADS, default 8, clamped to 1..16: never derived from the machine's CPU count"""
    try:
        n = int(os.environ.get("GOF_PNG_READ_THREADS", DEFAULT_THREADS))
    except ValueError:
        n = DEFAULT_THREADS
    return max(1, min(MAX_THREADS, n))


# ---- the host side: signature, chunks, CRC-32, IHDR, IDAT ---------------------------------------------------------------------------------
class Png(collections.namedtuple("Png", "width height bit_depth color_type interlace channels payloads not_taken name")):
    """A parsed file.  payloads: the IDAT chunks' data in file order (views of the file's bytes); not_taken: None, or why the unit does
    not take the file; channels: samples per pixel (0 where not taken for its colour type)."""
    __slots__ = ()

    @property
    def stream(self):
        """the zlib stream: the concatenated IDAT payloads"""
        return b"".join(bytes(p) for p in self.payloads)

    @property
    def stream_bytes(self):
        return sum(len(p) for p in self.payloads)


def parse(src):
    """a path or the file's bytes -> Png.  Every chunk's length and CRC-32 are checked; ancillary chunks are skipped.  ValueError for a
    corrupt file."""
    if isinstance(src, (bytes, bytearray, memoryview)):
        data, name = memoryview(src), "<bytes>"
    else:
        name = os.fspath(src)
        with open(name, "rb") as fh:
            data = memoryview(fh.read())

    def bad(why):
        return ValueError("png_reader: %s: %s" % (name, why))
    ihdr, payloads, trns, ended = None, [], False, False
    for kind, body in _walk(data, bad):
        if ihdr is None and kind != b"IHDR":
            raise bad("the first chunk is %r, not IHDR" % kind)
        if kind == b"IHDR":
            if ihdr is not None or len(body) != 13:
                raise bad("a second or malformed IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            payloads.append(body)
        elif kind == b"tRNS":
            trns = True
        elif kind == b"IEND":
            ended = True
            break
    if ihdr is None or not ended:
        raise bad("no IHDR or no IEND chunk")
    if not payloads:
        raise bad("no IDAT chunk")
    w, h, depth, ctype, comp, filt, lace = ihdr
    if comp != 0 or filt != 0 or lace > 1 or ctype not in (0, 2, 3, 4, 6) or depth not in (1, 2, 4, 8, 16):
        raise bad("IHDR: compression %d, filter %d, interlace %d, colour type %d, bit depth %d" % (comp, filt, lace, ctype, depth))
    why = None
    if lace:
        why = "interlaced"
    elif depth != 8:
        why = "bit depth %d" % depth
    elif ctype == 3:
        why = "palette"
    elif trns:
        why = "tRNS"
    elif not (1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM):
        why = "%d x %d pixels" % (w, h)
    return Png(w, h, depth, ctype, lace, CHANNELS.get(ctype, 0) if why is None else 0, tuple(payloads), why, name)


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
def _align(n, a=16):
    return (n + a - 1) // a * a


def _cost(p):
    """device bytes one image adds to its group: stream, scanlines and bytes in the workspace, planes"""
    px = p.width * p.height * p.channels
    return p.stream_bytes + p.height * (p.width * p.channels + 1) + px + 4 * px + 1024


def _decode_group(pngs, dev, planes):
    """pngs: taken files -> (tensors, status words on the host).  One pinned buffer, one upload, one call; no synchronisation but the
    status read."""
    n = len(pngs)
    descs = (GofPngImage * n)()
    s_off = o_off = 0
    for i, p in enumerate(pngs):
        px = p.width * p.height * p.channels
        descs[i] = GofPngImage(p.width, p.height, p.channels, 0, s_off, p.stream_bytes, o_off, o_off)
        s_off += _align(p.stream_bytes)
        o_off += _align(px) if not planes else _align(px, 4)
    host = _pinned(max(s_off, 16))
    view = host.numpy()
    for i, p in enumerate(pngs):
        at = int(descs[i].stream_offset)
        for body in p.payloads:                 # any number of IDAT chunks of any sizes, straight into the pinned buffer
            view[at:at + len(body)] = np.frombuffer(body, np.uint8)
            at += len(body)
    streams = _upload(host, dev)
    with _device_of(streams):
        need = int(lib.gof_png_decode_ws_bytes(n, descs, 1 if planes else 0))
        if need == 0:
            raise ValueError("png_reader: the library refuses a group of %d images" % n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        if planes:
            out = torch.empty(max(o_off, 1), dtype=torch.float32, device=dev)
            B._check(lib.gof_png_decode_batch(n, descs, _ptr(streams), s_off, None, 0, _ptr(out), out.numel(), _ptr(status), _ptr(ws), need, _stream()))
        else:
            out = torch.empty(max(o_off, 1), dtype=torch.uint8, device=dev)
            B._check(lib.gof_png_decode_batch(n, descs, _ptr(streams), s_off, _ptr(out), out.numel(), None, 0, _ptr(status), _ptr(ws), need, _stream()))
    tensors = []
    for i, p in enumerate(pngs):
        at, px = int(descs[i].bytes_offset), p.width * p.height * p.channels
        t = out[at:at + px]
        tensors.append(t.view(p.channels, p.height, p.width) if planes else t.view(p.height, p.width, p.channels))
    words = _download(status)                   # (waits for the group: the pinned buffer, the streams and the workspace may go)
    stats["groups"] += 1
    stats["device"] += n
    return tensors, [int(v) for v in words.tolist()]


def read_images(paths, device=None, planes=True):
    """PNG files -> a list in the order of `paths`: a (C,H,W) float32 tensor on `device` (planes=False: (H,W,C) uint8), or NOT_TAKEN for a
    file the unit does not take.  The tensors of a group are views of one allocation.  ValueError names the first corrupt file."""
    paths = [os.fspath(p) if not isinstance(p, (bytes, bytearray, memoryview)) else p for p in paths]
    dev = torch.device(device) if device is not None else _device()
    out = [NOT_TAKEN] * len(paths)
    with ThreadPoolExecutor(max_workers=read_threads(), thread_name_prefix="gof-png-read") as pool:
        parsed = pool.map(parse, paths)
        group, where, cost = [], [], 0

        def flush():
            nonlocal group, where, cost
            if group:
                tensors, words = _decode_group(group, dev, planes)
                for p, i, t, s in zip(group, where, tensors, words):
                    if s != 0:
                        raise ValueError("png_reader: %s: %s (status %d)" % (p.name, STATUS.get(s, "an unknown status"), s))
                    out[i] = t
            group, where, cost = [], [], 0
        for i, p in enumerate(parsed):
            if p.not_taken is not None:
                continue
            c = _cost(p)
            if group and (cost + c > GROUP_BYTES or len(group) >= MAX_IMAGES):
                flush()
            group.append(p)
            where.append(i)
            cost += c
        flush()
    return out


def read_image(path, device=None, planes=True):
    """one file; ValueError where the unit does not take it"""
    t = read_images([path], device, planes)[0]
    if t is NOT_TAKEN:
        raise ValueError("png_reader: %s is not taken: %s" % (path, parse(path).not_taken))
    return t


# ---- metrics.py ---------------------------------------------------------------------------------------------------------------------------
def _pillow_to_tensor(path):
    """metrics.py:30-34 for one file: Image.open, to_tensor, unsqueeze(0)[:, :3], .cuda()"""
    from PIL import Image
    import torchvision.transforms.functional as tf
    return tf.to_tensor(Image.open(path)).unsqueeze(0)[:, :3, :, :].cuda()


def _through_previous(renders_dir, gt_dir, names):
    """{name: (render, gt)} for these file names through the function bound before.  That function takes the two directories and lists
    the first, so it is given a temporary pair that holds links to these files only."""
    if previous is None:
        return {n: (_pillow_to_tensor(os.path.join(renders_dir, n)), _pillow_to_tensor(os.path.join(gt_dir, n))) for n in names}
    import shutil
    import tempfile
    from pathlib import Path
    with tempfile.TemporaryDirectory(prefix="gof-png-read-") as tmp:
        pair = (Path(tmp) / "renders", Path(tmp) / "gt")
        for d, src in zip(pair, (renders_dir, gt_dir)):
            d.mkdir()
            for n in names:
                s = os.path.abspath(os.path.join(os.fspath(src), n))
                try:
                    os.symlink(s, d / n)
                except OSError:
                    shutil.copyfile(s, d / n)
        renders, gts, listed = previous(*pair)
        return {n: (r, g) for n, r, g in zip(listed, renders, gts)}


def read_images_for_metrics(renders_dir, gt_dir):
    """metrics.py's readImages: the same file order (os.listdir(renders_dir)), the same three lists, each tensor (1, min(C, 3), H, W)
    float32 on the device, bit-identical to the script's own function.  The files that are not taken go through the function that was
    bound before, and only they."""
    names = list(os.listdir(renders_dir))
    paths = [os.path.join(os.fspath(renders_dir), n) for n in names] + [os.path.join(os.fspath(gt_dir), n) for n in names]
    got = read_images(paths)
    elsewhere = [n for k, n in enumerate(names) if got[k] is NOT_TAKEN or got[len(names) + k] is NOT_TAKEN]
    other = _through_previous(renders_dir, gt_dir, elsewhere) if elsewhere else {}
    stats["previous"] += len(elsewhere)
    renders, gts = [], []
    for k, n in enumerate(names):
        if n in other:
            r, g = other[n]
        else:
            r, g = got[k].unsqueeze(0)[:, :3, :, :], got[len(names) + k].unsqueeze(0)[:, :3, :, :]
        renders.append(r)
        gts.append(g)
    return renders, gts, names
