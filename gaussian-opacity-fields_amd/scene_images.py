"""The scene's training images on the GPU: the reference's loadCam / cameraList_from_camInfos (utils/camera_utils.py:19-62) with Pillow's
bicubic resize, the division by 255 and the permute to planes (utils/general_utils.py:21-27) done by one HIP unit, bit for bit.

    resize_to_planar(u8, (w, h))                                  # (H, W[, C]) uint8 array or tensor -> float32 [C, h, w] on the device
    load_cam(args, id, cam_info, resolution_scale)                # drop-in for loadCam
    camera_list_from_cam_infos(cam_infos, resolution_scale, args) # drop-in for cameraList_from_camInfos: decodes ahead in threads

The kernels are ``gof_image_resize`` of libgof_hip.so (csrc/scene_images.hip, include/gof_image_hip.h); the contract is DESIGN.md §3.15.
Decoding the files stays Pillow's, on the CPU: camera_list_from_cam_infos lets GOF_IMAGE_DECODE_THREADS workers (default 8, 1..16) call
``image.load()`` ahead of the main thread, which copies the decoded bytes through two pinned staging buffers on a side stream (ordered
by events, as model_io orders its buffers) and queues the resampler behind the upload.  An image whose mode is not RGB, RGBA or L goes
to the reference's own loadCam where the launcher kept one (`reference`): LA (which the reference resizes premultiplied), P, 1, 16-bit,
CMYK.  So does every image where there is no ROCm device.
"""
import collections
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from diff_gaussian_rasterization import _backend as B
import gof_native as gn

__all__ = ["resize_to_planar", "load_cam", "camera_list_from_cam_infos", "resolution_of", "decode_threads", "coefficients", "last_stats",
           "GofImageResize", "NATIVE_MODES", "STAGE_BYTES"]

lib = B.lib
_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32


class GofImageResize(C.Structure):
    """Mirror of ``GofImageResize`` in include/gof_image_hip.h."""
    _fields_ = [("in_w", _i32), ("in_h", _i32), ("channels", _i32), ("out_w", _i32), ("out_h", _i32), ("reserved", _i32), ("pitch", _i64)]


assert C.sizeof(GofImageResize) == 32
lib.gof_image_abi_version.restype = C.c_int
lib.gof_image_abi_version.argtypes = []
lib.gof_image_taps.restype = _i64
lib.gof_image_taps.argtypes = [_i32, _i32]
_i32p = C.POINTER(_i32)
gn.bind(lib, {"gof_image_resize_ws_bytes": [C.POINTER(GofImageResize)]},
        {"gof_image_coeffs": [_i32, _i32, _i32p, _i32p], "gof_image_resize": [C.POINTER(GofImageResize), _vp, _vp, _vp, C.c_size_t, _vp]})
if lib.gof_image_abi_version() != 1:
    raise ImportError("scene_images: libgof_hip.so has image ABI %d, this module is written for 1" % lib.gof_image_abi_version())

NATIVE_MODES = {"L": 1, "RGB": 3, "RGBA": 4}
# bytes per pinned staging buffer (two of them): a 16-megapixel RGB image is 50 MB and travels in two chunks
STAGE_BYTES = 32 << 20
DEFAULT_THREADS, MAX_THREADS = 8, 16

# the launcher keeps the reference's own functions here when it rebinds them ({"loadCam": f, "cameraList_from_camInfos": f})
reference = {}
_last = {}
_warned = False

# the device seams, by the names the host tests replace (tests/test_scene_images_host.py); one definition each: gof_native
_stream, _device_of, _on_device, _ptr = gn.stream, gn.device_of, gn.on_device, gn.ptr


def _have_device():
    return torch.cuda.is_available()


def _device():
    return gn.current_device("scene_images")


def _pinned(n):
    """a page-locked host buffer of n bytes: what an asynchronous copy needs on the host side"""
    return torch.empty(n, dtype=torch.uint8, pin_memory=True)


def _to_device(t, dev):
    return t.to(dev)


def _side_stream():
    return torch.cuda.Stream()


def _side_waits_for_caller(side):
    """what the caller's stream has queued so far (the last tenant of a buffer the allocator hands out again) precedes the side stream's copies"""
    side.wait_stream(torch.cuda.current_stream())


def _copy_on(side, dst, src):
    with torch.cuda.stream(side):
        dst.copy_(src, non_blocking=True)


def _record_on(side):
    e = torch.cuda.Event()
    e.record(side)
    return e


def _wait(e):
    e.synchronize()


def _caller_waits_for(e):
    torch.cuda.current_stream().wait_event(e)


def _camera_class():
    """the Camera loadCam constructs: the name in the reference's utils.camera_utils as it is bound when a camera is built"""
    import utils.camera_utils as cu
    return cu.Camera


def last_stats():
    """Statistics of the last camera_list_from_cam_infos: images, native, fallback, threads, chunks, bytes."""
    return dict(_last)


def decode_threads():
    """GOF_IMAGE_DECODE_THREADS, default 8, clamped to 1..16: never derived from the machine's CPU count"""
    try:
        n = int(os.environ.get("GOF_IMAGE_DECODE_THREADS", DEFAULT_THREADS))
    except ValueError:
        n = DEFAULT_THREADS
    return max(1, min(MAX_THREADS, n))


def coefficients(n_in, n_out):
    """the tables of one axis as the library computes them -> (taps, bounds (n_out, 2) int32, coefficients (n_out, taps) int32)"""
    taps = int(lib.gof_image_taps(int(n_in), int(n_out)))
    if taps < 0:
        raise ValueError("coefficients: lengths %r -> %r" % (n_in, n_out))
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, taps), np.int32)
    B._check(lib.gof_image_coeffs(int(n_in), int(n_out), bounds.ctypes.data_as(_i32p), coeffs.ctypes.data_as(_i32p)))
    return taps, bounds, coeffs


# ---- the kernels on plain tensors ----------------------------------------------------------------------------------------------------
def _as_rows(t):
    """a uint8 tensor (H, W) or (H, W, C) whose pixels are contiguous inside a row -> (tensor, H, W, C, pitch in bytes)"""
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise RuntimeError("resize_to_planar: the image must be uint8 with dimensions (H, W) or (H, W, C), got %s %s" % (t.dtype, tuple(t.shape)))
    Cn = 1 if t.dim() == 2 else int(t.shape[2])
    H, W = int(t.shape[0]), int(t.shape[1])
    if Cn not in (1, 3, 4):
        raise RuntimeError("resize_to_planar: %d channels (1, 3 or 4)" % Cn)
    if H < 1 or W < 1:
        raise RuntimeError("resize_to_planar: an image of %d x %d pixels" % (W, H))
    inner = t.stride(1) == Cn and (t.dim() == 2 or t.stride(2) == 1)
    if not inner or (H > 1 and t.stride(0) < W * Cn):
        t = t.contiguous()
    return t, H, W, Cn, (int(t.stride(0)) if H > 1 else W * Cn)


def _resize_device(src, H, W, Cn, pitch, size):
    """src: uint8 tensor on the device (any shape; rows of `pitch` bytes) -> float32 [Cn, h, w] on the caller's stream"""
    w, h = int(size[0]), int(size[1])
    a = GofImageResize(W, H, Cn, w, h, 0, pitch)
    if w < 1 or h < 1:
        raise ValueError("resize_to_planar: an output of %d x %d pixels" % (w, h))
    with _device_of(src):
        need = int(lib.gof_image_resize_ws_bytes(C.byref(a)))
        if need == 0:
            raise ValueError("resize_to_planar: %d x %d x %d -> %d x %d is outside what the library takes (sizes up to 65535)" % (W, H, Cn, w, h))
        ws = torch.empty(need, dtype=torch.uint8, device=src.device)
        out = torch.empty((Cn, h, w), dtype=torch.float32, device=src.device)
        B._check(lib.gof_image_resize(C.byref(a), _ptr(src), _ptr(out), _ptr(ws), need, _stream()))
    return out


def resize_to_planar(image, size):
    """(H, W) or (H, W, C) uint8, C in {1, 3, 4}: a numpy array, a host tensor (uploaded) or a device tensor (rows may have a pitch) ->
    float32 [C, h, w] on the device for size = (w, h): Pillow's bicubic Image.resize per channel, / 255.0, planar."""
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise RuntimeError("resize_to_planar: the image must be uint8, got %s" % image.dtype)
        image = torch.from_numpy(np.ascontiguousarray(image) if image.flags.writeable else np.array(image))
    if not isinstance(image, torch.Tensor):
        raise RuntimeError("resize_to_planar: the image must be a numpy array or a torch tensor")
    if not _on_device(image):
        image = _to_device(image.contiguous(), _device())
    t, H, W, Cn, pitch = _as_rows(image)
    return _resize_device(t, H, W, Cn, pitch, size)


# ---- loadCam -----------------------------------------------------------------------------------------------------------------------------
def resolution_of(args, orig_w, orig_h, resolution_scale):
    """the size loadCam resizes an image of orig_w x orig_h to (utils/camera_utils.py:20-39): -r 1..64 divides and rounds; -1 keeps the
    size up to a width of 1600 and scales larger images to 1600 (with one message per process); any other value is a width"""
    global _warned
    if args.resolution in [1, 2, 4, 8, 16, 32, 64]:
        return round(orig_w / (resolution_scale * args.resolution)), round(orig_h / (resolution_scale * args.resolution))
    if args.resolution == -1:
        if orig_w > 1600:
            cu = sys.modules.get("utils.camera_utils")
            if not _warned and not getattr(cu, "WARNED", False):
                print("[ INFO ] Encountered quite large input images (>1.6K pixels width), rescaling to 1.6K.\n "
                      "If this is not desired, please explicitly specify '--resolution/-r' as 1")
            _warned = True
            if cu is not None:
                cu.WARNED = True               # (the reference's own loadCam, serving another image mode, keeps quiet as well)
            global_down = orig_w / 1600
        else:
            global_down = 1
    else:
        global_down = orig_w / args.resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def _is_native(image):
    return getattr(image, "mode", None) in NATIVE_MODES and _have_device()


def _fall_back(args, id, cam_info, resolution_scale):
    ref = reference.get("loadCam")
    if ref is None:
        raise RuntimeError("load_cam (gfx950 backend) takes RGB, RGBA and L images on a ROCm device (got mode %r); there is no host "
                           "implementation here" % getattr(cam_info.image, "mode", None))
    return ref(args, id, cam_info, resolution_scale)


def _pixels(image):
    """a PIL image of a native mode -> its (H, W[, C]) uint8 pixels (decodes the file if nobody has)"""
    a = np.array(image)                 # (a copy, as in PILtoTorch: Pillow's own buffer is read-only)
    if a.dtype != np.uint8:
        raise RuntimeError("load_cam: a %s image gave %s pixels" % (image.mode, a.dtype))
    return a


def _camera(args, id, cam_info, planes):
    """what loadCam does with the resized tensors (:41-54): channels 0..2 are the image, channel 3 the [1, h, w] mask"""
    image, mask = (planes[:3], planes[3:4]) if planes.shape[0] == 4 else (planes, None)
    return _camera_class()(colmap_id=cam_info.uid, R=cam_info.R, T=cam_info.T, FoVx=cam_info.FovX, FoVy=cam_info.FovY, image=image,
                           gt_alpha_mask=mask, image_name=cam_info.image_name, uid=id, data_device=args.data_device)


def load_cam(args, id, cam_info, resolution_scale):
    """loadCam (utils/camera_utils.py:19-54)"""
    image = cam_info.image
    if not _is_native(image):
        return _fall_back(args, id, cam_info, resolution_scale)
    orig_w, orig_h = image.size
    resolution = resolution_of(args, orig_w, orig_h, resolution_scale)
    return _camera(args, id, cam_info, resize_to_planar(_pixels(image), resolution))


# ---- cameraList_from_camInfos ------------------------------------------------------------------------------------------------------------
def _decode(image, native):
    """runs in a worker: Pillow's decoder releases the GIL.  -> the pixels of a native image, None for one the reference will serve"""
    image.load()
    return _pixels(image) if native else None


class _Uploader:
    """Two pinned staging buffers and a side stream: chunk g of the bytes travels through buffer g & 1, which is written again only after
    the event behind its last copy."""

    def __init__(self, dev):
        self.dev = dev
        self.side = _side_stream()
        self.host = [None, None]
        self.free = [None, None]
        self.g = 0
        self.chunks = 0
        self.bytes = 0

    def upload(self, pixels):
        """(H, W[, C]) uint8 array -> a flat uint8 device tensor holding it; the caller's stream waits for the last copy"""
        flat = torch.from_numpy(np.ascontiguousarray(pixels).reshape(-1))
        n = flat.numel()
        per = max(1, int(STAGE_BYTES))
        dst = torch.empty(n, dtype=torch.uint8, device=self.dev)
        _side_waits_for_caller(self.side)
        for off in range(0, n, per):
            m = min(per, n - off)
            i = self.g & 1
            if self.host[i] is None:
                self.host[i] = _pinned(per)
            if self.free[i] is not None:
                _wait(self.free[i])
            self.host[i][:m].copy_(flat[off:off + m])
            _copy_on(self.side, dst[off:off + m], self.host[i][:m])
            self.free[i] = _record_on(self.side)
            self.g += 1
            self.chunks += 1
        _caller_waits_for(self.free[(self.g - 1) & 1])
        self.bytes += n
        return dst

    def finish(self):
        for e in self.free:
            if e is not None:
                _wait(e)


def camera_list_from_cam_infos(cam_infos, resolution_scale, args):
    """cameraList_from_camInfos (utils/camera_utils.py:56-62): the same cameras in the same order with the same uids"""
    cam_infos = list(cam_infos)
    threads = decode_threads()
    window = threads + 2                                            # decoded images alive at once: the workers' and two waiting
    native = [_is_native(c.image) for c in cam_infos]
    cameras = []
    up = None
    pool = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="gof-image-decode")
    pending = collections.deque()
    nxt = 0
    try:
        for id, c in enumerate(cam_infos):
            while nxt < len(cam_infos) and len(pending) < window:
                pending.append(pool.submit(_decode, cam_infos[nxt].image, native[nxt]))
                nxt += 1
            pixels = pending.popleft().result()                      # (an exception of the decoder leaves here, as itself)
            if not native[id]:
                cameras.append(_fall_back(args, id, c, resolution_scale))
                continue
            orig_w, orig_h = c.image.size
            resolution = resolution_of(args, orig_w, orig_h, resolution_scale)
            if up is None:
                up = _Uploader(_device())
            Cn = 1 if pixels.ndim == 2 else int(pixels.shape[2])
            raw = up.upload(pixels)
            del pixels
            cameras.append(_camera(args, id, c, _resize_device(raw, orig_h, orig_w, Cn, orig_w * Cn, resolution)))
    finally:
        for f in pending:
            f.cancel()
        pool.shutdown(wait=True)                                     # no thread outlives the call
        if up is not None:
            up.finish()
    _last.clear()
    _last.update({"images": len(cam_infos), "native": sum(native), "fallback": len(native) - sum(native), "threads": threads,
                  "chunks": up.chunks if up else 0, "bytes": up.bytes if up else 0})
    return cameras
