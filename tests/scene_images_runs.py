"""The runs and the checks the scene-image test files share: tests/test_scene_images_host.py performs the runs in a child process over the
emulated library (every buffer the product allocates poisoned with 0xA5 and guarded), tests/test_scene_images_gpu.py on the device.  A run
takes the product module and three helpers and returns arrays; a check takes what a run returned and asserts against the committed
golden (Pillow's bytes, the reference's PILtoTorch tensors) and the resampler restated in scene_images_cases.

    up(array) -> a uint8 tensor holding it, where the library can read it     alloc(nbytes) -> a uint8 buffer filled with 0xA5
    down(tensor) -> numpy array
"""
import collections
import ctypes as C
import os
import threading

import numpy as np

import scene_images_cases as K

# shapes that also run with a row pitch that is no multiple of 4 (every row misaligned: the byte-assembling loads, the vertical pass's byte path)
PITCHED = ("odd", "noh", "same", "rgba", "nov")


def u8(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


def _pitched(up, a, extra=5):
    """the image inside rows of W * C + extra bytes (the padding filled with 0xEE) as a strided (H, W, C) view"""
    H, W, Cn = a.shape
    rows = np.full((H, W * Cn + extra), 0xEE, np.uint8)
    rows[:, :W * Cn] = a.reshape(H, W * Cn)
    t = up(rows)[:, :W * Cn]
    return t.unflatten(1, (W, Cn)) if Cn > 1 else t


# ---- the shapes ------------------------------------------------------------------------------------------------------------------------
def run_shapes(SI, up, alloc, down, tmp, tags=None):
    res = {}
    for (tag, W, H, w, h, Cn), kind, a in K.inputs():
        if tags is not None and tag not in tags:
            continue
        src = up(a if Cn > 1 else a[..., 0])
        res["out_%s_%s" % (tag, kind)] = down(SI.resize_to_planar(src, (w, h)))
        if tag in PITCHED and kind == "random":
            res["pitched_%s" % tag] = down(SI.resize_to_planar(_pitched(up, a), (w, h)))
    return res


def check_shapes(res, g, tags=None):
    n = 0
    for (tag, W, H, w, h, Cn), kind, a in K.inputs():
        if tags is not None and tag not in tags:
            continue
        got = res["out_%s_%s" % (tag, kind)]
        want = g["planar_%s_%s" % (tag, kind)]
        assert got.shape == (Cn, h, w) and got.dtype == np.float32, (tag, kind, got.shape)
        assert K.same_bits(got, want), "%s %s: %d of %d values differ from the reference's PILtoTorch" % (tag, kind, (got != want).sum(), got.size)
        # the golden's two halves agree with each other and with the restatement (the restatement serves the loader tests)
        assert K.same_bits(K.planar(g["bytes_%s_%s" % (tag, kind)].reshape(h, w, Cn)), want), (tag, kind)
        assert K.same_bits(K.resize_bytes(a, w, h), g["bytes_%s_%s" % (tag, kind)].reshape(h, w, Cn)), (tag, kind)
        if kind == "white":
            assert (got == np.float32(1.0)).all(), tag
        if kind == "steps" and tag in ("half", "odd", "frac", "noh", "tall", "rgba", "up"):
            assert got.min() == 0.0 and got.max() == 1.0, "%s: the steps image does not reach both ends of the clamp" % tag
        if tag in PITCHED and kind == "random":
            assert K.same_bits(res["pitched_%s" % tag], want), "%s with a row pitch" % tag
        n += 1
    return n


# ---- all 256 byte values ----------------------------------------------------------------------------------------------------------------
def run_bytes(SI, up, alloc, down, tmp):
    ramp = np.arange(256, dtype=np.uint8)
    res = {"lut_L": down(SI.resize_to_planar(up(ramp.reshape(1, 256)), (256, 1)))}
    rgb = np.stack([ramp, ramp[::-1], np.roll(ramp, 77)], axis=-1).reshape(16, 16, 3)
    res["lut_RGB"] = down(SI.resize_to_planar(up(rgb), (16, 16)))
    return res


def check_bytes(res):
    import torch
    want = (torch.arange(256, dtype=torch.uint8) / 255.0).numpy()
    assert want.dtype == np.float32
    assert K.same_bits(res["lut_L"].reshape(256), want)
    ramp = np.arange(256)
    for c, idx in enumerate((ramp, ramp[::-1], np.roll(ramp, 77))):
        assert K.same_bits(res["lut_RGB"][c].reshape(256), want[idx]), c


# ---- the C entry: workspace contents, argument errors -------------------------------------------------------------------------------------
def _call(SI, src, out, ws, ws_bytes, W, H, Cn, w, h, pitch=None):
    a = SI.GofImageResize(W, H, Cn, w, h, 0, W * Cn if pitch is None else pitch)
    rc = SI.lib.gof_image_resize(C.byref(a), src.data_ptr() if src is not None else None, out.data_ptr() if out is not None else None,
                                 ws.data_ptr() if ws is not None else None, ws_bytes, SI._stream())
    return rc, SI.lib.gof_last_error().decode()


def run_entry(SI, up, alloc, down, tmp):
    res = {}
    tag, W, H, w, h, Cn = K.shape("odd")
    a = K.make_input(tag, "random")
    src = up(a)
    q = SI.GofImageResize(W, H, Cn, w, h, 0, W * Cn)
    need = int(SI.lib.gof_image_resize_ws_bytes(C.byref(q)))
    res["need"] = np.array(need)
    for fill in (0xA5, 0x00, 0xFF):
        ws = alloc(need + 64)
        ws[:need].fill_(fill)
        out = alloc(Cn * h * w * 4 + 64)
        rc, _ = _call(SI, src, out, ws, need, W, H, Cn, w, h)
        o = down(out)
        res["ws%02x" % fill] = o[:Cn * h * w * 4].copy()
        res["ws%02x_rc" % fill] = np.array(rc)
        res["ws%02x_tails" % fill] = np.array(bool((o[Cn * h * w * 4:] == 0xA5).all() and (down(ws)[need:] == 0xA5).all()))
    # argument errors: a code, a message, and an output that keeps its poison
    ws = alloc(need)
    out = alloc(Cn * h * w * 4)
    bad = {"zero_w": dict(W=0), "zero_out": dict(h=0), "two_channels": dict(Cn=2), "five_channels": dict(Cn=5), "pitch": dict(pitch=W * Cn - 1),
           "huge": dict(w=65536), "small_ws": dict(ws_bytes=need - 1), "null_src": dict(src=None), "null_ws": dict(ws=None)}
    for name, over in bad.items():
        kw = dict(src=src, out=out, ws=ws, ws_bytes=need, W=W, H=H, Cn=Cn, w=w, h=h, pitch=None)
        kw.update(over)
        rc, msg = _call(SI, **kw)
        res["err_" + name] = np.array("%d %s" % (rc, msg))
    res["err_out_poison"] = np.array(bool((down(out) == 0xA5).all() and (down(ws) == 0xA5).all()))
    res["err_query_zero"] = np.array([int(SI.lib.gof_image_resize_ws_bytes(C.byref(SI.GofImageResize(W, H, 2, w, h, 0, W * 2)))),
                                      int(SI.lib.gof_image_resize_ws_bytes(C.byref(SI.GofImageResize(W, H, 3, w, 0, 0, W * 3)))),
                                      int(SI.lib.gof_image_resize_ws_bytes(C.byref(SI.GofImageResize(W, H, 3, w, h, 0, W * 3 - 1))))])
    return res


def check_entry(res, g):
    tag, W, H, w, h, Cn = K.shape("odd")
    want = g["planar_odd_random"].tobytes()
    assert int(res["need"]) > 0
    for fill in (0xA5, 0x00, 0xFF):
        assert int(res["ws%02x_rc" % fill]) == 0
        assert res["ws%02x" % fill].tobytes() == want, "a workspace filled with 0x%02X changes the output" % fill
        assert bool(res["ws%02x_tails" % fill]), "bytes behind the output or the workspace were written (fill 0x%02X)" % fill
    for name, code, text in (("zero_w", -1, "1..65535"), ("zero_out", -1, "1..65535"), ("two_channels", -1, "channels"), ("five_channels", -1, "channels"),
                             ("pitch", -1, "pitch"), ("huge", -1, "1..65535"), ("small_ws", -2, "workspace"), ("null_src", -1, "NULL"), ("null_ws", -1, "NULL")):
        got = str(res["err_" + name])
        assert got.startswith("%d " % code) and text in got, (name, got)
    assert bool(res["err_out_poison"]), "a refused call wrote to its output or its workspace"
    assert list(res["err_query_zero"]) == [0, 0, 0]


# ---- the loader --------------------------------------------------------------------------------------------------------------------------
CamInfo = collections.namedtuple("CamInfo", "uid R T FovY FovX image image_path image_name width height")


class Args:
    def __init__(self, resolution, data_device="cuda"):
        self.resolution, self.data_device = resolution, data_device


class RecordingCamera:
    """what loadCam hands to Camera, kept"""
    built = 0

    def __init__(self, colmap_id, R, T, FoVx, FoVy, image, gt_alpha_mask, image_name, uid, data_device="cuda"):
        type(self).built += 1
        self.fields = dict(colmap_id=colmap_id, R=R, T=T, FoVx=FoVx, FoVy=FoVy, image_name=image_name, uid=uid, data_device=data_device)
        self.image, self.gt_alpha_mask = image, gt_alpha_mask


def write_scene(folder, files=None, truncate=None):
    """the PNG files of K.LOADER_FILES (or `files`: [(name, mode, pixels)]) -> cam_infos with lazily opened images"""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    infos = []
    if files is None:
        files = [(name, mode, K.loader_pixels(i)) for i, (name, mode, _, _) in enumerate(K.LOADER_FILES)]
    for i, (name, mode, px) in enumerate(files):
        path = os.path.join(folder, name + ".png")
        im = Image.fromarray(px, "L" if mode == "P" else mode)
        if mode == "P":
            im = im.convert("P")
        im.save(path)
        if truncate == i:
            data = open(path, "rb").read()
            with open(path, "wb") as fh:
                fh.write(data[:len(data) * 2 // 3])
        R = np.eye(3) * (i + 1)
        T = np.array([0.1 * i, 0.2, 0.3])
        infos.append(CamInfo(uid=100 + i, R=R, T=T, FovY=0.5 + 0.01 * i, FovX=0.7, image=Image.open(path), image_path=path, image_name=name,
                             width=px.shape[1], height=px.shape[0]))
    return infos


def _record(cams, down, prefix, res):
    res[prefix + "_n"] = np.array(len(cams))
    for i, c in enumerate(cams):
        if isinstance(c, tuple):                                       # the stand-in for the reference's loadCam: ("fallback", id, uid)
            res["%s_%d_fallback" % (prefix, i)] = np.array([c[1], c[2]])
            continue
        res["%s_%d_image" % (prefix, i)] = down(c.image)
        res["%s_%d_mask" % (prefix, i)] = down(c.gt_alpha_mask) if c.gt_alpha_mask is not None else np.zeros(0, np.float32)
        f = c.fields
        res["%s_%d_meta" % (prefix, i)] = np.array("%s|%s|%s|%r|%r|%s|%s" % (f["colmap_id"], f["uid"], f["image_name"], f["FoVx"], f["FoVy"],
                                                                             f["data_device"], np.asarray(f["R"]).tobytes().hex()[:32] + np.asarray(f["T"]).tobytes().hex()))


def run_loader(SI, up, alloc, down, tmp):
    res = {}
    SI._camera_class = lambda: RecordingCamera
    SI.reference = {"loadCam": lambda args, id, cam_info, scale: ("fallback", id, cam_info.uid)}
    args = Args(2)
    before = threading.active_count()
    serial = [SI.load_cam(args, i, c, 1.0) for i, c in enumerate(write_scene(os.path.join(tmp, "serial")))]
    _record(serial, down, "serial", res)
    for n in (1, 3):
        os.environ["GOF_IMAGE_DECODE_THREADS"] = str(n)
        try:
            cams = SI.camera_list_from_cam_infos(write_scene(os.path.join(tmp, "pool%d" % n)), 1.0, args)
        finally:
            del os.environ["GOF_IMAGE_DECODE_THREADS"]
        _record(cams, down, "pool%d" % n, res)
        res["pool%d_stats" % n] = np.array([SI.last_stats()[k] for k in ("images", "native", "fallback", "threads")])
    res["threads_after"] = np.array(threading.active_count() - before)
    # a truncated file in fifth place
    infos = write_scene(os.path.join(tmp, "broken"), truncate=4)
    RecordingCamera.built = 0
    os.environ["GOF_IMAGE_DECODE_THREADS"] = "3"
    try:
        SI.camera_list_from_cam_infos(infos, 1.0, args)
        res["broken"] = np.array("no error")
    except Exception as e:      # noqa: BLE001  (the test looks at the kind and the text)
        res["broken"] = np.array("%s: %s" % (type(e).__name__, e))
    finally:
        del os.environ["GOF_IMAGE_DECODE_THREADS"]
    try:
        from PIL import Image
        Image.open(infos[4].image_path).load()
        res["broken_pillow"] = np.array("no error")
    except Exception as e:      # noqa: BLE001
        res["broken_pillow"] = np.array("%s: %s" % (type(e).__name__, e))
    res["broken_built"] = np.array(RecordingCamera.built)
    res["broken_threads_after"] = np.array(threading.active_count() - before)
    # the clamp of the pool size
    sizes = []
    for v in ("0", "-3", "1", "8", "16", "17", "1000", "x"):
        os.environ["GOF_IMAGE_DECODE_THREADS"] = v
        sizes.append(SI.decode_threads())
    del os.environ["GOF_IMAGE_DECODE_THREADS"]
    sizes.append(SI.decode_threads())
    res["pool_sizes"] = np.array(sizes)
    return res


def check_loader(res):
    files = K.LOADER_FILES
    assert int(res["serial_n"]) == len(files) == 7
    for i, (name, mode, W, H) in enumerate(files):
        if mode == "P":
            for p in ("serial", "pool1", "pool3"):
                assert list(res["%s_%d_fallback" % (p, i)]) == [i, 100 + i], "the P image did not go to the reference's loadCam"
            continue
        px = K.loader_pixels(i)
        px = px[..., None] if px.ndim == 2 else px
        w, h = K.resolution_of(W, H, 2, 1.0)
        want = K.planar(K.resize_bytes(px, w, h))
        img, mask = (want[:3], want[3:4]) if mode == "RGBA" else (want, np.zeros(0, np.float32))
        assert K.same_bits(res["serial_%d_image" % i], img), name
        assert K.same_bits(res["serial_%d_mask" % i], mask), name
        assert str(res["serial_%d_meta" % i]).startswith("%d|%d|%s|0.7|%r|cuda|" % (100 + i, i, name, 0.5 + 0.01 * i))
        for p in ("pool1", "pool3"):
            assert int(res[p + "_n"]) == 7
            for field in ("image", "mask", "meta"):
                a, b = res["%s_%d_%s" % (p, i, field)], res["serial_%d_%s" % (i, field)]
                assert (str(a) == str(b)) if field == "meta" else K.same_bits(a, b), (p, name, field)
    assert list(res["pool1_stats"]) == [7, 6, 1, 1] and list(res["pool3_stats"]) == [7, 6, 1, 3]
    assert int(res["threads_after"]) == 0, "a decoding thread outlived the call"
    assert str(res["broken"]) != "no error" and str(res["broken"]) == str(res["broken_pillow"]), (res["broken"], res["broken_pillow"])
    assert str(res["broken"]).startswith("OSError")
    assert int(res["broken_built"]) == 4, "cameras built before the broken file: %d" % int(res["broken_built"])
    assert int(res["broken_threads_after"]) == 0
    assert list(res["pool_sizes"]) == [1, 1, 1, 8, 16, 16, 16, 8, 8]


RUNS = {"shapes": run_shapes, "bytes": run_bytes, "entry": run_entry, "loader": run_loader}
