#!/usr/bin/env python3
"""Developer tool, not a test: times the scene's image loading through the reference's cameraList_from_camInfos (GOF_PIL_IMAGES=1: the
parent path) and through scene_images' (DESIGN.md §3.15), and the decode-only floors, and writes profiles/scene_images_timing.md.

    python tests/devtools/dev_scene_images.py [--images 32] [--repeats 5] [--out profiles/scene_images_timing.md]

Needs a ROCm device, Pillow and the reference's scripts as build() stages them (oracle/_ref/refpy).  It writes `--images` synthetic JPEGs of
4946x3286 and of 1920x1080 to a temporary folder, then, per size and path, runs `--repeats` child processes (a fresh process per repeat:
no decoded image, table or pinned buffer survives) that time cameraList_from_camInfos at -r 4 and -r 2 respectively between device
synchronisations; next to them image.load() over the files serially and with the decoding pool.  Medians and spread (min .. max) go to the
record.  The bar for making the launcher's binding the default: faster than the parent path at both sizes by more than the spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "gaussian-opacity-fields_amd")
REF = os.path.join(ROOT, "oracle", "_ref", "refpy")
SIZES = (("4946x3286", 4946, 3286, 4), ("1920x1080", 1920, 1080, 2))


def write_images(folder, W, H, n):
    import numpy as np
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(W)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 255 // W), (yy * 255 // H), ((xx + yy) * 255 // (W + H))], axis=-1).astype(np.int16)
    for i in range(n):
        noise = rng.integers(-20, 21, (H // 8 + 1, W // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:H, :W]
        Image.fromarray(np.clip(base + noise + 3 * i, 0, 255).astype(np.uint8), "RGB").save(os.path.join(folder, "im%03d.jpg" % i), quality=92)


def child(path, folder, resolution):
    """one timed run in this process -> a JSON line"""
    import collections
    sys.path.insert(0, REF)
    sys.path.insert(0, PKG)
    import importlib.util
    spec = importlib.util.spec_from_file_location("gof_launcher", os.path.join(PKG, "launch", "run_reference_script.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    L.add_import_stand_ins()
    L.add_trimesh_stand_in()
    L.add_cv2_stand_in()
    import numpy as np
    import torch
    from PIL import Image
    names = sorted(os.listdir(folder))
    if path in ("decode_serial", "decode_pool"):
        images = [Image.open(os.path.join(folder, n)) for n in names]
        t0 = time.perf_counter()
        if path == "decode_serial":
            for im in images:
                im.load()
        else:
            from concurrent.futures import ThreadPoolExecutor
            import scene_images
            with ThreadPoolExecutor(scene_images.decode_threads()) as ex:
                list(ex.map(lambda im: im.load(), images))
        print("RESULT " + json.dumps({"seconds": time.perf_counter() - t0}))
        return
    import scene as ref_scene  # noqa: F401
    import utils.camera_utils as cu
    if path == "hip":
        os.environ["GOF_HIP_IMAGES"] = "1"
        L.rebind_scene_images()
        assert cu.cameraList_from_camInfos is L._camera_list_from_cam_infos
    CamInfo = collections.namedtuple("CamInfo", "uid R T FovY FovX image image_path image_name width height")
    infos = [CamInfo(i, np.eye(3), np.zeros(3), 0.6, 0.8, Image.open(os.path.join(folder, n)), os.path.join(folder, n), n, 0, 0) for i, n in enumerate(names)]
    args = type("Args", (), {"resolution": resolution, "data_device": "cuda"})()
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cams = cu.cameraList_from_camInfos(infos, 1.0, args)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("RESULT " + json.dumps({"seconds": dt, "cameras": len(cams), "size": [cams[0].image_width, cams[0].image_height]}))


def timed(path, folder, resolution, repeats):
    out = []
    for _ in range(repeats):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, folder, str(resolution)], capture_output=True, text=True, timeout=3000)
        if r.returncode != 0:
            raise RuntimeError("%s failed:\n%s\n%s" % (path, r.stdout[-2000:], r.stderr[-2000:]))
        out.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])["seconds"])
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_images_timing.md"))
    a = ap.parse_args()
    lines = ["# Scene images: loading time", "", "Seconds for %d images, median (min .. max) of %d fresh processes each; written by tests/devtools/dev_scene_images.py." % (a.images, a.repeats), "",
             "| images | reference (`GOF_PIL_IMAGES=1`) | scene_images (`GOF_HIP_IMAGES=1`) | `image.load()` serial | `image.load()` pool | faster by more than the spread |", "|---|---|---|---|---|---|"]
    with tempfile.TemporaryDirectory() as tmp:
        for tag, W, H, res in SIZES:
            folder = os.path.join(tmp, tag)
            write_images(folder, W, H, a.images)
            t = {p: timed(p, folder, res, a.repeats) for p in ("pil", "hip", "decode_serial", "decode_pool")}
            fmt = lambda v: "%.2f (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))      # noqa: E731
            spread = max(max(t["pil"]) - min(t["pil"]), max(t["hip"]) - min(t["hip"]))
            faster = statistics.median(t["pil"]) - statistics.median(t["hip"]) > spread
            lines.append("| %s at `-r %d` | %s | %s | %s | %s | %s |" % (tag, res, fmt(t["pil"]), fmt(t["hip"]), fmt(t["decode_serial"]), fmt(t["decode_pool"]), "yes" if faster else "NO"))
            print(lines[-1], flush=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
