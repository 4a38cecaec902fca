#!/usr/bin/env python3
"""Developer tool: what render.py's loop costs with the parent commit's save_image (torch arithmetic, a blocking copy,
Pillow's encoder) and with image_writer.save_image, next to the render-only floor.

    python tests/devtools/dev_png_encode.py [--views 32] [--repeats 5] [--out profiles/png_encode.md]

Per size (1237 x 822, 1600 x 1063): a synthetic scene rendered through GaussianRasterizer, and per view the two calls of render.py:35-36
(`rendering[:3]` of the nine planes, and a ground-truth image) into a temporary directory.  The three variants run interleaved
(floor, Pillow, HIP, floor, ...), `repeats` times after one warm-up round; a round ends with flush() and a device synchronisation, so the
files are on disk when the clock stops.  Also records the stream sizes of the test cases against zlib's Z_RLE stream and Pillow's files.
Asserts nothing."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "gaussian-opacity-fields_amd"), os.path.join(ROOT, "gaussian-opacity-fields_amd", "shims"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.append(p) if p.endswith("shims") else sys.path.insert(0, p)


def sizes_table():
    import png_encode_cases as K
    import image_writer as IW
    lines = ["| case | scanline bytes | blocks | stream | Z_RLE stream | ratio | our file | Pillow's file | ratio | size asserted |", "|---|---|---|---|---|---|---|---|---|---|"]
    for n in K.CASES:
        t = K.tensor(n)
        r = K.check_png(n, IW.encode_png(K.view(n, t.cuda())), t)
        lines.append("| %s | %d | %d | %d | %d | %.4f | %d | %d | %.4f | %s |" % (n, r["stream"], r["blocks"], r["ours"], r["zrle"], r["ours"] / r["zrle"], r["png"], r["pillow"],
                                                                            r["png"] / r["pillow"], "yes" if K.CASES[n][1] else "no"))
    return lines


def timing(W, H, views, repeats):
    import torch
    import synthetic_scenes as S
    from gpu_common import to_dev, settings_from
    from diff_gaussian_rasterization import GaussianRasterizer
    import torchvision.utils as tvu
    import image_writer as IW
    sc = S.scene_frustum(200000, W=W, H=H, focal=0.9 * W, seed=3, kernel_size=0.1)
    sd = to_dev(sc, "cuda:0")
    rast = GaussianRasterizer(settings_from(sd))
    gt = torch.rand((3, H, W), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 0.2 + 0.4
    pil = tvu.save_image
    IW.previous = pil
    variants = {"floor": lambda t, p: None, "pillow": pil, "hip": IW.save_image}
    times = {k: [] for k in variants}
    with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        for rep in range(repeats + 1):
            for name, save in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for v in range(views):
                    color, _ = rast(means3D=sd["means3D"], means2D=torch.zeros_like(sd["means3D"]), shs=sd["shs"], opacities=sd["opacities"],
                                    scales=sd["scales"], rotations=sd["rotations"])
                    save(color[:3], os.path.join(tmp, "%s_r%05d.png" % (name, v)))
                    save(gt, os.path.join(tmp, "%s_g%05d.png" % (name, v)))
                IW.flush()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
        one = os.path.getsize(os.path.join(tmp, "hip_r00000.png")), os.path.getsize(os.path.join(tmp, "pillow_r00000.png"))
    return times, one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_encode.md"))
    ap.add_argument("--sizes", default="1237x822,1600x1063")
    a = ap.parse_args()
    import torch
    lines = ["# PNG encoder: sizes and render.py's loop (tests/devtools/dev_png_encode.py)", "",
             "Device: %s.  %d views, %d repeats after one warm-up round, the variants interleaved; a round ends with flush() and a device" % (torch.cuda.get_device_name(0), a.views, a.repeats),
             "synchronisation.  Times are seconds per round: median (min .. max).", "",
             "| size | render only | Pillow path (parent) | HIP path | per view: Pillow - floor | per view: HIP - floor | file: HIP / Pillow bytes |", "|---|---|---|---|---|---|---|"]
    for s in a.sizes.split(","):
        W, H = (int(v) for v in s.split("x"))
        t, one = timing(W, H, a.views, a.repeats)
        f = lambda k: "%.3f (%.3f .. %.3f)" % (statistics.median(t[k]), min(t[k]), max(t[k]))      # noqa: E731
        m = {k: statistics.median(v) for k, v in t.items()}
        lines.append("| %d x %d | %s | %s | %s | %.1f ms | %.1f ms | %d / %d |" % (W, H, f("floor"), f("pillow"), f("hip"), 1e3 * (m["pillow"] - m["floor"]) / a.views,
                                                                            1e3 * (m["hip"] - m["floor"]) / a.views, one[0], one[1]))
        print(lines[-1], flush=True)
    lines += ["", "## Stream and file sizes of the test cases", ""] + sizes_table()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
