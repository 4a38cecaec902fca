#!/usr/bin/env python3
"""Times the decoupled-appearance L1, forward plus backward, in one process on one GPU:

    torch    train.py:67-88 and scene/appearance_network.py as torch composes them (tests/appearance_restatement.py on the device:
             F.conv2d through MIOpen, F.pixel_shuffle, F.interpolate, autograd)
    hip      train_epilogue.appearance.appearance_l1 (csrc/appearance.hip)

at 1600x1063 and 800x800, interleaved (torch, hip, torch, hip, ...) after a warm-up, each sample timed with device events around one
forward + backward; the table reports the median, the minimum and the spread (max - min) of each.  The torch path is the plain
composition (no retained intermediates).  Then, at 1600x1063, every kernel of the HIP path alone through the exported pieces (median
of --reps), and with --iterations N the complete iteration: the reference's unchanged train.py (oracle/_ref/refpy) through the
launcher with --use_decoupled_appearance on the synthetic Blender scene of tests/fixtures, under GOF_TORCH_APPEARANCE=1 and
GOF_HIP_APPEARANCE=1, as (wall(3N) - wall(N)) / 2N so that start-up cancels.

    python tests/devtools/dev_appearance_time.py [--reps 15] [--out profiles/appearance_timing.md]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "gaussian-opacity-fields_amd"))

import torch  # noqa: E402

import appearance_restatement as R  # noqa: E402
import train_epilogue.appearance as A  # noqa: E402

DEV = "cuda:0"


def case(W, H):
    image, gt = R.make_images(W, H, seed=1)
    return (image.to(DEV), gt.to(DEV), R.make_embedding(2).to(DEV), [p.to(DEV) for p in R.make_params(3)])


def torch_step(image, gt, emb, params):
    """train.py:67-88 + scene/appearance_network.py as torch composes them, forward + backward"""
    F = torch.nn.functional
    img = image.clone().requires_grad_(True)
    e = emb.clone().requires_grad_(True)
    ps = [p.detach().requires_grad_(True) for p in params]
    Hc, Wc, top, left = R.crop_box(*image.shape[1:])
    ci, cg = img[:, top:top + Hc, left:left + Wc], gt[:, top:top + Hc, left:left + Wc]
    down = F.interpolate(ci[None], size=(Hc // 32, Wc // 32), mode="bilinear", align_corners=True)[0]
    x = torch.cat([down, e[None].repeat(Hc // 32, Wc // 32, 1).permute(2, 0, 1)], dim=0)[None]
    for k in range(7):
        if 1 <= k <= 4:
            x = F.pixel_shuffle(x, 2)
        elif k == 5:
            x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        x = F.conv2d(x, ps[2 * k], ps[2 * k + 1], padding=1)
        if k < 6:
            x = torch.relu(x)
    loss = torch.abs(torch.sigmoid(x) * ci - cg).mean()
    loss.backward()
    return loss.detach()


X_MODE = ("embed", "shuffle", "shuffle", "shuffle", "shuffle", "up2", "plain")
DY_MODE = ("unshuffle", "unshuffle", "unshuffle", "unshuffle", "plain", "plain", "plain")


def kernel_table(W, H, reps):
    """every kernel of the HIP path alone, on random operands of the real shapes"""
    Hc, Wc = H // 32 * 32, W // 32 * 32
    h, w = Hc // 32, Wc // 32
    image, gt, emb, params = case(W, H)
    chans = R.channels()
    planes = [(h, w)] + [(h << k, w << k) for k in range(1, 5)] + [(Hc, Wc), (Hc, Wc)]
    g = torch.Generator(device=DEV).manual_seed(0)

    def rnd(*shape):
        return torch.randn(shape, generator=g, device=DEV)
    rows = []

    def add(name, fn):
        fn()
        v = [timed(fn, ()) for _ in range(reps)]
        rows.append((name, statistics.median(v)))
    for k, ((ci, co), (ph, pw)) in enumerate(zip(chans, planes)):
        stored = {"embed": (3, ph, pw), "shuffle": (4 * ci, ph // 2, pw // 2), "up2": (ci, ph // 2, pw // 2), "plain": (ci, ph, pw)}[X_MODE[k]]
        x, e = rnd(*stored), (emb if k == 0 else None)
        dy = rnd(*((co // 4, 2 * ph, 2 * pw) if DY_MODE[k] == "unshuffle" else (co, ph, pw)))
        mask = rnd(co, ph, pw) if k < 6 else None
        wt = A.weight_transpose(params[2 * k])
        name = R.PARAM_NAMES[k]
        add("%s forward (%d -> %d, %dx%d, %s)" % (name, ci, co, pw, ph, X_MODE[k]), lambda: A.conv3x3(x, params[2 * k], params[2 * k + 1], relu=k < 6, mode=X_MODE[k], emb=e))
        add("%s data gradient" % name, lambda: A.conv3x3(dy, wt, None, mode=DY_MODE[k], mask=mask))
        add("%s weight + bias gradient" % name, lambda: A.conv3x3_wgrad(x, dy, mode=X_MODE[k], emb=e, dy_mode=DY_MODE[k], mask=mask))
    gu = rnd(chans[5][0], Hc, Wc)
    add("transpose of the x2 up-sample", lambda: A.up2_backward(gu))
    z, m, dd, dL = rnd(3, Hc, Wc), torch.rand((3, Hc, Wc), generator=g, device=DEV), rnd(3, h, w), torch.tensor(1.0, device=DEV)
    add("sigmoid / product / L1 on a stored z", lambda: A.head_forward(z, image, gt))
    add("image gradient (g m + transpose of the down-sample)", lambda: A.image_grad(m, image, gt, dL, dd))
    add("down-sample", lambda: A.bilinear(image[:, :Hc, :Wc], (h, w)))
    rows.sort(key=lambda r: -r[1])
    return rows


def iteration_times(n):
    """ms per complete iteration of train.py --use_decoupled_appearance through the launcher, {setting: ms}"""
    import subprocess
    import tempfile
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_e2e_scripts_gpu as E
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene")
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fixtures", "make_blender_scene.py"), scene], env=E._env(), check=True, capture_output=True)
        for setting in ("GOF_TORCH_APPEARANCE", "GOF_HIP_APPEARANCE"):
            wall = []
            for iters in (n, 3 * n):
                cmd = [sys.executable, os.path.join(E.PKG, "launch", "run_reference_script.py"), os.path.join(E.REFPY, "train.py"), "-s", scene,
                       "-m", os.path.join(tmp, "%s_%d" % (setting, iters)), "--iterations", str(iters), "--densify_from_iter", "100000",
                       "--test_iterations", "100000", "--save_iterations", "100000", "--use_decoupled_appearance"]
                t0 = time.time()
                subprocess.run(cmd, env=E._env(**{setting: "1"}), cwd=ROOT, check=True, capture_output=True)
                wall.append(time.time() - t0)
            out[setting] = 1000.0 * (wall[1] - wall[0]) / (2 * n)
    return out


def hip_step(image, gt, emb, params):
    img = image.clone().requires_grad_(True)
    e = emb.clone().requires_grad_(True)
    ps = [p.detach().requires_grad_(True) for p in params]
    loss = A.appearance_l1(img, gt, e, ps)
    loss.backward()
    return loss.detach()


def timed(fn, args):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(*args)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--iterations", type=int, default=0, help="N: also time the complete iteration through the launcher (runs of N and 3N)")
    o = ap.parse_args()
    lines = ["| size (W x H) | path | median ms | min ms | spread ms | loss |", "|---|---|---|---|---|---|"]
    for W, H in ((1600, 1063), (800, 800)):
        args = case(W, H)
        for _ in range(o.warmup):
            torch_step(*args)
            hip_step(*args)
        torch.cuda.synchronize()
        t, h = [], []
        for _ in range(o.reps):
            t.append(timed(torch_step, args))
            h.append(timed(hip_step, args))
        lt, lh = torch_step(*args).item(), hip_step(*args).item()
        for name, v, loss in (("torch", t, lt), ("hip", h, lh)):
            lines.append("| %d x %d | %s | %.3f | %.3f | %.3f | %.9g |" % (W, H, name, statistics.median(v), min(v), max(v) - min(v), loss))
        print("\n".join(lines[-2:]), flush=True)
    lines += ["", "| kernel of the HIP path at 1600 x 1063, alone | median ms |", "|---|---|"]
    rows = kernel_table(1600, 1063, max(3, o.reps // 3))
    lines += ["| %s | %.3f |" % r for r in rows] + ["| sum | %.3f |" % sum(r[1] for r in rows)]
    if o.iterations:
        it = iteration_times(o.iterations)
        lines += ["", "| complete iteration, train.py --use_decoupled_appearance through the launcher | ms |", "|---|---|"]
        lines += ["| %s=1 | %.2f |" % kv for kv in it.items()]
    text = "\n".join(lines) + "\n"
    print(text)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
