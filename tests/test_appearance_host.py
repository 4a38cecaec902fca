"""CPU tests of the decoupled-appearance L1: the kernels of csrc/appearance.hip through the host emulator
(tests/hipemu) behind train_epilogue.appearance's own Python layer, each case in a child process, held to
tests/appearance_restatement.py.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context are host stand-ins, and EVERY buffer the module allocates (workspaces, saved activations, outputs) is filled
with 0xA5 (a third run: 0x3C) and followed by guard bytes that are checked after the run.  The emulated library runs the same kernel
source; the one thing it restates is the matrix instruction (cross-lane reads and fmaf in the same k order).

Image sizes (H x W), all at the network's real widths (64 embedding values, 67 -> 256 -> ... -> 16 -> 16 -> 3):
  32 x 32    the low-resolution image is 1 x 1 (the `out == 1` branch of the down-sample), the first up-block works on 2 x 2
  75 x 100   crop 64 x 96 at top 5 / left 2, low-resolution image 2 x 3; the full-resolution plane (6144 pixels) is two chunks of the
             weight gradient with a ragged last one, every other plane is far below one chunk
  64 x 45    the crop (64 x 32) is narrower than the image on one axis only

Bounds.  A K-term fmaf chain plus the bias addition: lpips_restatement.conv_bound.  The weight gradient: a chain of at most L =
GOF_APP_WGRAD_CHUNK terms per chunk, then n_chunks - 1 additions: (L + n_chunks + 2) 2^-24 sum |dY' X| (the kernel's order -- fp32
sub-chains of 16 terms, accumulated in fp64 -- is a refinement of that chain and lies well inside it).  The bilinear resampling
l0h (l0w a + l1w b) + l1h (l0w c + l1w d) with the weights taken as the contract forms them: every value passes through a product, a
sum, a product and a sum = 4 roundings, (1 + u)^4 - 1 < 5 u: 5 * 2^-24 of the magnitude sum.  Its transpose: a term (lh lw) g is two
roundings and then passes through at most n additions, n the number of terms of that source pixel: (n + 2) 2^-24 of the magnitude."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import conv3x3_pins as P  # noqa: E402
import appearance_restatement as R  # noqa: E402

SIZES = [(32, 32), (75, 100), (64, 45)]             # (H, W)
U = 2.0 ** -24
# per convolution: how the product reads its input and the gradient of its output
X_MODE = ("embed", "shuffle", "shuffle", "shuffle", "shuffle", "up2", "plain")
DY_MODE = ("unshuffle", "unshuffle", "unshuffle", "unshuffle", "plain", "plain", "plain")
DL = 0.75                       # the incoming gradient the head's backward pieces are run with


def _case(H, W):
    image, gt = R.make_images(W, H, seed=300 + W)
    return image, gt, R.make_embedding(seed=5 + H), R.make_params(seed=9 + W)


def _refilling(M, byte):
    """every buffer the module allocates from now on is filled with `byte` instead of the seam's 0xA5 (the guards stay)"""
    inner = M.torch.empty

    def empty(*a, **k):
        t = inner(*a, **k)
        t.reshape(-1).view(torch.uint8).fill_(byte)
        return t
    M.torch.empty = empty


def stored_operands(ref, k):
    """what the product reads for convolution k: (stored x, embedding or None, stored dy, mask or None)"""
    x = ref["down"] if k == 0 else ref["y"][k - 1]
    dy = ref["d_x"][k + 1] if DY_MODE[k] == "unshuffle" else ref["d_y"][k]
    return x, dy, (ref["y"][k] if k < 6 else None)


def _child(case, out):
    import train_epilogue.appearance as M
    check = host_child.install_seams(M, buffers="all")
    kind, name = case.split(":", 1)
    res = {}
    if kind == "net":
        H, W = (int(v) for v in name.split("x"))
        image, gt, emb, params = _case(H, W)
        ref = R.run(image, gt, emb, params, torch.float32)
        Hc, Wc, top, left = R.crop_box(H, W)
        res["down"] = M.bilinear(image[:, top:top + Hc, left:left + Wc], (Hc // 32, Wc // 32)).numpy().copy()
        res["up2_backward"] = M.up2_backward(ref["d_x"][5]).numpy().copy()
        res["resized"] = M.bilinear(ref["transformed"], (H, W)).numpy().copy()
        for k in range(7):
            x, dy, mask = stored_operands(ref, k)
            w, b = params[2 * k], params[2 * k + 1]
            e = emb if k == 0 else None
            xin = M.materialize(x, X_MODE[k], emb=e)
            res["xin%d" % k] = xin.numpy().copy()
            res["conv%d" % k] = M.conv3x3(x, w, b, relu=False, mode=X_MODE[k], emb=e).numpy().copy()
            res["conv_plain%d" % k] = M.conv3x3(xin, w, b, relu=False).numpy().copy()
            res["relu%d" % k] = M.conv3x3(x, w, b, relu=True, mode=X_MODE[k], emb=e).numpy().copy()
            dyin = M.materialize(dy, DY_MODE[k], mask=mask)
            res["dyin%d" % k] = dyin.numpy().copy()
            wt = M.weight_transpose(w)
            res["wt%d" % k] = wt.numpy().copy()
            res["dgrad%d" % k] = M.conv3x3(dy, wt, None, mode=DY_MODE[k], mask=mask).numpy().copy()
            res["dgrad_plain%d" % k] = M.conv3x3(dyin, wt, None).numpy().copy()
            dW, db = M.conv3x3_wgrad(x, dy, mode=X_MODE[k], emb=e, dy_mode=DY_MODE[k], mask=mask)
            res["dW%d" % k], res["db%d" % k] = dW.numpy().copy(), db.numpy().copy()
            dW2, db2 = M.conv3x3_wgrad(xin, dyin)
            res["dW_plain%d" % k], res["db_plain%d" % k] = dW2.numpy().copy(), db2.numpy().copy()
        runs = []
        for fill in (None, None, 0x3C):
            if fill is not None:
                _refilling(M, fill)
            img = image.clone().requires_grad_(True)
            e = emb.clone().requires_grad_(True)
            ps = [p.clone().requires_grad_(True) for p in params]
            loss = M.appearance_l1(img, gt, e, ps)
            loss.backward()
            runs.append(np.concatenate([loss.detach().reshape(1).numpy(), img.grad.reshape(-1).numpy(), e.grad.numpy()] + [p.grad.reshape(-1).numpy() for p in ps]).copy())
        res["runs"] = np.stack(runs)
        res["transformed"] = M._forward(image, gt, emb, params, True)[1].numpy().copy()
        loss_p, m_p, t_p = M.head_forward(ref["y"][6], image, gt)
        res["head_loss"], res["head_m"], res["head_t"] = loss_p.reshape(1).numpy().copy(), m_p.numpy().copy(), t_p.numpy().copy()
        res["head_dz"] = M.head_backward(ref["m"], image, gt, torch.tensor(DL)).numpy().copy()
        res["image_grad"] = M.image_grad(ref["m"], image, gt, torch.tensor(DL), ref["d_down"]).numpy().copy()
    elif kind == "errors":
        emb, params = R.make_embedding(seed=1), R.make_params(seed=1)
        for tag, (H, W) in (("h31", (31, 40)), ("w31", (40, 31))):
            image, gt = R.make_images(W, H, seed=3)
            try:
                M.appearance_l1(image, gt, emb, params)
                res[tag] = np.array("")
            except RuntimeError as e:
                res[tag] = np.array(str(e))
        image, gt = R.make_images(32, 32, seed=3)
        for tag, call in (("params13", lambda: M.appearance_l1(image, gt, emb, params[:13])),
                          ("emb63", lambda: M.appearance_l1(image, gt, emb[:63], params)),
                          ("gt_shape", lambda: M.appearance_l1(image, gt[:, :31], emb, params)),
                          ("shuffle6", lambda: M.conv3x3(torch.zeros((6, 4, 4)), torch.zeros((8, 1, 3, 3)), mode="shuffle")),
                          ("mask", lambda: M.conv3x3(torch.zeros((4, 4, 4)), torch.zeros((8, 4, 3, 3)), mask=torch.zeros((4, 4, 5))))):
            try:
                call()
                res[tag] = np.array("")
            except RuntimeError as e:
                res[tag] = np.array(str(e))
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path, buffers=True):
    res = host_child.run_child(__file__, case, tmp_path, timeout=1800)
    assert (int(res["buffers"]) > 0) == buffers
    return res


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    """one child per size, shared by the tests below (the results are only read)"""
    cache = {}

    def get(size):
        if size not in cache:
            cache[size] = _emulate("net:%dx%d" % size, tmp_path_factory.mktemp("appearance_%dx%d" % size))
        return cache[size]
    return get


@pytest.fixture(scope="module")
def restated():
    """per size: the case and its restatement at fp32 and fp64 (only read)"""
    cache = {}

    def get(size):
        if size not in cache:
            case = _case(*size)
            cache[size] = (case, R.run(*case, torch.float32), R.run(*case, torch.float64))
        return cache[size]
    return get


ids = dict(ids=lambda s: "%dx%d" % s)


@pytest.mark.parametrize("size", SIZES, **ids)
def test_the_views_are_what_torch_materialises(size, emulated, restated):
    """pixel-shuffle, its inverse with the ReLU mask, and the embedding planes are exact; the x2 up-sample is within the resampling bound"""
    res = emulated(size)
    (_, _, emb, _), ref, _ = restated(size)
    for k in range(7):
        if X_MODE[k] != "up2":
            assert np.array_equal(res["xin%d" % k], ref["x"][k].numpy()), "input view of convolution %d" % k
        else:
            truth, mag = R.bilinear_truth(ref["y"][k - 1], ref["x"][k].shape[1:])
            ratio = ((torch.from_numpy(res["xin%d" % k]).double() - truth).abs() / (5 * U * mag).clamp_min(1e-300)).max().item()
            print("x2 up-sample: max err / bound = %.3f" % ratio)
            assert 0 < ratio <= 1
        assert np.array_equal(res["dyin%d" % k], ref["d_pre"][k].numpy()), "gradient view of convolution %d" % k
        assert np.array_equal(res["wt%d" % k], R.transposed_weight(_case(*size)[3][2 * k]).numpy())


@pytest.mark.parametrize("size", SIZES, **ids)
def test_the_resamplings_are_within_the_bound_of_their_formula(size, emulated, restated):
    res = emulated(size)
    (image, _, _, _), ref, _ = restated(size)
    H, W = size
    Hc, Wc, top, left = R.crop_box(H, W)
    worst = 0.0
    for name, src, out_size in (("down", image[:, top:top + Hc, left:left + Wc], (Hc // 32, Wc // 32)), ("resized", ref["transformed"], (H, W))):
        truth, mag = R.bilinear_truth(src, out_size)
        got = torch.from_numpy(res[name]).double()
        ratio = ((got - truth).abs() / (5 * U * mag).clamp_min(1e-300)).max().item()
        print("%s: max err / bound = %.3f" % (name, ratio))
        assert got.shape == truth.shape and ratio <= 1
        worst = max(worst, ratio)
    # the fp32 framework's own result is near (its weights differ in the last bits of the coordinate, not in the formula)
    assert np.allclose(res["down"], ref["down"].numpy(), rtol=0, atol=1e-4)
    truth, mag, terms = R.bilinear_transpose_truth(ref["d_x"][5], ref["y"][4].shape[1:])
    got = torch.from_numpy(res["up2_backward"]).double()
    ratio = ((got - truth).abs() / ((terms + 2) * U * mag).clamp_min(1e-300)).max().item()
    print("transpose of the x2 up-sample: max err / bound = %.3f" % ratio)
    assert got.shape == truth.shape and ratio <= 1 and max(worst, ratio) > 0
    assert np.allclose(res["up2_backward"], ref["d_y"][4].numpy(), rtol=0, atol=1e-5 * float(ref["d_y"][4].abs().max()))


@pytest.mark.parametrize("size", SIZES, **ids)
def test_every_convolution_and_data_gradient_is_within_the_bound_of_a_k_term_chain(size, emulated, restated):
    """|out - fp64| <= (K + 2) 2^-24 (sum |w x| + |b|) on identical fp32 inputs, K = 9 C_in (forward) and 9 C_out (data gradient); the
    fused operand views give the bits of the materialised operand; the ReLU output is the max(., 0) of the plain one"""
    res = emulated(size)
    (_, _, _, params), _, _ = restated(size)
    worst = 0.0
    for k in range(7):
        w, b = params[2 * k], params[2 * k + 1]
        x = torch.from_numpy(res["xin%d" % k])
        truth = torch.nn.functional.conv2d(x.double()[None], w.double(), b.double(), padding=1)[0]
        got = torch.from_numpy(res["conv%d" % k]).double()
        r1 = ((got - truth).abs() / R.conv_bound(x, w, b)).max().item()
        dy = torch.from_numpy(res["dyin%d" % k])
        wt = R.transposed_weight(w)
        truth_d = torch.nn.functional.conv2d(dy.double()[None], wt.double(), None, padding=1)[0]
        got_d = torch.from_numpy(res["dgrad%d" % k]).double()
        r2 = ((got_d - truth_d).abs() / R.conv_bound(dy, wt).clamp_min(1e-300)).max().item()
        print("convolution %d (%d -> %d, %dx%d): forward max err / bound = %.3f, data gradient %.3f" % (k, w.shape[1], w.shape[0], x.shape[2], x.shape[1], r1, r2))
        assert got.shape == truth.shape and r1 <= 1 and got_d.shape == truth_d.shape and r2 <= 1, "convolution %d" % k
        assert np.array_equal(res["conv%d" % k].view(np.uint32), res["conv_plain%d" % k].view(np.uint32))
        assert np.array_equal(res["dgrad%d" % k].view(np.uint32), res["dgrad_plain%d" % k].view(np.uint32))
        assert np.array_equal(res["relu%d" % k], np.maximum(res["conv%d" % k], 0.0))
        worst = max(worst, r1, r2)
    assert worst > 0


@pytest.mark.parametrize("size", SIZES, **ids)
def test_every_weight_and_bias_gradient_is_within_the_bound_of_its_chunked_chain(size, emulated, restated):
    """(L + n_chunks + 2) 2^-24 sum |dY' X|, L = the chunk length; fused views = the materialised operands, bit for bit"""
    import train_epilogue.appearance as M
    res = emulated(size)
    worst = 0.0
    for k in range(7):
        x, dy = torch.from_numpy(res["xin%d" % k]), torch.from_numpy(res["dyin%d" % k])
        dW, db, mW, mb = R.wgrad_truth(x, dy)
        n_chunks = -(-(x.shape[1] * x.shape[2]) // M.WGRAD_CHUNK)
        f = (M.WGRAD_CHUNK + n_chunks + 2) * U
        rW = ((torch.from_numpy(res["dW%d" % k]).double() - dW).abs() / (f * mW).clamp_min(1e-300)).max().item()
        rb = ((torch.from_numpy(res["db%d" % k]).double() - db).abs() / (f * mb).clamp_min(1e-300)).max().item()
        print("convolution %d: %d chunk(s), weight gradient max err / bound = %.4f, bias gradient %.4f" % (k, n_chunks, rW, rb))
        assert res["dW%d" % k].shape == tuple(dW.shape) and rW <= 1 and rb <= 1, "convolution %d" % k
        assert np.array_equal(res["dW%d" % k].view(np.uint32), res["dW_plain%d" % k].view(np.uint32))
        assert np.array_equal(res["db%d" % k].view(np.uint32), res["db_plain%d" % k].view(np.uint32))
        worst = max(worst, rW, rb)
        if size == (75, 100) and k >= 5:
            assert n_chunks == 2 and (x.shape[1] * x.shape[2]) % M.WGRAD_CHUNK != 0
        elif k < 5:
            assert n_chunks == 1
    assert worst > 0


@pytest.mark.parametrize("size", SIZES, **ids)
def test_the_ends_are_within_the_bounds_of_their_formulas(size, emulated, restated):
    """sigmoid / product / L1 on the restatement's fp32 z, their backward on its fp32 sigmoid, and the image gradient (g m + the
    transpose of the down-sample, zero outside the crop) on its fp32 d_down: bounds derived in appearance_restatement.head_truth,
    head_backward_truth and image_grad_truth (a few units of 2^-24 of the magnitude)"""
    res = emulated(size)
    (image, gt, _, _), ref, _ = restated(size)
    (m, t, loss), (bm, bt, bl) = R.head_truth(ref["y"][6], image, gt)
    r = {"m": ((torch.from_numpy(res["head_m"]).double() - m).abs() / bm).max().item(),
         "t": ((torch.from_numpy(res["head_t"]).double() - t).abs() / bt.clamp_min(1e-300)).max().item(),
         "loss": abs(float(res["head_loss"][0]) - loss.item()) / bl.item()}
    dz, bdz = R.head_backward_truth(ref["m"], image, gt, DL)
    r["dz"] = ((torch.from_numpy(res["head_dz"]).double() - dz).abs() / bdz.clamp_min(1e-300)).max().item()
    di, bdi = R.image_grad_truth(ref["m"], image, gt, DL, ref["d_down"])
    got = torch.from_numpy(res["image_grad"]).double()
    r["d_image"] = ((got - di).abs() / bdi.clamp_min(1e-300)).max().item()
    print("the ends, max err / bound: %s" % r)
    assert all(v <= 1 for v in r.values()) and max(r.values()) > 0 and got.shape == di.shape
    assert (got[bdi == 0] == 0).all() and (bdi == 0).any() == (size != (32, 32))
    # and the fp32 framework's own values are near (same formulas, its own rounding)
    assert np.allclose(res["head_dz"], DL * ref["d_pre"][6].numpy(), rtol=0, atol=1e-5 * DL * float(ref["d_pre"][6].abs().max()))


@pytest.mark.parametrize("size", SIZES, **ids)
def test_loss_and_gradients_are_reproducible_and_close_to_the_truth(size, emulated, restated):
    """bit-identical across three runs and two fills of every buffer (0xA5, 0xA5, 0x3C); and near the fp64 restatement (1e-4 of each
    tensor's maximum: a sanity bound far above fp32 rounding at these sizes, the sharp comparison is the GPU suite's)"""
    res = emulated(size)
    runs = res["runs"].view(np.uint32)
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    _, ref32, ref64 = restated(size)
    got = res["runs"][0].astype(np.float64)
    parts = [ref64["loss"].reshape(1), ref64["d_image"].reshape(-1), ref64["d_embedding"]] + [p.reshape(-1) for p in ref64["d_params"]]
    at = 0
    for i, want in enumerate(parts):
        want = want.numpy()
        g = got[at:at + want.size]
        at += want.size
        err = np.abs(g - want).max() / np.abs(want).max()
        print("tensor %d (%d values): max error / max = %.3g" % (i, want.size, err))
        assert np.isfinite(g).all() and np.abs(want).max() > 0 and err <= 1e-4, "tensor %d" % i
    assert at == got.size
    H, W = size
    Hc, Wc, top, left = R.crop_box(H, W)
    d_image = got[1:1 + 3 * H * W].reshape(3, H, W)
    outside = np.ones((H, W), dtype=bool)
    outside[top:top + Hc, left:left + Wc] = False
    assert (d_image[:, outside] == 0).all()
    assert np.allclose(res["transformed"], ref64["transformed"].numpy(), rtol=0, atol=1e-5)


def test_refusals(tmp_path):
    res = _emulate("errors:all", tmp_path, buffers=False)          # (every refusal comes before the first allocation)
    assert "smaller than 32" in str(res["h31"]) and "40 x 31" in str(res["h31"])
    assert "smaller than 32" in str(res["w31"]) and "31 x 40" in str(res["w31"])
    assert "14 parameter tensors" in str(res["params13"])
    assert "conv1.weight" in str(res["emb63"]) and "66 input channels" in str(res["emb63"])
    assert "must both be (3, H, W)" in str(res["gt_shape"])
    assert "multiple of 4" in str(res["shuffle6"]) and "does not fit the view" in str(res["mask"])


def test_host_tensors_are_refused():
    import train_epilogue.appearance as M
    image, gt = R.make_images(32, 32, seed=1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        M.appearance_l1(image, gt, R.make_embedding(1), R.make_params(1))
    with pytest.raises(RuntimeError, match="ROCm device"):
        M.conv3x3(torch.zeros((3, 8, 8)), torch.zeros((5, 3, 3, 3)))
    with pytest.raises(RuntimeError, match="ROCm device"):
        M.bilinear(torch.zeros((3, 8, 8)), (4, 4))


def test_size_queries_and_argument_checks():
    """through the C ABI, with pointers that are never followed: every refusal comes before the first launch"""
    import train_epilogue.appearance as M
    L = M.lib
    net = M.GofAppNet(64, (C.c_int32 * 6)(*R.WIDTHS))
    small, big = L.gof_app_workspace_bytes(32, 32, net), L.gof_app_workspace_bytes(1600, 1063, net)
    assert 0 < small < big and big >= 2 * 16 * 1056 * 1600 * 4
    saved = L.gof_app_saved_bytes(1600, 1063, net)
    assert 16 * 1056 * 1600 * 4 < saved < 2 * 16 * 1056 * 1600 * 4
    assert L.gof_app_workspace_bytes(31, 64, net) == 0 and b"smaller than 32" in L.gof_last_error()
    assert L.gof_app_saved_bytes(64, 31, net) == 0
    odd = M.GofAppNet(64, (C.c_int32 * 6)(256, 128, 62, 32, 16, 16))
    assert L.gof_app_workspace_bytes(64, 64, odd) == 0 and b"multiples of 4" in L.gof_last_error()
    assert L.gof_app_conv3x3(0, 8, 8, 8, None, 0, None, None, None, None, 0, None, None) < 0 and b"[1, 4096]" in L.gof_last_error()
    assert L.gof_app_conv3x3(3, 5, 8, 8, None, 0, None, None, None, None, 0, None, None) < 0 and b"NULL" in L.gof_last_error()
    assert L.gof_app_conv3x3(3, 5, 7, 8, None, 1, None, None, None, None, 0, None, None) < 0 and b"even W and H" in L.gof_last_error()
    assert L.gof_app_conv3x3_wgrad(3, 5, 8, 8, 4096, 0, None, 8192, 0, None, 12288, 16384, 20480, 16, None) == -2      # GOF_E_WORKSPACE
    # overlapping output and input: d_image inside image; the workspace inside the saved buffer
    sb, wb = L.gof_app_saved_bytes(64, 64, net), L.gof_app_workspace_bytes(64, 64, net)
    fake = (C.c_void_p * 14)(*[1 << 20] * 14)
    base = 1 << 30
    args = dict(image=base, gt=base + (1 << 20), saved=base + (2 << 20), ws=base + (2 << 20) + sb + 4096)
    assert L.gof_app_l1_backward(64, 64, net, args["image"], args["gt"], 4096, fake, 4096, args["saved"], sb, args["image"] + 64, 8192, fake,
                                 args["ws"], wb, None) == -1 and b"overlaps" in L.gof_last_error()
    assert L.gof_app_l1_forward(64, 64, net, args["image"], args["gt"], 4096, fake, 8192, None, args["saved"], sb, args["saved"] + 256, wb, None) == -1
    assert b"overlaps" in L.gof_last_error()
    assert L.gof_app_l1_forward(64, 64, net, args["image"], args["gt"], 4096, fake, args["gt"] + 16, None, args["saved"], sb, args["ws"], wb, None) == -1
    assert b"overlaps" in L.gof_last_error()
    assert C.sizeof(M.GofAppNet) == 28 and M.WGRAD_CHUNK == 4096 and 300 <= -(-1056 * 1600 // M.WGRAD_CHUNK) <= 500
    assert tuple(M.PARAM_NAMES) == tuple(R.PARAM_NAMES)


def test_the_convolution_and_the_narrow_network_give_the_pinned_bits(tmp_path):
    """the SHA-256 of every output of tests/conv3x3_pins.py's appearance cases (every view, tile shape, zero-row pattern, with and without
    mask / bias / ReLU) and of the loss and the 16 gradients of the narrowest network at 32 x 32 (conv3's head epilogue) is the one
    recorded in tests/golden/conv3x3_pins.json: the order of K has not moved"""
    got = P.emulated("appearance", tmp_path)
    assert len(got) == len(P.app_cases()) + 17 and P.unpinned("appearance", "host", got) == []


def test_the_lpips_and_the_appearance_convolution_give_the_same_bits(tmp_path):
    """one main loop, one order of K: gof_lpips_conv3x3 on one image and gof_app_conv3x3 (PLAIN view, no mask, with the bias) are
    torch.equal for C_out 32, 64, 96 and 128 (96 runs different tiles in the two units) at C_in 3, 6 and 8 on the 17 x 9 plane"""
    assert P.emulated("contract", tmp_path) == []


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
