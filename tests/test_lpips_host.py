"""CPU tests of the LPIPS metric: the kernels of csrc/lpips.hip through the host emulator (tests/hipemu) behind
image_metrics' own Python layer, each case in a child process, held to tests/lpips_restatement.py.

In the child the product module runs unchanged except for its test seams: GOF_HIP_LIB names the emulated library, the device check /
stream / device context are host stand-ins, and EVERY buffer image_metrics allocates (workspace and outputs) is filled with 0xA5 (a
second run: 0x3C) and followed by guard bytes that are checked after the run.  The emulated library runs the same kernel source; the
one thing it restates is the matrix instruction (cross-lane reads and fmaf in the same k order).

Thin instances of the VGG structure (tap widths 32, 32, 64, 64, 128: every tile shape of the convolution) at 16x16 (the last tap is
1x1), 37x53 (odd at every pool level) and 24x20 (pixel counts that are no multiple of the pixel tile at any level)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "hipemu"))
import host_child  # noqa: E402
import conv3x3_pins as P  # noqa: E402
import lpips_restatement as R  # noqa: E402

SIZES = [(16, 16), (37, 53), (24, 20)]
LAYERS = R.vgg_layers(R.THIN_WIDTHS)
RELU_LAYERS = (0, 3, 12)        # the layers also run with their ReLU as single calls (one per tile shape); the network runs apply it everywhere


def _case(W, H):
    a, b = R.make_images(W, H, seed=100 + W)
    return a[0], b[0], R.make_weights(LAYERS, seed=7 + H)


def _refilling(M, byte):
    """every buffer the module allocates from now on is filled with `byte` instead of the seam's 0xA5 (the guards stay)"""
    inner = M.torch.empty

    def empty(*a, **k):
        t = inner(*a, **k)
        t.reshape(-1).view(torch.uint8).fill_(byte)
        return t
    M.torch.empty = empty


def _child(case, out):
    import image_metrics as M
    check = host_child.install_seams(M, buffers="all")
    kind, name = case.split(":", 1)
    res = {}
    if kind == "net":
        W, H = (int(v) for v in name.split("x"))
        img0, img1, weights = _case(W, H)
        ref = R.forward(img0, img1, LAYERS, weights, torch.float32)
        # every layer on the restatement's fp32 input, before the ReLU; every pool on the restatement's fp32 input
        for i, (x, w, b) in enumerate(zip(ref["layer_in"], weights[0], weights[1])):
            res["in%d" % i] = x.numpy()
            res["conv%d" % i] = M.conv3x3(x, w, b, relu=False).numpy().copy()
            if i in RELU_LAYERS:
                res["relu%d" % i] = M.conv3x3(x, w, b, relu=True).numpy().copy()
        k = 0
        for i, L in enumerate(LAYERS):
            if L[2]:
                src = torch.relu(ref["pre_relu"][i - 1])
                res["pool_in%d" % k] = src.numpy()
                res["pool%d" % k] = M.maxpool2(src).numpy().copy()
                k += 1
        runs = []
        for fill in (None, None, 0x3C):
            if fill is not None:
                _refilling(M, fill)
            v, taps = M.network_distance(img0, img1, LAYERS, *weights)
            runs.append(np.concatenate([v.reshape(1).numpy(), taps.numpy()]).copy())
        res["runs"] = np.stack(runs)
    elif kind == "errors":
        weights = R.make_weights(LAYERS, seed=1)
        for tag, (W, H) in (("w15", (15, 16)), ("h15", (16, 15))):
            a, b = R.make_images(W, H, seed=3)
            try:
                M.network_distance(a[0], b[0], LAYERS, *weights)
                res[tag] = np.array("")
            except RuntimeError as e:
                res[tag] = np.array(str(e))
        x = torch.zeros((1, 8, 8, 8))
        try:
            M.conv3x3(x, torch.zeros((48, 8, 3, 3)), torch.zeros(48))
            res["c48"] = np.array("")
        except RuntimeError as e:
            res["c48"] = np.array(str(e))
        bad = ((3, 48, 0, 1),)
        desc = (M.GofLpipsLayer * 1)(M.GofLpipsLayer(3, 48, 0, 1))
        res["ws48"] = np.array(int(M.lib.gof_lpips_workspace_bytes(16, 16, 1, desc)))
        try:
            a, b = R.make_images(16, 16, seed=3)
            M.network_distance(a[0], b[0], bad, [torch.zeros((48, 3, 3, 3))], [torch.zeros(48)], [torch.zeros(48)])
            res["net48"] = np.array("")
        except RuntimeError as e:
            res["net48"] = np.array(str(e))
    else:
        raise KeyError(case)
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def _emulate(case, tmp_path):
    res = host_child.run_child(__file__, case, tmp_path, timeout=1800)
    assert int(res["buffers"]) > 0
    return res


@pytest.fixture(scope="module")
def emulated(tmp_path_factory):
    """one child per size, shared by the tests below (the results are only read)"""
    cache = {}

    def get(size):
        if size not in cache:
            cache[size] = _emulate("net:%dx%d" % size, tmp_path_factory.mktemp("lpips_%dx%d" % size))
        return cache[size]
    return get


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_conv_layer_is_within_the_bound_of_a_k_term_chain(size, emulated):
    """|out - fp64| <= (K + 2) 2^-24 (sum |w x| + |b|) on identical fp32 inputs, before the ReLU; the ReLU output is its max(., 0)"""
    res = emulated(size)
    _, _, weights = _case(*size)
    for i, (w, b) in enumerate(zip(weights[0], weights[1])):
        x = torch.from_numpy(res["in%d" % i])
        truth = R.conv(x, w, b, torch.float64).numpy()
        bound = R.conv_bound(x, w, b).numpy()
        err = np.abs(res["conv%d" % i].astype(np.float64) - truth)
        print("layer %d (%d -> %d, %dx%d): max err / bound = %.3f" % (i, w.shape[1], w.shape[0], x.shape[3], x.shape[2], (err / bound).max()))
        assert res["conv%d" % i].shape == truth.shape and (err <= bound).all(), "layer %d: %g of the bound" % (i, (err / bound).max())
        if i in RELU_LAYERS:
            assert np.array_equal(res["relu%d" % i], np.maximum(res["conv%d" % i], 0.0))
        assert (truth < 0).any() and (truth > 0).any()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_pooled_maps_equal_the_restatement(size, emulated):
    res = emulated(size)
    W, H = size
    w, h = W, H
    for k in range(4):
        src = torch.from_numpy(res["pool_in%d" % k])
        want = R.pool(src).numpy()
        w, h = w // 2, h // 2
        assert want.shape[2:] == (h, w) and np.array_equal(res["pool%d" % k], want)
    if size == (37, 53):
        assert (w, h) == (2, 3)
    if size == (16, 16):
        assert (w, h) == (1, 1)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_value_is_reproducible_and_close_to_the_truth(size, emulated):
    """bit-identical across two runs and across two workspace fills (0xA5, 0x3C); value = the sum of the taps; and near the fp64
    restatement (1e-4 relative: a sanity bound far above fp32 rounding at these sizes, the sharp comparison is the GPU suite's)"""
    res = emulated(size)
    runs = res["runs"].view(np.uint32)
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    got = res["runs"][0]
    img0, img1, weights = _case(*size)
    truth = R.forward(img0, img1, LAYERS, weights, torch.float64)
    want = np.concatenate([[truth["value"].item()], truth["per_tap"].numpy()])
    print("value %.9g truth %.9g, relative errors %s" % (got[0], want[0], np.abs(got - want) / np.abs(want)))
    assert len(got) == 6 and np.isfinite(got).all() and (want > 1e-4).all()
    assert (np.abs(got - want) <= 1e-4 * np.abs(want)).all()
    s = np.float32(0)
    for v in got[1:]:
        s = np.float32(s + v)
    assert s == got[0]


def test_refusals(tmp_path):
    res = _emulate("errors:all", tmp_path)
    assert "nothing would be left" in str(res["w15"]) and "15 x 16" in str(res["w15"])
    assert "nothing would be left" in str(res["h15"]) and "16 x 15" in str(res["h15"])
    assert "multiple of 32" in str(res["c48"]) and "multiple of 32" in str(res["net48"])
    assert int(res["ws48"]) == 0


def test_host_tensors_and_other_nets_are_refused(monkeypatch, tmp_path):
    import image_metrics as M
    with pytest.raises(RuntimeError, match="ROCm device"):
        M.conv3x3(torch.zeros((1, 3, 8, 8)), torch.zeros((32, 3, 3, 3)), torch.zeros(32))
    with pytest.raises(RuntimeError, match="ROCm device"):
        M.maxpool2(torch.zeros((1, 3, 8, 8)))
    with pytest.raises(NotImplementedError):
        M.LPIPS(net="alex")
    # no weight files: FileNotFoundError at construction, naming every place searched
    monkeypatch.setenv("GOF_LPIPS_VGG16", str(tmp_path / "nowhere" / "vgg16.pth"))
    monkeypatch.delenv("GOF_LPIPS_LIN", raising=False)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    with pytest.raises(FileNotFoundError) as e:
        M.LPIPS(net="vgg")
    text = str(e.value)
    assert str(tmp_path / "nowhere" / "vgg16.pth") in text and "GOF_LPIPS_LIN (not set)" in text
    assert str(tmp_path / "torch_home" / "hub" / "checkpoints" / "vgg16-397923af.pth") in text
    assert str(tmp_path / "torch_home" / "hub" / "checkpoints" / "vgg.pth") in text and "lpips package" in text


def test_size_queries_and_argument_checks():
    import ctypes as C
    import image_metrics as M
    L = M.lib
    desc = (M.GofLpipsLayer * len(M.VGG_LAYERS))(*[M.GofLpipsLayer(*l) for l in M.VGG_LAYERS])
    small, big = L.gof_lpips_workspace_bytes(16, 16, 13, desc), L.gof_lpips_workspace_bytes(1600, 1063, 13, desc)
    assert 0 < small < big and big >= 2 * 2 * 64 * 1600 * 1063 * 4
    assert L.gof_lpips_workspace_bytes(15, 16, 13, desc) == 0 and b"nothing would be left" in L.gof_last_error()
    assert L.gof_lpips_workspace_bytes(16, 16, 0, desc) == 0
    assert L.gof_lpips_conv3x3(1, 3, 48, 8, 8, None, None, None, 1, None, None) < 0 and b"multiple of 32" in L.gof_last_error()
    assert L.gof_lpips_conv3x3(1, 3, 64, 8, 8, None, None, None, 1, None, None) < 0 and b"NULL" in L.gof_last_error()
    assert L.gof_lpips_maxpool2(1, 1, 8, None, None, None) < 0
    assert C.sizeof(M.GofLpipsLayer) == 16
    assert M.VGG_LAYERS == R.vgg_layers() and M.SHIFT == R.SHIFT and M.SCALE == R.SCALE


def test_the_convolution_gives_the_pinned_bits(tmp_path):
    """the SHA-256 of every output of tests/conv3x3_pins.py's LPIPS cases (two images of 17 x 9, C_in 3 / 6 / 8, every tile shape, with and
    without the ReLU) is the one recorded in tests/golden/conv3x3_pins.json: the order of K has not moved"""
    got = P.emulated("lpips", tmp_path)
    assert len(got) == len(P.lpips_cases()) and P.unpinned("lpips", "host", got) == []


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
