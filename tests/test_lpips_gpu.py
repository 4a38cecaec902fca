"""GPU tests of the LPIPS metric: the full-width VGG instance with seeded random weights at 16x16, 37x53 and 64x48,
N = 1 and N = 2, through image_metrics and the C ABI, against tests/lpips_restatement.py (fp64 = the truth, fp32 = the yardstick).
The restatements are computed once per module and only read."""
import os
import sys

import numpy as np
import pytest
import torch

import lpips_restatement as R
import conv3x3_pins as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIMS = os.path.join(ROOT, "gaussian-opacity-fields_amd", "shims")
SIZES = [(16, 16), (37, 53), (64, 48)]
LAYERS = R.vgg_layers()
DEV = "cuda:0"


@pytest.fixture(scope="module")
def net():
    import image_metrics as M
    weights = R.make_weights(LAYERS, seed=11)
    on_dev = tuple([t.to(DEV) for t in group] for group in weights)
    return M, weights, on_dev


@pytest.fixture(scope="module")
def reference(net):
    """per size: the two image pairs and, per pair, the restatement at fp64 and fp32 as [value, tap 0 .. tap 4]"""
    _, weights, _ = net
    out = {}
    for W, H in SIZES:
        a, b = R.make_images(W, H, seed=40 + W, n=2)
        rows = []
        for i in range(2):
            f64 = R.forward(a[i], b[i], LAYERS, weights, torch.float64)
            f32 = R.forward(a[i], b[i], LAYERS, weights, torch.float32)
            rows.append({"f64": np.concatenate([[f64["value"].item()], f64["per_tap"].numpy()]),
                         "f32": np.concatenate([[f32["value"].item()], f32["per_tap"].numpy()]).astype(np.float64),
                         "layer_in": f32["layer_in"] if i == 0 else None, "pre_relu": f32["pre_relu"] if i == 0 else None})
        out[(W, H)] = (a, b, rows)
    return out


def _product(M, on_dev, a, b, i):
    v, taps = M.network_distance(a[i].to(DEV), b[i].to(DEV), LAYERS, *on_dev)
    return np.concatenate([v.reshape(1).cpu().numpy(), taps.cpu().numpy()])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_every_conv_layer_is_within_the_bound_of_a_k_term_chain(size, net, reference):
    """through the C ABI (gof_lpips_conv3x3 / gof_lpips_maxpool2), on the restatement's fp32 inputs, before the ReLU:
    |out - fp64| <= (K + 2) 2^-24 (sum |w x| + |b|); the pooled maps are equal"""
    M, weights, on_dev = net
    _, _, rows = reference[size]
    worst = 0.0
    for i, (x, w, b) in enumerate(zip(rows[0]["layer_in"], weights[0], weights[1])):
        got = M.conv3x3(x.to(DEV), on_dev[0][i], on_dev[1][i], relu=False).cpu()
        truth = R.conv(x, w, b, torch.float64)
        ratio = ((got.double() - truth).abs() / R.conv_bound(x, w, b)).max().item()
        worst = max(worst, ratio)
        print("%dx%d layer %d (K = %d): max err / bound = %.4f" % (size[0], size[1], i, 9 * w.shape[1], ratio))
        assert got.shape == truth.shape and ratio <= 1.0, "layer %d" % i
        if LAYERS[i][2]:
            src = torch.relu(rows[0]["pre_relu"][i - 1])
            assert torch.equal(M.maxpool2(src.to(DEV)).cpu(), R.pool(src)) and torch.equal(R.pool(src), x)
    assert worst > 0.0


def test_value_and_taps_within_four_times_the_fp32_restatement_error(net, reference):
    """relative error against the fp64 restatement of the value and the per-tap values over all sizes and N = 1, 2; e_ref = the
    largest relative error of the fp32 torch-CPU restatement over the same cases; the product must stay within 4 e_ref.
    Measured on MI355X: see DESIGN.md §4."""
    M, _, on_dev = net
    e_ref = e_prod = 0.0
    for size in SIZES:
        a, b, rows = reference[size]
        for n in (1, 2):
            for i in range(n):
                got = _product(M, on_dev, a, b, i)
                truth = rows[i]["f64"]
                ep = np.abs(got - truth) / np.abs(truth)
                er = np.abs(rows[i]["f32"] - truth) / np.abs(truth)
                print("%dx%d N=%d pair %d: value %.9g truth %.9g | product rel err %s | fp32 restatement rel err %s" % (size[0], size[1], n, i, got[0], truth[0], ep, er))
                e_prod, e_ref = max(e_prod, ep.max()), max(e_ref, er.max())
    print("e_ref = %.4g   product = %.4g   ratio = %.3f" % (e_ref, e_prod, e_prod / e_ref))
    assert e_ref > 0 and e_prod <= 4.0 * e_ref, "product %.4g vs 4 x e_ref = %.4g" % (e_prod, 4 * e_ref)


class _Filled:
    """image_metrics' torch with every torch.empty filled with 0xA5"""

    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def empty(*a, **k):
        t = torch.empty(*a, **k)
        t.reshape(-1).view(torch.uint8).fill_(0xA5)
        return t


@pytest.mark.parametrize("size", [(37, 53), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_bit_reproducible_across_runs_a_side_stream_and_workspace_contents(size, net, reference, monkeypatch):
    M, _, on_dev = net
    a, b, _ = reference[size]
    first = _product(M, on_dev, a, b, 0).astype(np.float32).view(np.uint32)
    again = _product(M, on_dev, a, b, 0).astype(np.float32).view(np.uint32)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _product(M, on_dev, a, b, 0).astype(np.float32).view(np.uint32)
    torch.cuda.current_stream().wait_stream(side)
    monkeypatch.setattr(M, "torch", _Filled())
    filled = _product(M, on_dev, a, b, 0).astype(np.float32).view(np.uint32)
    assert np.array_equal(first, again) and np.array_equal(first, on_side) and np.array_equal(first, filled)


@pytest.fixture
def stand_ins():
    """`torchvision` and `lpips` resolved to the stand-ins of shims/ (in front of an installed package for the length of the test)"""
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("torchvision", "lpips")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, SHIMS)
    try:
        import torchvision
        import torchvision.transforms.functional as tf
        import lpips
        assert os.path.abspath(torchvision.__file__).startswith(SHIMS) and os.path.abspath(lpips.__file__).startswith(SHIMS)
        yield torchvision, tf, lpips
    finally:
        sys.path.remove(SHIMS)
        for k in [k for k in sys.modules if k.split(".")[0] in ("torchvision", "lpips")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_the_lines_of_metrics_py_restated(net, reference, stand_ins, tmp_path, monkeypatch):
    """render.py:35-36 and metrics.py:30-34,76,100: save_image -> PNG -> PIL -> to_tensor -> lpips.LPIPS(net='vgg').to(device) -> a
    call, with weight files in the two real key layouts; against the restatement on the quantised images"""
    from PIL import Image
    M, weights, _ = net
    torchvision, tf, lpips = stand_ins
    a, b, _ = reference[(64, 48)]
    tensors = []
    for name, img in (("render.png", a[0]), ("gt.png", b[0])):
        torchvision.utils.save_image(img.to(DEV), str(tmp_path / name))
        pic = Image.open(str(tmp_path / name))
        assert np.array_equal(np.asarray(pic), R.save_image_bytes(img))
        t = tf.to_tensor(pic)
        assert t.dtype == torch.float32 and torch.equal(t, torch.from_numpy(R.save_image_bytes(img).transpose(2, 0, 1).copy()).float() / 255)
        tensors.append(t.unsqueeze(0)[:, :3, :, :].to(DEV))
    vgg = {}
    for idx, w, bias in zip(M.VGG_FEATURE_INDICES, weights[0], weights[1]):
        vgg["features.%d.weight" % idx], vgg["features.%d.bias" % idx] = w, bias
    lin = {"lin%d.model.1.weight" % k: w.view(1, -1, 1, 1) for k, w in enumerate(weights[2])}
    torch.save(vgg, str(tmp_path / "vgg16.pth"))
    torch.save(lin, str(tmp_path / "lin.pth"))
    monkeypatch.setenv("GOF_LPIPS_VGG16", str(tmp_path / "vgg16.pth"))
    monkeypatch.setenv("GOF_LPIPS_LIN", str(tmp_path / "lin.pth"))
    device = torch.device(DEV)
    lpips_fn = lpips.LPIPS(net='vgg').to(device)
    got = lpips_fn(tensors[0], tensors[1]).detach()
    assert tuple(got.shape) == (1, 1, 1, 1) and got.device.type == "cuda"
    truth = R.forward(tensors[0][0].cpu(), tensors[1][0].cpu(), LAYERS, weights, torch.float64)["value"].item()
    f32 = R.forward(tensors[0][0].cpu(), tensors[1][0].cpu(), LAYERS, weights, torch.float32)["value"].item()
    e_prod, e_ref = abs(got.item() - truth) / truth, abs(f32 - truth) / truth
    print("metrics.py lines: product %.9g truth %.9g rel err %.3g (fp32 restatement %.3g)" % (got.item(), truth, e_prod, e_ref))
    # this test is about the wiring (PNG bytes, channel order, scaling, weight keys): 1e-4 is far above fp32 rounding (chains of at most
    # 4608 terms through 13 layers: ~1e-6, the sharp bound is the test above) and far below what any wiring mistake changes (percents)
    assert e_prod <= 1e-4
    two = lpips_fn(torch.cat(tensors), torch.cat(tensors[::-1]))
    assert tuple(two.shape) == (2, 1, 1, 1) and two[0].item() == got.item()
    # a missing weight file: FileNotFoundError at construction, with the paths searched
    monkeypatch.setenv("GOF_LPIPS_LIN", str(tmp_path / "absent.pth"))
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    with pytest.raises(FileNotFoundError) as e:
        lpips.LPIPS(net='vgg')
    assert str(tmp_path / "absent.pth") in str(e.value) and str(tmp_path / "torch_home" / "hub" / "checkpoints" / "vgg.pth") in str(e.value)
    with pytest.raises(NotImplementedError):
        lpips.LPIPS(net='alex')


def test_the_convolution_gives_the_pinned_bits(net):
    """the SHA-256 of every output of tests/conv3x3_pins.py's LPIPS cases is the one recorded in tests/golden/conv3x3_pins.json"""
    got = P.digests("lpips", DEV, lpips_module=net[0])
    assert len(got) == len(P.lpips_cases()) and P.unpinned("lpips", "gpu", got) == []


def test_refusals_on_the_device(net):
    M, _, on_dev = net
    a, b = R.make_images(15, 16, seed=1)
    with pytest.raises(RuntimeError, match="nothing would be left"):
        M.network_distance(a[0].to(DEV), b[0].to(DEV), LAYERS, *on_dev)
    a, b = R.make_images(16, 15, seed=1)
    with pytest.raises(RuntimeError, match="nothing would be left"):
        M.network_distance(a[0].to(DEV), b[0].to(DEV), LAYERS, *on_dev)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        M.conv3x3(torch.zeros((1, 8, 8, 8), device=DEV), torch.zeros((48, 8, 3, 3), device=DEV), torch.zeros(48, device=DEV))
