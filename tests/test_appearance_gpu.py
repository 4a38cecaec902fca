"""GPU tests of the decoupled-appearance L1: the network at its real widths with seeded random parameters at 32x32,
75x100, 64x45 and 136x200 (H x W; crop 128x192, low-resolution image 4x6), through train_epilogue.appearance and the C ABI, against
tests/appearance_restatement.py (fp64 = the truth, fp32 = the yardstick).  The restatements are computed once per module and only
read.  The piece bounds are those of tests/test_appearance_host.py (derived in its docstring)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import appearance_restatement as R
import conv3x3_pins as P

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (75, 100), (64, 45), (136, 200)]          # (H, W)
DEV = "cuda:0"
U = 2.0 ** -24
X_MODE = ("embed", "shuffle", "shuffle", "shuffle", "shuffle", "up2", "plain")
DY_MODE = ("unshuffle", "unshuffle", "unshuffle", "unshuffle", "plain", "plain", "plain")
NAMES = ["loss", "d_image", "d_embedding"] + ["d_%s.%s" % (n, p) for n in R.PARAM_NAMES for p in ("weight", "bias")]
ids = dict(ids=lambda s: "%dx%d" % s)


@pytest.fixture(scope="module")
def M():
    import train_epilogue.appearance as M
    return M


@pytest.fixture(scope="module")
def reference():
    """per size: the case, its restatement at fp32 and at fp64"""
    out = {}
    for H, W in SIZES:
        image, gt = R.make_images(W, H, seed=500 + W)
        case = (image, gt, R.make_embedding(seed=3 + H), R.make_params(seed=21 + W))
        out[(H, W)] = (case, R.run(*case, torch.float32), R.run(*case, torch.float64))
    return out


def _tensors(ref):
    return [ref["loss"].reshape(1), ref["d_image"], ref["d_embedding"]] + list(ref["d_params"])


def _product(M, case):
    """-> [loss, d_image, d_embedding, 14 parameter gradients] as CPU tensors"""
    image, gt, emb, params = case
    img = image.to(DEV).requires_grad_(True)
    e = emb.to(DEV).requires_grad_(True)
    ps = [p.to(DEV).requires_grad_(True) for p in params]
    loss = M.appearance_l1(img, gt.to(DEV), e, ps)
    loss.backward()
    return [loss.detach().reshape(1).cpu(), img.grad.cpu(), e.grad.cpu()] + [p.grad.cpu() for p in ps]


def _ratio(got, truth, bound):
    return ((got.double().cpu() - truth).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("size", SIZES, **ids)
def test_every_piece_is_within_its_bound_and_the_fused_views_give_the_same_bits(size, M, reference):
    """convolution and data gradient: (K + 2) 2^-24 (sum |w x| + |b|); weight / bias gradient: (L + n_chunks + 2) 2^-24 sum |dY' X|;
    resampling: 5 * 2^-24 of the magnitude, its transpose (n + 2) 2^-24; pixel-shuffle, its inverse, the ReLU mask and the embedding
    planes exact; every fused view bit-equal to the materialised operand"""
    (image, gt, emb, params), ref, _ = reference[size]
    H, W = size
    Hc, Wc, top, left = R.crop_box(H, W)
    worst = {"conv": 0.0, "dgrad": 0.0, "wgrad": 0.0, "resample": 0.0}
    crop = image[:, top:top + Hc, left:left + Wc]
    truth, mag = R.bilinear_truth(crop, (Hc // 32, Wc // 32))
    down = M.bilinear(image.to(DEV)[:, top:top + Hc, left:left + Wc], (Hc // 32, Wc // 32))
    worst["resample"] = max(worst["resample"], _ratio(down, truth, 5 * U * mag))
    truth, mag = R.bilinear_truth(ref["transformed"], (H, W))
    worst["resample"] = max(worst["resample"], _ratio(M.bilinear(ref["transformed"].to(DEV), (H, W)), truth, 5 * U * mag))
    truth, mag, terms = R.bilinear_transpose_truth(ref["d_x"][5], ref["y"][4].shape[1:])
    worst["resample"] = max(worst["resample"], _ratio(M.up2_backward(ref["d_x"][5].to(DEV)), truth, (terms + 2) * U * mag))
    for k in range(7):
        w, b = params[2 * k], params[2 * k + 1]
        x = (ref["down"] if k == 0 else ref["y"][k - 1]).to(DEV)
        dy = (ref["d_x"][k + 1] if DY_MODE[k] == "unshuffle" else ref["d_y"][k]).to(DEV)
        mask = ref["y"][k].to(DEV) if k < 6 else None
        e = emb.to(DEV) if k == 0 else None
        wd, bd = w.to(DEV), b.to(DEV)
        xin = M.materialize(x, X_MODE[k], emb=e)
        if X_MODE[k] == "up2":
            truth, mag = R.bilinear_truth(ref["y"][k - 1], ref["x"][k].shape[1:])
            worst["resample"] = max(worst["resample"], _ratio(xin, truth, 5 * U * mag))
        else:
            assert torch.equal(xin.cpu(), ref["x"][k]), "input view of convolution %d" % k
        dyin = M.materialize(dy, DY_MODE[k], mask=mask)
        assert torch.equal(dyin.cpu(), ref["d_pre"][k]), "gradient view of convolution %d" % k
        wt = M.weight_transpose(wd)
        assert torch.equal(wt.cpu(), R.transposed_weight(w))
        got = M.conv3x3(x, wd, bd, mode=X_MODE[k], emb=e)
        assert torch.equal(got, M.conv3x3(xin, wd, bd)) and torch.equal(M.conv3x3(x, wd, bd, relu=True, mode=X_MODE[k], emb=e), got.clamp_min(0))
        xc = xin.cpu()
        r1 = _ratio(got, F.conv2d(xc.double()[None], w.double(), b.double(), padding=1)[0], R.conv_bound(xc, w, b))
        got_d = M.conv3x3(dy, wt, None, mode=DY_MODE[k], mask=mask)
        assert torch.equal(got_d, M.conv3x3(dyin, wt, None))
        dc, wtc = dyin.cpu(), wt.cpu()
        r2 = _ratio(got_d, F.conv2d(dc.double()[None], wtc.double(), None, padding=1)[0], R.conv_bound(dc, wtc))
        dW, db = M.conv3x3_wgrad(x, dy, mode=X_MODE[k], emb=e, dy_mode=DY_MODE[k], mask=mask)
        dW2, db2 = M.conv3x3_wgrad(xin, dyin)
        assert torch.equal(dW, dW2) and torch.equal(db, db2)
        tW, tb, mW, mb = R.wgrad_truth(xc, dc)
        n_chunks = -(-(xc.shape[1] * xc.shape[2]) // M.WGRAD_CHUNK)
        f = (M.WGRAD_CHUNK + n_chunks + 2) * U
        r3 = max(_ratio(dW, tW, f * mW), _ratio(db, tb, f * mb))
        print("%dx%d convolution %d (%d -> %d, %d chunk(s)): forward %.3f  data gradient %.3f  weight gradient %.4f of the bound" % (H, W, k, w.shape[1], w.shape[0], n_chunks, r1, r2, r3))
        assert r1 <= 1 and r2 <= 1 and r3 <= 1, "convolution %d" % k
        worst["conv"], worst["dgrad"], worst["wgrad"] = max(worst["conv"], r1), max(worst["dgrad"], r2), max(worst["wgrad"], r3)
    print("%dx%d worst ratios: %s" % (H, W, worst))
    assert worst["resample"] <= 1 and all(v > 0 for v in worst.values())


@pytest.mark.parametrize("size", SIZES, **ids)
def test_the_ends_are_within_the_bounds_of_their_formulas(size, M, reference):
    """sigmoid / product / L1, their backward and the image gradient as pieces, on the restatement's fp32 z, sigmoid and d_down: the
    bounds of appearance_restatement.head_truth, head_backward_truth and image_grad_truth"""
    (image, gt, _, _), ref, _ = reference[size]
    img, g = image.to(DEV), gt.to(DEV)
    dL = 0.75
    loss_p, m_p, t_p = M.head_forward(ref["y"][6].to(DEV), img, g)
    (m, t, loss), (bm, bt, bl) = R.head_truth(ref["y"][6], image, gt)
    r = {"m": _ratio(m_p, m, bm), "t": _ratio(t_p, t, bt), "loss": abs(loss_p.item() - loss.item()) / bl.item()}
    dz, bdz = R.head_backward_truth(ref["m"], image, gt, dL)
    r["dz"] = _ratio(M.head_backward(ref["m"].to(DEV), img, g, torch.tensor(dL, device=DEV)), dz, bdz)
    di, bdi = R.image_grad_truth(ref["m"], image, gt, dL, ref["d_down"])
    got = M.image_grad(ref["m"].to(DEV), img, g, torch.tensor(dL, device=DEV), ref["d_down"].to(DEV)).cpu()
    r["d_image"] = _ratio(got, di, bdi)
    print("%dx%d the ends, max err / bound: %s" % (size[0], size[1], r))
    assert all(v <= 1 for v in r.values()) and max(r.values()) > 0 and (got[bdi == 0] == 0).all()


class _Filled:
    """the module's torch with every torch.empty filled with 0xA5"""

    def __getattr__(self, k):
        return getattr(torch, k)

    @staticmethod
    def empty(*a, **k):
        t = torch.empty(*a, **k)
        t.reshape(-1).view(torch.uint8).fill_(0xA5)
        return t


@pytest.mark.parametrize("size", [(75, 100), (136, 200)], **ids)
def test_bit_reproducible_across_runs_a_side_stream_and_buffer_contents(size, M, reference, monkeypatch):
    case = reference[size][0]

    def bits():
        return np.concatenate([t.reshape(-1).numpy() for t in _product(M, case)]).view(np.uint32)
    first, again = bits(), bits()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = bits()
    torch.cuda.current_stream().wait_stream(side)
    monkeypatch.setattr(M, "torch", _Filled())
    filled = bits()
    assert np.array_equal(first, again) and np.array_equal(first, on_side) and np.array_equal(first, filled)


@pytest.mark.parametrize("size", SIZES, **ids)
def test_loss_and_every_gradient_within_four_times_the_fp32_restatement_error(size, M, reference):
    """per tensor (the loss, d image, d embedding, the 14 parameter gradients), relative to the tensor's maximum: e_prod = the product's
    largest error against the fp64 restatement, e_ref = the fp32 torch-CPU restatement's; e_prod <= 4 e_ref and e_ref > 0.

    The measured ratios are in DESIGN.md §5."""
    case, ref32, ref64 = reference[size]
    got = _product(M, case)
    bad = []
    for name, g, r32, r64 in zip(NAMES, got, _tensors(ref32), _tensors(ref64)):
        top = r64.abs().max().item()
        e_prod = (g.double() - r64).abs().max().item() / top
        e_ref = (r32.double() - r64).abs().max().item() / top
        print("%dx%d %-18s e_ref = %.3g   product = %.3g   ratio = %.3f" % (size[0], size[1], name, e_ref, e_prod, e_prod / e_ref if e_ref else float("inf")))
        if not (e_ref > 0 and e_prod <= 4.0 * e_ref):
            bad.append("%s: product %.4g vs 4 x e_ref = %.4g" % (name, e_prod, 4 * e_ref))
    assert tuple(got[1].shape) == tuple(case[0].shape) and not bad, "; ".join(bad)


def test_the_reference_signature_with_a_stand_in_model(M, reference):
    """L1_loss_appearance(image, gt, gaussians, view_idx, return_transformed_image): parameters by the reference's names, the embedding
    through get_apperance_embedding; the loss differentiates into the module's parameters and the embedding table; the transformed
    image comes back resized to the image's size"""
    size = (75, 100)
    (image, gt, emb, params), ref32, ref64 = reference[size]
    ps = [torch.nn.Parameter(p.to(DEV)) for p in params]
    layers = [types.SimpleNamespace(weight=w, bias=b) for w, b in zip(ps[0::2], ps[1::2])]
    net = types.SimpleNamespace(conv1=layers[0], up1=types.SimpleNamespace(conv=layers[1]), up2=types.SimpleNamespace(conv=layers[2]),
                                up3=types.SimpleNamespace(conv=layers[3]), up4=types.SimpleNamespace(conv=layers[4]), conv2=layers[5], conv3=layers[6])
    table = torch.nn.Parameter(torch.stack([torch.zeros_like(emb), emb, torch.ones_like(emb)]).to(DEV))
    asked = []

    class Gaussians:
        appearance_network = net

        def get_apperance_embedding(self, idx):
            asked.append(idx)
            return table[idx]
    rendering = torch.cat([image, torch.zeros((2,) + tuple(image.shape[1:]))]).to(DEV).requires_grad_(True)
    loss = M.L1_loss_appearance(rendering[:3, :, :], gt.to(DEV), Gaussians(), 1)
    assert asked == [1] and loss.dim() == 0 and loss.requires_grad
    (0.8 * loss).backward()
    assert abs(loss.item() - ref64["loss"].item()) <= 1e-5 * ref64["loss"].item()
    assert torch.allclose(rendering.grad[:3].cpu().double(), 0.8 * ref64["d_image"], rtol=0, atol=1e-4 * ref64["d_image"].abs().max().item())
    assert (rendering.grad[3:] == 0).all() and (table.grad[0] == 0).all() and (table.grad[2] == 0).all()
    assert torch.allclose(table.grad[1].cpu().double(), 0.8 * ref64["d_embedding"], rtol=0, atol=1e-4 * ref64["d_embedding"].abs().max().item())
    for p, want in zip(ps, ref64["d_params"]):
        assert torch.allclose(p.grad.cpu().double(), 0.8 * want, rtol=0, atol=1e-4 * want.abs().max().item())
    with torch.no_grad():
        out = M.L1_loss_appearance(rendering[:3, :, :], gt.to(DEV), Gaussians(), 1, return_transformed_image=True)
    want = R.resized(ref64["transformed"], size, torch.float64)
    assert tuple(out.shape) == (3,) + size and not out.requires_grad
    assert torch.allclose(out.cpu().double(), want, rtol=0, atol=2e-5)


def test_the_convolution_and_the_narrow_network_give_the_pinned_bits(M):
    """the SHA-256 of every output of tests/conv3x3_pins.py's appearance cases and of the loss and the 16 gradients of the narrowest
    network at 32 x 32 (conv3's head epilogue) is the one recorded in tests/golden/conv3x3_pins.json"""
    got = P.digests("appearance", DEV, app_module=M)
    assert len(got) == len(P.app_cases()) + 17 and P.unpinned("appearance", "gpu", got) == []


def test_the_lpips_and_the_appearance_convolution_give_the_same_bits(M):
    """gof_lpips_conv3x3 on one image and gof_app_conv3x3 (PLAIN view, no mask, with the bias) are torch.equal for C_out 32, 64, 96 and
    128 (96 runs different tiles in the two units) at C_in 3, 6 and 8 on the 17 x 9 plane"""
    import image_metrics
    assert P.contract_mismatches(DEV, image_metrics, M) == []


def test_refusals_on_the_device(M):
    emb, params = R.make_embedding(1).to(DEV), [p.to(DEV) for p in R.make_params(1)]
    image, gt = R.make_images(40, 31, seed=1)
    with pytest.raises(RuntimeError, match="smaller than 32"):
        M.appearance_l1(image.to(DEV), gt.to(DEV), emb, params)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        M.conv3x3(torch.zeros((6, 4, 4), device=DEV), torch.zeros((8, 1, 3, 3), device=DEV), mode="shuffle")
