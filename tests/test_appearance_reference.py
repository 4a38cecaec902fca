"""CPU-only: tests/appearance_restatement.py -- the yardstick of every appearance test -- held to the reference itself.  Runs where
oracle/_ref/refpy exists (the byte-identical copies __graft_entry__.build() stages): `AppearanceNetwork` is taken from the staged
scene/appearance_network.py, the source of `L1_loss_appearance` out of the staged train.py by `ast` (given `torch` and an `l1_loss`),
both run at fp64 on the restatement's inputs; loss, transformed image and every gradient must agree to 1e-12 relative."""
import ast
import importlib.util
import os

import pytest
import torch

import appearance_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFPY = os.path.join(ROOT, "oracle", "_ref", "refpy")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REFPY, "scene", "appearance_network.py")),
                                reason="oracle/_ref/refpy not staged (build() stages it where the reference exists)")
SIZES = [(32, 32), (75, 100), (64, 45), (136, 200)]          # (H, W): the sizes of the host and GPU suites


def _reference():
    """(AppearanceNetwork of the staged module, L1_loss_appearance compiled from the staged train.py's own source)"""
    spec = importlib.util.spec_from_file_location("staged_appearance_network", os.path.join(REFPY, "scene", "appearance_network.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = os.path.join(REFPY, "train.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "L1_loss_appearance"]
    assert len(fn) == 1
    ns = {"torch": torch, "l1_loss": lambda a, b: torch.abs(a - b).mean()}        # utils/loss_utils.py:17-18
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return mod.AppearanceNetwork, ns["L1_loss_appearance"]


class _Gaussians:
    def __init__(self, network, table):
        self.appearance_network, self.table = network, table

    def get_apperance_embedding(self, idx):              # scene/gaussian_model.py's spelling
        return self.table[idx]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_restatement_is_the_references_function_at_fp64(size):
    H, W = size
    AppearanceNetwork, L1_loss_appearance = _reference()
    image, gt = R.make_images(W, H, seed=700 + W)
    emb, params = R.make_embedding(seed=H), R.make_params(seed=W)
    net = AppearanceNetwork(3 + R.N_EMBED, 3).double()
    with torch.no_grad():
        for name, w, b in zip(R.PARAM_NAMES, params[0::2], params[1::2]):
            m = net
            for part in name.split("."):
                m = getattr(m, part)
            assert m.weight.shape == w.shape and m.bias.shape == b.shape, name
            m.weight.copy_(w.double())
            m.bias.copy_(b.double())
    table = torch.stack([torch.zeros_like(emb), emb]).double().requires_grad_(True)
    img = image.double().requires_grad_(True)
    g = _Gaussians(net, table)
    loss = L1_loss_appearance(img, gt.double(), g, 1)
    loss.backward()
    ours = R.run(image, gt, emb, params, torch.float64)

    def same(a, b, what):
        scale = b.abs().max().item()
        assert a.shape == b.shape and scale > 0 and (a - b).abs().max().item() <= 1e-12 * scale, what
    same(loss.detach(), ours["loss"], "loss")
    same(img.grad, ours["d_image"], "d image")
    same(table.grad[1], ours["d_embedding"], "d embedding")
    assert (table.grad[0] == 0).all()
    for name, w_ref, b_ref in zip(R.PARAM_NAMES, ours["d_params"][0::2], ours["d_params"][1::2]):
        m = net
        for part in name.split("."):
            m = getattr(m, part)
        same(m.weight.grad, w_ref, name + ".weight")
        same(m.bias.grad, b_ref, name + ".bias")
    with torch.no_grad():
        out = L1_loss_appearance(img, gt.double(), g, 1, return_transformed_image=True)
    same(out, R.resized(ours["transformed"], (H, W), torch.float64), "transformed image, resized")
    assert R.crop_box(75, 100) == (64, 96, 5, 2)
