"""The decoupled-appearance L1 restated in torch on the CPU, in this project's own words: train.py:67-88 and
scene/appearance_network.py -- centre crop to multiples of 32, bilinear down-sample by 32 (align_corners=True), the embedding as 64
constant planes, conv1, four (pixel-shuffle, conv, ReLU) blocks, a bilinear x2 up-sample, conv2, ReLU, conv3, sigmoid, the product with
the cropped image, the mean absolute difference to the cropped ground truth.  Built from F.conv2d, F.pixel_shuffle and F.interpolate;
gradients by torch autograd.  Run at torch.float64 it is the truth, at torch.float32 the yardstick (what an fp32 framework computes).
Networks are data: (n_embed, the six widths), seeded random parameters."""
import torch
import torch.nn.functional as F

import lpips_restatement as LR

N_EMBED = 64
WIDTHS = (256, 128, 64, 32, 16, 16)             # conv1, up1.conv .. up4.conv, conv2 (conv3 gives 3): scene/appearance_network.py
PARAM_NAMES = ("conv1", "up1.conv", "up2.conv", "up3.conv", "up4.conv", "conv2", "conv3")


def channels(widths=WIDTHS, n_embed=N_EMBED):
    """(c_in, c_out) of the seven convolutions"""
    c_in = [3 + n_embed] + [w // 4 for w in widths[:4]] + [widths[4], widths[5]]
    return list(zip(c_in, list(widths) + [3]))


def make_params(seed, widths=WIDTHS, n_embed=N_EMBED):
    """the 14 parameter tensors (weight, bias per convolution, in PARAM_NAMES order): weights ~ N(0, 2 / (9 C_in)), small biases; fp32"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for ci, co in channels(widths, n_embed):
        out.append((torch.randn((co, ci, 3, 3), generator=g, dtype=torch.float64) * (2.0 / (9 * ci)) ** 0.5).float())
        out.append((0.05 * torch.randn((co,), generator=g, dtype=torch.float64)).float())
    return out


def make_embedding(seed, n_embed=N_EMBED):
    """~ N(0, 1e-4) as scene/gaussian_model.py:115-116 initialises it"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((n_embed,), generator=g, dtype=torch.float64) * 1e-4).float()


def make_images(W, H, seed):
    """(image, ground truth), (3,H,W) fp32 in [0,1]"""
    a, b = LR.make_images(W, H, seed)
    return a[0], b[0]


def crop_box(H, W):
    """train.py:70-74 -> (Hc, Wc, top, left)"""
    Hc, Wc = H // 32 * 32, W // 32 * 32
    return Hc, Wc, H // 2 - Hc // 2, W // 2 - Wc // 2


def run(image, gt, embedding, params, dtype, grads=True):
    """-> dict: loss, transformed (3,Hc,Wc), down (3,h,w), x[k] (the input of convolution k as a (C,H,W) tensor: what the views give),
    pre[k] (its output before the ReLU), y[k] (after), m (the sigmoid); with grads=True also d_image, d_embedding, d_params[14] and
    d_x[k], d_pre[k], d_y[k], d_down, d_m (the gradients of the loss with respect to those intermediates).  All at `dtype`, detached."""
    image = image.to(dtype).clone().requires_grad_(grads)
    emb = embedding.to(dtype).clone().requires_grad_(grads)
    ps = [p.to(dtype).clone().requires_grad_(grads) for p in params]
    gt = gt.to(dtype)
    Hc, Wc, top, left = crop_box(*image.shape[1:])
    ci, cg = image[:, top:top + Hc, left:left + Wc], gt[:, top:top + Hc, left:left + Wc]
    down = F.interpolate(ci[None], size=(Hc // 32, Wc // 32), mode="bilinear", align_corners=True)[0]
    x = torch.cat([down, emb[None].repeat(Hc // 32, Wc // 32, 1).permute(2, 0, 1)], dim=0)[None]
    xs, pre, ys = [], [], []
    for k in range(7):
        if 1 <= k <= 4:
            x = F.pixel_shuffle(x, 2)
        elif k == 5:
            x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        xs.append(x)
        y = F.conv2d(x, ps[2 * k], ps[2 * k + 1], padding=1)
        pre.append(y)
        x = torch.relu(y) if k < 6 else y
        ys.append(x)
    m = torch.sigmoid(ys[6])
    t = m[0] * ci
    loss = (t - cg).abs().mean()
    keep = [down, m] + xs + pre + ys
    if grads:
        for v in keep:
            v.retain_grad()
        loss.backward()
    out = {"loss": loss.detach(), "transformed": t.detach(), "down": down.detach(), "m": m.detach()[0],
           "x": [v.detach()[0] for v in xs], "pre": [v.detach()[0] for v in pre], "y": [v.detach()[0] for v in ys]}
    if grads:
        out.update({"d_image": image.grad, "d_embedding": emb.grad, "d_params": [p.grad for p in ps], "d_down": down.grad, "d_m": m.grad[0],
                    "d_x": [v.grad[0] for v in xs], "d_pre": [v.grad[0] for v in pre], "d_y": [v.grad[0] for v in ys]})
    return out


def resized(transformed, size, dtype):
    """train.py:87"""
    return F.interpolate(transformed.to(dtype)[None], size=size, mode="bilinear", align_corners=True)[0]


def bilinear_matrix(n_in, n_out):
    """one axis of the align_corners=True resampling with the WEIGHTS AS THE CONTRACT FORMS THEM IN fp32 (scale = (in - 1) / (out - 1) or
    0, s = scale * dst, i0 = (int)s, l1 = s - i0, l0 = 1 - l1; every step rounded to fp32) -> (A (n_out, n_in) fp64 with A[dst, i0] +=
    l0, A[dst, i1] += l1; cnt (n_in,): how many (dst, corner) pairs name each source index)"""
    import numpy as np
    f = np.float32
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    A, cnt = np.zeros((n_out, n_in)), np.zeros(n_in, dtype=np.int64)
    for d in range(n_out):
        s = f(scale * f(d))
        i0 = min(int(s), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = f(s - f(i0))
        l0 = f(f(1) - l1)
        A[d, i0] += float(l0)
        A[d, i1] += float(l1)
        cnt[i0] += 1
        cnt[i1] += 1
    return torch.from_numpy(A), torch.from_numpy(cnt)


def bilinear_truth(x, size):
    """x (C,H,W) -> (value, magnitude) at fp64 of the resampling to `size` with the contract's fp32 weights: value = A_h x A_w^T"""
    Ah, _ = bilinear_matrix(x.shape[1], size[0])
    Aw, _ = bilinear_matrix(x.shape[2], size[1])
    x = x.double()
    return Ah @ x @ Aw.T, Ah @ x.abs() @ Aw.T


def bilinear_transpose_truth(g, size):
    """g (C,Ho,Wo): a gradient on the destination -> (value, magnitude, terms) on a source of `size`: A_h^T g A_w; terms (H,W) = the
    number of additions a source pixel's sum has"""
    Ah, ch = bilinear_matrix(size[0], g.shape[1])
    Aw, cw = bilinear_matrix(size[1], g.shape[2])
    g = g.double()
    return Ah.T @ g @ Aw, Ah.T @ g.abs() @ Aw, (ch[:, None] * cw[None, :]).double()


def conv_bound(x, w, b=None):
    """(K + 2) 2^-24 (sum |w x| + |b|), K = 9 C_in, for an input x (C,H,W): lpips_restatement.conv_bound for one image"""
    bias = b if b is not None else torch.zeros(w.shape[0])
    return LR.conv_bound(x[None], w, bias)[0]


def transposed_weight(w):
    """W'[ci][co][ky][kx] = W[co][ci][2 - ky][2 - kx]: the weight of the data gradient"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def wgrad_truth(x, dy):
    """fp64 (dW, db, magnitude of dW, magnitude of db) of a 3x3 convolution from its input x (C_in,H,W) and the (masked) gradient of its
    output dy (C_out,H,W); magnitude = sum_p |dy x|"""
    x, dy = x.double(), dy.double()
    cols = F.unfold(x[None], 3, padding=1)[0]                      # (C_in * 9, H W), row = ci * 9 + ky * 3 + kx
    flat = dy.reshape(dy.shape[0], -1)
    shape = (dy.shape[0], x.shape[0], 3, 3)
    return (flat @ cols.T).reshape(shape), flat.sum(1), (flat.abs() @ cols.abs().T).reshape(shape), flat.abs().sum(1)


U = 2.0 ** -24


def _crops(image, gt):
    Hc, Wc, top, left = crop_box(*image.shape[1:])
    return image[:, top:top + Hc, left:left + Wc], gt[:, top:top + Hc, left:left + Wc]


def head_truth(z, image, gt):
    """z (3,Hc,Wc) fp32 -> fp64 (m, t, loss) and their bounds.  m = 1 / (1 + exp(-z)): the exponential (1 ulp = 2 units of 2^-24, scaled
    by e / (1 + e) <= 1), the addition and the division: 4 roundings, 5 units with the second-order terms; t = m I one more: 6 units of
    |t|; |t - G| one more on its own magnitude, the fp64 sum adds nothing, the division and the rounding of the mean two on the loss:
    2^-24 (6 mean|t| + 3 loss)."""
    I, G = (v.double() for v in _crops(image, gt))
    m = torch.sigmoid(z.double())
    t = m * I
    loss = (t - G).abs().mean()
    return (m, t, loss), (5 * U * m, 6 * U * t.abs(), U * (6 * t.abs().mean() + 3 * loss))


def _sign_and_scale(m, image, gt, dL):
    """the sign as the contract forms it (fp32 product, fp32 difference) and k = dL / (3 Hc Wc) at fp64"""
    I, G = _crops(image, gt)
    return torch.sign(m.float() * I - G).double(), float(dL) / m.numel()


def head_backward_truth(m, image, gt, dL):
    """m (3,Hc,Wc) fp32 (the saved sigmoid) -> fp64 dz = ((g I) m) (1 - m), g = sign(m I - G) dL / (3 Hc Wc), and its bound: the division,
    three products and the difference 1 - m are 5 roundings: 6 units of |dz|"""
    I, _ = _crops(image, gt)
    s, k = _sign_and_scale(m, image, gt, dL)
    dz = s * k * I.double() * m.double() * (1 - m.double())
    return dz, 6 * U * dz.abs()


def image_grad_truth(m, image, gt, dL, d_down):
    """-> fp64 d_image (3,H,W) and its bound: g m (the division and the product: 2 roundings) is the start of the gather's sum, whose
    terms (lh lw) d are 2 roundings each and pass through at most n additions: (n + 4) 2^-24 (|g m| + the gather's magnitude) inside the
    crop, exactly 0 outside"""
    H, W = image.shape[1:]
    Hc, Wc, top, left = crop_box(H, W)
    s, k = _sign_and_scale(m, image, gt, dL)
    gm = s * k * m.double()
    val, mag, terms = bilinear_transpose_truth(d_down, (Hc, Wc))
    out, bound = torch.zeros((3, H, W), dtype=torch.float64), torch.zeros((3, H, W), dtype=torch.float64)
    out[:, top:top + Hc, left:left + Wc] = gm + val
    bound[:, top:top + Hc, left:left + Wc] = (terms + 4) * U * (gm.abs() + mag)
    return out, bound
