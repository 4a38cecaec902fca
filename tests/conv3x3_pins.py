"""The pinned bits of the 3x3 convolution that the LPIPS metric and the appearance network share (csrc/conv3x3_f32.h, DESIGN.md §3.12,
§3.13): fixed inputs made by integer arithmetic alone (no library generator: the bits do not depend on a torch or numpy version), run
through the two product modules, and the SHA-256 of every output's raw bytes held against tests/golden/conv3x3_pins.json.  The order
of K is a written contract (k = ci * 9 + ky * 3 + kx, one fmaf per term, an odd K padded with 0 * 0), so any change of these digests
is a change of that contract.

The cases are the smallest shapes at which the kernel can go wrong: a plane of 17 x 9 pixels (M = 153: a ragged last tile of the 128-
and of the 256-pixel tiling, every border pattern of the taps; LPIPS with two images, M = 306: an image boundary inside a tile; 18 x 10
where a view needs even sizes), C_in = 3 (K = 27, odd: the pad term), 6 (a short second chunk) and 8 (two full chunks), and every
tile instantiation of each unit with full and with partly filled weight tiles.

Used by tests/test_{lpips,appearance}_{host,gpu}.py.  As a program:

    python tests/conv3x3_pins.py <unit> <out.npz>          the child process of the host tests (the emulated library, host seams)
    python tests/conv3x3_pins.py record <host|gpu> <out.json>      the digests of this build, for a deliberate change of the contract
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv3x3_pins.json")
H, W = 17, 9
C_INS = (3, 6, 8)
LPIPS_C_OUTS = (32, 64, 128)                # <1,1>, <2,1>, <2,2>
APP_C_OUTS = (3, 16, 40, 96, 128)           # partly filled <1,1> twice, <2,1> and <2,2> with zero rows, a full <2,2>
CONTRACT_C_OUTS = (32, 64, 96, 128)         # 96: <1,1> in the LPIPS unit, <2,2> with zero rows in the appearance unit
VIEWS = ("plain", "shuffle", "unshuffle", "up2", "embed")
# (bias, relu, mask)
VARIANTS = ((True, False, False), (False, False, True), (True, True, True), (False, True, False))
NARROW_WIDTHS = (4, 4, 4, 4, 1, 1)          # the narrowest network the plan accepts (the four in front of a pixel-shuffle: multiples of 4)
_M32 = np.uint64(0xFFFFFFFF)


def _hash(n, seed):
    """n 32-bit words, a function of (index, seed) in integer arithmetic alone"""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503) + np.uint64(12345)) & _M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & _M32
    h ^= h >> np.uint64(16)
    return h


def values(shape, seed, frac_bits=8, big=True):
    """fp32 tensor of signed 12-bit integers / 2^frac_bits (dyadic: exact in fp32), one in 32 of them times 1024 if `big`: products of
    24 bits and sums over magnitudes 2^10 apart, so that the chains round and their order shows in the bits"""
    n = int(np.prod(shape))
    h = _hash(n, seed)
    v = (((h >> np.uint64(8)) & np.uint64(0xFFF)).astype(np.int64) - 2048).astype(np.float64) / float(1 << frac_bits)
    if big:
        v = np.where((h & np.uint64(31)) == 0, v * 1024.0, v)
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def unit_values(shape, seed):
    """fp32 tensor of 12-bit integers / 4096: image values in [0, 1)"""
    h = _hash(int(np.prod(shape)), seed)
    return torch.from_numpy((((h >> np.uint64(8)) & np.uint64(0xFFF)).astype(np.float64) / 4096.0).astype(np.float32).reshape(shape))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def lpips_cases():
    """-> (name, c_in, c_out, relu)"""
    return [("lpips ci%d co%d relu%d" % (ci, co, relu), ci, co, relu) for ci in C_INS for co in LPIPS_C_OUTS for relu in (0, 1)]


def lpips_operands(ci, co, n_img=2):
    return values((n_img, ci, H, W), 1000 + ci), values((co, ci, 3, 3), 2000 + 10 * co + ci), values((co,), 3000 + co)


def app_cases():
    """-> (name, view, c_in, c_out, bias, relu, mask)"""
    out = []
    for view in VIEWS:
        for ci in C_INS:
            if (view == "unshuffle" and ci % 4) or (view == "embed" and ci <= 3):
                continue
            for co in APP_C_OUTS:
                for bias, relu, mask in VARIANTS:
                    out.append(("app %s ci%d co%d bias%d relu%d mask%d" % (view, ci, co, bias, relu, mask), view, ci, co, bias, relu, mask))
    return out


def app_operands(view, ci, co):
    """-> (stored x, embedding or None, mask (c_in, h, w), weight, bias): the view is (c_in, h, w), h x w = 17 x 9 or 18 x 10"""
    h, w = (H + 1, W + 1) if view in ("shuffle", "up2") else (H, W)
    stored = {"plain": (ci, h, w), "shuffle": (4 * ci, h // 2, w // 2), "unshuffle": (ci // 4, 2 * h, 2 * w), "up2": (ci, h // 2, w // 2),
              "embed": (3, h, w)}[view]
    seed = 100 * VIEWS.index(view) + ci
    emb = values((ci - 3,), 4000 + seed) if view == "embed" else None
    return values(stored, 5000 + seed), emb, values((ci, h, w), 6000 + seed, big=False), values((co, ci, 3, 3), 2000 + 10 * co + ci), values((co,), 3000 + co)


def narrow_network():
    """-> (image, gt (3, 32, 32), embedding (1,), the 14 parameters): the whole forward + backward, whose conv3 runs the head epilogue"""
    widths = list(NARROW_WIDTHS) + [3]
    c_in = [3 + 1] + [v // 4 for v in widths[:4]] + [widths[4], widths[5]]
    params = []
    for k, (ci, co) in enumerate(zip(c_in, widths)):
        params += [values((co, ci, 3, 3), 7000 + k, frac_bits=11, big=False), values((co,), 7100 + k, frac_bits=13, big=False)]
    return unit_values((3, 32, 32), 7200), unit_values((3, 32, 32), 7201), values((1,), 7202, frac_bits=11, big=False), params


def digests(unit, dev, lpips_module=None, app_module=None):
    """{case: sha256 of the output's bytes} of `unit` ("lpips" or "appearance") through the product modules, tensors on `dev`"""
    out = {}
    if unit == "lpips":
        M = lpips_module
        for name, ci, co, relu in lpips_cases():
            x, w, b = (t.to(dev) for t in lpips_operands(ci, co))
            out[name] = sha(M.conv3x3(x, w, b, relu=bool(relu)))
    elif unit == "appearance":
        A = app_module
        for name, view, ci, co, bias, relu, mask in app_cases():
            x, emb, m, w, b = (t.to(dev) if t is not None else None for t in app_operands(view, ci, co))
            out[name] = sha(A.conv3x3(x, w, b if bias else None, relu=bool(relu), mode=view, emb=emb, mask=m if mask else None))
        image, gt, emb, params = narrow_network()
        img = image.to(dev).requires_grad_(True)
        e = emb.to(dev).requires_grad_(True)
        ps = [p.to(dev).requires_grad_(True) for p in params]
        loss = A.appearance_l1(img, gt.to(dev), e, ps)
        loss.backward()
        outs = [("loss", loss), ("d_image", img.grad), ("d_embedding", e.grad)] + [("d_param%d" % i, p.grad) for i, p in enumerate(ps)]
        for name, t in outs:
            assert bool((t != 0).any()), "the narrow network gives an all-zero %s: it pins nothing" % name
            out["app network %s" % name] = sha(t)
    else:
        raise KeyError(unit)
    return out


def contract_mismatches(dev, lpips_module, app_module):
    """gof_lpips_conv3x3 on one image and gof_app_conv3x3 through the PLAIN view, no mask, with the bias: the cases whose outputs
    are not torch.equal (the two units choose different tiles for C_out = 96; the order of K is the same in every tile)"""
    bad = []
    for ci in C_INS:
        for co in CONTRACT_C_OUTS:
            for relu in (False, True):
                x, w, b = (t.to(dev) for t in lpips_operands(ci, co, n_img=1))
                a = lpips_module.conv3x3(x, w, b, relu=relu)[0]
                c = app_module.conv3x3(x[0], w, b, relu=relu)
                if not (a.shape == c.shape and torch.equal(a, c) and bool((a != 0).any())):
                    bad.append("ci%d co%d relu%d" % (ci, co, relu))
    return bad


def pinned(where):
    """{case: digest} of the golden file for `where` ("host": the emulated library, "gpu"); an entry is one digest, or one per place
    where the two differ"""
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    return {k: (v if isinstance(v, str) else v[where]) for k, v in cases.items()}


def unpinned(unit, where, got):
    """the cases of `unit` whose digest is not the pinned one (and the pinned cases that were not run)"""
    want = {k: v for k, v in pinned(where).items() if k.startswith("lpips " if unit == "lpips" else "app ")}
    return sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))


def _modules(host):
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import host_child          # (puts the package on sys.path)
    if host:
        os.environ.setdefault("GOF_HIP_LIB", host_child.emulated_library())      # (a child of the host tests has it set)
    import image_metrics as M
    import train_epilogue.appearance as A
    check = host_child.install_seams(M, A, buffers="all") if host else (lambda: 1)
    return M, A, check


def _child(unit, out):
    M, A, check = _modules(host=True)
    if unit == "contract":
        res = {"bad": np.array(json.dumps(contract_mismatches("cpu", M, A)))}
    else:
        res = {"digests": np.array(json.dumps(digests(unit, "cpu", M, A)))}
    res["buffers"] = np.array(check())
    np.savez(out, **res)


def emulated(unit, tmp_path):
    """the child's result for `unit` ("lpips", "appearance": the digests; "contract": the mismatches) over the emulated library"""
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import host_child
    res = host_child.run_child(__file__, unit, tmp_path, timeout=1800)
    assert int(res["buffers"]) > 0
    return json.loads(str(res["bad" if unit == "contract" else "digests"]))


if __name__ == "__main__":
    if sys.argv[1] == "record":
        where = sys.argv[2]
        M, A, _ = _modules(host=where == "host")
        dev = "cpu" if where == "host" else "cuda:0"
        got = dict(digests("lpips", dev, M, A), **digests("appearance", dev, M, A))
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
        with open(sys.argv[3], "w") as f:
            json.dump({"cases": got}, f, indent=0, sort_keys=True)
        print("%d cases recorded (%s)" % (len(got), where))
    else:
        _child(sys.argv[1], sys.argv[2])
