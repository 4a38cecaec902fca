"""The cases and the oracles the PNG-encoder test files share (tests/test_png_encode_{host,gpu,launcher}.py): the images,
torch's CPU arithmetic for the pixels, the scanline stream (filter choice included) restated in numpy, zlib's Z_RLE stream over the same
bytes, the size allowance, and what each case is there to exercise -- asserted on the restated stream, not assumed."""
import hashlib
import heapq
import io
import json
import os
import struct
import zlib

import numpy as np
import torch

from png_restatement import chunks, filter_rows, filtered_rows  # noqa: F401  (chunks: for the test files)

BLOCK = 16384           # GOF_PNG_BLOCK_BYTES: compared with the library's own value by the tests

# The allowance over zlib's Z_RLE stream of the same scanline bytes, per input block (DESIGN.md §3.16 derives it):
#   header      3 + 5 + 5 + 4 bits, 19 x 3 bits of code-length code lengths, (286 + 1) code lengths of at most 7 bits: 2083 bits = 261 bytes
#   terminator  the empty stored block behind a dynamic block: 3 bits and the padding (at most one byte), 00 00 FF FF: 5 bytes
#   boundary    tokens restart at a block start: the first byte is a literal, a match zlib carries across the boundary is cut in two and
#               each piece may leave up to two literals: at most 6 more tokens of at most 15 + 5 + 1 bits: 126 bits = 16 bytes
#   limiting    0: the codes are optimal among codes of at most 15 bits, and zlib's are such codes
HEADER_MAX = (17 + 19 * 3 + 287 * 7 + 7) // 8
ALLOW_PER_BLOCK = HEADER_MAX + 5 + 16
assert HEADER_MAX == 261


def quantised(t):
    """what torchvision's save_image computes, by torch on the CPU -> (H, W, 3) uint8"""
    t = t.detach().cpu()
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.size(0) == 1:
        t = t.expand(3, -1, -1)
    return t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()


def scanlines(px):
    """(H, W, 3) uint8 -> the PNG scanline stream: per row the filter (None, Sub, Up, Average, Paeth against the unfiltered previous row,
    zeros above row 0) with the smallest sum of |signed filtered byte|, the lowest number on a tie"""
    sums = np.abs(filtered_rows(px).view(np.int8).astype(np.int32)).sum(axis=2)
    return filter_rows(px, sums.argmin(axis=1))     # (the first minimum)


def zrle(raw):
    """the CPU reference for the strategy: zlib level 6, memLevel 9, Z_RLE"""
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return c.compress(raw) + c.flush()


def pillow_file(px, **kw):
    """(H, W, C) uint8, C in 1..4 -> Pillow's file"""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px if px.shape[2] > 1 else px[:, :, 0]).save(b, format="png", **kw)
    return b.getvalue()


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_encode_pins.json")) as _fh:
    PINS = json.load(_fh)["cases"]


def check_pin(name, png):
    """the file is byte for byte the pinned one (tests/golden/png_encode_pins.json, written by tests/golden/make_png_encode_pins.py):
    integer arithmetic and index tie-breaks leave the emulator and the device no room to differ"""
    pin = PINS[name]
    assert (len(png), hashlib.sha256(png).hexdigest()) == (pin["bytes"], pin["sha256"]), "%s: %d bytes, not the pinned file of %d bytes" % (name, len(png), pin["bytes"])


def has_run3(raw, lo=0, hi=None):
    a = np.frombuffer(raw, np.uint8)[lo:hi]
    return bool(((a[2:] == a[1:-1]) & (a[1:-1] == a[:-2])).any()) if a.size >= 3 else False


def huffman_depth(freqs):
    """the longest code of an UNLIMITED Huffman code for these frequencies"""
    h = [(f, i, 0) for i, f in enumerate(freqs) if f > 0]
    heapq.heapify(h)
    k = len(h)
    while len(h) > 1:
        f1, _, d1 = heapq.heappop(h)
        f2, _, d2 = heapq.heappop(h)
        k += 1
        heapq.heappush(h, (f1 + f2, k, max(d1, d2) + 1))
    return h[0][2]


# ---- the images ------------------------------------------------------------------------------------------------------------------------
def _from_bytes(px):
    """(H, W, 3) uint8 -> float32 (3, H, W) that quantises back to these bytes"""
    return torch.from_numpy(np.ascontiguousarray(px.transpose(2, 0, 1))).to(torch.float32) / 255.0


def _smooth(W, H, seed):
    """a photo-like image: gradients and a little noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([0.5 + 0.4 * np.sin(x / 17.0 + y / 29.0), (x + 2 * y) / (W + 2 * H + 1), 0.3 + 0.3 * np.cos(y / 11.0)], 0)
    base[:, : H // 3] = 1.0                                                   # a white background band (render.py's white_background scenes)
    noise = rng.normal(0, 0.004, base.shape).astype(np.float32)
    noise[:, : H // 3] = 0
    return torch.from_numpy((base + noise).astype(np.float32))


def _random(W, H, seed, C=3):
    return torch.from_numpy(np.random.default_rng(seed).random((C, H, W), dtype=np.float32))


def fibonacci_row():
    """one row whose scanline (the filter byte 1, then the Sub-filtered bytes) has the literal frequencies 1, 2, 3, 5, ..., 2584 (17 values,
    6763 bytes, no byte three times in a row): with the end-of-block symbol's 1 in front these are the Fibonacci numbers, and an unlimited
    Huffman code for them is 17 bits deep"""
    fib = [1, 2]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    counts = fib[::-1]                                                                   # the most frequent value is 0
    counts[1] -= 1                                                                       # (the filter byte is a 1)
    f = np.concatenate([np.full(n, v, np.uint8) for v, n in enumerate(counts)])         # 6762 = 3 x 2254
    rng = np.random.default_rng(11)
    rng.shuffle(f)
    for _ in range(100000):
        bad = np.nonzero((f[2:] == f[1:-1]) & (f[1:-1] == f[:-2]))[0]
        if bad.size == 0:
            break
        j = int(rng.integers(0, f.size))
        f[bad[0] + 1], f[j] = f[j], f[bad[0] + 1]
    raw = f.astype(np.int64).reshape(-1, 3).cumsum(axis=0) & 255                         # Sub with bpp 3 undoes the running sums
    return _from_bytes(raw.astype(np.uint8).reshape(1, -1, 3))


def special_values():
    """below 0, above 1, k / 255 and its two neighbours, NaN and the infinities"""
    k = torch.arange(256, dtype=torch.float32) / 255.0
    up = torch.nextafter(k, torch.full_like(k, 2.0))
    down = torch.nextafter(k, torch.full_like(k, -2.0))
    half = (torch.arange(256, dtype=torch.float32) + 0.5) / 255.0                          # the rounding boundaries themselves
    extra = torch.tensor([-0.5, -1e-8, -0.0, 1.0000001, 1.5, 300.0, -300.0, float("nan"), float("inf"), float("-inf"), 1e-45, 0.9999999, 0.00196, 0.00197, float("nan"), 3e38])
    v = torch.cat([k, up, down, half, torch.nextafter(half, torch.full_like(half, 2.0)), torch.nextafter(half, torch.full_like(half, -2.0)), extra])
    n = v.numel()
    W = 33
    H = -(-n // (3 * W)) + 1
    flat = torch.zeros(3 * H * W)
    flat[:n] = v
    flat[n:] = v[torch.arange(3 * H * W - n) * 7 % n]
    return flat.reshape(3, H, W).clone()


# name -> (builder of the (C, H, W) or (H, W) float32 tensor, asserted for size?, what it is there for)
CASES = {
    "1x1": (lambda: _random(1, 1, 1), False, "sub-block"),
    "1x7": (lambda: _random(1, 7, 2), False, "sub-block"),
    "7x1": (lambda: _random(7, 1, 3), False, "sub-block"),
    "w6": (lambda: _smooth(6, 9, 4), False, "sub-block; 3W + 1 = 19"),
    "w5": (lambda: _smooth(5, 4, 5), False, "sub-block; 3W + 1 = 16"),
    "block_minus_1": (lambda: _smooth(42, 129, 6), False, "sub-block: 16383 bytes"),
    "block_exact": (lambda: _smooth(85, 64, 7), True, "16384 bytes: one full block, the last"),
    "block_plus_1": (lambda: _smooth(48, 113, 8), True, "16385 bytes: a second block of one byte"),
    "black": (lambda: torch.zeros(3, 70, 200), True, "42070 zero bytes: one run over three blocks, chains of 258"),
    "gray": (lambda: torch.full((3, 90, 210), 0.5), True, "constant: runs of 3W zeros behind filter byte 2"),
    "nomatch": (lambda: _random(40, 40, 9), False, "sub-block, random: no three equal bytes, no distance code"),
    "random": (lambda: _random(100, 80, 10), False, "random: 24080 bytes, stored blocks or near-flat codes"),
    "fibonacci": (fibonacci_row, False, "sub-block: 6763 bytes, the 15-bit limit binds"),
    "mono": (lambda: _smooth(64, 90, 12)[1:2].clone(), True, "one channel -> three equal ones"),
    "mono2d": (lambda: _smooth(31, 17, 13)[0].clone(), False, "sub-block; (H, W)"),
    "strided": (lambda: torch.cat([_smooth(75, 80, 14), _random(75, 80, 15, C=6)], 0), True, "[:3] of nine planes, read in place"),
    "wide": (lambda: _smooth(1030, 6, 16), True, "W > 1024: two staging chunks per row"),
    "wider": (lambda: _smooth(2050, 3, 17), True, "W > 2048: three staging chunks per row"),
    "values": (special_values, False, "sub-block; clamp, rounding boundaries, NaN"),
    "photo": (lambda: _smooth(160, 120, 18), True, "four blocks of smooth content"),
}
EXCLUDED = sorted(n for n, c in CASES.items() if not c[1])


def tensor(name):
    return CASES[name][0]()


def view(name, t):
    """what the encoder is given for a case's (uploaded) tensor"""
    return t[:3] if name == "strided" else t


def check_png(name, png, t_cpu, block=BLOCK):
    """every oracle of one case -> a row of sizes {name, stream, ours, zrle, pillow, blocks}"""
    from PIL import Image
    px = quantised(view(name, t_cpu))
    H, W, _ = px.shape
    ch = chunks(png)
    kinds = [k for k, _ in ch]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"}, kinds
    assert ch[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    im = Image.open(io.BytesIO(png))
    assert im.mode == "RGB" and im.size == (W, H)
    assert np.array_equal(np.array(im), px), "%s: the decoded pixels differ from torch's CPU arithmetic" % name
    stream = b"".join(d for k, d in ch if k == b"IDAT")
    raw = scanlines(px)
    assert stream[:2] == b"\x78\x9c"
    assert zlib.decompress(stream) == raw, "%s: the scanline stream differs from the restatement" % name
    nblocks = -(-len(raw) // block)
    ref = zrle(raw)
    row = {"name": name, "stream": len(raw), "ours": len(stream), "zrle": len(ref), "pillow": len(pillow_file(px)), "png": len(png), "blocks": nblocks}
    print("%-14s %8d scanline bytes  %3d blocks  ours %8d  Z_RLE %8d (%.4f)  Pillow file %8d (%.4f)"
          % (name, len(raw), nblocks, len(stream), len(ref), len(stream) / len(ref), row["pillow"], len(png) / row["pillow"]))
    assert len(stream) <= len(raw) + 5 * nblocks + 6, "%s: larger than the stored bound" % name
    if CASES[name][1]:
        assert len(raw) >= block
        assert len(stream) <= len(ref) + nblocks * ALLOW_PER_BLOCK, "%s: %d bytes, Z_RLE %d + %d blocks x %d" % (name, len(stream), len(ref), nblocks, ALLOW_PER_BLOCK)
    else:
        assert len(raw) < block or name == "random", "%s is excluded from the size assertion but is neither random nor smaller than a block" % name
    return row


def check_purposes(block=BLOCK):
    """the cases exercise what they are there for: asserted on the restated streams"""
    raws = {n: scanlines(quantised(view(n, tensor(n)))) for n in ("black", "gray", "nomatch", "fibonacci", "random", "block_minus_1", "block_exact", "block_plus_1", "w6", "values")}
    assert [len(raws[n]) for n in ("block_minus_1", "block_exact", "block_plus_1")] == [block - 1, block, block + 1]
    assert raws["black"] == bytes(len(raws["black"])) and len(raws["black"]) > 2 * block          # one run across two boundaries
    g = np.frombuffer(raws["gray"], np.uint8).reshape(90, 631)
    assert (g[1:, 0] == 2).all() and not g[1:, 1:].any() and len(raws["gray"]) > 3 * block       # runs of 630 zeros: 258 + 258 + 113
    assert not has_run3(raws["nomatch"]) and len(raws["nomatch"]) < block
    assert len(raws["random"]) > block
    f = np.frombuffer(raws["fibonacci"], np.uint8)
    assert f[0] == 1 and not has_run3(raws["fibonacci"])
    hist = np.bincount(f, minlength=256).tolist() + [1]
    assert huffman_depth(hist) > 15, huffman_depth(hist)
    assert (len(raws["w6"]) // 9) % 4 != 0
    v = quantised(tensor("values"))
    assert v.min() == 0 and v.max() == 255 and torch.isnan(tensor("values")).any()


# ---- the runs the host and the GPU test files share: a run takes the product module and three helpers and returns arrays ----------------
#   up(tensor) -> the tensor where the library can read it     alloc(nbytes) -> a uint8 buffer filled with 0xA5     down(tensor) -> numpy
def run_cases(IW, up, alloc, down, names):
    res = {}
    for n in names:
        res["png_" + n] = np.frombuffer(IW.encode_png(view(n, up(tensor(n)))), np.uint8)
        res["again_" + n] = np.frombuffer(IW.encode_png(view(n, up(tensor(n)))), np.uint8)
    return res


def check_cases(res, names):
    rows = []
    for n in names:
        png = res["png_" + n].tobytes()
        assert res["again_" + n].tobytes() == png, "%s: two encodes of one input differ" % n
        check_pin(n, png)
        rows.append(check_png(n, png, tensor(n)))
    return rows


ENTRY_CASE = "block_plus_1"
FILLS = (0xA5, 0x00, 0xFF)


def _call(IW, a, planes, out, cap, size, ws, ws_bytes):
    import ctypes as C
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    rc = IW.lib.gof_png_encode(C.byref(a) if a is not None else None, p(planes), p(out), cap, p(size), p(ws), ws_bytes, IW._stream())
    return rc, IW.lib.gof_last_error().decode()


def run_entry(IW, up, alloc, down, names=None):
    """the C entry itself: workspace and output pre-filled with 0xA5, 0x00 and 0xFF; every invalid argument"""
    res = {}
    t = tensor(ENTRY_CASE)
    _, H, W = t.shape
    planes = up(t)
    need, cap = int(IW.lib.gof_png_ws_bytes(W, H)), int(IW.lib.gof_png_max_bytes(W, H))
    res["need_cap"] = np.array([need, cap, int(IW.lib.gof_png_block_bytes()), int(IW.lib.gof_png_abi_version()), int(IW.lib.gof_abi_version())])
    good = IW.GofPngEncode(W, H, 3, 0, H * W)
    for fill in FILLS:
        ws, out, size = alloc(need + 64), alloc(cap + 64), alloc(8 + 64)
        ws.fill_(fill)
        out.fill_(fill)
        rc, _ = _call(IW, good, planes, out, cap, size, ws, need)
        n = int(down(size)[:8].view(np.uint64)[0])
        o = down(out)
        res["fill%02x" % fill] = o[:n].copy()
        res["fill%02x_rc" % fill] = np.array(rc)
        res["fill%02x_tails" % fill] = np.array(bool((o[cap:] == fill).all() and (down(ws)[need:] == fill).all() and (down(size)[8:] == 0xA5).all()))
    ws, out, size = alloc(need + 16), alloc(cap), alloc(8)
    G = IW.GofPngEncode
    bad = {"zero_w": dict(a=G(0, H, 3, 0, H * W)), "zero_h": dict(a=G(W, 0, 3, 0, H * W)), "huge_w": dict(a=G(65536, 1, 3, 0, 65536)),
           "huge_stream": dict(a=G(65535, 65535, 3, 0, 65535 * 65535)), "two_channels": dict(a=G(W, H, 2, 0, H * W)), "four_channels": dict(a=G(W, H, 4, 0, H * W)),
           "stride": dict(a=G(W, H, 3, 0, H * W - 1)), "null_args": dict(a=None), "null_planes": dict(planes=None), "null_out": dict(out=None),
           "null_size": dict(size=None), "null_ws": dict(ws=None), "odd_ws": dict(ws=ws[8:]), "small_ws": dict(ws_bytes=need - 1), "small_out": dict(cap=cap - 1)}
    for name, over in bad.items():
        kw = dict(a=good, planes=planes, out=out, cap=cap, size=size, ws=ws, ws_bytes=need)
        kw.update(over)
        rc, msg = _call(IW, **kw)
        res["err_" + name] = np.array("%d %s" % (rc, msg))
    res["err_poison"] = np.array(bool((down(out) == 0xA5).all() and (down(ws) == 0xA5).all() and (down(size) == 0xA5).all()))
    res["err_queries"] = np.array([int(IW.lib.gof_png_ws_bytes(0, 5)), int(IW.lib.gof_png_ws_bytes(5, 65536)), int(IW.lib.gof_png_max_bytes(65535, 65535)),
                                   int(IW.lib.gof_png_max_bytes(-1, 1))])
    res["png_" + ENTRY_CASE] = np.frombuffer(IW.encode_png(up(t)), np.uint8)
    return res


def check_entry(res, block=BLOCK):
    from image_writer import stream_of
    need, cap, blk, abi, main_abi = (int(v) for v in res["need_cap"])
    t = tensor(ENTRY_CASE)
    _, H, W = t.shape
    stream_bytes = H * (3 * W + 1)
    assert blk == block and abi == 1 and main_abi == 12
    assert need > 0 and cap == stream_bytes + 5 * (-(-stream_bytes // block)) + 6, "gof_png_max_bytes is the stored bound"
    check_pin(ENTRY_CASE, res["png_" + ENTRY_CASE].tobytes())
    want = stream_of(res["png_" + ENTRY_CASE].tobytes())
    for fill in FILLS:
        assert int(res["fill%02x_rc" % fill]) == 0
        assert res["fill%02x" % fill].tobytes() == want, "a workspace and an output filled with 0x%02X change the stream" % fill
        assert bool(res["fill%02x_tails" % fill]), "bytes behind the output, the workspace or the size word were written (fill 0x%02X)" % fill
    table = (("zero_w", -1, "1..65535"), ("zero_h", -1, "1..65535"), ("huge_w", -1, "1..65535"), ("huge_stream", -1, "2^31"), ("two_channels", -1, "channels"),
             ("four_channels", -1, "channels"), ("stride", -1, "stride"), ("null_args", -1, "NULL"), ("null_planes", -1, "NULL"), ("null_out", -1, "NULL"),
             ("null_size", -1, "NULL"), ("null_ws", -1, "NULL"), ("odd_ws", -1, "aligned"), ("small_ws", -2, "workspace"), ("small_out", -1, "gof_png_max_bytes"))
    for name, code, text in table:
        got = str(res["err_" + name])
        assert got.startswith("%d " % code) and text in got, (name, got)
    assert bool(res["err_poison"]), "a refused call wrote to its output, its workspace or its size word"
    assert list(res["err_queries"]) == [0, 0, 0, 0]


GROUPS = (("1x1", "1x7", "7x1", "w6", "w5", "values", "mono2d", "nomatch", "fibonacci"), ("block_minus_1", "block_exact", "block_plus_1", "mono"),
          ("black", "gray", "random"), ("strided", "wide", "wider", "photo"))
