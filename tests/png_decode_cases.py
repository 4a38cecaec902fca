"""The cases and the oracles the PNG-decoder test files share (tests/test_png_decode_{host,gpu,launcher}.py): the files,
made here from zlib.compressobj, Pillow, the project's own framing and a small deflate writer for the streams no library writes; the
PNG unfilter restated in numpy; a puff-style inflate TOKENIZER that is used only to assert what each case is there to exercise (block
types, code lengths, distances, lengths, the code-length symbols 16 / 17 / 18), the way png_encode_cases.check_purposes does.  The
oracles need no tolerance: scanlines == zlib.decompress(stream), bytes == the numpy unfilter == Pillow's decode, planes bit-equal to
to_tensor's bytes.to(float32).div(255)."""
import io
import struct
import zlib

import numpy as np
import torch

import png_encode_cases as E
from png_encode_cases import pillow_file
from png_restatement import chunk, filter_rows, frame, header, idat_of, paeth  # noqa: F401  (chunk: for the test files)

# the status words of include/gof_png_read_hip.h
OK, E_ZLIB_HEADER, E_TRUNCATED, E_BLOCK_TYPE, E_STORED, E_CODE_LENGTHS, E_SYMBOL, E_DISTANCE, E_LONG, E_SHORT, E_ADLER, E_FILTER = range(12)


def unfilter(scan, h, w, c):
    """the restatement: scanline bytes -> (h, w, c) uint8, byte by byte along a row (Sub, Average and Paeth are serial)"""
    s = np.frombuffer(scan, np.uint8).reshape(h, w * c + 1)
    out = np.zeros((h, w * c), np.int32)
    prev = np.zeros(w * c, np.int32)
    for y in range(h):
        ft, raw, cur = int(s[y, 0]), s[y, 1:].astype(np.int32), out[y]
        assert ft <= 4
        if ft == 0:
            cur[:] = raw
        elif ft == 2:
            cur[:] = (raw + prev) & 255
        else:
            for i in range(w * c):
                a = cur[i - c] if i >= c else 0
                b = prev[i]
                cc = prev[i - c] if i >= c else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    p = int(paeth(a, b, cc))
                cur[i] = (raw[i] + p) & 255
        prev = cur
    return out.astype(np.uint8).reshape(h, w, c)


def to_tensor(px):
    """torchvision's to_tensor for 8-bit bytes: (H, W, C) uint8 -> (C, H, W) float32"""
    return torch.from_numpy(np.ascontiguousarray(px.transpose(2, 0, 1))).to(torch.float32).div(255)


def pillow_pixels(png):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(png)))
    return a if a.ndim == 3 else a[:, :, None]


# ---- a small deflate writer: the streams no library writes ---------------------------------------------------------------------------------
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                        # a value, low bit first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                       # a Huffman code, high bit first
        self.put(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical code (no validity check: corrupt sets are written with it too)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 16):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def flat_lens(used, n):
    """a complete code over the used symbols: lengths L - 1 and L (one symbol: one bit, which deflate accepts as it stands)"""
    used = sorted(used)
    lens = [0] * n
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    L = (len(used) - 1).bit_length()
    short = (1 << L) - len(used)
    for i, s in enumerate(used):
        lens[s] = L - 1 if i < short else L
    return lens


def _sym_of(v, base):
    return max(i for i, b in enumerate(base) if b <= v)


def stored_block(bw, data, final, nlen=None):
    bw.put(1 if final else 0, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    bw.out += data


def huffman_block(bw, tokens, final, lit_lens=None, dist_lens=None, eob=True, hlit=None):
    """tokens: ints (literals) and (length, distance) pairs.  lit_lens None: a fixed block; otherwise a dynamic block with exactly these
    code lengths, sent as ONE run-length coded sequence (a run may cross from the literal / length set into the distances); hlit: more
    literal / length code lengths than the last used one needs."""
    bw.put(1 if final else 0, 1)
    if lit_lens is None:
        bw.put(1, 2)
        lit_lens, dist_lens = FIXED_LIT, FIXED_DIST
    else:
        bw.put(2, 2)
        hlit = hlit or max(257, max(i + 1 for i, l in enumerate(lit_lens) if l))
        hdist = max(1, max([i + 1 for i, l in enumerate(dist_lens) if l] or [1]))
        seq = list(lit_lens[:hlit]) + [0] * (hlit - len(lit_lens[:hlit])) + list(dist_lens[:hdist]) + [0] * (hdist - len(dist_lens[:hdist]))
        cl, i = [], 0                           # (symbol, extra bits, extra value)
        while i < len(seq):
            j = i
            while j < len(seq) and seq[j] == seq[i]:
                j += 1
            run = j - i
            if seq[i] == 0 and run >= 3:
                r = min(run, 138)
                cl.append((17, 3, r - 3) if r <= 10 else (18, 7, r - 11))
                i += r
            elif seq[i] != 0 and run >= 4:
                cl.append((seq[i], 0, 0))
                r = min(run - 1, 6)
                cl.append((16, 2, r - 3))
                i += 1 + r
            else:
                cl.append((seq[i], 0, 0))
                i += 1
        used = {s for s, _, _ in cl}
        if len(used) == 1:
            used.add(0 if 0 not in used else 1)                 # (the code-length code must be complete)
        cl_lens = flat_lens(used, 19)
        hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
        bw.put(hlit - 257, 5)
        bw.put(hdist - 1, 5)
        bw.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            bw.put(cl_lens[s], 3)
        codes = canonical(cl_lens)
        for s, eb, ev in cl:
            bw.code(*codes[s])
            bw.put(ev, eb)
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, tuple):
            ls, ds = _sym_of(t[0], LBASE), _sym_of(t[1], DBASE)
            bw.code(*lit[257 + ls])
            bw.put(t[0] - LBASE[ls], LEXT[ls])
            bw.code(*dist[ds])
            bw.put(t[1] - DBASE[ds], DEXT[ds])
        else:
            bw.code(*lit[t])
    if eob:
        bw.code(*lit[256])


def expand(tokens, out=None):
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return out


def zwrap(body, raw, adler=None):
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(bytes(raw)) if adler is None else adler)


def literals(data):
    return list(bytes(data))


def greedy(raw, dist, longest=258):
    """tokens for raw: at every position the longest match (3..longest) at exactly this distance, a literal otherwise (byte i of a match
    is byte i - dist of the output, so a match may overlap itself)"""
    toks, p = [], 0
    while p < len(raw):
        n = 0
        while p >= dist and n < longest and p + n < len(raw) and raw[p + n] == raw[p + n - dist]:
            n += 1
        if n >= 3 and len(raw) - p - n not in (1, 2):
            toks.append((n, dist))
            p += n
        else:
            toks.append(raw[p])
            p += 1
    assert bytes(expand(toks)) == bytes(raw)
    return toks


def tokens_for(used_lits, used_lens=(), used_dists=()):
    """(lit_lens, dist_lens) of flat complete codes over what a hand-made block uses"""
    lit = flat_lens(set(used_lits) | {256} | {257 + _sym_of(l, LBASE) for l in used_lens}, 286)
    dist = flat_lens({_sym_of(d, DBASE) for d in used_dists}, 30) if used_dists else [0] * 30
    return lit, dist


# ---- the tokenizer: what a stream consists of (puff's structure; only ever used to assert a case's purpose) --------------------------------
def tokenize(stream):
    """-> dict: types (block types in order), stored (their lengths), lit_bits / dist_bits (longest code used in a header), max_len,
    max_dist, cl (code-length symbols used), ndist (distance codes per dynamic block), cross (a repeat ran across HLIT), starts (the bit
    each block starts at, mod 8), straddle (a match whose source starts in an earlier block and ends in its own), out (the bytes)"""
    data = stream[2:]
    pos = 0

    def get(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((data[(pos + i) >> 3] >> ((pos + i) & 7)) & 1) << i
        pos += n
        return v

    def table(lens):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        offs = [0] * 17
        for l in range(1, 16):
            offs[l + 1] = offs[l] + count[l]
        symbol = [0] * len(lens)
        for s, l in enumerate(lens):
            if l:
                symbol[offs[l]] = s
                offs[l] += 1
        return count, symbol

    def decode(t):
        count, symbol = t
        code = first = index = 0
        for l in range(1, 16):
            code |= get(1)
            if code - count[l] < first:
                return symbol[index + (code - first)]
            index += count[l]
            first = (first + count[l]) << 1
            code <<= 1
        raise ValueError("no code")
    r = dict(types=[], stored=[], lit_bits=0, dist_bits=0, max_len=0, max_dist=0, cl=set(), ndist=[], cross=False, starts=[], straddle=False)
    out = bytearray()
    final = 0
    while not final:
        r["starts"].append(pos & 7)
        block_at = len(out)
        final, typ = get(1), get(2)
        r["types"].append(typ)
        if typ == 0:
            pos = (pos + 7) & ~7
            n, nn = get(16), get(16)
            assert n ^ nn == 0xFFFF
            out += data[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
            r["stored"].append(n)
            continue
        if typ == 1:
            lit, dist = table(FIXED_LIT), table(FIXED_DIST)
        else:
            hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
            cl = [0] * 19
            for s in CL_ORDER[:hclen]:
                cl[s] = get(3)
            ct = table(cl)
            lens = []
            while len(lens) < hlit + hdist:
                s = decode(ct)
                r["cl"].add(s) if s >= 16 else None
                if s < 16:
                    lens.append(s)
                else:
                    rep = 3 + get(2) if s == 16 else 3 + get(3) if s == 17 else 11 + get(7)
                    if len(lens) < hlit < len(lens) + rep:
                        r["cross"] = True
                    lens += [lens[-1] if s == 16 else 0] * rep
            assert len(lens) == hlit + hdist
            r["lit_bits"] = max(r["lit_bits"], max(lens[:hlit]))
            r["dist_bits"] = max(r["dist_bits"], max(lens[hlit:]))
            r["ndist"].append(sum(1 for l in lens[hlit:] if l))
            lit, dist = table(lens[:hlit]), table(lens[hlit:])
        while True:
            s = decode(lit)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                n = LBASE[s - 257] + get(LEXT[s - 257])
                ds = decode(dist)
                d = DBASE[ds] + get(DEXT[ds])
                r["max_len"], r["max_dist"] = max(r["max_len"], n), max(r["max_dist"], d)
                if len(out) - d < block_at and len(out) - d + n > block_at:
                    r["straddle"] = True
                r.setdefault("pairs", set()).add((n, d))
                for _ in range(n):
                    out.append(out[-d])
    r["out"] = bytes(out)
    return r


# ---- the images ---------------------------------------------------------------------------------------------------------------------------
def _noisy(h, w, c, seed):
    """smooth with a little noise: every filter does something, matches and literals mix"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 3 + y * 5)[..., None] + 40 * np.arange(c) + rng.integers(0, 5, (h, w, c))).astype(np.uint8)


def _random(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def _mix(h, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 5, h)]


def _z(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, at = b"", 0
    for f in list(flush_at) + [len(raw)]:
        out += c.compress(raw[at:f])
        if f < len(raw):
            out += c.flush(flush)
        at = f
    return out + c.flush()


def _case(px, filters=None, stream=None, **kw):
    """a file of the project's own framing around zlib's stream of the filtered pixels (or the given stream)"""
    h, w, c = px.shape
    raw = filter_rows(px, filters if filters is not None else _mix(h, h * 131 + w))
    return frame(w, h, c, _z(raw) if stream is None else stream(raw), **kw)


def _hand(px, build):
    """a file around a hand-made deflate stream: build(bw, raw) writes the blocks for the scanlines of px with filter 0"""
    h, w, c = px.shape
    raw = filter_rows(px, [0] * h)
    bw = BitWriter()
    build(bw, raw)
    return frame(w, h, c, zwrap(bw.bytes(), raw))


def _stored_blocks(sizes):
    def build(bw, raw):
        at = 0
        for k, n in enumerate(sizes):
            stored_block(bw, raw[at:at + n], k == len(sizes) - 1)
            at += n
        assert at == len(raw)
    return build


def _dist32768():
    """gray, W = 127 (rows of 128 bytes), H = 300, row r + 256 = row r: 256 rows of literals, then matches at distance exactly 32768"""
    px = _random(300, 127, 1, 41)
    px[256:] = px[:44]
    raw = filter_rows(px, [0] * 300)
    rest, toks = 44 * 128, literals(raw[:32768])
    while rest:
        n = min(258, rest) if rest - min(258, rest) not in (1, 2) else 255
        toks.append((n, 32768))
        rest -= n
    assert bytes(expand(toks)) == raw
    bw = BitWriter()
    huffman_block(bw, toks, True)
    return frame(127, 300, 1, zwrap(bw.bytes(), raw))


def _dist32725():
    """128 x 100 RGB, rows 85.. repeat rows 0..: 85 rows of 385 bytes = 32725"""
    px = _random(100, 128, 3, 42)
    px[85:] = px[:15]
    raw = filter_rows(px, [0] * 100)
    toks, rest = literals(raw[:32725]), 15 * 385
    while rest:
        n = min(258, rest) if rest - min(258, rest) not in (1, 2) else 255
        toks.append((n, 32725))
        rest -= n
    assert bytes(expand(toks)) == raw
    lit, dist = tokens_for(set(raw[:32725]), [t[0] for t in toks if isinstance(t, tuple)], [32725])
    bw = BitWriter()
    huffman_block(bw, toks, True, lit, dist)
    return frame(128, 100, 3, zwrap(bw.bytes(), raw))


def _len258(dist):
    """a row pattern of period `dist`: literals, then matches of 258 at that distance (overlapping: dist < len)"""
    h, w = 4, 300
    px = np.zeros((h, w, 1), np.uint8)
    flat = np.tile(np.arange(7, 7 + dist, dtype=np.uint8), h * (w + 1))[:h * (w + 1)]
    flat = flat.reshape(h, w + 1).copy()
    flat[:, 0] = 0                                                  # (the filter bytes)
    raw = flat.tobytes()
    px[:] = flat[:, 1:, None]
    toks = greedy(raw, dist)
    bw = BitWriter()
    huffman_block(bw, toks, True)
    return frame(w, h, 1, zwrap(bw.bytes(), raw))


def _straddle():
    """two fixed blocks: the second starts with a match whose source begins in the first block and runs on into the second's own output"""
    raw = bytearray(filter_rows(_noisy(6, 40, 1, 43), [0] * 6))      # rows of 41 bytes; 90..119 lie inside row 2
    cut = 90
    raw[cut:cut + 30] = raw[cut - 10:cut] * 3                      # the 10 bytes in front of the cut, three times
    raw = bytes(raw)
    bw = BitWriter()
    huffman_block(bw, literals(raw[:cut]), False)
    huffman_block(bw, [(30, 10)] + literals(raw[cut + 30:]), True)
    return frame(40, 6, 1, zwrap(bw.bytes(), raw))


def _literals_only():
    """a dynamic block of literals with NO distance code (HDIST = 1, its length 0)"""
    px = (_random(9, 20, 1, 44) & 15)
    def build(bw, raw):
        lit, dist = tokens_for(set(raw))
        huffman_block(bw, literals(raw), True, lit, dist)
    return _hand(px, build)


def _one_distance():
    """a dynamic block whose distance alphabet is a single code of one bit"""
    px = np.full((9, 40, 1), 9, np.uint8)
    def build(bw, raw):
        toks = greedy(raw, 1)
        lit, dist = tokens_for([t for t in toks if not isinstance(t, tuple)], [t[0] for t in toks if isinstance(t, tuple)], [1])
        huffman_block(bw, toks, True, lit, dist)
    return _hand(px, build)


def _cl_across():
    """a dynamic block whose run of zero code lengths starts in the literal / length set and ends in the distance set"""
    px = np.full((5, 30, 1), 200, np.uint8)
    px[:, ::7] = 3
    def build(bw, raw):
        toks = greedy(raw, 31, 31)
        toks = [t if not isinstance(t, tuple) or t[0] == 31 else None for t in toks]
        assert None not in toks and (31, 31) in toks
        lit, dist = tokens_for([t for t in toks if not isinstance(t, tuple)], [31], [31])      # length symbol 281, distance symbol 9
        huffman_block(bw, toks, True, lit, dist, hlit=286)       # 273..285 unused, then the distances 0..8
    return _hand(px, build)


def _own_encoder(t):
    """the project's own encoder's file (image_writer.encode_png: every dynamic block followed by an empty stored block); made where
    the encoder can run, so the builder takes the module"""
    return lambda IW, up: IW.encode_png(up(t))


def _fib15():
    raw = E.scanlines(E.quantised(E.fibonacci_row()))
    return frame(2254, 1, 3, _z(raw, 6, zlib.Z_HUFFMAN_ONLY))


def _adam7(px):
    """an interlaced file (filter 0, seven passes)"""
    h, w, c = px.shape
    raw = b""
    for ys, xs, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = px[ys::dy, xs::dx]
        if sub.size:
            raw += filter_rows(np.ascontiguousarray(sub), [0] * sub.shape[0])
    return frame(w, h, c, zlib.compress(raw), interlace=1)


GRID = [(h, w) for w in (63, 64, 65) for h in (63, 64, 65, 129)]

# name -> builder of the file's bytes.  A builder with arguments (IW, up) needs the encoder: see _own_encoder.
CASES = {
    "1x1": lambda: _case(_random(1, 1, 3, 1)),
    "1x300": lambda: _case(_noisy(300, 1, 3, 2)),
    "300x1": lambda: _case(_noisy(1, 300, 3, 3)),
    "c1": lambda: _case(_noisy(129, 65, 1, 4)),
    "c2": lambda: _case(_noisy(129, 65, 2, 5)),
    "c4": lambda: _case(_noisy(129, 65, 4, 6)),
    "mix": lambda: _case(_random(70, 37, 3, 7)),
    "paeth_ties": lambda: _case(_random(20, 20, 1, 8) & 3, [4] * 20),
    "average_carry": lambda: _case(np.full((10, 10, 3), 255, np.uint8), [3] * 10),
    "stored_65535": lambda: _hand(_random(255, 256, 1, 9), _stored_blocks([65535])),
    "stored_many": lambda: _hand(_random(20, 30, 3, 10), _stored_blocks([0, 700, 0, 1, 1119, 0])),
    "fixed": lambda: _case(_noisy(40, 50, 3, 11), stream=lambda raw: _z(raw, 6, zlib.Z_FIXED)),
    "rle": lambda: _case(_noisy(40, 50, 3, 12), stream=lambda raw: _z(raw, 6, zlib.Z_RLE)),
    "huffman_only": lambda: _case(_noisy(40, 50, 3, 13), stream=lambda raw: _z(raw, 6, zlib.Z_HUFFMAN_ONLY)),
    "filtered": lambda: _case(_noisy(40, 50, 3, 14), stream=lambda raw: _z(raw, 6, zlib.Z_FILTERED)),
    "level0": lambda: _case(_noisy(40, 50, 3, 15), stream=lambda raw: _z(raw, 0)),
    "sync_flush": lambda: _case(_noisy(40, 50, 3, 16), stream=lambda raw: _z(raw, 6, flush_at=(1000, 1001, 3500))),
    "full_flush": lambda: _case(_noisy(40, 50, 3, 17), stream=lambda raw: _z(raw, 9, flush_at=(777, 4000), flush=zlib.Z_FULL_FLUSH)),
    "fib15": _fib15,
    "literals_only": _literals_only,
    "one_distance": _one_distance,
    "cl_across": _cl_across,
    "len258_d1": lambda: _len258(1),
    "len258_d2": lambda: _len258(2),
    "dist32768": _dist32768,
    "dist32725": _dist32725,
    "straddle": _straddle,
    "idat_1byte": lambda: _case(_noisy(12, 14, 3, 18), idat=1),
    "idat_one": lambda: _case(_noisy(12, 14, 3, 18)),
    "ancillary": lambda: _case(_noisy(12, 14, 3, 19), idat=50, before=((b"gAMA", struct.pack(">I", 45455)), (b"tEXt", b"Title\0x")), after=((b"tIME", bytes(7)),)),
    "pillow_1": lambda: pillow_file(_noisy(120, 160, 3, 20), compress_level=1),
    "pillow_6": lambda: pillow_file(_noisy(120, 160, 4, 21), compress_level=6),
    "pillow_9": lambda: pillow_file(_noisy(120, 160, 1, 22), compress_level=9),
    "pillow_optimize": lambda: pillow_file(_noisy(120, 160, 3, 23), optimize=True),
    "pillow_la": lambda: pillow_file(_noisy(33, 47, 2, 24)),
    "own_photo": _own_encoder(E.tensor("photo")),
    "own_black": _own_encoder(E.tensor("black")),
    "own_nomatch": _own_encoder(E.tensor("nomatch")),
    "own_fibonacci": _own_encoder(E.tensor("fibonacci")),
}
for _h, _w in GRID:
    CASES["grid_%dx%d" % (_w, _h)] = (lambda h=_h, w=_w: _case(_noisy(h, w, 3, h * 1000 + w)))
for _f in range(5):
    CASES["all_f%d" % _f] = (lambda f=_f: _case(_noisy(70, 37, 3, 30 + f), [f] * 70))
    CASES["band_f%d" % _f] = (lambda f=_f: _case(_noisy(130, 21, 3, 35 + f), [f if y in (0, 64, 128) else m for y, m in enumerate(_mix(130, 50 + f))]))

GROUPS = (
    ("1x1", "1x300", "300x1", "c1", "c2", "c4", "mix", "paeth_ties", "average_carry"),
    tuple("grid_%dx%d" % (w, h) for h, w in GRID),
    tuple("all_f%d" % f for f in range(5)) + tuple("band_f%d" % f for f in range(5)),
    ("stored_65535", "stored_many", "fixed", "rle", "huffman_only", "filtered", "level0", "sync_flush", "full_flush"),
    ("fib15", "literals_only", "one_distance", "cl_across", "len258_d1", "len258_d2", "dist32768", "dist32725", "straddle"),
    ("idat_1byte", "idat_one", "ancillary", "pillow_1", "pillow_6", "pillow_9", "pillow_optimize", "pillow_la"),
    ("own_photo", "own_black", "own_nomatch", "own_fibonacci"),
)
ORDER_GROUP = GROUPS[4]                          # the group that also runs under other fiber orders


def needs_encoder(name):
    return name.startswith("own_")


def build(name, IW=None, up=None):
    return CASES[name](IW, up) if needs_encoder(name) else CASES[name]()


def check_file(name, png, planes, pixels):
    """every oracle of one good case.  planes: (C, H, W) float32, pixels: (H, W, C) uint8 -- what the decoder gave for `png`"""
    w, h, c = header(png)
    scan = zlib.decompress(idat_of(png))
    assert len(scan) == h * (w * c + 1), name
    want = unfilter(scan, h, w, c)
    assert np.array_equal(want, pillow_pixels(png)), "%s: the restated unfilter differs from Pillow" % name
    assert pixels.shape == (h, w, c) and np.array_equal(pixels, want), "%s: the bytes differ" % name
    t = to_tensor(want)
    assert planes.shape == t.shape and planes.dtype == np.float32
    assert np.array_equal(planes.view(np.uint32), t.numpy().view(np.uint32)), "%s: the planes are not bit-equal to to_tensor's" % name


def check_purposes(files):
    """files: {name: bytes} of every case that needs no encoder (and, where given, the encoder's) -- the cases exercise what they are
    there for: asserted on the streams"""
    tk = {n: tokenize(idat_of(f)) for n, f in files.items()}
    for n, f in files.items():
        assert tk[n]["out"] == zlib.decompress(idat_of(f)), n
    assert tk["stored_65535"]["types"] == [0] and tk["stored_65535"]["stored"] == [65535]
    assert tk["stored_many"]["stored"] == [0, 700, 0, 1, 1119, 0]
    assert set(tk["level0"]["types"]) == {0}
    assert set(tk["fixed"]["types"]) == {1} and tk["fixed"]["max_len"] >= 3
    assert 2 in tk["rle"]["types"] and tk["rle"]["max_dist"] == 1
    assert tk["huffman_only"]["max_len"] == 0 and tk["huffman_only"]["ndist"]
    assert tk["sync_flush"]["stored"].count(0) == 3 and len(set(tk["sync_flush"]["starts"])) > 1, "blocks start at several bit offsets"
    assert tk["full_flush"]["stored"].count(0) == 2
    assert tk["fib15"]["lit_bits"] == 15
    assert tk["literals_only"]["types"] == [2] and tk["literals_only"]["ndist"] == [0] and tk["literals_only"]["max_len"] == 0
    assert tk["one_distance"]["ndist"] == [1] and tk["one_distance"]["dist_bits"] == 1 and tk["one_distance"]["max_dist"] == 1
    assert tk["cl_across"]["cross"] and tk["cl_across"]["max_dist"] == 31
    assert {16, 17, 18} <= set().union(*(t["cl"] for t in tk.values())), "the code-length symbols 16, 17 and 18 all occur"
    assert (258, 1) in tk["len258_d1"]["pairs"] and (258, 2) in tk["len258_d2"]["pairs"]
    assert tk["dist32768"]["max_dist"] == 32768 and tk["dist32725"]["max_dist"] == 32725 and tk["dist32725"]["types"] == [2]
    assert tk["straddle"]["straddle"] and tk["straddle"]["types"] == [1, 1]
    assert max(t["max_len"] for t in tk.values()) == 258 and min(min(p[0] for p in t.get("pairs", {(3, 1)})) for t in tk.values()) == 3
    for n in ("pillow_1", "pillow_6", "pillow_9", "pillow_optimize"):
        assert 2 in tk[n]["types"] and tk[n]["max_len"] >= 3, n
    # the filter cases
    for n, f in files.items():
        w, h, c = header(f)
        ft = np.frombuffer(tk[n]["out"], np.uint8).reshape(h, w * c + 1)[:, 0]
        if n.startswith("all_f"):
            assert (ft == int(n[-1])).all()
        if n.startswith("band_f"):
            assert h > 128 and (ft[[0, 64, 128]] == int(n[-1])).all() and len(set(ft.tolist())) == 5
        if n == "mix" or n.startswith("grid_"):
            assert len(set(ft.tolist())) == 5, n
    px = unfilter(tk["paeth_ties"]["out"], 20, 20, 1)[:, :, 0].astype(int)
    a, b, c = px[1:, :-1], px[:-1, 1:], px[:-1, :-1]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    for tie in ((pa == pb) & (pb == pc), (pa == pb) & (pa < pc), (pa == pc) & (pa < pb), (pb == pc) & (pb < pa)):
        assert tie.any()
    assert (a == b).any() and ((a == b) & (b == c)).any()
    assert (unfilter(tk["average_carry"]["out"], 10, 10, 3) == 255).all(), "Average of 255 + 255"
    if "own_photo" in files:
        t = tk["own_photo"]
        assert t["types"].count(2) >= 3 and t["stored"].count(0) == t["types"].count(2) - (1 if t["types"][-1] == 2 else 0)
        assert tk["own_nomatch"]["types"] == [0] and set(tk["own_black"]["ndist"]) == {1}
        assert tk["own_fibonacci"]["ndist"] == [0] and tk["own_fibonacci"]["lit_bits"] == 15, "15-bit literals and no distance code"


# ---- files the unit does not take ---------------------------------------------------------------------------------------------------------
def not_taken_files():
    """{name: (bytes, the reason parse() gives)}: valid PNG files Pillow reads and the unit refuses"""
    from PIL import Image
    def pil(im, **kw):
        b = io.BytesIO()
        im.save(b, format="png", **kw)
        return b.getvalue()
    rgb = _noisy(9, 11, 3, 60)
    return {
        "interlaced": (_adam7(rgb), "interlaced"),
        "sixteen": (pil(Image.fromarray((_noisy(9, 11, 1, 61)[:, :, 0].astype(np.uint16) * 257))), "bit depth 16"),
        "palette": (pil(Image.fromarray(rgb).convert("P")), "palette"),
        "one_bit": (pil(Image.fromarray(rgb[:, :, 0] > 100)), "bit depth 1"),
        "trns": (pil(Image.fromarray(rgb), transparency=(1, 2, 3)), "tRNS"),
    }


# ---- corrupt streams -----------------------------------------------------------------------------------------------------------------------
def corrupt_files():
    """[(name, bytes, the status its image must get)]: files whose chunks are sound and whose stream is not"""
    px = _noisy(12, 14, 3, 70)
    h, w, c = px.shape
    raw = filter_rows(px, _mix(h, 71))
    good = _z(raw)
    out = []
    for k in range(1, 9):
        out.append(("cut_%d" % k, frame(w, h, c, good[:-k]), E_TRUNCATED))
    out.append(("cut_mid", frame(w, h, c, good[:len(good) // 2]), E_TRUNCATED))
    out.append(("cut_header", frame(w, h, c, good[:1]), E_TRUNCATED))
    out.append(("adler", frame(w, h, c, good[:-1] + bytes([good[-1] ^ 1])), E_ADLER))
    out.append(("zlib_cm", frame(w, h, c, b"\x79\x9c" + good[2:]), E_ZLIB_HEADER))
    out.append(("zlib_fdict", frame(w, h, c, b"\x78\xbb" + good[2:]), E_ZLIB_HEADER))
    out.append(("zlib_fcheck", frame(w, h, c, b"\x78\x9d" + good[2:]), E_ZLIB_HEADER))

    def hand(build, raw_=raw):
        bw = BitWriter()
        build(bw)
        return frame(w, h, c, zwrap(bw.bytes(), raw_))
    out.append(("distance_front", hand(lambda bw: huffman_block(bw, literals(raw[:5]) + [(10, 6)] + literals(raw[15:]), True)), E_DISTANCE))
    out.append(("distance_first", hand(lambda bw: huffman_block(bw, [(3, 1)] + literals(raw[3:]), True)), E_DISTANCE))
    lit, dist = tokens_for(set(raw))
    over = list(lit)
    over[[i for i, l in enumerate(over) if l][0]] -= 1                      # one code a bit shorter: over-subscribed
    out.append(("over_subscribed", hand(lambda bw: huffman_block(bw, [], True, over, dist)), E_CODE_LENGTHS))
    under = list(lit)
    under[[i for i, l in enumerate(under) if l][0]] += 1                    # one code a bit longer: incomplete
    out.append(("incomplete", hand(lambda bw: huffman_block(bw, [], True, under, dist)), E_CODE_LENGTHS))
    dist2 = [0] * 30
    dist2[0] = dist2[1] = dist2[2] = 1                                      # three distance codes of one bit
    out.append(("over_subscribed_dist", hand(lambda bw: huffman_block(bw, [], True, lit, dist2)), E_CODE_LENGTHS))

    def type3(bw):
        bw.put(1, 1)
        bw.put(3, 2)
    out.append(("block_type_3", hand(type3), E_BLOCK_TYPE))
    out.append(("stored_nlen", hand(lambda bw: stored_block(bw, raw, True, nlen=len(raw))), E_STORED))
    out.append(("fixed_symbol_286", hand(lambda bw: (bw.put(1, 1), bw.put(1, 2), bw.code(0b11000110, 8))), E_SYMBOL))
    bad = bytearray(raw)
    bad[(w * c + 1) * 7] = 5
    out.append(("filter_5", frame(w, h, c, _z(bytes(bad))), E_FILTER))
    out.append(("short_1", frame(w, h, c, _z(raw[:-1])), E_SHORT))
    out.append(("long_1", frame(w, h, c, _z(raw + b"\0")), E_LONG))
    out.append(("long_stored", hand(lambda bw: stored_block(bw, raw + b"\1", True), raw + b"\1"), E_LONG))
    out.append(("long_match", hand(lambda bw: huffman_block(bw, literals(raw[:-2]) + [(258, 1)], True)), E_LONG))
    return out


def good_neighbours():
    return [_case(_noisy(12, 14, 3, 80)), _case(_noisy(65, 9, 4, 81)), _case(_noisy(7, 30, 1, 82))]


# ---- the runs the host and the GPU test files share: a run takes the product modules and helpers and returns arrays ---------------------
def run_cases(R, IW, up, down, names):
    """every named case through read_images twice, as planes and as bytes"""
    files = [build(n, IW, up) for n in names]
    res = {}
    planes, again, pixels = R.read_images(files), R.read_images(files), R.read_images(files, planes=False)
    for n, f, p, a, b in zip(names, files, planes, again, pixels):
        res["file_" + n] = np.frombuffer(f, np.uint8)
        res["planes_" + n], res["again_" + n], res["pixels_" + n] = down(p), down(a), down(b)
    return res


def check_cases(res, names):
    files = {}
    for n in names:
        f = res["file_" + n].tobytes()
        files[n] = f
        check_file(n, f, res["planes_" + n], res["pixels_" + n])
        assert np.array_equal(res["again_" + n].view(np.uint32), res["planes_" + n].view(np.uint32)), "%s: two decodes differ" % n
    return files


def run_corrupt(R, down):
    """every corrupt file between good neighbours in ONE batch (statuses and the neighbours' planes), and read_images' error for one"""
    good = good_neighbours()
    bad = corrupt_files()
    files = []
    for k, (_, f, _) in enumerate(bad):
        files += [good[k % len(good)], f]
    files.append(good[0])
    pngs = [R.parse(f) for f in files]
    tensors, words = R._decode_group(pngs, R._device(), True)
    res = {"words": np.array(words)}
    for k in range(0, len(files), 2):
        res["good_%d" % (k // 2)] = down(tensors[k])
    try:
        R.read_images([good[0], bad[0][1], good[1]])
        res["error"] = np.array("no error")
    except ValueError as e:
        res["error"] = np.array(str(e))
    return res


def check_corrupt(res):
    good = good_neighbours()
    bad = corrupt_files()
    words = [int(v) for v in res["words"]]
    assert len(words) == 2 * len(bad) + 1
    for k, (name, _, want) in enumerate(bad):
        assert words[2 * k + 1] == want, "%s: status %d, expected %d" % (name, words[2 * k + 1], want)
        assert words[2 * k] == OK, "the good image in front of %s got status %d" % (name, words[2 * k])
    assert words[-1] == OK
    for k in range(len(bad) + 1):
        f = good[k % len(good)] if k < len(bad) else good[0]
        w, h, c = header(f)
        want = to_tensor(unfilter(zlib.decompress(idat_of(f)), h, w, c)).numpy()
        assert np.array_equal(res["good_%d" % k].view(np.uint32), want.view(np.uint32)), "the good image %d of the batch is not bit-exact" % k
    assert "<bytes>" in str(res["error"]) and "truncated" in str(res["error"]), str(res["error"])


def _call(R, n, descs, streams, nstream, out_b, cap_b, out_p, cap_p, status, ws, ws_bytes):
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    rc = R.lib.gof_png_decode_batch(n, descs, p(streams), nstream, p(out_b), cap_b, p(out_p), cap_p, p(status), p(ws), ws_bytes, R._stream())
    return rc, R.lib.gof_last_error().decode()


FILLS = (0xA5, 0x00, 0xFF)


def run_entry(R, up_bytes, alloc, down):
    """the C entry itself: workspace and outputs pre-filled with 0xA5, 0x00 and 0xFF give the same bits; every invalid argument returns
    < 0 with text and writes nothing; the workspace query is monotone"""
    import ctypes as C
    files = [_case(_noisy(70, 33, 3, 90)), _case(_noisy(5, 66, 2, 91)), _case(_noisy(1, 1, 4, 92))]
    pngs = [R.parse(f) for f in files]
    n = len(pngs)
    G = R.GofPngImage
    descs = (G * n)()
    s_off = o_off = 0
    blob = b""
    for i, p in enumerate(pngs):
        px = p.width * p.height * p.channels
        descs[i] = G(p.width, p.height, p.channels, 0, s_off, p.stream_bytes, o_off, o_off)
        blob += p.stream + bytes(-p.stream_bytes % 16)
        s_off += p.stream_bytes + (-p.stream_bytes % 16)
        o_off += px + (-px % 16)
    streams = up_bytes(blob)
    need = int(R.lib.gof_png_decode_ws_bytes(n, descs, 0))
    res = {"need": np.array([need, int(R.lib.gof_png_decode_ws_bytes(n, descs, 1)), int(R.lib.gof_png_decode_ws_bytes(1, descs, 0)),
                             int(R.lib.gof_png_decode_ws_bytes(2, descs, 0)), int(R.lib.gof_png_decode_ws_bytes(0, descs, 0)),
                             int(R.lib.gof_png_read_abi_version()), int(R.lib.gof_png_abi_version()), int(R.lib.gof_abi_version())])}
    for fill in FILLS:
        ws, ob, op, st = alloc(need + 64), alloc(o_off + 64), alloc(4 * o_off + 64), alloc(4 * n + 64)
        for t in (ws, ob, op, st):
            t.fill_(fill)
        rc, _ = _call(R, n, descs, streams, s_off, ob, o_off, op, o_off, st, ws, need)
        res["fill%02x_rc" % fill] = np.array(rc)
        res["fill%02x_bytes" % fill], res["fill%02x_planes" % fill] = down(ob)[:o_off], down(op)[:4 * o_off]
        res["fill%02x_status" % fill] = down(st)[:4 * n]
        res["fill%02x_tails" % fill] = np.array(bool((down(ws)[need:] == fill).all() and (down(ob)[o_off:] == fill).all() and (down(op)[4 * o_off:] == fill).all()
                                                     and (down(st)[4 * n:] == fill).all()))
    res["offsets"] = np.array([[int(d.bytes_offset), p.width * p.height * p.channels] for d, p in zip(descs, pngs)])
    for i, f in enumerate(files):
        res["entry_file_%d" % i] = np.frombuffer(f, np.uint8)
    ws, ob, op, st = alloc(need + 16), alloc(o_off), alloc(4 * o_off), alloc(4 * n)

    def with_image(i, **over):
        d = (G * n)(*[G(*[getattr(x, f[0]) for f in G._fields_]) for x in descs])
        for k, v in over.items():
            setattr(d[i], k, v)
        return d
    bad = {"negative_n": dict(n=-1), "too_many": dict(n=65536), "null_images": dict(descs=None), "null_streams": dict(streams=None), "null_status": dict(status=None),
           "null_ws": dict(ws=None), "no_output": dict(out_b=None, out_p=None), "odd_ws": dict(ws=ws[8:]), "odd_planes": dict(out_p=op[2:]),
           "small_ws": dict(ws_bytes=need - 1), "zero_w": dict(descs=with_image(1, width=0)), "huge_h": dict(descs=with_image(0, height=65536)),
           "five_channels": dict(descs=with_image(2, channels=5)), "reserved": dict(descs=with_image(0, reserved=1)),
           "stream_outside": dict(descs=with_image(2, stream_bytes=int(descs[2].stream_bytes) + 17)), "stream_offset": dict(descs=with_image(1, stream_offset=s_off + 1)),
           "bytes_outside": dict(cap_b=o_off - 16), "planes_outside": dict(descs=with_image(2, planes_offset=o_off)),
           "huge_scan": dict(descs=with_image(0, width=65535, height=65535, channels=4))}
    for name, over in bad.items():
        kw = dict(n=n, descs=descs, streams=streams, nstream=s_off, out_b=ob, cap_b=o_off, out_p=op, cap_p=o_off, status=st, ws=ws, ws_bytes=need)
        kw.update(over)
        rc, msg = _call(R, **kw)
        res["err_" + name] = np.array("%d %s" % (rc, msg))
    res["err_poison"] = np.array(bool(all((down(t) == 0xA5).all() for t in (ws, ob, op, st))))
    res["err_queries"] = np.array([int(R.lib.gof_png_decode_ws_bytes(-1, descs, 0)), int(R.lib.gof_png_decode_ws_bytes(65536, descs, 0)),
                                   int(R.lib.gof_png_decode_ws_bytes(1, None, 0)), int(R.lib.gof_png_decode_ws_bytes(n, with_image(1, channels=0), 0))])
    rc, _ = _call(R, 0, None, None, 0, None, 0, None, 0, None, None, 0)
    res["empty_rc"] = np.array(rc)
    _ = C
    return res


def check_entry(res):
    need, need_ws_bytes, need1, need2, need0, abi, enc_abi, main_abi = (int(v) for v in res["need"])
    assert abi == 1 and enc_abi == 1 and main_abi == 12, "the encoder's and the library's ABI versions do not move"
    assert 0 < need0 <= need1 < need2 < need < need_ws_bytes, "gof_png_decode_ws_bytes is monotone"
    want_b, want_p = None, None
    for fill in FILLS:
        assert int(res["fill%02x_rc" % fill]) == 0 and not res["fill%02x_status" % fill].any()
        assert bool(res["fill%02x_tails" % fill]), "bytes behind a buffer were written (fill 0x%02X)" % fill
        b, p = res["fill%02x_bytes" % fill], res["fill%02x_planes" % fill]
        got_b = np.concatenate([b[o:o + n] for o, n in res["offsets"]])
        got_p = np.concatenate([p[4 * o:4 * (o + n)] for o, n in res["offsets"]])
        if want_b is None:
            want_b, want_p = got_b, got_p
        assert np.array_equal(got_b, want_b) and np.array_equal(got_p, want_p), "a workspace filled with 0x%02X changes the output" % fill
    at = 0
    for i, (o, n) in enumerate(res["offsets"]):
        f = res["entry_file_%d" % i].tobytes()
        w, h, c = header(f)
        px = unfilter(zlib.decompress(idat_of(f)), h, w, c)
        assert np.array_equal(want_b[at:at + n], px.reshape(-1))
        assert np.array_equal(want_p[4 * at:4 * (at + n)].view(np.uint32), to_tensor(px).numpy().reshape(-1).view(np.uint32))
        at += n
    table = (("negative_n", -1, "images"), ("too_many", -1, "images"), ("null_images", -1, "NULL"), ("null_streams", -1, "NULL"), ("null_status", -1, "NULL"),
             ("null_ws", -1, "NULL"), ("no_output", -1, "both NULL"), ("odd_ws", -1, "aligned"), ("odd_planes", -1, "aligned"), ("small_ws", -2, "workspace"),
             ("zero_w", -1, "image 1"), ("huge_h", -1, "image 0"), ("five_channels", -1, "image 2"), ("reserved", -1, "reserved"), ("stream_outside", -1, "stream"),
             ("stream_offset", -1, "stream"), ("bytes_outside", -1, "out_bytes"), ("planes_outside", -1, "out_planes"), ("huge_scan", -1, "image 0"))
    for name, code, text in table:
        got = str(res["err_" + name])
        assert got.startswith("%d " % code) and text in got, (name, got)
    assert bool(res["err_poison"]), "a refused call wrote to an output, the workspace or the status words"
    assert list(res["err_queries"]) == [0, 0, 0, 0] and int(res["empty_rc"]) == 0
