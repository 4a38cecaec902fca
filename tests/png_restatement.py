"""The PNG container and the five PNG filters restated for the tests of the encoder and the decoder (tests/png_encode_cases.py,
tests/png_decode_cases.py): one restatement, written from the specification and independent of the product -- it imports nothing of
png_chunks, image_writer or png_reader, so that an oracle never shares code with what it checks."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CTYPE = {1: 0, 2: 4, 3: 2, 4: 6}                # samples per pixel -> colour type


# ---- framing -------------------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def chunks(png):
    """[(kind, data)] of a PNG file, every CRC checked"""
    assert png[:8] == SIGNATURE
    off, out = 8, []
    while off < len(png):
        n, kind = struct.unpack(">I4s", png[off:off + 8])
        data = png[off + 8:off + 8 + n]
        assert struct.unpack(">I", png[off + 8 + n:off + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF, kind
        out.append((kind, data))
        off += 12 + n
    assert off == len(png)
    return out


def frame(w, h, c, stream, idat=None, before=(), after=(), depth=8, ctype=None, interlace=0):
    """the file around a zlib stream; idat: bytes per IDAT chunk (None: one chunk); before / after: ancillary chunks around the IDATs"""
    parts = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, CTYPE[c] if ctype is None else ctype, 0, 0, interlace))]
    parts += [chunk(k, d) for k, d in before]
    per = len(stream) if idat is None else idat
    parts += [chunk(b"IDAT", stream[o:o + per]) for o in range(0, max(1, len(stream)), max(1, per))]
    parts += [chunk(k, d) for k, d in after]
    return b"".join(parts + [chunk(b"IEND", b"")])


def idat_of(png):
    """the zlib stream: the concatenated IDAT payloads"""
    return b"".join(d for k, d in chunks(png) if k == b"IDAT")


def header(png):
    """-> (width, height, samples per pixel)"""
    w, h, depth, ctype, _, _, lace = struct.unpack(">IIBBBBB", chunks(png)[0][1])
    return w, h, {t: c for c, t in CTYPE.items()}[ctype]


# ---- filters -------------------------------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    """a = left, b = up, c = up-left (arrays or single values): the one nearest to a + b - c, ties to a, then b"""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filtered_rows(px):
    """(H, W, C) uint8 -> (H, 5, W C) uint8: every row under None, Sub, Up, Average and Paeth, against the unfiltered previous row (zeros
    above row 0)"""
    H, W, C = px.shape
    rows = px.reshape(H, W * C).astype(np.int32)
    out = np.zeros((H, 5, W * C), np.uint8)
    prev = np.zeros(W * C, np.int32)
    for y in range(H):
        cur = rows[y]
        a = np.concatenate([np.zeros(C, np.int32), cur[:-C]])
        c = np.concatenate([np.zeros(C, np.int32), prev[:-C]])
        for k, pred in enumerate((0 * cur, a, prev, (a + prev) >> 1, paeth(a, prev, c))):
            out[y, k] = (cur - pred) & 255
        prev = cur
    return out


def filter_rows(px, filters):
    """(H, W, C) uint8, one filter type per row -> the scanline bytes"""
    cands = filtered_rows(px)
    kinds = np.asarray(filters, np.uint8).reshape(-1, 1)
    return np.concatenate([kinds, cands[np.arange(len(cands)), kinds[:, 0]]], axis=1).tobytes()
