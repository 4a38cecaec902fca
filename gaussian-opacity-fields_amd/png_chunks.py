"""The PNG container, for the writer (image_writer.py) and the reader (png_reader.py): the signature and the chunk framing -- length,
kind, data, CRC-32 over kind and data -- written by `chunk` and walked, with every length and CRC-32 checked, by `walk`."""
import struct
import zlib

__all__ = ["SIGNATURE", "chunk", "walk"]

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _crc(kind, data):
    return zlib.crc32(data, zlib.crc32(kind)) & 0xFFFFFFFF


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", _crc(kind, data))


def _bad(why):
    return ValueError("png_chunks: " + why)


def walk(data, bad=_bad):
    """the file's bytes -> (kind, data as a view of the file's bytes) per chunk, in file order, up to the end of the bytes (the caller
    stops at IEND).  A wrong signature, a chunk that is cut off or fails its CRC-32: raises bad(why)."""
    data = memoryview(data)
    if bytes(data[:8]) != SIGNATURE:
        raise bad("not a PNG file (signature)")
    off = 8
    while off < len(data):
        if off + 12 > len(data):
            raise bad("a chunk header is cut off at byte %d" % off)
        n, kind = struct.unpack(">I4s", data[off:off + 8])
        if off + 12 + n > len(data):
            raise bad("chunk %r at byte %d claims %d bytes, the file ends before them" % (kind, off, n))
        body = data[off + 8:off + 8 + n]
        if struct.unpack(">I", data[off + 8 + n:off + 12 + n])[0] != _crc(kind, body):
            raise bad("chunk %r at byte %d fails its CRC-32" % (kind, off))
        yield kind, body
        off += 12 + n
