/*
 * gof_png_hip.h -- C ABI of the PNG encoder in libgof_hip.so.
 *
 * What torchvision.utils.save_image (render.py:35-36) does with mul(255).add_(0.5).clamp_(0, 255), a blocking copy to the host and
 * Pillow's encoder on one CPU thread: float32 planes -> the finished zlib stream of an 8-bit RGB PNG, on the device.  The host frames
 * the stream (signature, IHDR, IDAT, IEND and their CRCs) and writes the file.
 *
 * Conventions as in gof_hip.h: extern "C", device pointers, a caller-owned workspace sized by a query whose contents do not matter on
 * entry, launches on `stream`, 0 = ok, negative = GOF_E_* with text in gof_last_error().  Nothing is launched or written where the
 * return code is not 0.  The same input gives the same bytes on every call and every stream.
 *
 * The stream, in the order it is made:
 *   byte     b = (uint8)clamp(x * 255.0f + 0.5f, 0, 255), the product and the sum rounded separately (what torch's CPU kernels give);
 *            NaN -> 0 (torch 2.x on x86-64: clamp_ keeps the NaN and the conversion to uint8 gives 0), +inf -> 255, -inf -> 0.
 *            channels == 1 is written as three equal channels.
 *   scanline one filter byte, then 3 W filtered bytes (bpp = 3).  The five filters None, Sub, Up, Average, Paeth are formed against the
 *            unfiltered previous row (row 0: zeros); the one whose filtered bytes, read as signed, have the smallest sum of absolute
 *            values is taken, the lowest filter number on a tie.
 *   deflate  the scanline bytes are cut into input blocks of GOF_PNG_BLOCK_BYTES; each becomes one dynamic-Huffman block whose tokens
 *            are literals and matches of distance 1 and length 3..258 (zlib's Z_RLE, greedy, restarted at every input block), with
 *            optimal length-limited codes (15 bits; 7 bits for the code-length alphabet, whose symbols 16/17/18 are not used), or a
 *            stored block where that is smaller.  A dynamic block that is not the last is followed by an empty stored block
 *            (00 00 FF FF behind the padding), so every block starts on a byte boundary; the last block carries BFINAL.
 *   zlib     78 9C, the blocks, Adler-32 of the scanline bytes (big endian).
 */
#ifndef GOF_PNG_HIP_H_INCLUDED
#define GOF_PNG_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOF_PNG_ABI_VERSION 1
/* the version of THIS header's entry points (gof_abi_version() of gof_hip.h does not move with them) */
int gof_png_abi_version(void);

#define GOF_PNG_MAX_DIM 65535                   /* the largest width or height */
#define GOF_PNG_MAX_STREAM 0x7FFFFFFFll         /* the largest height * (3 width + 1): the scanline bytes of one image */
#define GOF_PNG_BLOCK_BYTES 16384               /* scanline bytes per deflate block */
/* GOF_PNG_BLOCK_BYTES as the library was compiled */
int32_t gof_png_block_bytes(void);

typedef struct GofPngEncode {
    int32_t width, height;                      /* 1..GOF_PNG_MAX_DIM, height * (3 width + 1) <= GOF_PNG_MAX_STREAM */
    int32_t channels;                           /* 1 or 3 planes are read */
    int32_t reserved;                           /* 0 */
    int64_t plane_stride;                       /* floats from one plane to the next, >= width * height (ignored for 1 channel) */
} GofPngEncode;

/* Workspace: the scanline bytes, one slot per deflate block, the blocks' sizes, offsets and Adler-32 partial sums, scan scratch.
 * 0 for a size the encoder refuses. */
size_t gof_png_ws_bytes(int32_t width, int32_t height);

/* The largest stream gof_png_encode can produce for this size: every block stored (5 bytes of header each) + 2 + 4 bytes of zlib
 * framing = height * (3 width + 1) + 5 * blocks + 6.  0 for a size the encoder refuses. */
size_t gof_png_max_bytes(int32_t width, int32_t height);

/* planes: float32 [channels][height][width], rows contiguous, planes plane_stride floats apart; out: out_capacity bytes (any
 * alignment) that receive the zlib stream; out_size_dev: 8-byte aligned, receives the stream's length.  Bytes of `out` behind
 * that length are not defined.
 * GOF_E_INVALID: a size outside the limits above, channels not 1 or 3, plane_stride < width * height (3 channels), a NULL pointer, a
 * workspace that is not 16-byte aligned, out_size_dev not 8-byte aligned, out_capacity < gof_png_max_bytes(width, height);
 * GOF_E_WORKSPACE: ws_bytes < gof_png_ws_bytes(width, height). */
int gof_png_encode(const GofPngEncode* args, const float* planes, void* out, size_t out_capacity, uint64_t* out_size_dev, void* ws,
                   size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
