/*
 * gof_png_read_hip.h -- C ABI of the PNG decoder in libgof_hip.so.
 *
 * What metrics.py:25-36 (readImages) does per file with Pillow (inflate and unfilter on one CPU thread), to_tensor (/ 255) and an upload
 * from pageable memory: the zlib streams of a batch of 8-bit, non-interlaced PNG files -> interleaved bytes and float32 planes, on the
 * device.  The host reads the files, checks the chunks' CRCs and concatenates the IDAT payloads (png_reader.py); gof_png_hip.h is the
 * encoder and does not move with this header.
 *
 * Conventions as in gof_hip.h: extern "C", device pointers, a caller-owned workspace sized by a host-only query whose contents do not
 * matter on entry, launches on `stream`, 0 = ok, negative = GOF_E_* with text in gof_last_error().  Nothing is launched or written where
 * the return code is not 0.  The same input gives the same bytes on every call and every stream.
 *
 * Three launches over the whole batch:
 *   inflate   one workgroup per stream.  zlib header (CM = 8, CINFO <= 7, no FDICT, FCHECK); stored, fixed and dynamic blocks; the
 *             scanline bytes height * (width * channels + 1) go to the workspace; their Adler-32 is compared with the trailer.  No read
 *             leaves [stream, stream + length), no write leaves the image's scanline buffer, every loop is bounded by the two sizes.
 *   unfilter  one wave per image, 64 rows at a time, lane k one pixel behind lane k - 1; the five PNG filters; interleaved bytes.
 *   convert   bytes -> planes, (float)b / 255.0f with a correctly rounded division (what to_tensor's .to(float32).div(255) gives).
 * A stream that does not decode fails its own image only: its status word says why, its outputs are not defined, the other images of
 * the batch are not touched by it.
 */
#ifndef GOF_PNG_READ_HIP_H_INCLUDED
#define GOF_PNG_READ_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOF_PNG_READ_ABI_VERSION 1
/* the version of THIS header's entry points (gof_abi_version() of gof_hip.h and gof_png_abi_version() do not move with them) */
int gof_png_read_abi_version(void);

#define GOF_PNG_READ_MAX_DIM 65535              /* the largest width or height */
#define GOF_PNG_READ_MAX_BYTES 0x7FFFFFFFll     /* the largest height * (width * channels + 1), and the largest zlib stream */
#define GOF_PNG_READ_MAX_IMAGES 65535           /* images per call */

/* the status word of an image */
#define GOF_PNG_READ_OK 0
#define GOF_PNG_READ_E_ZLIB_HEADER 1            /* CM != 8, CINFO > 7, FDICT set or FCHECK wrong */
#define GOF_PNG_READ_E_TRUNCATED 2              /* the stream ends inside a block or in front of the Adler-32 */
#define GOF_PNG_READ_E_BLOCK_TYPE 3             /* block type 3 */
#define GOF_PNG_READ_E_STORED 4                 /* a stored block whose NLEN is not ~LEN */
#define GOF_PNG_READ_E_CODE_LENGTHS 5           /* HLIT > 286, HDIST > 30, a repeat with nothing to repeat or past the end, an
                                                   over-subscribed or incomplete code, no end-of-block code */
#define GOF_PNG_READ_E_SYMBOL 6                 /* bits that are no code of the block, or the symbols 286, 287 / 30, 31 */
#define GOF_PNG_READ_E_DISTANCE 7               /* a match that starts in front of the output */
#define GOF_PNG_READ_E_LONG 8                   /* more than height * (width * channels + 1) bytes */
#define GOF_PNG_READ_E_SHORT 9                  /* the last block ends with fewer */
#define GOF_PNG_READ_E_ADLER 10                 /* the Adler-32 of the output is not the trailer's */
#define GOF_PNG_READ_E_FILTER 11                /* a filter byte > 4 */

typedef struct GofPngImage {
    int32_t width, height;                      /* 1..GOF_PNG_READ_MAX_DIM, height * (width * channels + 1) <= GOF_PNG_READ_MAX_BYTES */
    int32_t channels;                           /* 1, 2, 3 or 4 samples of 8 bits per pixel */
    int32_t reserved;                           /* 0 */
    uint64_t stream_offset, stream_bytes;       /* the image's zlib stream inside `streams` (the concatenated IDAT payloads) */
    uint64_t bytes_offset;                      /* bytes from out_bytes to the image's [height][width][channels] uint8 */
    uint64_t planes_offset;                     /* floats from out_planes to the image's [channels][height][width] float32 */
} GofPngImage;

/* Workspace: the device copy of the descriptors, every image's scanline bytes and, where bytes_in_workspace != 0 (out_bytes will be
 * NULL), every image's interleaved bytes.  0 where n < 0, n > GOF_PNG_READ_MAX_IMAGES, images is NULL with n > 0 or an image is outside
 * the limits above.  Monotone in n for a prefix of the same images. */
size_t gof_png_decode_ws_bytes(int32_t n, const GofPngImage* images, int32_t bytes_in_workspace);

/* images: n descriptors in HOST memory (copied before the call returns); streams: streams_bytes bytes on the device; out_bytes:
 * out_bytes_capacity bytes or NULL; out_planes: out_planes_capacity floats or NULL (not both NULL); status: n words on the device, one
 * GOF_PNG_READ_* per image.  n == 0 returns 0 and launches nothing.
 * GOF_E_INVALID: n outside 0..GOF_PNG_READ_MAX_IMAGES, a NULL pointer, an image outside the limits above, reserved != 0, a stream
 * outside [0, streams_bytes) or of more than GOF_PNG_READ_MAX_BYTES (a stream that is too short is its image's
 * GOF_PNG_READ_E_TRUNCATED, not an argument error), an output outside its capacity, a workspace that is not 16-byte aligned, planes or
 * status not 4-byte aligned; GOF_E_WORKSPACE: ws_bytes < gof_png_decode_ws_bytes(n, images, out_bytes == NULL). */
int gof_png_decode_batch(int32_t n, const GofPngImage* images, const void* streams, size_t streams_bytes, void* out_bytes,
                         size_t out_bytes_capacity, float* out_planes, size_t out_planes_capacity, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
