/*
 * gof_image_hip.h -- C ABI of the training-image resampler in libgof_hip.so.
 *
 * What the reference's loadCam (utils/camera_utils.py:19-54, utils/general_utils.py:21-27) does on one CPU thread per camera with
 * Pillow's Image.resize, np.array, a division by 255.0 and a permute: the bicubic resampling of an interleaved 8-bit image and its
 * conversion to float32 planes, on the device, bit for bit.
 *
 * Conventions as in gof_hip.h: extern "C", device pointers (unless a parameter says HOST), a caller-owned workspace sized by a query
 * whose contents do not matter on entry, launches on `stream`, 0 = ok, negative = GOF_E_* with text in gof_last_error().  Every
 * element of the output is written by the call; nothing is launched or written where the return code is not 0.
 *
 * The resampler is Pillow's ImagingResample for 8-bit bands with the bicubic filter (a = -0.5), the default of Image.resize for the
 * modes L and RGB.  Per axis (n_in -> n_out), computed on the host in double with no fused multiply-add:
 *   scale = n_in / n_out, filterscale = max(scale, 1), support = 2 filterscale, taps = 2 ceil(support) + 1
 *   output i: center = (i + 0.5) scale, first = max(0, (int)(center - support + 0.5)),
 *             count = min(n_in, (int)(center + support + 0.5)) - first,
 *             w_j = bicubic((j + first - center + 0.5) * (1 / filterscale)), normalised by their sum taken left to right,
 *             k_j = (int)(0.5 + w_j 2^22) for w_j >= 0, (int)(-0.5 + w_j 2^22) otherwise.
 * A pass gives clamp((2^21 + sum_j pixel_j k_j) >> 22, 0, 255) in 32-bit integers (no overflow: sum |k_j| 255 < 2^31, so the order
 * of the sum does not matter).  The horizontal pass runs first and is rounded to 8 bits before the vertical pass reads it; a pass whose
 * length does not change is the identity.  The last step stores byte b as the float32 nearest to b / 255 (what torch's
 * uint8_tensor / 255.0 gives on the CPU) into planes [channels][out_h][out_w].  Channels are independent: no alpha premultiplication.
 */
#ifndef GOF_IMAGE_HIP_H_INCLUDED
#define GOF_IMAGE_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOF_IMAGE_ABI_VERSION 1
/* the version of THIS header's entry points (gof_abi_version() of gof_hip.h does not move with them) */
int gof_image_abi_version(void);

#define GOF_IMAGE_MAX_DIM 65535                 /* the largest width or height, input or output */

typedef struct GofImageResize {
    int32_t in_w, in_h;                         /* source size in pixels, 1..GOF_IMAGE_MAX_DIM */
    int32_t channels;                           /* 1, 3 or 4, interleaved */
    int32_t out_w, out_h;                       /* output size in pixels, 1..GOF_IMAGE_MAX_DIM */
    int32_t reserved;                           /* 0 */
    int64_t pitch;                              /* bytes from one source row to the next, >= in_w * channels */
} GofImageResize;

/* ---- coefficient tables (HOST only: no device call, usable without a device) -------------------------------------------------------
 * taps per output of the axis n_in -> n_out (= the row length of `coeffs`), -1 for a length outside 1..GOF_IMAGE_MAX_DIM */
int64_t gof_image_taps(int32_t n_in, int32_t n_out);
/* bounds (HOST, [n_out][2]): first input index and count per output; coeffs (HOST, [n_out][taps]): the integer weights, 0 behind the
 * count.  An axis with n_in == n_out gets the tables of the formulas above like any other (the resize entry does not use them). */
int gof_image_coeffs(int32_t n_in, int32_t n_out, int32_t* bounds, int32_t* coeffs);

/* ---- resize ---------------------------------------------------------------------------------------------------------------------------
 * Workspace: the two axes' tables and the 8-bit image between the passes; 0 for arguments the resize entry refuses. */
size_t gof_image_resize_ws_bytes(const GofImageResize* args);

/* src: in_h rows of `pitch` bytes, in_w * channels of them used (any alignment); out: float32 [channels][out_h][out_w].
 * GOF_E_INVALID: a size of 0 or above GOF_IMAGE_MAX_DIM, channels not in {1, 3, 4}, pitch < in_w * channels, a NULL pointer, a workspace
 * that is not 16-byte aligned;
 * GOF_E_WORKSPACE: ws_bytes < gof_image_resize_ws_bytes(args).  Nothing outside src[0, (in_h - 1) * pitch + in_w * channels) is read.
 * The tables of an axis are computed once per (n_in, n_out) and kept in page-locked host memory by the library (thread-safe); the
 * call copies them into the workspace on `stream` in front of its kernels. */
int gof_image_resize(const GofImageResize* args, const void* src, float* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
