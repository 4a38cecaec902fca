/*
 * gof_appearance_hip.h -- C ABI of the decoupled-appearance L1 in libgof_hip.so (csrc/appearance.hip): what the
 * reference's train.py:67-88 (L1_loss_appearance) and scene/appearance_network.py ask of torch -- centre crop to multiples of 32,
 * bilinear down-sample by 32, a per-camera embedding as constant planes, seven 3x3 convolutions with four pixel-shuffles and one
 * bilinear x2 up-sample between them, a sigmoid, the product with the rendering and the L1 against the ground truth -- forward AND
 * backward.  Tensors are fp32, planar ([channel][y][x]); one image per call.
 *
 * THE ORDER OF EVERY SUM IS PART OF THE CONTRACT (no floating-point atomics; results are bit-reproducible):
 *
 *   convolution (forward and data gradient), on v_mfma_f32_32x32x2_f32 exactly as gof_lpips_conv3x3 (gof_lpips_hip.h):
 *       out = fl(fmaf(x_{K-1}, w_{K-1}, ... fmaf(x_0, w_0, 0) ...) + bias),   k = ci * 9 + ky * 3 + kx,   K = 9 C_in
 *     a tap outside the image is the term x = 0; without a bias the chain is the result.  Any C_in, C_out in [1, GOF_APP_MAX_CHANNELS]:
 *     output channels that do not fill a tile of 32 are staged as zero weight rows and not stored, an odd K is padded with one term
 *     0 * 0 (non-finite-safe only in the sense gof_lpips_hip.h states: a zero row times a non-finite x is not stored anywhere).
 *     The data gradient is this convolution with the weight W'[ci][co][ky][kx] = W[co][ci][2 - ky][2 - kx] (gof_app_weight_transpose)
 *     on dY' = (Y > 0 ? dY : 0) where the layer had a ReLU (a masked term is x = 0): k = co * 9 + ky * 3 + kx, no bias.
 *
 *   THE OPERAND x IS READ THROUGH A VIEW (GOF_APP_SRC_*), never materialised:
 *       PLAIN      x[c][y][x]                       = src[c][y][x]
 *       SHUFFLE    x[c][y][x]                       = src[4 c + 2 (y & 1) + (x & 1)][y / 2][x / 2]          (nn.PixelShuffle(2))
 *       UNSHUFFLE  x[c][y][x]                       = src[c / 4][2 y + ((c >> 1) & 1)][2 x + (c & 1)]       (its inverse: the gradient)
 *       UP2        x[c][y][x], plane (H, W)         = bilinear(src[c], plane (H / 2, W / 2)), align_corners=True (formula below)
 *       EMBED      x[c][y][x]                       = c < 3 ? src[c][y][x] : emb[c - 3]                      (constant planes)
 *     each optionally masked by `mask` [C][H][W]: value = mask > 0 ? value : 0.  gof_app_materialize writes exactly the values the
 *     convolutions stage, so a fused view and the materialised tensor give the same bits.
 *
 *   bilinear, align_corners=True (torch's formula, fp32): scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0;  s = scale * dst;
 *       i0 = (int)s (at most in - 1);  i1 = i0 + (i0 < in - 1);  l1 = s - i0;  l0 = 1 - l1;
 *       value = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d),   a, b, c, d = src[i0h][i0w], [i0h][i1w], [i1h][i0w], [i1h][i1w]
 *     its transpose (gof_app_up2_backward, and the down-sample's inside gof_app_l1_backward) is a GATHER: a source pixel adds
 *     (lh * lw) * g for every destination pixel whose footprint holds it, destination pixels in ascending (y, x), per destination the
 *     corners in the order a, b, c, d, plain fp32 additions starting from 0 (the down-sample's: from the product term g * m).
 *
 *   weight and bias gradient: dW[co][ci][ky][kx] = sum_p dY'[co][p] X[ci][p + (ky - 1, kx - 1)],  db[co] = sum_p dY'[co][p] * 1.
 *     The pixels p = y * W + x of the plane are cut into chunks of GOF_APP_WGRAD_CHUNK (the unit of parallelism) and every chunk into
 *     sub-chains of GOF_APP_WGRAD_SUB pixels.  A sub-chain is ONE fp32 fmaf chain in ascending p on the matrix instruction, started
 *     from 0 (M = co, N = 9 ci + the bias column, K = pixels; a ragged end is padded with terms 0 * 0).  The sub-chain results are
 *     added in ascending order to an fp64 accumulator, from 0; the chunk partials lie in the workspace as fp64 and are summed in
 *     ascending chunk order in fp64, starting from chunk 0's; ONE rounding to fp32 at the end.  The result lies inside
 *     (CHUNK + n_chunks + 2) 2^-24 sum |dY' X|, the bound of one fp32 chain over the chunk, with room to spare.
 *
 *   the ends: m = 1 / (1 + exp(-z)) (the library's deterministic fp32 exp), t = m * I, loss = (sum |t - G|) / (3 H W): the fp32
 *     elements |t - G| are summed IN fp64, in conv3's epilogue: per workgroup of 256 consecutive pixels of the crop the three channels
 *     of a pixel are added in channel order, then the pixels in a fixed tree (strides 128, 64 .. 1 over the pixel's index in the
 *     workgroup), then one workgroup sums the partials (per thread those at t, t + 256, .. in
 *     ascending order, then the same tree), then ONE fp64 division and ONE rounding to fp32.  Backward: k = dL / (3 H W); g = sign(t - G) * k; dI = g * m;
 *     dz = ((g * I) * m) * (1 - m).  dE[c] = sum over the low-resolution pixels in ascending p of dX1[3 + c][p], plain additions from 0.
 *
 * Conventions as in gof_lpips_hip.h / gof_train_hip.h: extern "C", device pointers unless the name ends in `_host`, caller-owned
 * buffers, asynchronous on `stream` (a hipStream_t passed as void*), 0 = ok / negative GOF_E_* with text in gof_last_error().
 * The contents of a workspace do not matter on entry.
 */
#ifndef GOF_APPEARANCE_HIP_H_INCLUDED
#define GOF_APPEARANCE_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOF_APP_MAX_CHANNELS 4096
#define GOF_APP_WGRAD_CHUNK 4096          /* pixels per chunk of the weight gradient: 1056 x 1600 is 413 chunks */
#define GOF_APP_WGRAD_SUB 16              /* pixels per fp32 sub-chain inside a chunk (divides the chunk and the kernel's stage of 64)   */
#define GOF_APP_N_PARAMS 14

#define GOF_APP_SRC_PLAIN 0
#define GOF_APP_SRC_SHUFFLE 1
#define GOF_APP_SRC_UNSHUFFLE 2
#define GOF_APP_SRC_UP2 3
#define GOF_APP_SRC_EMBED 4

/* The network as data: scene/appearance_network.py is { 64, { 256, 128, 64, 32, 16, 16 } }. */
typedef struct GofAppNet {
    int32_t n_embed;       /* values of the per-camera embedding: conv1 takes 3 + n_embed channels                                  */
    int32_t width[6];      /* output channels of conv1, up1.conv .. up4.conv (the first four: multiples of 4) and conv2; conv3: 3  */
} GofAppNet;

/* ---- the pieces (what the tests hold alone; the two entry points below run the same kernels) ---------------------------------- */
/* out [c_out][H][W] = conv3x3(view of x, weight [c_out][c_in][3][3], zero padding 1) (+ bias [c_out] unless NULL), max(., 0) where
 * relu != 0.  (W, H): the plane of the VIEW; x is stored as the view's mode says; emb: [c_in - 3] for EMBED; mask: NULL or
 * [c_in][H][W].  SHUFFLE needs even W, H; UNSHUFFLE c_in % 4 == 0; UP2 even W, H.  out must not overlap x. */
int gof_app_conv3x3(int32_t c_in, int32_t c_out, int32_t W, int32_t H, const float* x, int32_t x_mode, const float* emb, const float* mask,
                    const float* weight, const float* bias, int32_t relu, float* out, void* stream);
/* out [C][H][W] = the view itself. */
int gof_app_materialize(int32_t mode, int32_t C, int32_t W, int32_t H, const float* x, const float* emb, const float* mask, float* out, void* stream);
/* out [c_in][c_out][3][3] = weight[co][ci][2 - ky][2 - kx] */
int gof_app_weight_transpose(int32_t c_in, int32_t c_out, const float* weight, float* out, void* stream);
/* dW [c_out][c_in][3][3], db [c_out] from the view of x ([c_in][H][W]) and the view of dy ([c_out][H][W], masked by `mask`
 * [c_out][H][W] unless NULL). */
size_t gof_app_wgrad_workspace_bytes(int32_t c_in, int32_t c_out, int32_t W, int32_t H);
int gof_app_conv3x3_wgrad(int32_t c_in, int32_t c_out, int32_t W, int32_t H, const float* x, int32_t x_mode, const float* emb,
                          const float* dy, int32_t dy_mode, const float* mask, float* dW, float* db, void* ws, size_t ws_bytes, void* stream);
/* out [C][out_H][out_W] = bilinear(x, align_corners=True); plane c of x starts at x + c * in_plane_stride, its rows are in_row_stride
 * floats apart (a crop of a larger image is a view). */
int gof_app_bilinear(int32_t C, int32_t in_W, int32_t in_H, int64_t in_row_stride, int64_t in_plane_stride, const float* x,
                     int32_t out_W, int32_t out_H, float* out, void* stream);
/* out [C][H][W] = the transpose of the x2 up-sample applied to g [C][2 H][2 W] (a gather, order above). */
int gof_app_up2_backward(int32_t C, int32_t W, int32_t H, const float* g, float* out, void* stream);

/* The ends, on stored tensors ((W, H): the image; the crop as below).  In gof_app_l1_forward / _backward the same arithmetic runs inside
 * conv3's epilogue (z is never stored) and while conv3's gradient kernels stage their operand (dz is never stored).
 * head_forward: z [3][Hc][Wc] -> m_out = sigmoid(z), transformed (nullable) = m * crop(image), loss = mean |m I - G|.
 * head_backward: m [3][Hc][Wc], dL (1 float) -> dz [3][Hc][Wc].
 * image_grad: d_image [3][H][W] = 0 outside the crop, inside g * m + the transpose of the down-sample applied to d_down [3][Hc/32][Wc/32]. */
size_t gof_app_head_workspace_bytes(int32_t W, int32_t H);
int gof_app_head_forward(int32_t W, int32_t H, const float* z, const float* image, const float* gt, float* m_out, float* transformed, float* loss,
                         void* ws, size_t ws_bytes, void* stream);
int gof_app_head_backward(int32_t W, int32_t H, const float* m, const float* image, const float* gt, const float* dL, float* dz, void* stream);
int gof_app_image_grad(int32_t W, int32_t H, const float* m, const float* image, const float* gt, const float* dL, const float* d_down,
                       float* d_image, void* stream);

/* ---- the loss ------------------------------------------------------------------------------------------------------------------ */
/* (W, H): the image as train.py has it; the crop is (H / 32 * 32, W / 32 * 32) at top = H / 2 - Hc / 2, left = W / 2 - Wc / 2. */
size_t gof_app_saved_bytes(int32_t W, int32_t H, const GofAppNet* net_host);
size_t gof_app_workspace_bytes(int32_t W, int32_t H, const GofAppNet* net_host);
/* image, gt [3][H][W]; embedding [n_embed]; params_host: GOF_APP_N_PARAMS DEVICE pointers in a host array: weight, bias of conv1,
 * up1.conv .. up4.conv, conv2, conv3.  loss (1 float) = mean |sigmoid(net) * crop(image) - crop(gt)|; transformed (nullable,
 * [3][Hc][Wc]) = sigmoid(net) * crop(image).  saved: what gof_app_l1_backward reads (the low-resolution image, the six ReLU outputs,
 * the sigmoid).  Refused with GOF_E_INVALID: W or H < 32, a width that does not fit, an output that overlaps an input. */
int gof_app_l1_forward(int32_t W, int32_t H, const GofAppNet* net_host, const float* image, const float* gt, const float* embedding,
                       const float* const* params_host, float* loss, float* transformed, void* saved, size_t saved_bytes,
                       void* ws, size_t ws_bytes, void* stream);
/* dL (1 float) in; d_image [3][H][W] (zero outside the crop), d_embedding [n_embed] and d_params_host (GOF_APP_N_PARAMS DEVICE
 * pointers, shapes of params_host) out.  image, gt, embedding, params_host, saved: as given to / left by the forward. */
int gof_app_l1_backward(int32_t W, int32_t H, const GofAppNet* net_host, const float* image, const float* gt, const float* embedding,
                        const float* const* params_host, const float* dL, const void* saved, size_t saved_bytes,
                        float* d_image, float* d_embedding, float* const* d_params_host, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
