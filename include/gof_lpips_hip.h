/*
 * gof_lpips_hip.h -- C ABI of the LPIPS perceptual metric in libgof_hip.so (csrc/lpips.hip): what the reference's
 * metrics.py:19,76,100 asks of the `lpips` pip package (`lpips.LPIPS(net='vgg')`, a torchvision VGG16 through MIOpen convolutions).
 *
 * The network is DATA: a host array of layer descriptors and device pointers to the weights.  LPIPS-VGG is the instance
 *     3->64->64 | pool | 128->128 | pool | 256 x3 | pool | 512 x3 | pool | 512 x3,   taps after the 2nd, 4th, 7th, 10th and 13th layer.
 * Every layer is a 3x3 convolution with zero padding 1, bias and ReLU, computed as an implicit GEMM on the exact fp32 matrix
 * instruction of gfx950 (v_mfma_f32_32x32x2_f32): M = the pixels of both images, N = C_out, K = 9 C_in.
 *
 * THE ORDER OF K IS PART OF THE CONTRACT: k = ci * 9 + ky * 3 + kx, torch's own flattening of a [C_out, C_in, 3, 3] weight, and
 *     out = fl(fmaf(x_{K-1}, w_{K-1}, ... fmaf(x_1, w_1, fmaf(x_0, w_0, 0)) ...) + bias)
 * one fp32 fused multiply-add per term in ascending k (a tap outside the image is the term x = 0), then ONE fp32 addition of the bias.
 * An odd K (C_in = 3: K = 27) is padded with one term 0 * 0 at the end of the chain, which changes no bit of a finite result.
 *
 * Channel counts: C_in in [1, GOF_LPIPS_MAX_CHANNELS], C_out a multiple of 32 in [32, GOF_LPIPS_MAX_CHANNELS]; anything else is refused
 * with GOF_E_INVALID.  Tensors are fp32, planar ([image][channel][y][x], torch's contiguous NCHW).
 *
 * Conventions as in gof_train_hip.h: extern "C", device pointers unless the name ends in `_host`, caller-owned buffers, asynchronous
 * on `stream` (a hipStream_t passed as void*), 0 = ok / negative GOF_E_* with text in gof_last_error().  The contents of the
 * workspace do not matter on entry.  No floating-point atomics: every sum has a fixed order, results are bit-reproducible.
 */
#ifndef GOF_LPIPS_HIP_H_INCLUDED
#define GOF_LPIPS_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOF_LPIPS_MAX_LAYERS 64
#define GOF_LPIPS_MAX_CHANNELS 4096

typedef struct GofLpipsLayer {
    int32_t c_in;          /* input channels of the 3x3 convolution (the first layer's: 3, the scaled image)                      */
    int32_t c_out;         /* output channels: a multiple of 32                                                                  */
    int32_t pool_before;   /* != 0: a 2x2 max-pool with stride 2 (flooring: an odd last row / column is dropped) in front of it  */
    int32_t tap_after;     /* != 0: the ReLU output of this layer is a tap (lin weights [c_out])                                 */
} GofLpipsLayer;

/* ---- the pieces (what the tests hold to the per-layer bounds; gof_lpips_forward runs the same kernels) ----------------------- */
/* out [n_img, c_out, H, W] = conv3x3(x [n_img, c_in, H, W], weight [c_out, c_in, 3, 3], zero padding 1) + bias [c_out], with
 * max(., 0) applied where relu != 0.  out must not overlap x. */
int gof_lpips_conv3x3(int32_t n_img, int32_t c_in, int32_t c_out, int32_t W, int32_t H, const float* x, const float* weight,
                      const float* bias, int32_t relu, float* out, void* stream);
/* out [planes, H / 2, W / 2] = the 2x2 / stride 2 max-pool of x [planes, H, W] (nn.MaxPool2d(2, 2)); W, H >= 2. */
int gof_lpips_maxpool2(int64_t planes, int32_t W, int32_t H, const float* x, float* out, void* stream);

/* ---- the metric --------------------------------------------------------------------------------------------------------------- */
size_t gof_lpips_workspace_bytes(int32_t W, int32_t H, int32_t n_layers, const GofLpipsLayer* layers_host);
/* img0, img1: [3, H, W] as the caller has them (metrics.py: values in [0, 1]); both go through the scaling layer
 * (x - shift_host[c]) / scale_host[c] (3 floats each, host memory) and the network as one batch of 2.
 * conv_weights_host / conv_biases_host: n_layers DEVICE pointers each, held in host arrays; lin_weights_host: one DEVICE pointer
 * ([c_out] floats) per layer with tap_after != 0, in layer order.
 * out (device, 1 float) = sum over the taps of  1 / (H_l W_l) * sum_px sum_c w_c (f0_c / (||f0|| + 1e-10) - f1_c / (||f1|| + 1e-10))^2,
 * ||.|| the square root of the sum of squares over the channels; per_tap (device, nullable): the value of every tap, in layer order.
 * Refused with GOF_E_INVALID: an image a pool would reduce to nothing (for the VGG instance W or H < 16), channel counts as above,
 * a layer whose c_in is not the c_out in front of it (the first: 3), a network without a tap. */
int gof_lpips_forward(int32_t W, int32_t H, const float* img0, const float* img1, const float* shift_host, const float* scale_host,
                      int32_t n_layers, const GofLpipsLayer* layers_host, const float* const* conv_weights_host,
                      const float* const* conv_biases_host, const float* const* lin_weights_host,
                      float* out, float* per_tap, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
