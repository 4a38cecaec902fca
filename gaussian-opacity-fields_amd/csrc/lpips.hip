// lpips.hip -- the LPIPS perceptual metric (replaces what the reference's metrics.py:19,76,100 asks of the `lpips` pip package: a
// torchvision VGG16 through MIOpen convolutions): scaling layer, 3x3 convolutions as implicit GEMMs on the exact fp32 matrix
// instruction, 2x2 max-pools, and the normalised, weighted feature distance at the taps.  Contract: DESIGN.md 3.12,
// include/gof_lpips_hip.h.
//
// Arithmetic: compiled with -ffp-contract=off like the whole library; every fused multiply-add is written (fmaf) or is the matrix
// instruction's own, which is bit for bit a k-ordered fmaf chain.  No floating-point atomics: every sum has a fixed order.
//
// The convolution is the main loop of conv3x3_f32.h (the GEMM view, the LDS layout and the order of K are written there) over a batch
// [img][C][H][W]: M = the pixels of all images, so a tile may span an image boundary; bias and optional ReLU in the store.
//   C_out % 128 == 0: tile <2, 2>;  C_out % 64 == 0: <2, 1>;  C_out % 32 == 0: <1, 1> -- every weight tile is full.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_lpips_hip.h"
#include "gof_common.h"
#include "gof_geom.h"
#include "conv3x3_f32.h"

namespace gof {
namespace lpips {

// =====================================================================================================================================
// 3x3 convolution, zero padding 1, + bias (+ ReLU)
// =====================================================================================================================================
// pixel p of the batch: image p / HW, offset p % HW in each of its channel planes
struct BatchOperand {
    const float* __restrict__ in;
    int M, C_in, W, H, HW, y, x;
    size_t base;            // of the pixel this thread stages, in channel 0 of its image

    __device__ __forceinline__ bool prepare(int p)
    {
        if (p >= M) return false;
        const int img = p / HW, rem = p - img * HW;
        y = rem / W; x = rem - y * W;
        base = (size_t)img * (size_t)C_in * (size_t)HW + (size_t)rem;
        return true;
    }
    __device__ __forceinline__ float load(int ci, int tap) const { return in[base + (size_t)ci * (size_t)HW + (size_t)((tap / 3 - 1) * W + (tap % 3 - 1))]; }
};

template <int WN, int WGN>
__global__ void __launch_bounds__(256)
conv3x3_kernel(int M, int C_in, int C_out, int W, int H, const float* __restrict__ x, const float* __restrict__ w,
               const float* __restrict__ bias, int relu, float* __restrict__ out)
{
    const int HW = H * W;
    conv3x3::main_loop<WN, WGN, true>(C_in, C_out, BatchOperand{ x, M, C_in, W, H, HW, 0, 0, 0 }, w,
        [=](const f32x16 (&acc)[2][WN], int m0, int n0, int wm_base, int wn_base, int lane, float*) {
            conv3x3::for_each_output<WN>(acc, M, m0, n0, wm_base, wn_base, lane, [=](int q) {
                const int img = q / HW, rem = q - img * HW;
                float* o = out + (size_t)img * (size_t)C_out * (size_t)HW + (size_t)rem;
                return [=](int co, float v) {
                    v = v + bias[co];
                    if (relu) v = (v < 0.0f) ? 0.0f : v;
                    o[(size_t)co * (size_t)HW] = v;
                };
            });
        });
}

// =====================================================================================================================================
// scaling layer, max-pool
// =====================================================================================================================================
struct ScaleArgs { float shift[3], scale[3]; };

// out [2][3][HW]: image 0 and image 1 as one batch
__global__ void __launch_bounds__(256)
scale_kernel(int HW, const float* __restrict__ img0, const float* __restrict__ img1, ScaleArgs s, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)6 * HW) return;
    const int plane = (int)(i / HW), c = plane % 3;
    const int64_t px = i - (int64_t)plane * HW;
    const float v = (plane < 3 ? img0 : img1)[(int64_t)c * HW + px];
    out[i] = (v - s.shift[c]) / s.scale[c];
}

__global__ void __launch_bounds__(256)
maxpool2_kernel(int64_t planes, int W, int H, const float* __restrict__ x, float* __restrict__ out)
{
    const int Wo = W / 2, Ho = H / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * Ho * Wo) return;
    const int64_t plane = i / ((int64_t)Ho * Wo);
    const int rem = (int)(i - plane * Ho * Wo), yo = rem / Wo, xo = rem - yo * Wo;
    const float* s = x + plane * (int64_t)H * W + (int64_t)(2 * yo) * W + 2 * xo;
    out[i] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1]));
}

// =====================================================================================================================================
// taps: stage 1 = one partial sum per workgroup of 256 pixels, stage 2 = one workgroup sums a tap's partials; fixed orders
// =====================================================================================================================================
// the sum of v over the workgroup in a fixed tree order, valid in thread 0
__device__ __forceinline__ float block_sum_256(float v, float* s_part)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    __syncthreads();
    return r;
}

// f [2][C][HW] (the two images' features), lin_w [C] -> partial[block] = sum over the block's pixels of
//     sum_c w_c (f0_c / (||f0|| + 1e-10) - f1_c / (||f1|| + 1e-10))^2
__global__ void __launch_bounds__(256)
tap_partial_kernel(int C, int HW, const float* __restrict__ f, const float* __restrict__ lin_w, float* __restrict__ partial)
{
    __shared__ float s_part[4];
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    float d = 0.0f;
    if (p < HW) {
        const float* f0 = f + p;
        const float* f1 = f + (size_t)C * (size_t)HW + p;
        float s0 = 0.0f, s1 = 0.0f;
        for (int c = 0; c < C; c++) {
            const float a = f0[(size_t)c * HW], b = f1[(size_t)c * HW];
            s0 = fmaf(a, a, s0);
            s1 = fmaf(b, b, s1);
        }
        const float n0 = sqrtf(s0) + 1e-10f, n1 = sqrtf(s1) + 1e-10f;
        for (int c = 0; c < C; c++) {
            const float u = f0[(size_t)c * HW] / n0 - f1[(size_t)c * HW] / n1;
            d = fmaf(lin_w[c], u * u, d);
        }
    }
    const float total = block_sum_256(d, s_part);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// value[0] = (sum of partial[0 .. n)) / count
__global__ void __launch_bounds__(256)
tap_finish_kernel(int n, const float* __restrict__ partial, float count, float* __restrict__ value)
{
    __shared__ float s_part[4];
    float s = 0.0f;
    for (int i = (int)threadIdx.x; i < n; i += 256) s = s + partial[i];
    const float total = block_sum_256(s, s_part);
    if (threadIdx.x == 0) value[0] = total / count;
}

// out[0] = values[0] + values[1] + ... in order; per_tap (nullable) = values
__global__ void lpips_total_kernel(int n_taps, const float* __restrict__ values, float* __restrict__ out, float* __restrict__ per_tap)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float s = 0.0f;
    for (int i = 0; i < n_taps; i++) {
        s = s + values[i];
        if (per_tap) per_tap[i] = values[i];
    }
    out[0] = s;
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
static bool bad_channels(int32_t c_in, int32_t c_out, const char* who)
{
    if (c_in < 1 || c_in > GOF_LPIPS_MAX_CHANNELS || c_out < 32 || c_out > GOF_LPIPS_MAX_CHANNELS || c_out % 32 != 0) {
        set_error("%s: channel counts %d -> %d: the convolution takes C_in in [1, %d] and C_out a multiple of 32 in [32, %d]", who, c_in, c_out,
                  GOF_LPIPS_MAX_CHANNELS, GOF_LPIPS_MAX_CHANNELS);
        return true;
    }
    return false;
}

static int launch_conv(int32_t n_img, int32_t c_in, int32_t c_out, int32_t W, int32_t H, const float* x, const float* w, const float* bias,
                       int32_t relu, float* out, hipStream_t stream)
{
    const int M = n_img * H * W;
    const int relu_i = relu != 0;
#define GOF_LAUNCH_CONV(WN, WGN) hipLaunchKernelGGL((conv3x3_kernel<WN, WGN>), (conv3x3::grid<WN, WGN>(M, c_out)), dim3(256), 0, stream, M, (int)c_in, (int)c_out, (int)W, (int)H, x, w, bias, relu_i, out)
    if (c_out % 128 == 0) GOF_LAUNCH_CONV(2, 2);
    else if (c_out % 64 == 0) GOF_LAUNCH_CONV(2, 1);
    else GOF_LAUNCH_CONV(1, 1);
#undef GOF_LAUNCH_CONV
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

struct Plan {
    size_t act_floats;        // the larger of any activation tensor [2][C][h][w]
    size_t partial_floats;    // sum over the taps of their workgroup counts
    int n_taps;
};

// walks the network: 0 and the sizes, or GOF_E_INVALID with the text set
static int make_plan(int32_t W, int32_t H, int32_t n_layers, const GofLpipsLayer* layers, Plan* plan)
{
    if (W < 1 || H < 1 || (int64_t)W * H > ((int64_t)1 << 29)) { set_error("lpips: bad image size (%d x %d)", W, H); return GOF_E_INVALID; }
    if (n_layers < 1 || n_layers > GOF_LPIPS_MAX_LAYERS || !layers) { set_error("lpips: the network must have 1 to %d layers", GOF_LPIPS_MAX_LAYERS); return GOF_E_INVALID; }
    Plan pl{ (size_t)6 * (size_t)W * (size_t)H, 0, 0 };
    int w = W, h = H, c = 3;
    for (int i = 0; i < n_layers; i++) {
        const GofLpipsLayer& L = layers[i];
        if (L.pool_before) {
            if (w < 2 || h < 2) {
                set_error("lpips: an image of %d x %d is %d x %d in front of the pool of layer %d: nothing would be left (the VGG network needs W, H >= 16)", W, H, w, h, i);
                return GOF_E_INVALID;
            }
            w /= 2; h /= 2;
            const size_t n = (size_t)2 * c * w * h;
            if (n > pl.act_floats) pl.act_floats = n;
        }
        if (L.c_in != c) { set_error("lpips: layer %d takes %d channels, the layer in front of it gives %d", i, L.c_in, c); return GOF_E_INVALID; }
        if (bad_channels(L.c_in, L.c_out, "lpips")) return GOF_E_INVALID;
        c = L.c_out;
        const size_t n = (size_t)2 * c * w * h;
        if (n > pl.act_floats) pl.act_floats = n;
        if (L.tap_after) { pl.partial_floats += (size_t)(w * h + 255) / 256; pl.n_taps++; }
    }
    if (pl.n_taps == 0) { set_error("lpips: the network has no tap"); return GOF_E_INVALID; }
    if (plan) *plan = pl;
    return GOF_OK;
}

struct Ws { float* act[2]; float* partial; float* values; };
static size_t ws_layout(const Plan& pl, void* base, Ws* out)
{
    Carver c{ static_cast<char*>(base), 0 };
    Ws w;
    w.act[0] = c.take<float>(pl.act_floats);
    w.act[1] = c.take<float>(pl.act_floats);
    w.partial = c.take<float>(pl.partial_floats);
    w.values = c.take<float>((size_t)pl.n_taps);
    if (out) *out = w;
    return c.total();
}

} // namespace lpips
} // namespace gof

using namespace gof;
using namespace gof::lpips;

extern "C" {

int gof_lpips_conv3x3(int32_t n_img, int32_t c_in, int32_t c_out, int32_t W, int32_t H, const float* x, const float* weight,
                      const float* bias, int32_t relu, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_img < 1 || W < 1 || H < 1 || (int64_t)n_img * W * H >= ((int64_t)1 << 31) - 256) { set_error("lpips_conv3x3: bad sizes (%d images of %d x %d)", n_img, W, H); return GOF_E_INVALID; }
    if (bad_channels(c_in, c_out, "lpips_conv3x3")) return GOF_E_INVALID;
    if (!x || !weight || !bias || !out) { set_error("lpips_conv3x3: x / weight / bias / out is NULL"); return GOF_E_INVALID; }
    GOF_PROFILE("lpips_conv3x3", stream);
    return launch_conv(n_img, c_in, c_out, W, H, x, weight, bias, relu, out, stream);
}

int gof_lpips_maxpool2(int64_t planes, int32_t W, int32_t H, const float* x, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (planes < 1 || W < 2 || H < 2 || planes * (int64_t)(W / 2) * (H / 2) >= ((int64_t)1 << 39)) { set_error("lpips_maxpool2: bad sizes (%lld planes of %d x %d)", (long long)planes, W, H); return GOF_E_INVALID; }
    if (!x || !out) { set_error("lpips_maxpool2: x / out is NULL"); return GOF_E_INVALID; }
    GOF_PROFILE("lpips_maxpool2", stream);
    hipLaunchKernelGGL(maxpool2_kernel, grid_of(planes * (int64_t)(W / 2) * (H / 2)), dim3(256), 0, stream, planes, (int)W, (int)H, x, out);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

size_t gof_lpips_workspace_bytes(int32_t W, int32_t H, int32_t n_layers, const GofLpipsLayer* layers_host)
{
    Plan pl;
    if (make_plan(W, H, n_layers, layers_host, &pl) != GOF_OK) return 0;
    return ws_layout(pl, nullptr, nullptr);
}

int gof_lpips_forward(int32_t W, int32_t H, const float* img0, const float* img1, const float* shift_host, const float* scale_host,
                      int32_t n_layers, const GofLpipsLayer* layers_host, const float* const* conv_weights_host,
                      const float* const* conv_biases_host, const float* const* lin_weights_host,
                      float* out, float* per_tap, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Plan pl;
    const int rc = make_plan(W, H, n_layers, layers_host, &pl);
    if (rc != GOF_OK) return rc;
    if (!img0 || !img1 || !shift_host || !scale_host || !conv_weights_host || !conv_biases_host || !lin_weights_host || !out) { set_error("lpips_forward: an argument is NULL"); return GOF_E_INVALID; }
    for (int i = 0; i < n_layers; i++)
        if (!conv_weights_host[i] || !conv_biases_host[i]) { set_error("lpips_forward: the weights / biases of layer %d are NULL", i); return GOF_E_INVALID; }
    for (int i = 0; i < pl.n_taps; i++)
        if (!lin_weights_host[i]) { set_error("lpips_forward: the lin weights of tap %d are NULL", i); return GOF_E_INVALID; }
    if (!ws) { set_error("lpips_forward: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < ws_layout(pl, nullptr, nullptr)) { set_error("lpips_forward: workspace too small"); return GOF_E_WORKSPACE; }
    Ws w;
    ws_layout(pl, ws_aligned(ws), &w);
    GOF_PROFILE("lpips_forward", stream);

    ScaleArgs sa;
    for (int c = 0; c < 3; c++) { sa.shift[c] = shift_host[c]; sa.scale[c] = scale_host[c]; }
    const int HW0 = W * H;
    hipLaunchKernelGGL(scale_kernel, grid_of((int64_t)6 * HW0), dim3(256), 0, stream, HW0, img0, img1, sa, w.act[0]);
    GOF_LAUNCH_CHECK(stream, 0);
    int cur = 0, cw = W, ch = H, cc = 3, tap = 0;
    size_t part_off = 0;
    for (int i = 0; i < n_layers; i++) {
        const GofLpipsLayer& L = layers_host[i];
        if (L.pool_before) {
            hipLaunchKernelGGL(maxpool2_kernel, grid_of((int64_t)2 * cc * (cw / 2) * (ch / 2)), dim3(256), 0, stream, (int64_t)2 * cc, cw, ch, w.act[cur], w.act[cur ^ 1]);
            GOF_LAUNCH_CHECK(stream, 0);
            cur ^= 1; cw /= 2; ch /= 2;
        }
        const int r = launch_conv(2, L.c_in, L.c_out, cw, ch, w.act[cur], conv_weights_host[i], conv_biases_host[i], 1, w.act[cur ^ 1], stream);
        if (r != GOF_OK) return r;
        cur ^= 1; cc = L.c_out;
        if (L.tap_after) {
            const int hw = cw * ch, blocks = (hw + 255) / 256;
            hipLaunchKernelGGL(tap_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, cc, hw, w.act[cur], lin_weights_host[tap], w.partial + part_off);
            hipLaunchKernelGGL(tap_finish_kernel, dim3(1), dim3(256), 0, stream, blocks, w.partial + part_off, (float)hw, w.values + tap);
            GOF_LAUNCH_CHECK(stream, 0);
            part_off += (size_t)blocks;
            tap++;
        }
    }
    hipLaunchKernelGGL(lpips_total_kernel, dim3(1), dim3(64), 0, stream, pl.n_taps, w.values, out, per_tap);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // extern "C"
