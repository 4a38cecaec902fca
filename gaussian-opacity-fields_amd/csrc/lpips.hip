// lpips.hip -- the LPIPS perceptual metric (replaces what the reference's metrics.py:19,76,100 asks of the `lpips` pip package: a
// torchvision VGG16 through MIOpen convolutions): scaling layer, 3x3 convolutions as implicit GEMMs on the exact fp32 matrix
// instruction, 2x2 max-pools, and the normalised, weighted feature distance at the taps.  Contract: DESIGN.md 3.12,
// include/gof_lpips_hip.h.
//
// Arithmetic: compiled with -ffp-contract=off like the whole library; every fused multiply-add is written (fmaf) or is the matrix
// instruction's own, which is bit for bit a k-ordered fmaf chain.  No floating-point atomics: every sum has a fixed order.
//
// The convolution.  GEMM view: M = pixels of all images, N = C_out, K = 9 C_in with k = ci * 9 + ky * 3 + kx (torch's flattening of
// the weight, so the weight tensor is read as it lies).  A workgroup of 4 waves owns BM pixels x BN output channels and walks K in
// chunks of 4 input channels (36 terms; the last chunk of a C_in that is no multiple of 4 is shorter and padded to an even length
// with a term 0 * 0).  Per chunk the pixel operand X[k][m] (the shifted image values, 0 outside the image: the zero padding) and the
// weight operand Wt[n][k] are staged in LDS, then every wave runs the chunk's k-steps on its 2 x WN accumulator tiles of 32 x 32.
// The instruction takes the WEIGHTS in its A slot and the PIXELS in its B slot, i.e. it forms the transposed tile: an accumulator
// register then holds 32 consecutive pixels of one output channel across lanes 0-31, and the planar output is stored in 128-byte rows.
//   LDS: X [36][BM + 32] (the pad makes the two k rows a k-step reads fall into different bank halves), Wt [BN][37].
//   C_out % 128 == 0: BM = 128, BN = 128 (waves 2 x 2);  C_out % 64 == 0: BM = 256, BN = 64;  C_out % 32 == 0: BM = 256, BN = 32.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_lpips_hip.h"
#include "gof_common.h"
#include "gof_geom.h"
#include "mma_f32.h"

namespace gof {
namespace lpips {

// the matrix step mma_32x32x2 (one v_mfma_f32_32x32x2_f32; restated with fmaf for the CPU suite): mma_f32.h

constexpr int KC = 36;          // terms of a full K chunk: 4 input channels x 9 taps
constexpr int KP = 37;          // row pitch of the weight operand in LDS (odd: a wave's 32 rows fall into 32 banks)

// =====================================================================================================================================
// 3x3 convolution, zero padding 1, + bias (+ ReLU)
// =====================================================================================================================================
template <int WN, int WGN>
__global__ void __launch_bounds__(256)
conv3x3_kernel(int M, int C_in, int C_out, int W, int H, const float* __restrict__ x, const float* __restrict__ w,
               const float* __restrict__ bias, int relu, float* __restrict__ out)
{
    constexpr int WGM = 4 / WGN, BM = 64 * WGM, BN = 32 * WN * WGN, BMP = BM + 32;
    constexpr int RPT = KC * BM / 256;                     // X rows a thread stages per chunk (36 or 18: whole input channels)
    __shared__ float Xs[KC * BMP];
    __shared__ float Ws[BN * KP];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * BN;
    const int HW = H * W, K = 9 * C_in;

    // the pixel this thread stages: its offset in a channel plane and which of its 9 taps lie inside the image
    const int lm = t % BM, lk0 = t / BM;
    const int p = m0 + lm;
    size_t base = 0;
    unsigned inside = 0;
    if (p < M) {
        const int img = p / HW, rem = p - img * HW, y = rem / W, xx = rem - y * W;
        base = (size_t)img * (size_t)C_in * (size_t)HW + (size_t)rem;
        for (int ky = 0; ky < 3; ky++)
            for (int kx = 0; kx < 3; kx++)
                if (y + ky - 1 >= 0 && y + ky - 1 < H && xx + kx - 1 >= 0 && xx + kx - 1 < W) inside |= 1u << (ky * 3 + kx);
    }

    const int wm_base = (wave % WGM) * 64, wn_base = (wave / WGM) * 32 * WN;
    f32x16 acc[2][WN];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;

    for (int c0 = 0; c0 < C_in; c0 += 4) {
        const int nci = (C_in - c0 < 4) ? C_in - c0 : 4;
        const int klen = 9 * nci, kpad = (klen + 1) & ~1;
        // pixel operand: rows kk = lk0 * RPT + j, all KC of them (rows behind klen are zeros: the pad term, and never NaN)
#pragma unroll
        for (int j = 0; j < RPT; j++) {
            const int kk = lk0 * RPT + j;
            const int ci = lk0 * (RPT / 9) + j / 9, tap = j % 9;
            float v = 0.0f;
            if (kk < klen && ((inside >> tap) & 1u))
                v = x[base + (size_t)(c0 + ci) * (size_t)HW + (size_t)((tap / 3 - 1) * W + (tap % 3 - 1))];
            Xs[kk * BMP + lm] = v;
        }
        // weight operand: row n = 36 consecutive floats of the weight tensor
        for (int e = t; e < BN * KC; e += 256) {
            const int n = e / KC, kk = e - n * KC;
            Ws[n * KP + kk] = (kk < klen) ? w[(size_t)(n0 + n) * (size_t)K + (size_t)(c0 * 9 + kk)] : 0.0f;
        }
        __syncthreads();
        for (int ks = 0; ks < kpad; ks += 2) {
            const int kk = ks + (lane >> 5);
            float a[WN], b[2];
#pragma unroll
            for (int j = 0; j < WN; j++) a[j] = Ws[(wn_base + 32 * j + (lane & 31)) * KP + kk];
#pragma unroll
            for (int i = 0; i < 2; i++) b[i] = Xs[kk * BMP + wm_base + 32 * i + (lane & 31)];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < WN; j++) acc[i][j] = mma_32x32x2(a[j], b[i], acc[i][j]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int q = m0 + wm_base + 32 * i + (lane & 31);
        if (q >= M) continue;
        const int img = q / HW, rem = q - img * HW;
        float* o = out + (size_t)img * (size_t)C_out * (size_t)HW + (size_t)rem;
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int co = n0 + wn_base + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float v = acc[i][j][r] + bias[co];
                if (relu) v = (v < 0.0f) ? 0.0f : v;
                o[(size_t)co * (size_t)HW] = v;
            }
    }
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
    if (c_out % 128 == 0) {
        const dim3 grid((unsigned)((M + 127) / 128), (unsigned)(c_out / 128));
        hipLaunchKernelGGL((conv3x3_kernel<2, 2>), grid, dim3(256), 0, stream, M, (int)c_in, (int)c_out, (int)W, (int)H, x, w, bias, relu_i, out);
    } else if (c_out % 64 == 0) {
        const dim3 grid((unsigned)((M + 255) / 256), (unsigned)(c_out / 64));
        hipLaunchKernelGGL((conv3x3_kernel<2, 1>), grid, dim3(256), 0, stream, M, (int)c_in, (int)c_out, (int)W, (int)H, x, w, bias, relu_i, out);
    } else {
        const dim3 grid((unsigned)((M + 255) / 256), (unsigned)(c_out / 32));
        hipLaunchKernelGGL((conv3x3_kernel<1, 1>), grid, dim3(256), 0, stream, M, (int)c_in, (int)c_out, (int)W, (int)H, x, w, bias, relu_i, out);
    }
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
