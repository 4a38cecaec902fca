// appearance.hip -- the decoupled-appearance L1 of the reference's train.py:67-88 and scene/appearance_network.py, forward and backward:
// crop, bilinear down-sample, the embedding as constant planes, seven 3x3 convolutions as implicit GEMMs on the exact fp32 matrix
// instruction (their operands read THROUGH the pixel-shuffles and the bilinear x2 up-sample), the sigmoid / product / L1, and the
// gradients of the image, the embedding and the 14 parameters.  Contract: DESIGN.md 3.13, include/gof_appearance_hip.h.
//
// Arithmetic: compiled with -ffp-contract=off like the whole library; every fused multiply-add is written (fmaf) or is the matrix
// instruction's own (mma_f32.h).  No floating-point atomics: every sum has a fixed order.
//
// The convolution is the main loop of conv3x3_f32.h (the one csrc/lpips.hip runs: same tiles, same LDS layout, same order of K) on one
// plane: the pixel operand is staged through fetch() (the views of the header), output channels that do not fill the tile are zero
// weight rows that are not stored, the bias is optional, and conv3's epilogue is the head (sigmoid, product, L1 partial sums).
//
// The weight gradient.  GEMM view: M = C_out, N = 9 C_in + 1 (column n = ci * 9 + ky * 3 + kx; the last column is the constant 1:
// the bias gradient), K = the pixels of one chunk.  A workgroup of 4 waves owns one chunk x 32 output channels x 128 columns (one
// 32 x 32 accumulator tile per wave) and walks its pixels in stages of 64: dY' [32][64] and the shifted X [128][64] are staged in
// LDS (row pitch 65: the 32 rows a wave reads fall into 32 banks), then 32 matrix steps in sub-chains of GOF_APP_WGRAD_SUB pixels whose
// results are accumulated in fp64.  Chunk partials (fp64) go to the workspace.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_appearance_hip.h"
#include "gof_common.h"
#include "gof_geom.h"
#include "conv3x3_f32.h"

namespace gof {
namespace app {

constexpr int WG_PS = 64;       // pixels per stage of the weight gradient
constexpr int WG_PP = 65;       // row pitch of its operands in LDS
constexpr int WG_BN = 128;      // columns per workgroup
constexpr int SRC_HEAD = 5;     // internal operand view: dz computed from the saved sigmoid while staging (not part of the ABI's GOF_APP_SRC_*)

// =====================================================================================================================================
// operand views
// =====================================================================================================================================
struct Crop { int W, H, Wc, Hc, top, left; };       // the image, the crop

// the sum of v over the workgroup in fp64, in a fixed tree order (stride 128, 64, ... 1 over the thread index), valid in thread 0.
// The elements are fp32 values; their SUM is formed in fp64 so that the loss is the correctly rounded mean of what the kernels computed.
__device__ __forceinline__ double block_sum_256(double v, double* s_val)
{
    const int t = (int)threadIdx.x;
    s_val[t] = v;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) s_val[t] = s_val[t] + s_val[t + d];
        __syncthreads();
    }
    const double r = s_val[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float l1_sign(float u) { return (u > 0.0f) ? 1.0f : ((u < 0.0f) ? -1.0f : 0.0f); }

// what the sigmoid / product / L1 need next to z: forward (conv3's epilogue) and backward (the head of conv3's gradient)
struct Head {
    const float* image; const float* gt;      // [3][H][W]
    float* m_out; float* transformed;         // forward: [3][Hc][Wc], transformed nullable
    double* partial;                          // forward: one fp64 sum per 256 pixels
    const float* dL; float count;             // backward: dL (1 float), 3 Hc Wc
    Crop cr;
    int on;
};

// element (c, pixel q of the crop) of the forward: stores m (and t), returns |m I - G|
__device__ __forceinline__ float head_element(const Head& h, float z, int c, int q)
{
    const int y = q / h.cr.Wc, x = q - y * h.cr.Wc;
    const size_t at = ((size_t)c * h.cr.H + (size_t)(h.cr.top + y)) * h.cr.W + (size_t)(h.cr.left + x);
    const size_t i = (size_t)c * h.cr.Hc * h.cr.Wc + (size_t)q;
    const float m = 1.0f / (1.0f + gexpf(-z));
    const float tv = m * h.image[at];
    h.m_out[i] = m;
    if (h.transformed) h.transformed[i] = tv;
    return fabsf(tv - h.gt[at]);
}

// dz = ((g I) m) (1 - m),  g = sign(m I - G) (dL / count), at (c, y, x) of the crop
__device__ __forceinline__ float head_dz(const Head& h, float m, int c, int y, int x)
{
    const size_t at = ((size_t)c * h.cr.H + (size_t)(h.cr.top + y)) * h.cr.W + (size_t)(h.cr.left + x);
    const float I = h.image[at];
    const float g = l1_sign(m * I - h.gt[at]) * (h.dL[0] / h.count);
    return ((g * I) * m) * (1.0f - m);
}

struct Src {
    const float* p;         // the stored tensor
    const float* mask;      // nullable, [C][H][W]
    const float* emb;       // SRC_EMBED: [C - 3]
    int mode;
    int W, H;               // plane of the view
    float sy, sx;           // SRC_UP2: the scales (H / 2 - 1) / (H - 1), (W / 2 - 1) / (W - 1)
    Head head;              // SRC_HEAD: p = the saved sigmoid [3][H][W], the view is dz (the head of conv3's gradient)
};

static float lerp_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f; }

__device__ __forceinline__ void lerp_axis(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1)
{
    const float s = scale * (float)dst;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + ((i0 < in - 1) ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.0f - l1;
}

// plane: rows `pitch` floats apart
__device__ __forceinline__ float bilerp(const float* __restrict__ plane, size_t pitch, int inW, int inH, float sy, float sx, int y, int x)
{
    int y0, y1, x0, x1;
    float l0h, l1h, l0w, l1w;
    lerp_axis(sy, y, inH, y0, y1, l0h, l1h);
    lerp_axis(sx, x, inW, x0, x1, l0w, l1w);
    const float a = plane[(size_t)y0 * pitch + x0], b = plane[(size_t)y0 * pitch + x1];
    const float c = plane[(size_t)y1 * pitch + x0], d = plane[(size_t)y1 * pitch + x1];
    return l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d);
}

// the value of the view at (c, y, x), 0 <= y < H, 0 <= x < W
__device__ __forceinline__ float fetch(const Src& s, int c, int y, int x)
{
    float v;
    switch (s.mode) {
    case GOF_APP_SRC_SHUFFLE: {
        const int w2 = s.W >> 1, h2 = s.H >> 1;
        v = s.p[((size_t)(4 * c + 2 * (y & 1) + (x & 1)) * h2 + (y >> 1)) * w2 + (x >> 1)];
        break;
    }
    case GOF_APP_SRC_UNSHUFFLE:
        v = s.p[((size_t)(c >> 2) * (2 * s.H) + (2 * y + ((c >> 1) & 1))) * (2 * s.W) + 2 * x + (c & 1)];
        break;
    case GOF_APP_SRC_UP2: {
        const int w2 = s.W >> 1, h2 = s.H >> 1;
        v = bilerp(s.p + (size_t)c * h2 * w2, (size_t)w2, w2, h2, s.sy, s.sx, y, x);
        break;
    }
    case GOF_APP_SRC_EMBED:
        v = (c < 3) ? s.p[((size_t)c * s.H + y) * s.W + x] : s.emb[c - 3];
        break;
    case SRC_HEAD:
        v = head_dz(s.head, s.p[((size_t)c * s.H + y) * s.W + x], c, y, x);
        break;
    default:
        v = s.p[((size_t)c * s.H + y) * s.W + x];
    }
    if (s.mask) v = (s.mask[((size_t)c * s.H + y) * s.W + x] > 0.0f) ? v : 0.0f;
    return v;
}

__global__ void __launch_bounds__(256)
materialize_kernel(int C, Src src, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)src.H * src.W;
    if (i >= (int64_t)C * HW) return;
    const int c = (int)(i / HW), rem = (int)(i - (int64_t)c * HW), y = rem / src.W, x = rem - y * src.W;
    out[i] = fetch(src, c, y, x);
}

// =====================================================================================================================================
// 3x3 convolution, zero padding 1 (+ bias) (+ ReLU): M = the pixels of the plane, N = C_out, K = 9 C_in
// =====================================================================================================================================
// pixel p of the view's plane, read through fetch()
struct ViewOperand {
    const Src& src;
    int W, H, y, x;

    __device__ __forceinline__ bool prepare(int p) { y = p / W; x = p - y * W; return p < H * W; }
    __device__ __forceinline__ float load(int ci, int tap) const { return fetch(src, ci, y + tap / 3 - 1, x + tap % 3 - 1); }
};

template <int WN, int WGN>
__global__ void __launch_bounds__(256)
conv3x3_kernel(int C_in, int C_out, Src src, const float* __restrict__ w, const float* __restrict__ bias, int relu, float* __restrict__ out, Head head)
{
    const int M = src.H * src.W;
    conv3x3::main_loop<WN, WGN, false>(C_in, C_out, ViewOperand{ src, src.W, src.H, 0, 0 }, w,
        [&](const f32x16 (&acc)[2][WN], int m0, int n0, int wm_base, int wn_base, int lane, float* Xs) {
            // conv3 of the appearance network: sigmoid, product with the image and the L1 partial sum in the epilogue; z is never stored.
            // (host: only with C_out == 3 and the 256-pixel tile.)  Per workgroup: the three channels of a pixel are added in channel
            // order, then the 256 pixels in the tree of block_sum_256, all in fp64.  Xs: the main loop's LDS, free by now.
            if (head.on) {
                __shared__ double s_val[256];
                constexpr int BM = 256 / WGN;
                if (BM == 256) {
                    const int t = (int)threadIdx.x;
                    Xs[t] = 0.0f; Xs[BM + t] = 0.0f; Xs[2 * BM + t] = 0.0f;
                    __syncthreads();
                    // (n0 = wn_base = 0 here, so co < 3 is tile (., 0), registers 0 - 2 of lanes 0 - 31: one lane holds a pixel's three channels)
                    conv3x3::for_each_output<WN>(acc, M, m0, n0, wm_base, wn_base, lane, [&](int q) {
                        return [&, q](int co, float v) { if (co < 3) Xs[co * BM + (q - m0)] = head_element(head, v + bias[co], co, q); };
                    });
                    __syncthreads();
                    const double v = ((double)Xs[t] + (double)Xs[BM + t]) + (double)Xs[2 * BM + t];
                    const double total = block_sum_256(v, s_val);
                    if (t == 0) head.partial[blockIdx.x] = total;
                }
                return;
            }
            conv3x3::for_each_output<WN>(acc, M, m0, n0, wm_base, wn_base, lane, [&](int q) {
                return [&, q](int co, float v) {
                    if (co >= C_out) return;
                    if (bias) v = v + bias[co];
                    if (relu) v = (v < 0.0f) ? 0.0f : v;
                    out[(size_t)co * (size_t)M + (size_t)q] = v;
                };
            });
        });
}

// out [C_in][C_out][9] = w [C_out][C_in][8 - tap]
__global__ void __launch_bounds__(256)
weight_transpose_kernel(int C_in, int C_out, const float* __restrict__ w, float* __restrict__ out)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= C_in * C_out * 9) return;
    const int ci = i / (C_out * 9), rem = i - ci * C_out * 9, co = rem / 9, tap = rem - co * 9;
    out[i] = w[((size_t)co * C_in + ci) * 9 + (8 - tap)];
}

// =====================================================================================================================================
// weight and bias gradient
// =====================================================================================================================================
// partial [n_chunks][C_out][9 C_in + 1], fp64.  Within a chunk the pixels are cut into sub-chains of GOF_APP_WGRAD_SUB: each is ONE fmaf
// chain in ascending p on the matrix instruction, started from 0; the sub-chain results are added in ascending order to an fp64
// accumulator (a chain of 16 terms keeps the accuracy of an fp32 framework's blocked sums; the fp64 additions add nothing to it).
__global__ void __launch_bounds__(256)
wgrad_kernel(int C_in, int C_out, Src xs, Src dys, double* __restrict__ partial)
{
    __shared__ float As[32 * WG_PP];
    __shared__ float Bs[WG_BN * WG_PP];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int chunk = (int)blockIdx.x, n0 = (int)blockIdx.y * WG_BN, m0 = (int)blockIdx.z * 32;
    const int W = xs.W, H = xs.H, HW = H * W, NT = 9 * C_in + 1;
    const int p_begin = chunk * GOF_APP_WGRAD_CHUNK;
    const int p_end = (HW - p_begin < GOF_APP_WGRAD_CHUNK) ? HW : p_begin + GOF_APP_WGRAD_CHUNK;
    double total[16];
#pragma unroll
    for (int r = 0; r < 16; r++) total[r] = 0.0;
    const int px = t & 63, r0 = t >> 6;
    for (int s0 = p_begin; s0 < p_end; s0 += WG_PS) {
        const int p = s0 + px;
        const bool live = p < p_end;       // (the ragged end of the last chunk: terms 0 * 0)
        int y = 0, x = 0;
        if (live) { y = p / W; x = p - y * W; }
        for (int j = 0; j < 8; j++) {
            const int row = r0 + 4 * j, co = m0 + row;
            As[row * WG_PP + px] = (live && co < C_out) ? fetch(dys, co, y, x) : 0.0f;
        }
        for (int j = 0; j < WG_BN / 4; j++) {
            const int col = r0 + 4 * j, n = n0 + col;
            float v = 0.0f;
            if (live && n < NT) {
                if (n == NT - 1) {
                    v = 1.0f;
                } else {
                    const int ci = n / 9, tap = n - 9 * ci;
                    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = fetch(xs, ci, yy, xx);
                }
            }
            Bs[col * WG_PP + px] = v;
        }
        __syncthreads();
        for (int sub = 0; sub < WG_PS; sub += GOF_APP_WGRAD_SUB) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < GOF_APP_WGRAD_SUB; ks += 2) {
                const int kk = sub + ks + (lane >> 5);
                const float a = As[(lane & 31) * WG_PP + kk];
                const float b = Bs[(wave * 32 + (lane & 31)) * WG_PP + kk];
                acc = mma_32x32x2(a, b, acc);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) total[r] = total[r] + (double)acc[r];
        }
        __syncthreads();
    }
    const int n = n0 + wave * 32 + (lane & 31);
    if (n < NT) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int co = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (co < C_out) partial[((size_t)chunk * C_out + co) * NT + n] = total[r];
        }
    }
}

__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(int n_chunks, int C_in, int C_out, const double* __restrict__ partial, float* __restrict__ dW, float* __restrict__ db)
{
    const int NT = 9 * C_in + 1, total = C_out * NT;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= total) return;
    double s = partial[i];
    for (int c = 1; c < n_chunks; c++) s = s + partial[(size_t)c * total + i];
    const int co = i / NT, n = i - co * NT;
    if (n == NT - 1) db[co] = (float)s;                    // (the one rounding to fp32)
    else dW[(size_t)co * (NT - 1) + n] = (float)s;
}

// =====================================================================================================================================
// resampling
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
bilinear_kernel(int C, int inW, int inH, int64_t row_stride, int64_t plane_stride, const float* __restrict__ x, int outW, int outH,
                float sy, float sx, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)outH * outW;
    if (i >= (int64_t)C * HW) return;
    const int c = (int)(i / HW), rem = (int)(i - (int64_t)c * HW), y = rem / outW, xx = rem - y * outW;
    out[i] = bilerp(x + (int64_t)c * plane_stride, (size_t)row_stride, inW, inH, sy, sx, y, xx);
}

// the destination indices whose footprint can hold source index i: [lo, hi], a superset (the caller tests each with lerp_axis)
__device__ __forceinline__ void footprint_range(float scale, int i, int out, int& lo, int& hi)
{
    lo = 0; hi = out - 1;
    if (scale > 0.0f) {
        const int a = (int)((float)(i - 1) / scale) - 1, b = (int)((float)(i + 1) / scale) + 2;
        if (a > lo) lo = a;
        if (b < hi) hi = b;
    }
}

// acc + the contributions of g [outH][outW] (one plane) to source pixel (y, x) of the [inH][inW] plane it was interpolated from
__device__ __forceinline__ float bilinear_gather(float acc, const float* __restrict__ g, int inW, int inH, int outW, int outH, float sy, float sx,
                                                 int y, int x)
{
    int Ylo, Yhi, Xlo, Xhi;
    footprint_range(sy, y, outH, Ylo, Yhi);
    footprint_range(sx, x, outW, Xlo, Xhi);
    for (int Y = Ylo; Y <= Yhi; Y++) {
        int y0, y1; float l0h, l1h;
        lerp_axis(sy, Y, inH, y0, y1, l0h, l1h);
        if (y0 != y && y1 != y) continue;
        for (int X = Xlo; X <= Xhi; X++) {
            int x0, x1; float l0w, l1w;
            lerp_axis(sx, X, inW, x0, x1, l0w, l1w);
            if (x0 != x && x1 != x) continue;
            const float gv = g[(size_t)Y * outW + X];
            if (y0 == y && x0 == x) acc = acc + (l0h * l0w) * gv;
            if (y0 == y && x1 == x) acc = acc + (l0h * l1w) * gv;
            if (y1 == y && x0 == x) acc = acc + (l1h * l0w) * gv;
            if (y1 == y && x1 == x) acc = acc + (l1h * l1w) * gv;
        }
    }
    return acc;
}

// out [C][h][w] from g [C][2 h][2 w]
__global__ void __launch_bounds__(256)
up2_backward_kernel(int C, int w, int h, float sy, float sx, const float* __restrict__ g, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t hw = (int64_t)h * w;
    if (i >= (int64_t)C * hw) return;
    const int c = (int)(i / hw), rem = (int)(i - (int64_t)c * hw), y = rem / w, x = rem - y * w;
    out[i] = bilinear_gather(0.0f, g + (size_t)c * 4 * hw, w, h, 2 * w, 2 * h, sy, sx, y, x);
}

// =====================================================================================================================================
// the ends
// =====================================================================================================================================
// the same head on a stored z [3][Hc][Wc] (the piece the tests hold alone): the order of conv3's epilogue
__global__ void __launch_bounds__(256)
head_forward_kernel(Head head, const float* __restrict__ z)
{
    __shared__ double s_val[256];
    const int HWc = head.cr.Hc * head.cr.Wc;
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    double v = 0.0;
    if (q < HWc) {
        const float d0 = head_element(head, z[q], 0, q), d1 = head_element(head, z[(size_t)HWc + q], 1, q), d2 = head_element(head, z[(size_t)2 * HWc + q], 2, q);
        v = ((double)d0 + (double)d1) + (double)d2;
    }
    const double total = block_sum_256(v, s_val);
    if (threadIdx.x == 0) head.partial[blockIdx.x] = total;
}

// value[0] = (float)((sum of partial[0 .. n)) / count): per thread the partials i = t, t + 256, ... in ascending order, then the tree
__global__ void __launch_bounds__(256)
sum_finish_kernel(int n, const double* __restrict__ partial, double count, float* __restrict__ value)
{
    __shared__ double s_val[256];
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += 256) s = s + partial[i];
    const double total = block_sum_256(s, s_val);
    if (threadIdx.x == 0) value[0] = (float)(total / count);
}

// d_image [3][H][W]: 0 outside the crop; inside g m + the transpose of the down-sample applied to dD [3][h][w] (a gather)
__global__ void __launch_bounds__(256)
image_grad_kernel(Crop cr, int w, int h, float sy, float sx, const float* __restrict__ m_in, const float* __restrict__ image,
                  const float* __restrict__ gt, const float* __restrict__ dL, float count, const float* __restrict__ dD, float* __restrict__ d_image)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)cr.H * cr.W;
    if (i >= 3 * HW) return;
    const int c = (int)(i / HW), rem = (int)(i - (int64_t)c * HW), Y = rem / cr.W, X = rem - Y * cr.W;
    const int y = Y - cr.top, x = X - cr.left;
    float v = 0.0f;
    if (y >= 0 && y < cr.Hc && x >= 0 && x < cr.Wc) {
        const float m = m_in[((size_t)c * cr.Hc + y) * cr.Wc + x];
        const float g = l1_sign(m * image[i] - gt[i]) * (dL[0] / count);
        // (the roles are exchanged: the crop is the SOURCE of the down-sample, dD lives on its destination)
        v = bilinear_gather(g * m, dD + (size_t)c * h * w, cr.Wc, cr.Hc, w, h, sy, sx, y, x);
    }
    d_image[i] = v;
}

// dE[c] = sum_p dX1[3 + c][p] in ascending p
__global__ void __launch_bounds__(256)
embedding_grad_kernel(int n_embed, int hw, const float* __restrict__ dX1, float* __restrict__ dE)
{
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= n_embed) return;
    const float* s = dX1 + (size_t)(3 + c) * hw;
    float a = 0.0f;
    for (int p = 0; p < hw; p++) a = a + s[p];
    dE[c] = a;
}

// =====================================================================================================================================
// host side
// =====================================================================================================================================
static bool bad_channels(int32_t c_in, int32_t c_out, const char* who)
{
    if (c_in < 1 || c_in > GOF_APP_MAX_CHANNELS || c_out < 1 || c_out > GOF_APP_MAX_CHANNELS) {
        set_error("%s: channel counts %d -> %d: the convolution takes C_in and C_out in [1, %d]", who, c_in, c_out, GOF_APP_MAX_CHANNELS);
        return true;
    }
    return false;
}

static bool bad_plane(int32_t c_max, int32_t W, int32_t H, const char* who)
{
    if (W < 1 || H < 1 || (int64_t)W * H * (int64_t)c_max >= ((int64_t)1 << 31) - 256) {
        set_error("%s: bad sizes (%d channels of %d x %d)", who, c_max, W, H);
        return true;
    }
    return false;
}

static bool bad_view(int32_t mode, int32_t C, int32_t W, int32_t H, const float* emb, const char* who)
{
    if (mode < GOF_APP_SRC_PLAIN || mode > GOF_APP_SRC_EMBED) { set_error("%s: unknown operand view %d", who, mode); return true; }
    if ((mode == GOF_APP_SRC_SHUFFLE || mode == GOF_APP_SRC_UP2) && ((W | H) & 1)) { set_error("%s: this view needs even W and H, got %d x %d", who, W, H); return true; }
    if (mode == GOF_APP_SRC_UNSHUFFLE && (C & 3)) { set_error("%s: the inverse pixel-shuffle needs a channel count that is a multiple of 4, got %d", who, C); return true; }
    if (mode == GOF_APP_SRC_EMBED && (C < 3 || (C > 3 && !emb))) { set_error("%s: the embedding view needs at least 3 channels and the embedding", who); return true; }
    return false;
}

static Src make_src(const float* p, int mode, int W, int H, const float* emb, const float* mask)
{
    Src s{ p, mask, emb, mode, W, H, 0.0f, 0.0f };
    if (mode == GOF_APP_SRC_UP2) { s.sy = lerp_scale(H / 2, H); s.sx = lerp_scale(W / 2, W); }
    return s;
}

static int launch_conv(int c_in, int c_out, const Src& src, const float* w, const float* bias, int relu, float* out, hipStream_t stream,
                       const Head* head_or_null = nullptr)
{
    Head head{};
    if (head_or_null) head = *head_or_null;       // (only with c_out == 3: the 256-pixel tile below)
    const int M = src.H * src.W;
#define GOF_LAUNCH_CONV(WN, WGN) hipLaunchKernelGGL((conv3x3_kernel<WN, WGN>), (conv3x3::grid<WN, WGN>(M, c_out)), dim3(256), 0, stream, c_in, c_out, src, w, bias, relu, out, head)
    if (c_out > 64) GOF_LAUNCH_CONV(2, 2);
    else if (c_out > 32) GOF_LAUNCH_CONV(2, 1);
    else GOF_LAUNCH_CONV(1, 1);
#undef GOF_LAUNCH_CONV
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

static int n_chunks_of(int HW) { return (HW + GOF_APP_WGRAD_CHUNK - 1) / GOF_APP_WGRAD_CHUNK; }
static size_t wgrad_partial_floats /* values, fp64 each */(int c_in, int c_out, int HW) { return (size_t)n_chunks_of(HW) * (size_t)c_out * (size_t)(9 * c_in + 1); }

static int launch_wgrad(int c_in, int c_out, const Src& xs, const Src& dys, double* partial, float* dW, float* db, hipStream_t stream)
{
    const int HW = xs.H * xs.W, nc = n_chunks_of(HW), NT = 9 * c_in + 1;
    const dim3 grid((unsigned)nc, (unsigned)((NT + WG_BN - 1) / WG_BN), (unsigned)((c_out + 31) / 32));
    hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, stream, c_in, c_out, xs, dys, partial);
    GOF_LAUNCH_CHECK(stream, 0);
    hipLaunchKernelGGL(wgrad_reduce_kernel, grid_of((int64_t)c_out * NT), dim3(256), 0, stream, nc, c_in, c_out, (const double*)partial, dW, db);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

// ---- the network ------------------------------------------------------------------------------------------------------------------
struct Layer { int c_in, c_out, W, H, mode, relu; };
struct Plan {
    Crop cr;
    int w, h;                 // the low-resolution plane
    Layer L[7];
    size_t act[6];            // floats of the ReLU output of layers 0 .. 5
    size_t grad_floats;       // the larger of any gradient tensor a data gradient writes
    size_t wt_floats;         // the largest weight
    size_t partial_floats;    // the largest set of weight-gradient chunk partials (values; fp64 each)
    size_t l1_blocks;
};

static int make_plan(int32_t W, int32_t H, const GofAppNet* net, Plan* plan)
{
    if (!net) { set_error("appearance: the network description is NULL"); return GOF_E_INVALID; }
    if (W < 32 || H < 32) { set_error("appearance: an image of %d x %d is smaller than 32 in a direction: nothing is left of its crop to multiples of 32", W, H); return GOF_E_INVALID; }
    if ((int64_t)W * H > ((int64_t)1 << 24)) { set_error("appearance: bad image size (%d x %d)", W, H); return GOF_E_INVALID; }
    if (net->n_embed < 0 || net->n_embed > GOF_APP_MAX_CHANNELS - 3) { set_error("appearance: bad embedding length %d", net->n_embed); return GOF_E_INVALID; }
    for (int i = 0; i < 6; i++)
        if (net->width[i] < 1 || net->width[i] > GOF_APP_MAX_CHANNELS || (i < 4 && net->width[i] % 4 != 0)) {
            set_error("appearance: width %d of the network is %d: widths lie in [1, %d] and the four in front of a pixel-shuffle are multiples of 4", i, net->width[i], GOF_APP_MAX_CHANNELS);
            return GOF_E_INVALID;
        }
    Plan pl;
    pl.cr.W = W; pl.cr.H = H;
    pl.cr.Hc = H / 32 * 32; pl.cr.Wc = W / 32 * 32;
    pl.cr.left = W / 2 - pl.cr.Wc / 2; pl.cr.top = H / 2 - pl.cr.Hc / 2;
    pl.h = pl.cr.Hc / 32; pl.w = pl.cr.Wc / 32;
    pl.L[0] = Layer{ 3 + net->n_embed, net->width[0], pl.w, pl.h, GOF_APP_SRC_EMBED, 1 };
    for (int k = 1; k <= 4; k++) pl.L[k] = Layer{ net->width[k - 1] / 4, net->width[k], pl.w << k, pl.h << k, GOF_APP_SRC_SHUFFLE, 1 };
    pl.L[5] = Layer{ net->width[4], net->width[5], pl.cr.Wc, pl.cr.Hc, GOF_APP_SRC_UP2, 1 };
    pl.L[6] = Layer{ net->width[5], 3, pl.cr.Wc, pl.cr.Hc, GOF_APP_SRC_PLAIN, 0 };
    pl.grad_floats = pl.wt_floats = pl.partial_floats = 0;
    for (int k = 0; k < 7; k++) {
        const Layer& l = pl.L[k];
        const size_t px = (size_t)l.W * l.H;
        const int cmax = l.c_in > l.c_out ? l.c_in : l.c_out;
        if ((int64_t)px * cmax >= ((int64_t)1 << 31) - 256) { set_error("appearance: layer %d (%d -> %d channels of %d x %d) is too large", k, l.c_in, l.c_out, l.W, l.H); return GOF_E_INVALID; }
        if (k < 6) pl.act[k] = px * l.c_out;
        if (px * l.c_in > pl.grad_floats) pl.grad_floats = px * l.c_in;
        if ((size_t)9 * l.c_in * l.c_out > pl.wt_floats) pl.wt_floats = (size_t)9 * l.c_in * l.c_out;
        const size_t pf = wgrad_partial_floats(l.c_in, l.c_out, (int)px);
        if (pf > pl.partial_floats) pl.partial_floats = pf;
    }
    pl.l1_blocks = ((size_t)pl.cr.Hc * pl.cr.Wc + 255) / 256;        // = conv3's workgroups (256 pixels each)
    if (plan) *plan = pl;
    return GOF_OK;
}

struct Saved { float* D; float* Y[6]; float* M; };
static size_t saved_layout(const Plan& pl, void* base, Saved* out)
{
    Carver c{ static_cast<char*>(base), 0 };
    Saved s;
    s.D = c.take<float>((size_t)3 * pl.h * pl.w);
    for (int k = 0; k < 6; k++) s.Y[k] = c.take<float>(pl.act[k]);
    s.M = c.take<float>((size_t)3 * pl.cr.Hc * pl.cr.Wc);
    if (out) *out = s;
    return c.total();
}

struct Ws { float* buf[2]; float* wt; double* partial; double* l1; };
static size_t ws_layout(const Plan& pl, void* base, Ws* out)
{
    Carver c{ static_cast<char*>(base), 0 };
    Ws w;
    w.buf[0] = c.take<float>(pl.grad_floats);
    w.buf[1] = c.take<float>(pl.grad_floats);
    w.wt = c.take<float>(pl.wt_floats);
    w.partial = c.take<double>(pl.partial_floats);
    w.l1 = c.take<double>(pl.l1_blocks);
    if (out) *out = w;
    return c.total();
}

static bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const char* pa = static_cast<const char*>(a);
    const char* pb = static_cast<const char*>(b);
    return a && b && pa < pb + nb && pb < pa + na;
}

// the forward operand of layer k
static Src layer_src(const Plan& pl, const Saved& s, int k, const float* embedding)
{
    const Layer& l = pl.L[k];
    return make_src(k == 0 ? s.D : s.Y[k - 1], l.mode, l.W, l.H, k == 0 ? embedding : nullptr, nullptr);
}

} // namespace app
} // namespace gof

using namespace gof;
using namespace gof::app;

extern "C" {

int gof_app_conv3x3(int32_t c_in, int32_t c_out, int32_t W, int32_t H, const float* x, int32_t x_mode, const float* emb, const float* mask,
                    const float* weight, const float* bias, int32_t relu, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_channels(c_in, c_out, "app_conv3x3")) return GOF_E_INVALID;
    if (bad_plane(c_in > c_out ? c_in : c_out, W, H, "app_conv3x3") || bad_view(x_mode, c_in, W, H, emb, "app_conv3x3")) return GOF_E_INVALID;
    if (!x || !weight || !out) { set_error("app_conv3x3: x / weight / out is NULL"); return GOF_E_INVALID; }
    GOF_PROFILE("app_conv3x3", stream);
    return launch_conv(c_in, c_out, make_src(x, x_mode, W, H, emb, mask), weight, bias, relu != 0, out, stream);
}

int gof_app_materialize(int32_t mode, int32_t C, int32_t W, int32_t H, const float* x, const float* emb, const float* mask, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (C < 1 || C > GOF_APP_MAX_CHANNELS || bad_plane(C, W, H, "app_materialize") || bad_view(mode, C, W, H, emb, "app_materialize")) {
        if (C < 1 || C > GOF_APP_MAX_CHANNELS) set_error("app_materialize: bad channel count %d", C);
        return GOF_E_INVALID;
    }
    if (!x || !out) { set_error("app_materialize: x / out is NULL"); return GOF_E_INVALID; }
    hipLaunchKernelGGL(materialize_kernel, grid_of((int64_t)C * W * H), dim3(256), 0, stream, (int)C, make_src(x, mode, W, H, emb, mask), out);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_app_weight_transpose(int32_t c_in, int32_t c_out, const float* weight, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_channels(c_in, c_out, "app_weight_transpose")) return GOF_E_INVALID;
    if (!weight || !out) { set_error("app_weight_transpose: weight / out is NULL"); return GOF_E_INVALID; }
    hipLaunchKernelGGL(weight_transpose_kernel, grid_of((int64_t)9 * c_in * c_out), dim3(256), 0, stream, (int)c_in, (int)c_out, weight, out);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

size_t gof_app_wgrad_workspace_bytes(int32_t c_in, int32_t c_out, int32_t W, int32_t H)
{
    if (bad_channels(c_in, c_out, "app_wgrad") || bad_plane(c_in > c_out ? c_in : c_out, W, H, "app_wgrad")) return 0;
    Carver c{ nullptr, 0 };
    c.take<double>(wgrad_partial_floats(c_in, c_out, W * H));
    return c.total();
}

int gof_app_conv3x3_wgrad(int32_t c_in, int32_t c_out, int32_t W, int32_t H, const float* x, int32_t x_mode, const float* emb,
                          const float* dy, int32_t dy_mode, const float* mask, float* dW, float* db, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t need = gof_app_wgrad_workspace_bytes(c_in, c_out, W, H);
    if (need == 0) return GOF_E_INVALID;
    if (bad_view(x_mode, c_in, W, H, emb, "app_wgrad") || bad_view(dy_mode, c_out, W, H, nullptr, "app_wgrad")) return GOF_E_INVALID;
    if (dy_mode == GOF_APP_SRC_EMBED) { set_error("app_wgrad: dy cannot be read through the embedding view"); return GOF_E_INVALID; }
    if (!x || !dy || !dW || !db) { set_error("app_wgrad: x / dy / dW / db is NULL"); return GOF_E_INVALID; }
    if (!ws) { set_error("app_wgrad: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < need) { set_error("app_wgrad: workspace too small"); return GOF_E_WORKSPACE; }
    GOF_PROFILE("app_wgrad", stream);
    return launch_wgrad(c_in, c_out, make_src(x, x_mode, W, H, emb, nullptr), make_src(dy, dy_mode, W, H, nullptr, mask),
                        static_cast<double*>(ws_aligned(ws)), dW, db, stream);
}

int gof_app_bilinear(int32_t C, int32_t in_W, int32_t in_H, int64_t in_row_stride, int64_t in_plane_stride, const float* x,
                     int32_t out_W, int32_t out_H, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (C < 1 || C > GOF_APP_MAX_CHANNELS || in_W < 1 || in_H < 1 || in_row_stride < in_W || in_plane_stride < 0 || bad_plane(C, out_W, out_H, "app_bilinear")) {
        set_error("app_bilinear: bad sizes (%d planes of %d x %d -> %d x %d)", C, in_W, in_H, out_W, out_H);
        return GOF_E_INVALID;
    }
    if (!x || !out) { set_error("app_bilinear: x / out is NULL"); return GOF_E_INVALID; }
    hipLaunchKernelGGL(bilinear_kernel, grid_of((int64_t)C * out_W * out_H), dim3(256), 0, stream, (int)C, (int)in_W, (int)in_H, in_row_stride,
                       in_plane_stride, x, (int)out_W, (int)out_H, lerp_scale(in_H, out_H), lerp_scale(in_W, out_W), out);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_app_up2_backward(int32_t C, int32_t W, int32_t H, const float* g, float* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (C < 1 || C > GOF_APP_MAX_CHANNELS || bad_plane(4 * C, W, H, "app_up2_backward")) {
        if (C < 1 || C > GOF_APP_MAX_CHANNELS) set_error("app_up2_backward: bad channel count %d", C);
        return GOF_E_INVALID;
    }
    if (!g || !out) { set_error("app_up2_backward: g / out is NULL"); return GOF_E_INVALID; }
    hipLaunchKernelGGL(up2_backward_kernel, grid_of((int64_t)C * W * H), dim3(256), 0, stream, (int)C, (int)W, (int)H, lerp_scale(H, 2 * H),
                       lerp_scale(W, 2 * W), g, out);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

static bool crop_of(int32_t W, int32_t H, Crop* cr, const char* who)
{
    if (W < 32 || H < 32 || (int64_t)W * H > ((int64_t)1 << 24)) { set_error("%s: bad image size (%d x %d): at least 32 in both directions", who, W, H); return false; }
    cr->W = W; cr->H = H;
    cr->Hc = H / 32 * 32; cr->Wc = W / 32 * 32;
    cr->left = W / 2 - cr->Wc / 2; cr->top = H / 2 - cr->Hc / 2;
    return true;
}

size_t gof_app_head_workspace_bytes(int32_t W, int32_t H)
{
    Crop cr;
    if (!crop_of(W, H, &cr, "app_head")) return 0;
    Carver c{ nullptr, 0 };
    c.take<double>(((size_t)cr.Hc * cr.Wc + 255) / 256);
    return c.total();
}

int gof_app_head_forward(int32_t W, int32_t H, const float* z, const float* image, const float* gt, float* m_out, float* transformed, float* loss,
                         void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Crop cr;
    if (!crop_of(W, H, &cr, "app_head_forward")) return GOF_E_INVALID;
    if (!z || !image || !gt || !m_out || !loss || !ws) { set_error("app_head_forward: an argument is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_app_head_workspace_bytes(W, H)) { set_error("app_head_forward: workspace too small"); return GOF_E_WORKSPACE; }
    const int blocks = (cr.Hc * cr.Wc + 255) / 256;
    double* partial = static_cast<double*>(ws_aligned(ws));
    const Head head{ image, gt, m_out, transformed, partial, nullptr, 0.0f, cr, 1 };
    hipLaunchKernelGGL(head_forward_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, head, z);
    GOF_LAUNCH_CHECK(stream, 0);
    hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, stream, blocks, (const double*)partial, (double)((size_t)3 * cr.Hc * cr.Wc), loss);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_app_head_backward(int32_t W, int32_t H, const float* m, const float* image, const float* gt, const float* dL, float* dz, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Crop cr;
    if (!crop_of(W, H, &cr, "app_head_backward")) return GOF_E_INVALID;
    if (!m || !image || !gt || !dL || !dz) { set_error("app_head_backward: an argument is NULL"); return GOF_E_INVALID; }
    Src src = make_src(m, SRC_HEAD, cr.Wc, cr.Hc, nullptr, nullptr);
    src.head = Head{ image, gt, nullptr, nullptr, nullptr, dL, (float)((size_t)3 * cr.Hc * cr.Wc), cr, 0 };
    hipLaunchKernelGGL(materialize_kernel, grid_of((int64_t)3 * cr.Wc * cr.Hc), dim3(256), 0, stream, 3, src, dz);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_app_image_grad(int32_t W, int32_t H, const float* m, const float* image, const float* gt, const float* dL, const float* d_down,
                       float* d_image, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Crop cr;
    if (!crop_of(W, H, &cr, "app_image_grad")) return GOF_E_INVALID;
    if (!m || !image || !gt || !dL || !d_down || !d_image) { set_error("app_image_grad: an argument is NULL"); return GOF_E_INVALID; }
    const int h = cr.Hc / 32, w = cr.Wc / 32;
    hipLaunchKernelGGL(image_grad_kernel, grid_of((int64_t)3 * W * H), dim3(256), 0, stream, cr, w, h, lerp_scale(cr.Hc, h), lerp_scale(cr.Wc, w),
                       m, image, gt, dL, (float)((size_t)3 * cr.Hc * cr.Wc), d_down, d_image);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

size_t gof_app_saved_bytes(int32_t W, int32_t H, const GofAppNet* net_host)
{
    Plan pl;
    if (make_plan(W, H, net_host, &pl) != GOF_OK) return 0;
    return saved_layout(pl, nullptr, nullptr);
}

size_t gof_app_workspace_bytes(int32_t W, int32_t H, const GofAppNet* net_host)
{
    Plan pl;
    if (make_plan(W, H, net_host, &pl) != GOF_OK) return 0;
    return ws_layout(pl, nullptr, nullptr);
}

int gof_app_l1_forward(int32_t W, int32_t H, const GofAppNet* net_host, const float* image, const float* gt, const float* embedding,
                       const float* const* params_host, float* loss, float* transformed, void* saved, size_t saved_bytes,
                       void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Plan pl;
    const int rc = make_plan(W, H, net_host, &pl);
    if (rc != GOF_OK) return rc;
    if (!image || !gt || !params_host || !loss || (net_host->n_embed > 0 && !embedding)) { set_error("app_l1_forward: an argument is NULL"); return GOF_E_INVALID; }
    for (int i = 0; i < GOF_APP_N_PARAMS; i++)
        if (!params_host[i]) { set_error("app_l1_forward: parameter %d is NULL", i); return GOF_E_INVALID; }
    if (!saved || !ws) { set_error("app_l1_forward: the saved buffer / workspace is NULL"); return GOF_E_INVALID; }
    const size_t sb = saved_layout(pl, nullptr, nullptr), wb = ws_layout(pl, nullptr, nullptr);
    if (saved_bytes < sb || ws_bytes < wb) { set_error("app_l1_forward: the saved buffer / workspace is too small"); return GOF_E_WORKSPACE; }
    const size_t img_bytes = (size_t)3 * W * H * sizeof(float), crop_bytes = (size_t)3 * pl.cr.Wc * pl.cr.Hc * sizeof(float);
    const void* ins[2] = { image, gt };
    for (int i = 0; i < 2; i++)
        if (overlaps(ins[i], img_bytes, loss, sizeof(float)) || overlaps(ins[i], img_bytes, transformed, crop_bytes) || overlaps(ins[i], img_bytes, saved, saved_bytes)
            || overlaps(ins[i], img_bytes, ws, ws_bytes)) {
            set_error("app_l1_forward: an output overlaps an input image");
            return GOF_E_INVALID;
        }
    if (overlaps(saved, saved_bytes, ws, ws_bytes) || overlaps(saved, saved_bytes, transformed, crop_bytes) || overlaps(saved, saved_bytes, loss, sizeof(float))) {
        set_error("app_l1_forward: the saved buffer overlaps another output");
        return GOF_E_INVALID;
    }
    Saved s;
    saved_layout(pl, ws_aligned(saved), &s);
    Ws w;
    ws_layout(pl, ws_aligned(ws), &w);
    GOF_PROFILE("app_l1_forward", stream);

    const Crop& cr = pl.cr;
    hipLaunchKernelGGL(bilinear_kernel, grid_of((int64_t)3 * pl.h * pl.w), dim3(256), 0, stream, 3, cr.Wc, cr.Hc, (int64_t)W, (int64_t)W * H,
                       image + (size_t)cr.top * W + cr.left, pl.w, pl.h, lerp_scale(cr.Hc, pl.h), lerp_scale(cr.Wc, pl.w), s.D);
    GOF_LAUNCH_CHECK(stream, 0);
    Head head{ image, gt, s.M, transformed, w.l1, nullptr, 0.0f, cr, 1 };
    for (int k = 0; k < 7; k++) {
        const Layer& l = pl.L[k];
        const int r = launch_conv(l.c_in, l.c_out, layer_src(pl, s, k, embedding), params_host[2 * k], params_host[2 * k + 1], l.relu,
                                  k < 6 ? s.Y[k] : nullptr, stream, k < 6 ? nullptr : &head);      // conv3: the head is its epilogue
        if (r != GOF_OK) return r;
    }
    hipLaunchKernelGGL(sum_finish_kernel, dim3(1), dim3(256), 0, stream, (int)pl.l1_blocks, (const double*)w.l1, (double)((size_t)3 * cr.Hc * cr.Wc), loss);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_app_l1_backward(int32_t W, int32_t H, const GofAppNet* net_host, const float* image, const float* gt, const float* embedding,
                        const float* const* params_host, const float* dL, const void* saved, size_t saved_bytes,
                        float* d_image, float* d_embedding, float* const* d_params_host, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Plan pl;
    const int rc = make_plan(W, H, net_host, &pl);
    if (rc != GOF_OK) return rc;
    if (!image || !gt || !params_host || !dL || !d_image || !d_params_host || (net_host->n_embed > 0 && (!embedding || !d_embedding))) {
        set_error("app_l1_backward: an argument is NULL");
        return GOF_E_INVALID;
    }
    for (int i = 0; i < GOF_APP_N_PARAMS; i++)
        if (!params_host[i] || !d_params_host[i]) { set_error("app_l1_backward: parameter %d or its gradient is NULL", i); return GOF_E_INVALID; }
    if (!saved || !ws) { set_error("app_l1_backward: the saved buffer / workspace is NULL"); return GOF_E_INVALID; }
    const size_t sb = saved_layout(pl, nullptr, nullptr), wb = ws_layout(pl, nullptr, nullptr);
    if (saved_bytes < sb || ws_bytes < wb) { set_error("app_l1_backward: the saved buffer / workspace is too small"); return GOF_E_WORKSPACE; }
    const size_t img_bytes = (size_t)3 * W * H * sizeof(float);
    if (overlaps(d_image, img_bytes, image, img_bytes) || overlaps(d_image, img_bytes, gt, img_bytes) || overlaps(d_image, img_bytes, saved, saved_bytes)
        || overlaps(d_image, img_bytes, ws, ws_bytes) || overlaps(saved, saved_bytes, ws, ws_bytes)) {
        set_error("app_l1_backward: an output overlaps an input");
        return GOF_E_INVALID;
    }
    Saved s;
    saved_layout(pl, ws_aligned(const_cast<void*>(saved)), &s);
    Ws w;
    ws_layout(pl, ws_aligned(ws), &w);
    GOF_PROFILE("app_l1_backward", stream);

    const Crop& cr = pl.cr;
    const float count = (float)((size_t)3 * cr.Hc * cr.Wc);
    // dys: the gradient with respect to the output of layer k as the layer's backward reads it; cur: the buffer the next data gradient writes
    // conv3's gradient reads dz through the head view: sign, product and sigmoid' are formed from the saved sigmoid while staging
    Src dys = make_src(s.M, SRC_HEAD, cr.Wc, cr.Hc, nullptr, nullptr);
    dys.head = Head{ image, gt, nullptr, nullptr, nullptr, dL, count, cr, 0 };
    int cur = 0;
    for (int k = 6; k >= 0; k--) {
        const Layer& l = pl.L[k];
        int r = launch_wgrad(l.c_in, l.c_out, layer_src(pl, s, k, embedding), dys, w.partial, d_params_host[2 * k], d_params_host[2 * k + 1], stream);
        if (r != GOF_OK) return r;
        hipLaunchKernelGGL(weight_transpose_kernel, grid_of((int64_t)9 * l.c_in * l.c_out), dim3(256), 0, stream, l.c_in, l.c_out, params_host[2 * k], w.wt);
        GOF_LAUNCH_CHECK(stream, 0);
        r = launch_conv(l.c_out, l.c_in, dys, w.wt, nullptr, 0, w.buf[cur], stream);       // dX [c_in][l.H][l.W]: the view's plane
        if (r != GOF_OK) return r;
        if (k == 0) break;
        const Layer& b = pl.L[k - 1];                                                       // the layer whose ReLU output the view reads
        if (l.mode == GOF_APP_SRC_UP2) {
            hipLaunchKernelGGL(up2_backward_kernel, grid_of((int64_t)l.c_in * b.W * b.H), dim3(256), 0, stream, l.c_in, b.W, b.H, lerp_scale(b.H, l.H),
                               lerp_scale(b.W, l.W), (const float*)w.buf[cur], w.buf[cur ^ 1]);
            GOF_LAUNCH_CHECK(stream, 0);
            cur ^= 1;
            dys = make_src(w.buf[cur], GOF_APP_SRC_PLAIN, b.W, b.H, nullptr, s.Y[k - 1]);
        } else if (l.mode == GOF_APP_SRC_SHUFFLE) {
            dys = make_src(w.buf[cur], GOF_APP_SRC_UNSHUFFLE, b.W, b.H, nullptr, s.Y[k - 1]);
        } else {
            dys = make_src(w.buf[cur], GOF_APP_SRC_PLAIN, b.W, b.H, nullptr, s.Y[k - 1]);
        }
        cur ^= 1;
    }
    // w.buf[cur]: dX1 [3 + n_embed][h][w]
    const int hw = pl.h * pl.w;
    if (net_host->n_embed > 0) {
        hipLaunchKernelGGL(embedding_grad_kernel, grid_of(net_host->n_embed), dim3(256), 0, stream, (int)net_host->n_embed, hw, (const float*)w.buf[cur], d_embedding);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    hipLaunchKernelGGL(image_grad_kernel, grid_of((int64_t)3 * W * H), dim3(256), 0, stream, cr, pl.w, pl.h, lerp_scale(cr.Hc, pl.h), lerp_scale(cr.Wc, pl.w),
                       (const float*)s.M, image, gt, dL, count, (const float*)w.buf[cur], d_image);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // extern "C"
