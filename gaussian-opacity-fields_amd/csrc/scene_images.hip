// scene_images.hip -- the training images' resampler on HIP (C ABI in include/gof_image_hip.h).
//
// loadCam (reference utils/camera_utils.py:19-54) shrinks every image of the scene with Pillow's bicubic Image.resize, turns it into
// float with np.array(...) / 255.0 and permutes it to planes (utils/general_utils.py:21-27), on one CPU thread.  Here: the coefficient
// tables of Pillow's 8-bit resampler on the host (double, no contraction), and two kernels that apply them in integers -- every sum is
// exact, so any tiling gives Pillow's bytes:
//
//   resize_h:  interleaved bytes [in_h][pitch] -> interleaved bytes [in_h][out_w * C] (the 8-bit image between the passes).  One
//              workgroup = 4 waves = 4 source rows x 64 output pixels; a wave stages its row's input window in LDS with aligned dword
//              loads (the ragged first and last word byte by byte: nothing outside the row is read), in chunks of 2 KB, so a window of
//              any width (257 taps at a 64-fold reduction, a whole row for one output pixel) goes through the same loop; lane = output
//              pixel, all channels.  The table is stored transposed ([tap][output]) so that the lanes read it coalesced.
//   resize_v:  interleaved bytes -> float planes [C][out_h][out_w].  One workgroup = one output row x 256 pixels; a lane accumulates 4
//              consecutive bytes of the row (one dword load per tap where the rows are 4-byte aligned: the rows are contiguous along x,
//              the coefficient is the same for the whole workgroup), the 8-bit results pass through LDS so that each plane is stored
//              as 256 consecutive floats.  byte -> float goes through a 256-entry table in LDS, each entry the IEEE quotient
//              (float)b / 255.0f (correctly rounded: the division torch's CPU kernel performs).  A vertical axis whose length does not
//              change runs as the identity (first = y, one tap of 2^22): the conversion with no table.
// Both are bound by memory: ~2 C bytes moved per source pixel, 4 C per output pixel.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>
#include "../../include/gof_hip.h"
#include "../../include/gof_image_hip.h"
#include "gof_common.h"

namespace gof {
namespace scene_images {

constexpr int THREADS = 256;
constexpr int PRECISION_BITS = 22;              // 32 - 8 - 2: Pillow's fixed point for 8-bit bands
constexpr int H_PIXELS = 64;                    // output pixels per wave of resize_h
constexpr int H_ROWS = THREADS / 64;            // source rows per workgroup: one per wave
constexpr int H_CHUNK = 2048;                   // bytes of a row's window staged at a time
constexpr int H_ROW_LDS = H_CHUNK + 16;         // + the misalignment (<= 3) and the rounding up to a whole word, kept a multiple of 16
constexpr int V_PIXELS = 256;                   // output pixels per workgroup of resize_v

__device__ __forceinline__ int clip8(int32_t s)
{
    const int32_t v = s >> PRECISION_BITS;      // (arithmetic shift: a negative sum stays negative)
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// bounds: [out_w][2] (first, count); coef_t: [taps][out_w]
template <int C>
__global__ void __launch_bounds__(THREADS)
resize_h(const uint8_t* __restrict__ src, int64_t pitch, int in_h, int out_w, const int32_t* __restrict__ bounds,
         const int32_t* __restrict__ coef_t, uint8_t* __restrict__ tmp, int64_t tpitch)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[H_ROWS][H_ROW_LDS];
    constexpr int CHUNK_PIXELS = H_CHUNK / C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * H_PIXELS;
    const int x = x0 + lane;
    const int y = blockIdx.y * H_ROWS + wave;
    const bool row_ok = y < in_h;
    const int last = min(x0 + H_PIXELS, out_w) - 1;
    const int lo = bounds[2 * x0], hi = bounds[2 * last] + bounds[2 * last + 1];        // the workgroup's window [lo, hi): first and first + count grow with x
    int first = 0, count = 0;
    if (x < out_w) { first = bounds[2 * x]; count = bounds[2 * x + 1]; }
    int32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << (PRECISION_BITS - 1);
    uint8_t* s_row = s_win[wave];
    for (int c0 = lo; c0 < hi; c0 += CHUNK_PIXELS) {
        const int c1 = min(hi, c0 + CHUNK_PIXELS);
        int mis = 0;
        if (row_ok) {
            const uint8_t* g = src + (int64_t)y * pitch + (int64_t)c0 * C;
            const int nbytes = (c1 - c0) * C;
            mis = (int)(reinterpret_cast<uintptr_t>(g) & 3u);
            const uint8_t* base = g - mis;                                              // 4-byte aligned; base[mis .. mis + nbytes) is the row's
            const int nd = (mis + nbytes + 3) >> 2;
            uint32_t* s32 = reinterpret_cast<uint32_t*>(s_row);
            for (int d = lane; d < nd; d += 64) {
                const int b0 = 4 * d;
                uint32_t word;
                if (b0 >= mis && b0 + 4 <= mis + nbytes) {
                    word = *reinterpret_cast<const uint32_t*>(base + b0);
                } else {
                    word = 0u;
                    for (int b = 0; b < 4; b++)
                        if (b0 + b >= mis && b0 + b < mis + nbytes) word |= (uint32_t)base[b0 + b] << (8 * b);
                }
                s32[d] = word;
            }
        }
        __syncthreads();
        if (row_ok) {
            const int k0 = max(0, c0 - first), k1 = min(count, c1 - first);
            for (int k = k0; k < k1; k++) {
                const int32_t w = coef_t[(int64_t)k * out_w + x];
                const uint8_t* p = s_row + mis + (first + k - c0) * C;                  // first + k lies in [c0, c1)
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] += (int32_t)p[c] * w;
            }
        }
        __syncthreads();
    }
    if (row_ok && x < out_w) {
        uint8_t* o = tmp + (int64_t)y * tpitch + (int64_t)x * C;
#pragma unroll
        for (int c = 0; c < C; c++) o[c] = (uint8_t)clip8(acc[c]);
    }
}

// img: [rows][ipitch] interleaved bytes of width w; bounds: [out_h][2]; coef: [out_h][taps]; identity: out_h == rows, no table
template <int C>
__global__ void __launch_bounds__(THREADS)
resize_v(const uint8_t* __restrict__ img, int64_t ipitch, int w, int out_h, const int32_t* __restrict__ bounds,
         const int32_t* __restrict__ coef, int taps, int identity, int vec, float* __restrict__ out)
{
    __shared__ float s_lut[256];
    __shared__ __attribute__((aligned(16))) uint8_t s_res[V_PIXELS * C];
    const int tid = threadIdx.x;
    s_lut[tid] = (float)tid / 255.0f;                                                   // IEEE division, correctly rounded
    const int y = blockIdx.y;
    const int x0 = blockIdx.x * V_PIXELS;
    const int npix = min(V_PIXELS, w - x0);
    const int n = npix * C;                                                             // bytes of the row this workgroup owns
    const int e0 = 4 * tid;
    int first = y, count = 1;
    if (!identity) { first = bounds[2 * y]; count = bounds[2 * y + 1]; }
    if (e0 < n) {
        int32_t acc[4];
#pragma unroll
        for (int b = 0; b < 4; b++) acc[b] = 1 << (PRECISION_BITS - 1);
        const bool whole = vec && e0 + 4 <= n;
        const uint8_t* col = img + (int64_t)first * ipitch + (int64_t)x0 * C + e0;
        for (int k = 0; k < count; k++) {
            const int32_t wk = identity ? (1 << PRECISION_BITS) : coef[(int64_t)y * taps + k];
            const uint8_t* p = col + (int64_t)k * ipitch;
            if (whole) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
                for (int b = 0; b < 4; b++) acc[b] += (int32_t)((v >> (8 * b)) & 0xFFu) * wk;
            } else {
#pragma unroll
                for (int b = 0; b < 4; b++)
                    if (e0 + b < n) acc[b] += (int32_t)p[b] * wk;
            }
        }
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (e0 + b < n) s_res[e0 + b] = (uint8_t)clip8(acc[b]);
    }
    __syncthreads();
    if (tid < npix) {
        const size_t plane = (size_t)out_h * (size_t)w;
        float* o = out + (size_t)y * (size_t)w + (size_t)(x0 + tid);
#pragma unroll
        for (int c = 0; c < C; c++) o[c * plane] = s_lut[s_res[tid * C + c]];
    }
}

// ---- the coefficient tables (host) ----------------------------------------------------------------------------------------------------
// Compiled with floating-point contraction OFF (the library's -ffp-contract=off, and the pragmas below for whoever builds this file
// alone): a fused multiply-add in the polynomial can move a weight by one unit in the last place and flip a rounded coefficient.
static double bicubic(double x)
{
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

static bool bad_len(int64_t n) { return n < 1 || n > GOF_IMAGE_MAX_DIM; }

static int taps_of(int n_in, int n_out)
{
    const double scale = (double)n_in / (double)n_out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    return (int)std::ceil(2.0 * filterscale) * 2 + 1;
}

// bounds [n_out][2]; coeffs [n_out][taps], or transposed [taps][n_out]
static void fill_tables(int n_in, int n_out, int32_t* bounds, int32_t* coeffs, bool transposed)
{
#pragma clang fp contract(off)
    const double scale = (double)n_in / (double)n_out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const int taps = taps_of(n_in, n_out);
    std::vector<double> w((size_t)taps);
    for (int xx = 0; xx < n_out; xx++) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        if (xmax > taps) xmax = taps;               // (cannot happen: two truncations of numbers 2 support apart; keeps the row inside its table whatever the rounding)
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) {
            w[x] = bicubic((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        for (int x = 0; x < taps; x++) {
            int32_t k = 0;
            if (x < xmax) {
                const double v = ww != 0.0 ? w[x] / ww : w[x];
                k = v < 0 ? (int32_t)(-0.5 + v * (1 << PRECISION_BITS)) : (int32_t)(0.5 + v * (1 << PRECISION_BITS));
            }
            coeffs[transposed ? (size_t)x * n_out + xx : (size_t)xx * taps + x] = k;
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

static size_t table_bytes(int n_in, int n_out) { return ((size_t)2 + (size_t)taps_of(n_in, n_out)) * (size_t)n_out * sizeof(int32_t); }

// The tables of the axes seen so far, in page-locked host memory (an asynchronous copy reads them after the call has returned): found or
// made under a lock, never moved.  A scene has a handful of image sizes; when the cache is full the device is drained once and the
// cache emptied.
struct Table { int n_in, n_out, transposed, taps; int32_t* host; size_t bytes; };
static std::mutex g_lock;
static std::vector<Table> g_tables;
constexpr size_t MAX_TABLES = 64;

static int get_table(int n_in, int n_out, bool transposed, Table* out)
{
    std::lock_guard<std::mutex> hold(g_lock);
    for (const Table& t : g_tables)
        if (t.n_in == n_in && t.n_out == n_out && t.transposed == (int)transposed) { *out = t; return GOF_OK; }
    if (g_tables.size() >= MAX_TABLES) {
        GOF_HIP_CHECK(hipDeviceSynchronize());
        for (Table& t : g_tables) (void)hipHostFree(t.host);
        g_tables.clear();
    }
    Table t{ n_in, n_out, (int)transposed, taps_of(n_in, n_out), nullptr, table_bytes(n_in, n_out) };
    GOF_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&t.host), t.bytes, 0));
    fill_tables(n_in, n_out, t.host, t.host + 2 * (size_t)n_out, transposed);
    g_tables.push_back(t);
    *out = t;
    return GOF_OK;
}

struct Layout { size_t tab_h, tab_v, tmp, total; int64_t tpitch; bool do_h, do_v; };

static bool bad_args(const GofImageResize* a)
{
    return !a || bad_len(a->in_w) || bad_len(a->in_h) || bad_len(a->out_w) || bad_len(a->out_h)
           || (a->channels != 1 && a->channels != 3 && a->channels != 4) || a->pitch < (int64_t)a->in_w * a->channels;
}

static Layout layout_of(const GofImageResize* a)
{
    Layout l{};
    l.do_h = a->out_w != a->in_w;
    l.do_v = a->out_h != a->in_h;
    l.tpitch = ((int64_t)a->out_w * a->channels + 3) / 4 * 4;
    size_t off = 0;
    l.tab_h = off; off += l.do_h ? align_up(table_bytes(a->in_w, a->out_w)) : 0;
    l.tab_v = off; off += l.do_v ? align_up(table_bytes(a->in_h, a->out_h)) : 0;
    l.tmp = off;   off += l.do_h ? align_up((size_t)l.tpitch * (size_t)a->in_h) : 0;
    l.total = off < ALIGN ? ALIGN : off;
    return l;
}

template <int C>
static int launch(const GofImageResize* a, const Layout& l, const uint8_t* src, float* out, uint8_t* ws, hipStream_t stream)
{
    const uint8_t* img = src;
    int64_t ipitch = a->pitch;
    if (l.do_h) {
        Table t;
        if (int rc = get_table(a->in_w, a->out_w, true, &t)) return rc;
        int32_t* tab = reinterpret_cast<int32_t*>(ws + l.tab_h);
        GOF_HIP_CHECK(hipMemcpyAsync(tab, t.host, t.bytes, hipMemcpyHostToDevice, stream));
        uint8_t* tmp = ws + l.tmp;
        GOF_PROFILE("image_resize_h", stream);
        hipLaunchKernelGGL(resize_h<C>, dim3((unsigned)((a->out_w + H_PIXELS - 1) / H_PIXELS), (unsigned)((a->in_h + H_ROWS - 1) / H_ROWS)), dim3(THREADS), 0,
                           stream, src, a->pitch, (int)a->in_h, (int)a->out_w, tab, tab + 2 * (size_t)a->out_w, tmp, l.tpitch);
        GOF_LAUNCH_CHECK(stream, 0);
        img = tmp;
        ipitch = l.tpitch;
    }
    const int32_t* vb = nullptr;
    int taps = 0;
    if (l.do_v) {
        Table t;
        if (int rc = get_table(a->in_h, a->out_h, false, &t)) return rc;
        int32_t* tab = reinterpret_cast<int32_t*>(ws + l.tab_v);
        GOF_HIP_CHECK(hipMemcpyAsync(tab, t.host, t.bytes, hipMemcpyHostToDevice, stream));
        vb = tab;
        taps = t.taps;
    }
    const int vec = ((reinterpret_cast<uintptr_t>(img) | (uintptr_t)ipitch) & 3u) == 0 ? 1 : 0;     // (a workgroup's span starts at a multiple of 256 C bytes)
    GOF_PROFILE("image_resize_v", stream);
    hipLaunchKernelGGL(resize_v<C>, dim3((unsigned)((a->out_w + V_PIXELS - 1) / V_PIXELS), (unsigned)a->out_h), dim3(THREADS), 0, stream, img, ipitch,
                       (int)a->out_w, (int)a->out_h, vb, vb ? vb + 2 * (size_t)a->out_h : nullptr, taps, l.do_v ? 0 : 1, vec, out);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // namespace scene_images
} // namespace gof

using namespace gof;
using namespace gof::scene_images;

extern "C" {

int gof_image_abi_version(void) { return GOF_IMAGE_ABI_VERSION; }

int64_t gof_image_taps(int32_t n_in, int32_t n_out)
{
    return (bad_len(n_in) || bad_len(n_out)) ? -1 : (int64_t)taps_of(n_in, n_out);
}

int gof_image_coeffs(int32_t n_in, int32_t n_out, int32_t* bounds, int32_t* coeffs)
{
    if (bad_len(n_in) || bad_len(n_out)) { set_error("image_coeffs: lengths %d -> %d: both must lie in 1..%d", n_in, n_out, GOF_IMAGE_MAX_DIM); return GOF_E_INVALID; }
    if (!bounds || !coeffs) { set_error("image_coeffs: a pointer is NULL"); return GOF_E_INVALID; }
    fill_tables(n_in, n_out, bounds, coeffs, false);
    return GOF_OK;
}

size_t gof_image_resize_ws_bytes(const GofImageResize* args)
{
    return bad_args(args) ? 0 : layout_of(args).total;
}

int gof_image_resize(const GofImageResize* a, const void* src, float* out, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!a) { set_error("image_resize: the arguments are NULL"); return GOF_E_INVALID; }
    if (bad_len(a->in_w) || bad_len(a->in_h) || bad_len(a->out_w) || bad_len(a->out_h)) {
        set_error("image_resize: %d x %d -> %d x %d: every size must lie in 1..%d", a->in_w, a->in_h, a->out_w, a->out_h, GOF_IMAGE_MAX_DIM);
        return GOF_E_INVALID;
    }
    if (a->channels != 1 && a->channels != 3 && a->channels != 4) { set_error("image_resize: %d channels (1, 3 or 4)", a->channels); return GOF_E_INVALID; }
    if (a->pitch < (int64_t)a->in_w * a->channels) {
        set_error("image_resize: a pitch of %lld bytes is smaller than a row of %d pixels of %d channels", (long long)a->pitch, a->in_w, a->channels);
        return GOF_E_INVALID;
    }
    if (!src || !out || !ws) { set_error("image_resize: a pointer is NULL"); return GOF_E_INVALID; }
    if (reinterpret_cast<uintptr_t>(ws) & 15u) { set_error("image_resize: the workspace must be 16-byte aligned"); return GOF_E_INVALID; }
    const Layout l = layout_of(a);
    if (ws_bytes < l.total) { set_error("image_resize: the workspace has %zu bytes, gof_image_resize_ws_bytes gives %zu", ws_bytes, l.total); return GOF_E_WORKSPACE; }
    const uint8_t* s = static_cast<const uint8_t*>(src);
    uint8_t* w = static_cast<uint8_t*>(ws);
    switch (a->channels) {
    case 1: return launch<1>(a, l, s, out, w, stream);
    case 3: return launch<3>(a, l, s, out, w, stream);
    default: return launch<4>(a, l, s, out, w, stream);
    }
}

} // extern "C"
