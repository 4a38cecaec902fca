// mesh_raster_dev.h -- what the two rasterisers share: the geometry, coverage and z-buffer of DESIGN.md 3.19 (csrc/mesh_raster.hip: the depth
// image of include/gof_mesh_hip.h (e)) with the pixel word as a template parameter (csrc/mesh_render.hip: depth and face of (g2)), the
// check of faces and view records, and the workspace both carve.  FACE = false is the 32-bit path of (e), instruction for instruction.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cfloat>
#include "../../include/gof_hip.h"
#include "../../include/gof_mesh_hip.h"
#include "gof_common.h"
#include "gof_geom.h"

namespace gof {

namespace raster {

constexpr int INLINE_MAX = 4;                 // box side in pixels up to which the setup thread rasterises
constexpr int TILE_W = 8, TILE_H = 8;         // one wave, one pixel per lane
constexpr int STRIPES = 8;                    // workgroups that share one list entry
constexpr int LARGE_GROUPS = 256;             // entries in flight: the grid of raster_large is LARGE_GROUPS * STRIPES workgroups
constexpr int GUARD_PX = 4096;                // the guard band around the image (why no edge function can overflow)
constexpr int MAX_SIDE = 16384;               // W, H <= MAX_SIDE
constexpr int DEFAULT_BATCH = 8;              // views rendered before they are counted (gof_mesh_visibility with batch = 0)
constexpr int MAX_BATCH = 4096;
constexpr int64_t LIST_MIN = 4096;            // list capacity = LIST_MIN + NF / 8 entries
constexpr uint32_t F_INDEX = 1u, F_VIEW = 2u;
constexpr int HDR_WORDS = 8;                  // u32: [0] flags, [1] list cursor
constexpr int STAT_WORDS = 8;                 // u64: [0] fan triangles with a pixel box, [1] of them listed, [2] of them refused by a full list,
                                              //      [3] atomics issued, [4] pixels that passed coverage and depth range
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr int64_t RASTER_MAX_COUNT = ((int64_t)1 << 31) - 1;
constexpr int M_STATS = 1, M_FACE = 2;        // MODE of the kernels: count what is drawn; the pixel word carries the face (g2)
constexpr u64 EMPTY64 = ~0ull;

struct P3 { double x, y, z; };
struct PV { double x, y, w; };                // image plane: pixel coordinates and 1 / z
struct Tri { int32_t ax, ay, bx, by, cx, cy; double wa, wb, wc; };
struct __attribute__((aligned(64))) LargeTri { Tri t; int32_t view; int32_t pad[3]; };      // pad[0]: the face (M_FACE; else 0)
static_assert(sizeof(LargeTri) == 64, "one line per list entry");

__device__ __forceinline__ int64_t mul64(int32_t a, int32_t b) { return (int64_t)a * (int64_t)b; }
__device__ __forceinline__ bool top_left(int32_t dx, int32_t dy) { return dy < 0 || (dy == 0 && dx > 0); }

// snap and orient: false for a zero-area triangle.  B and C change places where the area is negative (both orientations are drawn).
__device__ __forceinline__ bool tri_setup(const PV& A, const PV& B, const PV& C, Tri& t, int64_t& area)
{
    t.ax = (int32_t)rint(A.x * 256.0); t.ay = (int32_t)rint(A.y * 256.0);
    t.bx = (int32_t)rint(B.x * 256.0); t.by = (int32_t)rint(B.y * 256.0);
    t.cx = (int32_t)rint(C.x * 256.0); t.cy = (int32_t)rint(C.y * 256.0);
    t.wa = A.w; t.wb = B.w; t.wc = C.w;
    area = mul64(t.bx - t.ax, t.cy - t.ay) - mul64(t.by - t.ay, t.cx - t.ax);
    if (area == 0) return false;
    if (area < 0) {
        int32_t i = t.bx; t.bx = t.cx; t.cx = i;
        i = t.by; t.by = t.cy; t.cy = i;
        const double w = t.wb; t.wb = t.wc; t.wc = w;
        area = -area;
    }
    return true;
}

__device__ __forceinline__ int64_t tri_area(const Tri& t) { return mul64(t.bx - t.ax, t.cy - t.ay) - mul64(t.by - t.ay, t.cx - t.ax); }

// the pixel (i, j): covered and inside the depth range -> the bits of its float depth
__device__ __forceinline__ bool tri_pixel(const Tri& t, int64_t area, int i, int j, double zfar, uint32_t& bits)
{
    const int32_t px = 256 * i + 128, py = 256 * j + 128;
    const int64_t e0 = mul64(t.cx - t.bx, py - t.by) - mul64(t.cy - t.by, px - t.bx);
    const int64_t e1 = mul64(t.ax - t.cx, py - t.cy) - mul64(t.ay - t.cy, px - t.cx);
    const int64_t e2 = mul64(t.bx - t.ax, py - t.ay) - mul64(t.by - t.ay, px - t.ax);
    const bool in = (e0 > 0 || (e0 == 0 && top_left(t.cx - t.bx, t.cy - t.by))) &&
                    (e1 > 0 || (e1 == 0 && top_left(t.ax - t.cx, t.ay - t.cy))) &&
                    (e2 > 0 || (e2 == 0 && top_left(t.bx - t.ax, t.by - t.ay)));
    if (!in) return false;
    const double num = ((double)e0 * t.wa + (double)e1 * t.wb) + (double)e2 * t.wc;
    const double z = (double)area / num;
    if (!(z > 0.0 && z <= zfar)) return false;
    bits = __float_as_uint((float)z);
    return true;
}

template <bool STATS>
__device__ __forceinline__ void depth_min(uint32_t* __restrict__ p, uint32_t bits, int32_t, u64& n_atomic)
{
    if (bits < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        atomicMin(p, bits);
        if (STATS) n_atomic++;
    }
}
// (g2): the word (bits << 32) | face: the smallest depth, among equal depth bits the smallest face
template <bool STATS>
__device__ __forceinline__ void depth_min(u64* __restrict__ p, uint32_t bits, int32_t face, u64& n_atomic)
{
    const u64 word = ((u64)bits << 32) | (u64)(uint32_t)face;
    if (word < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        atomicMin(p, word);
        if (STATS) n_atomic++;
    }
}
template <int MODE> struct PixelOf { typedef uint32_t type; };
template <> struct PixelOf<M_FACE> { typedef u64 type; };
template <> struct PixelOf<M_FACE | M_STATS> { typedef u64 type; };

// the box of the pixel centres a triangle can cover, cut to the image: false when it is empty
__device__ __forceinline__ bool tri_box(const Tri& t, int W, int H, int& i0, int& i1, int& j0, int& j1)
{
    const int32_t xlo = min(t.ax, min(t.bx, t.cx)), xhi = max(t.ax, max(t.bx, t.cx));
    const int32_t ylo = min(t.ay, min(t.by, t.cy)), yhi = max(t.ay, max(t.by, t.cy));
    i0 = max(0, (xlo + 127) >> 8); i1 = min(W - 1, (xhi - 128) >> 8);       // 256 i + 128 >= xlo, <= xhi (>>: floor for negatives)
    j0 = max(0, (ylo + 127) >> 8); j1 = min(H - 1, (yhi - 128) >> 8);
    return i0 <= i1 && j0 <= j1;
}

struct Counters { u64 tris, listed, refused, atomics, pixels; };

template <int MODE>
__device__ void emit_triangle(const PV& A, const PV& B, const PV& C, int view, int32_t face, int W, int H, double zfar,
                              typename PixelOf<MODE>::type* __restrict__ img, uint32_t* __restrict__ hdr, LargeTri* __restrict__ list, uint32_t cap,
                              Counters& n)
{
    constexpr bool STATS = (MODE & M_STATS) != 0;
    Tri t;
    int64_t area;
    if (!tri_setup(A, B, C, t, area)) return;
    int i0, i1, j0, j1;
    if (!tri_box(t, W, H, i0, i1, j0, j1)) return;
    if (STATS) n.tris++;
    if (i1 - i0 >= INLINE_MAX || j1 - j0 >= INLINE_MAX) {
        const uint32_t pos = atomicAdd(&hdr[1], 1u);
        if (pos < cap) {
            LargeTri r;
            r.t = t; r.view = view; r.pad[0] = (MODE & M_FACE) ? face : 0; r.pad[1] = r.pad[2] = 0;
            list[pos] = r;
            if (STATS) n.listed++;
            return;
        }
        if (STATS) n.refused++;
    }
    for (int j = j0; j <= j1; j++)
        for (int i = i0; i <= i1; i++) {
            uint32_t bits;
            if (!tri_pixel(t, area, i, j, zfar, bits)) continue;
            if (STATS) n.pixels++;
            depth_min<STATS>(&img[(int64_t)j * W + i], bits, face, n.atomics);
        }
}

// Sutherland-Hodgman against one side of the guard rectangle, in the image plane: Y: the coordinate, UPPER: c <= bound (else c >= bound).
// The new vertex is computed from the inside endpoint towards the outside one and its clipped coordinate is the bound itself.
template <bool Y, bool UPPER>
__device__ int clip_side(const PV* in, int n, PV* out, double bound)
{
    int m = 0;
    for (int k = 0; k < n; k++) {
        const PV cur = in[k], nxt = in[k + 1 == n ? 0 : k + 1];
        const double cc = Y ? cur.y : cur.x, nc = Y ? nxt.y : nxt.x;
        const bool ci = UPPER ? cc <= bound : cc >= bound, ni = UPPER ? nc <= bound : nc >= bound;
        if (ci) out[m++] = cur;
        if (ci != ni) {
            const PV a = ci ? cur : nxt, b = ci ? nxt : cur;
            const double ac = ci ? cc : nc, bc = ci ? nc : cc;
            const double tt = (bound - ac) / (bc - ac);
            PV p;
            p.x = Y ? a.x + tt * (b.x - a.x) : bound;
            p.y = Y ? bound : a.y + tt * (b.y - a.y);
            p.w = a.w + tt * (b.w - a.w);
            out[m++] = p;
        }
    }
    return m;
}

__device__ __forceinline__ bool finite1(double x) { return fabs(x) <= DBL_MAX; }

template <int MODE>
__global__ void __launch_bounds__(256)
raster_faces(int64_t NV, const float* __restrict__ vertices, int64_t NF, const int32_t* __restrict__ faces, const GofRasterView* __restrict__ views,
             int64_t view_stride, typename PixelOf<MODE>::type* __restrict__ depth, uint32_t* __restrict__ hdr, LargeTri* __restrict__ list, uint32_t cap,
             u64* __restrict__ stats)
{
    constexpr bool STATS = (MODE & M_STATS) != 0;
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const int view = (int)blockIdx.y;
    const GofRasterView& V = views[view];
    const int W = V.W, H = V.H;
    const double zn = V.znear, zfar = V.zfar;
    typename PixelOf<MODE>::type* img = depth + (int64_t)view * view_stride;
    Counters n = { 0, 0, 0, 0, 0 };
    P3 c[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int64_t v = faces[3 * f + k];                                    // (checked by raster_check before this launch)
        const double vx = (double)vertices[3 * v], vy = (double)vertices[3 * v + 1], vz = (double)vertices[3 * v + 2];
        c[k].x = ((V.w2c[0] * vx + V.w2c[1] * vy) + V.w2c[2] * vz) + V.w2c[3];
        c[k].y = ((V.w2c[4] * vx + V.w2c[5] * vy) + V.w2c[6] * vz) + V.w2c[7];
        c[k].z = ((V.w2c[8] * vx + V.w2c[9] * vy) + V.w2c[10] * vz) + V.w2c[11];
        ok = ok && finite3(vx, vy, vz) && finite3(c[k].x, c[k].y, c[k].z);
    }
    if (ok && (c[0].z >= zn || c[1].z >= zn || c[2].z >= zn)) {
        const double xmin = -(double)GUARD_PX, xmax = (double)(W + GUARD_PX), ymin = -(double)GUARD_PX, ymax = (double)(H + GUARD_PX);
        bool simple = c[0].z >= zn && c[1].z >= zn && c[2].z >= zn;
        PV p[3];
        if (simple) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                p[k].x = V.fx * (c[k].x / c[k].z) + V.cx;
                p[k].y = V.fy * (c[k].y / c[k].z) + V.cy;
                p[k].w = 1.0 / c[k].z;
                simple = simple && p[k].x >= xmin && p[k].x <= xmax && p[k].y >= ymin && p[k].y <= ymax;      // (false for NaN and Inf)
            }
        }
        if (simple) {
            // nothing to clip: the polygon is the triangle (what the general path below gives for it, without its arrays)
            emit_triangle<MODE>(p[0], p[1], p[2], view, (int32_t)f, W, H, zfar, img, hdr, list, cap, n);
        } else {
            P3 q[4];
            int m = 0;
            for (int k = 0; k < 3; k++) {
                const P3 cur = c[k], nxt = c[k == 2 ? 0 : k + 1];
                const bool ci = cur.z >= zn, ni = nxt.z >= zn;
                if (ci) q[m++] = cur;
                if (ci != ni) {
                    const P3 a = ci ? cur : nxt, b = ci ? nxt : cur;
                    const double tt = (zn - a.z) / (b.z - a.z);
                    P3 r;
                    r.x = a.x + tt * (b.x - a.x);
                    r.y = a.y + tt * (b.y - a.y);
                    r.z = zn;
                    q[m++] = r;
                }
            }
            PV s0[9], s1[9];
            bool fin = true;
            for (int k = 0; k < m; k++) {
                s0[k].x = V.fx * (q[k].x / q[k].z) + V.cx;
                s0[k].y = V.fy * (q[k].y / q[k].z) + V.cy;
                s0[k].w = 1.0 / q[k].z;
                fin = fin && finite1(s0[k].x) && finite1(s0[k].y);
            }
            if (fin) {
                m = clip_side<false, false>(s0, m, s1, xmin);
                m = clip_side<false, true>(s1, m, s0, xmax);
                m = clip_side<true, false>(s0, m, s1, ymin);
                m = clip_side<true, true>(s1, m, s0, ymax);
                for (int k = 1; k + 1 < m; k++) emit_triangle<MODE>(s0[0], s0[k], s0[k + 1], view, (int32_t)f, W, H, zfar, img, hdr, list, cap, n);
            }
        }
    }
    if (STATS) {
        if (n.tris) atomicAdd(&stats[0], n.tris);
        if (n.listed) atomicAdd(&stats[1], n.listed);
        if (n.refused) atomicAdd(&stats[2], n.refused);
        if (n.atomics) atomicAdd(&stats[3], n.atomics);
        if (n.pixels) atomicAdd(&stats[4], n.pixels);
    }
}

template <int MODE>
__global__ void __launch_bounds__(256)
raster_large(const GofRasterView* __restrict__ views, int64_t view_stride, typename PixelOf<MODE>::type* __restrict__ depth, const uint32_t* __restrict__ hdr,
             const LargeTri* __restrict__ list, uint32_t cap, u64* __restrict__ stats)
{
    constexpr bool STATS = (MODE & M_STATS) != 0;
    const uint32_t count = min(hdr[1], cap);
    const int stripe = (int)(blockIdx.x % STRIPES), wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int lx = lane % TILE_W, ly = lane / TILE_W;
    u64 n_atomic = 0, n_pixel = 0;
    for (uint32_t e = blockIdx.x / STRIPES; e < count; e += LARGE_GROUPS) {
        const LargeTri r = list[e];
        const GofRasterView& V = views[r.view];
        const int W = V.W, H = V.H;
        const double zfar = V.zfar;
        typename PixelOf<MODE>::type* img = depth + (int64_t)r.view * view_stride;
        const int64_t area = tri_area(r.t);
        int i0, i1, j0, j1;
        if (!tri_box(r.t, W, H, i0, i1, j0, j1)) continue;
        const int tx = (i1 - i0) / TILE_W + 1, ty = (j1 - j0) / TILE_H + 1;
        for (int tile = stripe * 4 + wave; tile < tx * ty; tile += 4 * STRIPES) {
            const int i = i0 + (tile % tx) * TILE_W + lx, j = j0 + (tile / tx) * TILE_H + ly;
            uint32_t bits;
            if (i > i1 || j > j1 || !tri_pixel(r.t, area, i, j, zfar, bits)) continue;
            if (STATS) n_pixel++;
            depth_min<STATS>(&img[(int64_t)j * W + i], bits, r.pad[0], n_atomic);
        }
    }
    if (STATS) {
        if (n_atomic) atomicAdd(&stats[3], n_atomic);
        if (n_pixel) atomicAdd(&stats[4], n_pixel);
    }
}

// before anything is written: the face indices and the view records
static __global__ void __launch_bounds__(256)
raster_check(int64_t NV, int64_t NF, const int32_t* __restrict__ faces, int num_views, const GofRasterView* __restrict__ views, int64_t view_stride,
             uint32_t* __restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NF) {
        const int64_t a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
        if (a < 0 || a >= NV || b < 0 || b >= NV || c < 0 || c >= NV) atomicOr(&hdr[0], F_INDEX);
    }
    if (i < num_views) {
        const GofRasterView& V = views[i];
        const bool ok = V.W >= 1 && V.H >= 1 && V.W <= MAX_SIDE && V.H <= MAX_SIDE && (int64_t)V.W * V.H <= view_stride && V.znear > 0.0 && V.zfar > V.znear;
        if (!ok) atomicOr(&hdr[0], F_VIEW);
    }
}

static __global__ void raster_init_hdr(uint32_t* hdr, u64* stats, int clear_stats)
{
    if (threadIdx.x < HDR_WORDS) hdr[threadIdx.x] = 0u;
    if (clear_stats && threadIdx.x < STAT_WORDS) stats[threadIdx.x] = 0ull;
}

struct RasterWs { uint32_t* hdr; u64* stats; LargeTri* list; uint32_t cap; uint32_t* depth; };
static size_t raster_layout(int64_t NF, int64_t depth_words, void* base, RasterWs* out)
{
    Carver c{ static_cast<char*>(base), 0 };
    RasterWs w;
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    w.stats = c.take<u64>(STAT_WORDS);
    w.cap = (uint32_t)(LIST_MIN + (NF < 0 ? 0 : NF) / 8);
    w.list = c.take<LargeTri>(w.cap);
    w.depth = c.take<uint32_t>((size_t)(depth_words < 0 ? 0 : depth_words));
    if (out) *out = w;
    return c.total();
}

static int image_blocks(int64_t view_stride) { const int64_t b = (view_stride + 255) / 256; return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b)); }

// the shared argument checks and the check launch: 0, or the error with nothing but the workspace's header written
static int raster_validate(const char* who, int64_t NV, int64_t NF, const int32_t* faces, int num_views, const GofRasterView* views, int64_t view_stride,
                           const RasterWs& w, bool clear_stats, hipStream_t stream)
{
    hipLaunchKernelGGL(raster_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr, w.stats, clear_stats ? 1 : 0);
    const int64_t n = NF > num_views ? NF : num_views;
    if (n) hipLaunchKernelGGL(raster_check, grid_of(n), dim3(256), 0, stream, NV, NF, faces, num_views, views, view_stride, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t flags = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (flags & F_INDEX) { set_error("%s: a face index lies outside [0, %lld)", who, (long long)NV); return GOF_E_INVALID; }
    if (flags & F_VIEW) {
        set_error("%s: a view record needs 1 <= W, H <= %d, W * H <= the view stride (%lld), znear > 0 and zfar > znear", who, MAX_SIDE, (long long)view_stride);
        return GOF_E_INVALID;
    }
    return GOF_OK;
}

static int read_stats(const RasterWs& w, int64_t* stats, hipStream_t stream)
{
    u64 h[STAT_WORDS];
    GOF_HIP_CHECK(hipMemcpyAsync(h, w.stats, sizeof(h), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    for (int k = 0; k < STAT_WORDS; k++) stats[k] = (int64_t)h[k];
    return GOF_OK;
}

} // namespace raster
} // namespace gof
