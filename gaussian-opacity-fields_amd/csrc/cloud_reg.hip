// cloud_reg.hip -- registration primitives of the Tanks-and-Temples F-score evaluation (replaces what the reference's
// eval_tnt/registration.py and evaluation.py ask of Open3D besides the nearest-neighbour search, which is cloud.hip's):
// (a) transformation + polygon-volume crop, (b) voxel down-sampling, (c) the correspondence sums of one ICP iteration.
// Contract: DESIGN.md 3.9, include/gof_cloud_reg_hip.h.
//
// Arithmetic: fp64, compiled with -ffp-contract=off like the whole library and no fma() is written here, so every operation below
// is the IEEE operation numpy performs on the host, in the order written.  No floating-point atomics: counts and flags only.
//
// (a) one lane per point, the polygon's (u, v) pairs in LDS (16 B per vertex, dynamic: K <= 4096 = 64 KB); pass 1 writes a keep flag,
//     the library's scan turns the flags into output rows, pass 2 evaluates the transformation again (12 multiplications: cheaper
//     than keeping 24 B per point) and writes the kept points in input order.
// (b) 3 x 21-bit cell key, radix.h's sort_keys63, so that a voxel's points are consecutive and
//     in input order; the first point of every voxel is flagged, the scan numbers the voxels in ascending key order, and the lane
//     of a first point adds its voxel's points one after the other (serial by contract: the sum has ONE order).
// (c) a sum = the balanced binary tree over the source points in index order: xor butterfly inside a wave (both lanes of a pair
//     compute a + b = b + a: the same bits), four wave results in LDS, one partial per workgroup of 256, and further launches over
//     the partials.  Levels above the next power of two of N would add padding to the root: they are skipped (x + 0.0 is x except
//     for x = -0.0, so the contract's tree ends at the root).
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_cloud_reg_hip.h"
#include "radix.h"
#include "gof_geom.h"

namespace gof {

namespace reg {

constexpr uint32_t F_NONFINITE = 1u, F_INDEX = 2u, F_CELLS = 4u;
// header words of every workspace: u64 [0..2] per-axis minimum (ordered encoding), [3] flags, [4] a count
constexpr int H_FLAGS = 3, H_COUNT = 4, HDR_WORDS = 8;
constexpr int MAX_POLYGON = 4096;
constexpr int64_t VOX_MAXC = (1 << 21) - 1;

__global__ void reg_init_hdr(u64* hdr)
{
    const int t = threadIdx.x;
    if (t < HDR_WORDS) hdr[t] = t < 3 ? ~0ull : 0ull;
}

// the first three rows of the matrix, by value (has = 0: no transformation)
struct Mat34 { double m[12]; int has; };
__device__ __forceinline__ void reg_apply(const Mat34& M, double x, double y, double z, double (&o)[3])
{
    if (!M.has) { o[0] = x; o[1] = y; o[2] = z; return; }
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = ((M.m[4 * r] * x + M.m[4 * r + 1] * y) + M.m[4 * r + 2] * z) + M.m[4 * r + 3];
}

// =====================================================================================================================================
// transformation, (a) crop
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
reg_transform(int64_t N, const double* __restrict__ pts, Mat34 M, double* __restrict__ out, u64* __restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    double o[3];
    reg_apply(M, x, y, z, o);
    if (!finite3(x, y, z) || !finite3(o[0], o[1], o[2])) atomicOr(&hdr[H_FLAGS], (u64)F_NONFINITE);
    out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

// flags[i] = 1 iff the transformed point i lies inside the volume; flags[N] = 0 (the scan's last word = the total)
__global__ void __launch_bounds__(256)
reg_crop_flags(int64_t N, const double* __restrict__ pts, Mat34 M, int axis, double axis_min, double axis_max, int K,
               const double* __restrict__ polygon, uint32_t* __restrict__ flags, u64* __restrict__ hdr)
{
    extern __shared__ double s_poly[];
    const int ua = (axis + 1) % 3, va = (axis + 2) % 3;
    for (int k = threadIdx.x; k < K; k += 256) { s_poly[2 * k] = polygon[3 * k + ua]; s_poly[2 * k + 1] = polygon[3 * k + va]; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == N) flags[i] = 0;
    if (i >= N) return;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    double o[3];
    reg_apply(M, x, y, z, o);
    if (!finite3(x, y, z) || !finite3(o[0], o[1], o[2])) { atomicOr(&hdr[H_FLAGS], (u64)F_NONFINITE); flags[i] = 0; return; }
    const double pw = o[axis], pu = o[ua], pv = o[va];
    uint32_t keep = 0;
    if (axis_min <= pw && pw <= axis_max) {
        uint32_t crossings = 0;
        for (int k = 0; k < K; k++) {
            const int j = k == 0 ? K - 1 : k - 1;
            const double iu = s_poly[2 * k], iv = s_poly[2 * k + 1], ju = s_poly[2 * j], jv = s_poly[2 * j + 1];
            if ((iv < pv && jv >= pv) || (jv < pv && iv >= pv)) {
                if (iu + (pv - iv) / (jv - iv) * (ju - iu) < pu) crossings++;
            }
        }
        keep = crossings & 1u;
    }
    flags[i] = keep;
}

// off = exclusive scan of the flags over N + 1 words: point i is kept iff off[i + 1] > off[i], and lands in row off[i]
__global__ void __launch_bounds__(256)
reg_crop_emit(int64_t N, const double* __restrict__ pts, Mat34 M, const uint32_t* __restrict__ off, double* __restrict__ out, int32_t* __restrict__ out_index)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t r = off[i];
    if (off[i + 1] == r) return;
    double o[3];
    reg_apply(M, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], o);
    out[3 * (int64_t)r] = o[0]; out[3 * (int64_t)r + 1] = o[1]; out[3 * (int64_t)r + 2] = o[2];
    out_index[r] = (int32_t)i;
}

struct CropWs { u64* hdr; uint32_t* flags; uint32_t* tmp; };
static size_t crop_layout(int64_t N, void* base, CropWs* out)
{
    const size_t n = (size_t)(N < 0 ? 0 : N) + 1;
    Carver c{ static_cast<char*>(base), 0 };
    CropWs w;
    w.hdr = c.take<u64>(HDR_WORDS);
    w.flags = c.take<uint32_t>(n);
    w.tmp = c.take<uint32_t>(scan_tmp_words(n));
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// (b) voxel down-sampling
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
reg_min(int64_t N, const double* __restrict__ pts, u64* __restrict__ hdr)
{
    double lo[3] = { DBL_MAX, DBL_MAX, DBL_MAX };
    bool bad = false, any = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (!finite3(x, y, z)) { bad = true; continue; }
        lo[0] = fmin(lo[0], x); lo[1] = fmin(lo[1], y); lo[2] = fmin(lo[2], z);
        any = true;
    }
    // the wave's minimum first (every lane gets here): three atomics per wave, not per lane
#pragma unroll
    for (int c = 0; c < 3; c++)
        for (int o = 32; o > 0; o >>= 1) lo[c] = fmin(lo[c], __shfl_xor(lo[c], o));
    const bool wave_any = wave_sum(any ? 1ull : 0ull) != 0;
    if ((threadIdx.x & 63) == 0 && wave_any) {
#pragma unroll
        for (int c = 0; c < 3; c++) atomicMin(&hdr[c], ordered64(lo[c]));
    }
    if (bad) atomicOr(&hdr[H_FLAGS], (u64)F_NONFINITE);
}

__global__ void __launch_bounds__(256)
reg_vox_keys(int64_t N, const double* __restrict__ pts, double v, u64* __restrict__ hdr, u64* __restrict__ keys, uint32_t* __restrict__ lo32, uint32_t* __restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    u64 c[3];
    bool big = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double o = unordered64(hdr[a]) - 0.5 * v;
        const double f = floor((pts[3 * i + a] - o) / v);
        if (!(f >= 0.0 && f <= (double)VOX_MAXC)) { big = true; c[a] = 0; }       // (NaN too: a non-finite point, flagged by reg_min)
        else c[a] = (u64)f;
    }
    if (big) atomicOr(&hdr[H_FLAGS], (u64)F_CELLS);
    const u64 key = (c[0] << 42) | (c[1] << 21) | c[2];
    keys[i] = key;
    lo32[i] = (uint32_t)key;
    idx[i] = (uint32_t)i;
}
// heads[s] = 1 iff the s-th point in key order is the first of its voxel; heads[N] = 0
__global__ void __launch_bounds__(256)
reg_vox_heads(int64_t N, const u64* __restrict__ keys, const uint32_t* __restrict__ order, uint32_t* __restrict__ heads)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s == N) heads[s] = 0;
    if (s >= N) return;
    heads[s] = (s == 0 || keys[order[s]] != keys[order[s - 1]]) ? 1u : 0u;
}
// vid = exclusive scan of the heads over N + 1 words: s is a first point iff vid[s + 1] > vid[s]; its lane adds the voxel's points
// in key order = input order (the sorts are stable), one after the other, and divides by their number
__global__ void __launch_bounds__(256)
reg_vox_reduce(int64_t N, const double* __restrict__ pts, const uint32_t* __restrict__ order, const uint32_t* __restrict__ vid,
               double* __restrict__ out, int32_t* __restrict__ out_counts)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const uint32_t me = vid[s];
    if (vid[s + 1] == me) return;
    const int64_t p0 = order[s];
    double ax = pts[3 * p0], ay = pts[3 * p0 + 1], az = pts[3 * p0 + 2];
    int64_t q = s + 1;
    for (; q < N && vid[q + 1] == vid[q]; q++) {
        const int64_t p = order[q];
        ax = ax + pts[3 * p]; ay = ay + pts[3 * p + 1]; az = az + pts[3 * p + 2];
    }
    const double cnt = (double)(q - s);
    out[3 * (int64_t)me] = ax / cnt; out[3 * (int64_t)me + 1] = ay / cnt; out[3 * (int64_t)me + 2] = az / cnt;
    out_counts[me] = (int32_t)(q - s);
}

struct VoxWs { u64* hdr; u64* keys; uint32_t* heads; Sort63Ws s; };      // (s.tmp serves the scan of the heads as well)
static size_t vox_layout(int64_t N, void* base, VoxWs* out)
{
    const size_t n = (size_t)(N < 1 ? 1 : N);
    Carver c{ static_cast<char*>(base), 0 };
    VoxWs w;
    w.hdr = c.take<u64>(HDR_WORDS);
    w.keys = c.take<u64>(n);
    w.heads = c.take<uint32_t>(n + 1);
    const size_t t1 = rs_tmp_words(n), t2 = scan_tmp_words(n + 1);
    sort63_carve(c, n, w.s);
    w.s.tmp = c.take<uint32_t>(t1 > t2 ? t1 : t2);
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// (c) correspondence sums
// =====================================================================================================================================
// The workgroup's 256 values (one per thread, in thread order) -> the root of their balanced tree, written by thread 0 to
// out[c * out_stride + blockIdx.x].  span = leaves of the whole tree under one value, P2 = leaves of the whole tree: the step that
// joins nodes of span * o leaves is a level of the tree iff span * o < P2 (uniform over the launch).
template <int C>
__device__ __forceinline__ void tree_block(double (&v)[C], double (&s_w)[C][4], int64_t span, int64_t P2, double* __restrict__ out, int64_t out_stride)
{
    for (int o = 1; o < 64; o <<= 1) {
        if (span * o < P2) {
#pragma unroll
            for (int c = 0; c < C; c++) v[c] = v[c] + __shfl_xor(v[c], o);
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < C; c++) s_w[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool l6 = span * 64 < P2, l7 = span * 128 < P2;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double a = l6 ? s_w[c][0] + s_w[c][1] : s_w[c][0];
            const double b = s_w[c][2] + s_w[c][3];
            out[c * out_stride + blockIdx.x] = l7 ? a + b : a;
        }
    }
}

template <int C>
__global__ void __launch_bounds__(256)
reg_tree_reduce(int64_t M, const double* __restrict__ in, int64_t in_stride, int64_t span, int64_t P2, double* __restrict__ out, int64_t out_stride)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[C];
#pragma unroll
    for (int c = 0; c < C; c++) v[c] = i < M ? in[c * in_stride + i] : 0.0;
    __shared__ double s_w[C][4];
    tree_block<C>(v, s_w, span, P2, out, out_stride);
}

__device__ __forceinline__ bool is_pair(int64_t i, int64_t N, int64_t NT, const double* __restrict__ dist, const int32_t* __restrict__ nearest,
                                        double threshold, int64_t& j, u64* __restrict__ hdr)
{
    if (i >= N) return false;
    j = nearest[i];
    if (!(dist[i] < threshold) || j < 0) return false;
    if (j >= NT) { atomicOr(&hdr[H_FLAGS], (u64)F_INDEX); return false; }
    return true;
}

__global__ void __launch_bounds__(256)
reg_sums1(int64_t N, const double* __restrict__ src, int64_t NT, const double* __restrict__ tgt, const double* __restrict__ dist,
          const int32_t* __restrict__ nearest, double threshold, int64_t P2, double* __restrict__ out, int64_t out_stride, u64* __restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    int64_t j = 0;
    u64 cnt = 0;
    if (is_pair(i, N, NT, dist, nearest, threshold, j, hdr)) {
        const double d = dist[i];
        v[0] = src[3 * i]; v[1] = src[3 * i + 1]; v[2] = src[3 * i + 2];
        v[3] = tgt[3 * j]; v[4] = tgt[3 * j + 1]; v[5] = tgt[3 * j + 2];
        v[6] = d * d;
        cnt = 1;
        if (!finite3(v[0], v[1], v[2]) || !finite3(v[3], v[4], v[5]) || !(v[6] <= DBL_MAX)) atomicOr(&hdr[H_FLAGS], (u64)F_NONFINITE);
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&hdr[H_COUNT], cnt);
    __shared__ double s_w[7][4];
    tree_block<7>(v, s_w, 1, P2, out, out_stride);
}

struct Means { double s[3], t[3]; };
__global__ void __launch_bounds__(256)
reg_sums2(int64_t N, const double* __restrict__ src, int64_t NT, const double* __restrict__ tgt, const double* __restrict__ dist,
          const int32_t* __restrict__ nearest, double threshold, Means mu, int64_t P2, double* __restrict__ out, int64_t out_stride, u64* __restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[10] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    int64_t j = 0;
    if (is_pair(i, N, NT, dist, nearest, threshold, j, hdr)) {
        const double dx = src[3 * i] - mu.s[0], dy = src[3 * i + 1] - mu.s[1], dz = src[3 * i + 2] - mu.s[2];
        const double e[3] = { tgt[3 * j] - mu.t[0], tgt[3 * j + 1] - mu.t[1], tgt[3 * j + 2] - mu.t[2] };
#pragma unroll
        for (int r = 0; r < 3; r++) { v[3 * r] = e[r] * dx; v[3 * r + 1] = e[r] * dy; v[3 * r + 2] = e[r] * dz; }
        v[9] = (dx * dx + dy * dy) + dz * dz;
        bool ok = v[9] <= DBL_MAX;
#pragma unroll
        for (int k = 0; k < 9; k++) ok = ok && fabs(v[k]) <= DBL_MAX;
        if (!ok) atomicOr(&hdr[H_FLAGS], (u64)F_NONFINITE);
    }
    __shared__ double s_w[10][4];
    tree_block<10>(v, s_w, 1, P2, out, out_stride);
}

constexpr int SUMS_MAX_C = 10;
struct SumsWs { u64* hdr; double* a; double* b; };
static size_t sums_layout(int64_t N, void* base, SumsWs* out)
{
    const size_t n = (size_t)(N < 1 ? 1 : N);
    const size_t m1 = (n + 255) / 256, m2 = (m1 + 255) / 256;
    Carver c{ static_cast<char*>(base), 0 };
    SumsWs w;
    w.hdr = c.take<u64>(HDR_WORDS);
    w.a = c.take<double>(SUMS_MAX_C * m1);
    w.b = c.take<double>(SUMS_MAX_C * m2);
    if (out) *out = w;
    return c.total();
}

static int flags_error(u64 flags, const char* who)
{
    if (flags & F_NONFINITE) { set_error("%s: a coordinate is not finite", who); return GOF_E_INVALID; }
    if (flags & F_INDEX) { set_error("%s: a nearest index lies outside [0, num_target)", who); return GOF_E_INVALID; }
    if (flags & F_CELLS) { set_error("%s: the cloud spans more than 2^21 - 1 voxels per axis", who); return GOF_E_INVALID; }
    return GOF_OK;
}

// false: a value of the matrix is not finite
static bool load_matrix(const double* matrix, Mat34& M)
{
    M.has = matrix ? 1 : 0;
    for (int k = 0; k < 12; k++) {
        M.m[k] = matrix ? matrix[k] : 0.0;
        if (!(std::fabs(M.m[k]) <= DBL_MAX)) return false;
    }
    return true;
}

// the rest of a tree whose first level left `M` partials of C values in w.a (stride M): launches over the partials until one is left,
// then the C values to the host (waits for the stream)
template <int C>
static int finish_tree(const SumsWs& w, int64_t M, int64_t P2, double* sums, hipStream_t stream)
{
    double *in = w.a, *out = w.b;
    int64_t span = 256;
    while (M > 1) {
        const int64_t M2 = (M + 255) / 256;
        hipLaunchKernelGGL(reg_tree_reduce<C>, dim3((unsigned)M2), dim3(256), 0, stream, M, in, M, span, P2, out, M2);
        GOF_LAUNCH_CHECK(stream, 0);
        double* t = in; in = out; out = t;
        M = M2;
        span *= 256;
    }
    GOF_HIP_CHECK(hipMemcpyAsync(sums, in, C * sizeof(double), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    return GOF_OK;
}

static int64_t next_pow2(int64_t n) { int64_t p = 1; while (p < n) p <<= 1; return p; }

static int sums_check(const char* who, int64_t N, const double* src, int64_t NT, const double* tgt, const double* dist, const int32_t* nearest,
                      double threshold, void* ws, size_t ws_bytes, const void* sums)
{
    if (bad_count(N) || bad_count(NT)) { set_error("%s: bad counts (%lld source, %lld target points)", who, (long long)N, (long long)NT); return GOF_E_INVALID; }
    if (threshold != threshold) { set_error("%s: threshold is NaN", who); return GOF_E_INVALID; }
    if (!ws || !sums) { set_error("%s: workspace / sums is NULL", who); return GOF_E_INVALID; }
    if (N && (!src || !dist || !nearest || (NT && !tgt))) { set_error("%s: source / target / dist / nearest is NULL", who); return GOF_E_INVALID; }
    if (ws_bytes < sums_layout(N, nullptr, nullptr)) { set_error("%s: workspace too small", who); return GOF_E_WORKSPACE; }
    return GOF_OK;
}

} // namespace reg
} // namespace gof

using namespace gof;
using namespace gof::reg;

extern "C" {

size_t gof_cloud_transform_ws_bytes(int64_t) { return align_up(HDR_WORDS * 8) + ALIGN; }

int gof_cloud_transform(int64_t N, const double* points, const double* matrix, double* out, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(N)) { set_error("cloud_transform: bad number of points (%lld)", (long long)N); return GOF_E_INVALID; }
    Mat34 M;
    if (!load_matrix(matrix, M)) { set_error("cloud_transform: the matrix is not finite"); return GOF_E_INVALID; }
    if (!ws) { set_error("cloud_transform: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_cloud_transform_ws_bytes(N)) { set_error("cloud_transform: workspace too small"); return GOF_E_WORKSPACE; }
    if (N == 0) return GOF_OK;
    if (!points || !out || points == out) { set_error("cloud_transform: points / out is NULL or the same buffer"); return GOF_E_INVALID; }
    GOF_PROFILE("cloud_transform", stream);
    u64* hdr = static_cast<u64*>(ws_aligned(ws));
    hipLaunchKernelGGL(reg_init_hdr, dim3(1), dim3(64), 0, stream, hdr);
    hipLaunchKernelGGL(reg_transform, grid_of(N), dim3(256), 0, stream, N, points, M, out, hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    u64 flags = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, hdr + H_FLAGS, 8, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    return flags_error(flags, "cloud_transform");
}

size_t gof_cloud_crop_ws_bytes(int64_t N) { return crop_layout(N, nullptr, nullptr); }

int gof_cloud_crop(int64_t N, const double* points, const double* matrix, int axis, double axis_min, double axis_max, int64_t K,
                   const double* polygon, double* out_points, int32_t* out_index, void* ws, size_t ws_bytes, int64_t* num_kept, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_kept) { set_error("cloud_crop: num_kept is NULL"); return GOF_E_INVALID; }
    *num_kept = 0;
    if (bad_count(N)) { set_error("cloud_crop: bad number of points (%lld)", (long long)N); return GOF_E_INVALID; }
    if (axis < 0 || axis > 2) { set_error("cloud_crop: the orthogonal axis must be 0 (X), 1 (Y) or 2 (Z)"); return GOF_E_INVALID; }
    if (K < 0) { set_error("cloud_crop: bad number of polygon vertices (%lld)", (long long)K); return GOF_E_INVALID; }
    if (K > MAX_POLYGON) { set_error("cloud_crop: a polygon of %lld vertices (at most %d)", (long long)K, MAX_POLYGON); return GOF_E_CAPACITY; }
    if (axis_min != axis_min || axis_max != axis_max) { set_error("cloud_crop: axis_min / axis_max is NaN"); return GOF_E_INVALID; }
    Mat34 M;
    if (!load_matrix(matrix, M)) { set_error("cloud_crop: the matrix is not finite"); return GOF_E_INVALID; }
    if (!ws || (K && !polygon)) { set_error("cloud_crop: workspace / polygon is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_cloud_crop_ws_bytes(N)) { set_error("cloud_crop: workspace too small"); return GOF_E_WORKSPACE; }
    if (N == 0) return GOF_OK;
    if (!points || !out_points || !out_index) { set_error("cloud_crop: points / out_points / out_index is NULL"); return GOF_E_INVALID; }
    CropWs w;
    crop_layout(N, ws_aligned(ws), &w);
    GOF_PROFILE("cloud_crop", stream);
    hipLaunchKernelGGL(reg_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(reg_crop_flags, grid_of(N + 1), dim3(256), (size_t)(K > 0 ? K : 1) * 16, stream, N, points, M, axis, axis_min, axis_max, (int)K,
                       polygon, w.flags, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.flags, nullptr, w.flags, (size_t)N + 1, false, w.tmp, nullptr, stream));
    hipLaunchKernelGGL(reg_crop_emit, grid_of(N), dim3(256), 0, stream, N, points, M, w.flags, out_points, out_index);
    GOF_LAUNCH_CHECK(stream, 0);
    u64 flags = 0;
    uint32_t kept = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr + H_FLAGS, 8, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipMemcpyAsync(&kept, w.flags + N, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (int e = flags_error(flags, "cloud_crop")) return e;
    *num_kept = (int64_t)kept;
    return GOF_OK;
}

size_t gof_cloud_voxel_ws_bytes(int64_t N) { return vox_layout(N, nullptr, nullptr); }

int gof_cloud_voxel(int64_t N, const double* points, double voxel, double* out_points, int32_t* out_counts, void* ws, size_t ws_bytes,
                    int64_t* num_voxels, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_voxels) { set_error("cloud_voxel: num_voxels is NULL"); return GOF_E_INVALID; }
    *num_voxels = 0;
    if (bad_count(N)) { set_error("cloud_voxel: bad number of points (%lld)", (long long)N); return GOF_E_INVALID; }
    if (!(voxel > 0.0) || !(voxel <= DBL_MAX)) { set_error("cloud_voxel: the voxel size must be positive and finite"); return GOF_E_INVALID; }
    if (!ws) { set_error("cloud_voxel: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_cloud_voxel_ws_bytes(N)) { set_error("cloud_voxel: workspace too small"); return GOF_E_WORKSPACE; }
    if (N == 0) return GOF_OK;
    if (!points || !out_points || !out_counts) { set_error("cloud_voxel: points / out_points / out_counts is NULL"); return GOF_E_INVALID; }
    VoxWs w;
    vox_layout(N, ws_aligned(ws), &w);
    GOF_PROFILE("cloud_voxel", stream);
    hipLaunchKernelGGL(reg_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(reg_min, dim3((unsigned)min((int64_t)2048, (N + 255) / 256)), dim3(256), 0, stream, N, points, w.hdr);
    hipLaunchKernelGGL(reg_vox_keys, grid_of(N), dim3(256), 0, stream, N, points, voxel, w.hdr, w.keys, w.s.lo[0], w.s.idx[0]);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t* order = nullptr;
    GOF_HIP_CHECK(sort_keys63(w.keys, (size_t)N, w.s, &order, stream));
    hipLaunchKernelGGL(reg_vox_heads, grid_of(N + 1), dim3(256), 0, stream, N, w.keys, order, w.heads);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.heads, nullptr, w.heads, (size_t)N + 1, false, w.s.tmp, nullptr, stream));
    // the flags first: a non-finite point has no cell, and nothing is written for a cloud that is refused
    u64 flags = 0;
    uint32_t nv = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr + H_FLAGS, 8, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipMemcpyAsync(&nv, w.heads + N, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (int e = flags_error(flags, "cloud_voxel")) return e;
    hipLaunchKernelGGL(reg_vox_reduce, grid_of(N), dim3(256), 0, stream, N, points, order, w.heads, out_points, out_counts);
    GOF_LAUNCH_CHECK(stream, 0);
    *num_voxels = (int64_t)nv;
    return GOF_OK;
}

size_t gof_cloud_icp_sums_ws_bytes(int64_t N) { return sums_layout(N, nullptr, nullptr); }

int gof_cloud_icp_sums1(int64_t N, const double* src, int64_t NT, const double* tgt, const double* dist, const int32_t* nearest,
                        double threshold, void* ws, size_t ws_bytes, int64_t* n, double* sums, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!n) { set_error("cloud_icp_sums1: n is NULL"); return GOF_E_INVALID; }
    *n = 0;
    if (int e = sums_check("cloud_icp_sums1", N, src, NT, tgt, dist, nearest, threshold, ws, ws_bytes, sums)) return e;
    for (int c = 0; c < 7; c++) sums[c] = 0.0;
    if (N == 0) return GOF_OK;
    SumsWs w;
    sums_layout(N, ws_aligned(ws), &w);
    GOF_PROFILE("cloud_icp_sums1", stream);
    const int64_t M = (N + 255) / 256, P2 = next_pow2(N);
    hipLaunchKernelGGL(reg_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(reg_sums1, dim3((unsigned)M), dim3(256), 0, stream, N, src, NT, tgt, dist, nearest, threshold, P2, w.a, M, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    u64 h[2] = { 0, 0 };
    GOF_HIP_CHECK(hipMemcpyAsync(h, w.hdr + H_FLAGS, sizeof(h), hipMemcpyDeviceToHost, stream));
    if (int e = finish_tree<7>(w, M, P2, sums, stream)) return e;
    if (int e = flags_error(h[0], "cloud_icp_sums1")) return e;
    *n = (int64_t)h[1];
    return GOF_OK;
}

int gof_cloud_icp_sums2(int64_t N, const double* src, int64_t NT, const double* tgt, const double* dist, const int32_t* nearest,
                        double threshold, const double* means, void* ws, size_t ws_bytes, double* sums, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = sums_check("cloud_icp_sums2", N, src, NT, tgt, dist, nearest, threshold, ws, ws_bytes, sums)) return e;
    if (!means) { set_error("cloud_icp_sums2: means is NULL"); return GOF_E_INVALID; }
    Means mu;
    for (int c = 0; c < 3; c++) { mu.s[c] = means[c]; mu.t[c] = means[3 + c]; }
    for (int c = 0; c < 6; c++) if (!(std::fabs(means[c]) <= DBL_MAX)) { set_error("cloud_icp_sums2: a mean is not finite"); return GOF_E_INVALID; }
    for (int c = 0; c < 10; c++) sums[c] = 0.0;
    if (N == 0) return GOF_OK;
    SumsWs w;
    sums_layout(N, ws_aligned(ws), &w);
    GOF_PROFILE("cloud_icp_sums2", stream);
    const int64_t M = (N + 255) / 256, P2 = next_pow2(N);
    hipLaunchKernelGGL(reg_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(reg_sums2, dim3((unsigned)M), dim3(256), 0, stream, N, src, NT, tgt, dist, nearest, threshold, mu, P2, w.a, M, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    u64 flags = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr + H_FLAGS, 8, hipMemcpyDeviceToHost, stream));
    if (int e = finish_tree<10>(w, M, P2, sums, stream)) return e;
    return flags_error(flags, "cloud_icp_sums2");
}

} // extern "C"
