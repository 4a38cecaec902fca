// cloud.hip -- point-cloud primitives of the DTU Chamfer evaluation (replaces the work of the reference's dtu_eval/eval.py, which
// needs Open3D and scikit-learn): (a) lattice sampling of triangles, (b) greedy radius thinning, (c) exact nearest neighbour between
// two clouds.  Contract: DESIGN.md 3.8, include/gof_cloud_hip.h.
//
// Arithmetic: fp64, the unit is compiled with -ffp-contract=off like the whole library and no fma() is written here, so every
// operation below is the IEEE operation numpy performs on the host, in the order written.
//
// (a) count pass: one thread per triangle evaluates the lattice (n1, n2) and counts its samples row by row (a row's count is a
//     monotone predicate in j: a closed-form guess, then corrected by evaluating the predicate itself); the library's scan.  emit
//     pass: one wave per slice of CLOUD_SLICE consecutive OUTPUT slots; a lane finds its triangle with a search into the scanned
//     counts and its row by walking the rows -- in a wave whose lanes share one triangle (every wave inside a large triangle) the
//     rows in front of the slice are skipped 64 at a time by the whole wave first.
// (b) grid of cells (edge r (1 + 2^-20): see thin_cell), 3 x 21-bit key, radix.h's sort_keys63, points
//     gathered into key order; rounds over the undecided: a point looks at the lower-index points within r in its 27 cells (9 key
//     ranges of 3 cells, one binary search each): a kept one removes it, none undecided keeps it.  States move undecided -> decided
//     only, so a stale read is conservative and the result does not depend on the schedule.
// (c) knn.hip's structure in fp64 with two clouds: the reference cloud in Morton order, boxes of 256 / groups of 32 boxes with fp64
//     bounds (box_index.h, the one definition both units use); the queries are sorted by Morton code of the SAME bounding box
//     (clamped), so a workgroup's 256 queries are neighbours; a first bound from the query's Morton neighbours in the sorted
//     reference; then groups / boxes whose conservative distance does not exceed the bound are staged in LDS (256 x (24 + 4) B =
//     7 KB) and scanned.  Pruning is exact (box_dist, box_index.h): a box is skipped only if its distance exceeds the best so far,
//     ties are visited and resolved to the smallest index.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_cloud_hip.h"
#include "radix.h"
#include "box_index.h"

namespace gof {

constexpr uint32_t CLOUD_F_NONFINITE = 1u, CLOUD_F_INDEX = 2u, CLOUD_F_CELLS = 4u;

// header words shared by the three workspaces: u64 [0..2] min, [3..5] max (ordered encoding), [6] flags, [7..] counters
constexpr int H_FLAGS = 6, H_CNT0 = 7, H_CNT1 = 8, H_CNT2 = 9, H_CNT3 = 10, HDR_WORDS = 16;

__global__ void cloud_init_hdr(u64* hdr)
{
    const int t = threadIdx.x;
    if (t < HDR_WORDS) hdr[t] = t < 3 ? ~0ull : 0ull;
}
__global__ void cloud_set_words(u64* p, u64 a, u64 b) { if (threadIdx.x == 0) { p[0] = a; p[1] = b; } }
__global__ void cloud_set_u32(uint32_t* p, uint32_t v) { if (threadIdx.x == 0) *p = v; }

// bounding box of a cloud + the finiteness flag
__global__ void __launch_bounds__(256)
cloud_bbox(int64_t N, const double* __restrict__ pts, u64* __restrict__ hdr)
{
    double lo[3] = { DBL_MAX, DBL_MAX, DBL_MAX }, hi[3] = { -DBL_MAX, -DBL_MAX, -DBL_MAX };
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (!finite3(x, y, z)) { bad = true; continue; }
        lo[0] = fmin(lo[0], x); hi[0] = fmax(hi[0], x);
        lo[1] = fmin(lo[1], y); hi[1] = fmax(hi[1], y);
        lo[2] = fmin(lo[2], z); hi[2] = fmax(hi[2], z);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (lo[c] <= hi[c]) { atomicMin(&hdr[c], ordered64(lo[c])); atomicMax(&hdr[3 + c], ordered64(hi[c])); }
    }
    if (bad) atomicOr(&hdr[H_FLAGS], (u64)CLOUD_F_NONFINITE);
}

// =====================================================================================================================================
// (a) triangle sampling
// =====================================================================================================================================
constexpr int CLOUD_SLICE = 512;                  // output slots per wave
constexpr int64_t CLOUD_MAX_N = (int64_t)1 << 30; // lattice steps per edge

struct Tri { double p0[3], v1[3], v2[3], d1, d2; int64_t n1, n2; };

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// 0 = no samples, 1 = ok, 2 = bad index / vertex, 3 = lattice too fine
__device__ __forceinline__ int tri_setup(int64_t NV, const double* __restrict__ V, const int32_t* __restrict__ T, int64_t t, double thresh, Tri& tr)
{
    const int32_t i0 = T[3 * t], i1 = T[3 * t + 1], i2 = T[3 * t + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= NV || i1 >= NV || i2 >= NV) return 2;
    double p1[3], p2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { tr.p0[c] = V[3 * (int64_t)i0 + c]; p1[c] = V[3 * (int64_t)i1 + c]; p2[c] = V[3 * (int64_t)i2 + c]; }
    if (!finite3(tr.p0[0], tr.p0[1], tr.p0[2]) || !finite3(p1[0], p1[1], p1[2]) || !finite3(p2[0], p2[1], p2[2])) return 2;
#pragma unroll
    for (int c = 0; c < 3; c++) { tr.v1[c] = p1[c] - tr.p0[c]; tr.v2[c] = p2[c] - tr.p0[c]; }
    const double l1 = norm3(tr.v1[0], tr.v1[1], tr.v1[2]), l2 = norm3(tr.v2[0], tr.v2[1], tr.v2[2]);
    const double cx = tr.v1[1] * tr.v2[2] - tr.v1[2] * tr.v2[1];
    const double cy = tr.v1[2] * tr.v2[0] - tr.v1[0] * tr.v2[2];
    const double cz = tr.v1[0] * tr.v2[1] - tr.v1[1] * tr.v2[0];
    const double area2 = norm3(cx, cy, cz);
    if (!(area2 > 0.0)) return 0;
    const double thr = thresh * sqrt(l1 * l2 / area2);
    const double n1 = floor(l1 / thr), n2 = floor(l2 / thr);
    if (!(n1 >= 1.0) || !(n2 >= 1.0)) return 0;          // n = 0: a = 0.5 / 1e-7 >= 1, no sample passes a + b < 1 (NaN: none either)
    if (n1 > (double)CLOUD_MAX_N || n2 > (double)CLOUD_MAX_N) return 3;
    tr.n1 = (int64_t)n1; tr.n2 = (int64_t)n2; tr.d1 = n1; tr.d2 = n2;    // max(n, 1e-7) = n
    return 1;
}

// samples of row i: #{ j in [0, n2] : (i + 0.5) / d1 + (j + 0.5) / d2 < 1 } -- the predicate is monotone in j (IEEE division and
// addition are monotone), so the count is the first j that fails: guessed in closed form, settled by the predicate itself
__device__ __forceinline__ bool tri_pred(double a, int64_t j, double d2) { return a + ((double)j + 0.5) / d2 < 1.0; }
__device__ __forceinline__ int64_t tri_row_count(const Tri& tr, int64_t i)
{
    const double a = ((double)i + 0.5) / tr.d1;
    const double jf = (1.0 - a) * tr.d2 - 0.5;
    int64_t c = !(jf >= 0.0) ? 0 : (jf >= (double)tr.n2 ? tr.n2 + 1 : (int64_t)jf + 1);
    while (c > 0 && !tri_pred(a, c - 1, tr.d2)) c--;
    while (c <= tr.n2 && tri_pred(a, c, tr.d2)) c++;
    return c;
}

__global__ void __launch_bounds__(256)
cloud_sample_count(int64_t NV, const double* __restrict__ V, int64_t NT, const int32_t* __restrict__ T, double thresh,
                   uint32_t* __restrict__ counts, u64* __restrict__ hdr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    u64 total = 0;
    uint32_t flags = 0;
    if (t < NV && !finite3(V[3 * t], V[3 * t + 1], V[3 * t + 2])) flags |= CLOUD_F_NONFINITE;
    if (t < NT) {
        Tri tr;
        const int s = tri_setup(NV, V, T, t, thresh, tr);
        if (s == 2) flags |= CLOUD_F_INDEX;
        if (s == 3) total = 1ull << 40;
        if (s == 1) {
            for (int64_t i = 0; i <= tr.n1; i++) {
                const int64_t c = tri_row_count(tr, i);
                if (c == 0) break;                          // rows only get shorter
                total += (u64)c;
            }
        }
        counts[t] = total < (1ull << 31) ? (uint32_t)total : 0u;
    }
    if (t == NT) counts[t] = 0;
    total = wave_sum(total);
    if ((threadIdx.x & 63) == 0 && total) atomicAdd(&hdr[H_CNT0], total);
    if (flags) atomicOr(&hdr[H_FLAGS], (u64)flags);
}

__global__ void __launch_bounds__(256)
cloud_sample_emit(int64_t NV, const double* __restrict__ V, int64_t NT, const int32_t* __restrict__ T, double thresh,
                  const uint32_t* __restrict__ off, int64_t total, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t k0 = wave * CLOUD_SLICE;
    for (int it = 0; it < CLOUD_SLICE / 64; it++) {
        const int64_t k = k0 + it * 64 + lane;
        if (k0 + it * 64 >= total) break;                   // (wave-uniform)
        const bool valid = k < total;
        int64_t t = -1 - lane, m = 0;
        Tri tr;
        bool ok = false;
        if (valid) {
            // last t in [0, NT) with off[t] <= k  (off[NT] = total > k)
            int64_t lo = 0, hi = NT;
            while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)off[mid] <= k) lo = mid; else hi = mid; }
            t = lo;
            m = k - (int64_t)off[t];
            ok = tri_setup(NV, V, T, t, thresh, tr) == 1;
        }
        int64_t i = 0, base = 0;
        const int64_t t_first = ((int64_t)(uint32_t)__shfl((int)(uint32_t)((u64)t >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)(u64)t, 0);
        const bool uniform = __ballot(ok && t == t_first) == ~0ull;
        if (uniform) {
            // the whole wave lies in one triangle and lane 0 holds the smallest offset: skip the rows in front of it 64 at a time
            const int64_t m0 = ((int64_t)(uint32_t)__shfl((int)(uint32_t)((u64)m >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)(u64)m, 0);
            for (;;) {
                const int64_t row = i + lane;
                const u64 c = row <= tr.n1 ? (u64)tri_row_count(tr, row) : 0ull;
                const int64_t sum = (int64_t)wave_sum(c);
                if (sum == 0 || base + sum > m0) break;
                base += sum;
                i += 64;
            }
        }
        if (ok) {
            int64_t c = 0;
            for (; i <= tr.n1; i++) {
                c = tri_row_count(tr, i);
                if (m < base + c) break;
                base += c;
            }
            if (i <= tr.n1) {                               // (always: m < the triangle's count)
                const int64_t j = m - base;
                const double a = ((double)i + 0.5) / tr.d1, b = ((double)j + 0.5) / tr.d2;
#pragma unroll
                for (int cc = 0; cc < 3; cc++) out[3 * k + cc] = (tr.v1[cc] * a + tr.v2[cc] * b) + tr.p0[cc];
            }
        }
    }
}

struct SampleWs { u64* hdr; uint32_t* counts; uint32_t* tmp; };
static size_t sample_layout(int64_t NT, void* base, SampleWs* out)
{
    const size_t n = (size_t)(NT < 0 ? 0 : NT) + 1;
    Carver c{ static_cast<char*>(base), 0 };
    SampleWs w;
    w.hdr = c.take<u64>(HDR_WORDS);
    w.counts = c.take<uint32_t>(n);
    w.tmp = c.take<uint32_t>(scan_tmp_words(n));
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// (b) greedy radius thinning
// =====================================================================================================================================
constexpr int64_t THIN_MAXC = (1 << 21) - 1;
constexpr uint32_t ST_UNDECIDED = 0u, ST_KEPT = 1u, ST_REMOVED = 2u;
constexpr int THIN_BATCH_MAX = 64;

// Cell edge: r (1 + 2^-20), not r.  The test is fl((dx dx + dy dy) + dz dz) <= fl(r r), which a pair whose exact distance exceeds r
// by a few ulp can pass, and the cell coordinate floor(fl(fl(p - min) / h)) carries an absolute rounding error of up to 2^21 2^-52.
// With h = r (1 + 2^-20) two points that pass the test have quotients less than 1 - 2^-21 apart: their cells differ by at most one
// per axis, rounding included, so the 27 cells around a point hold every neighbour the sequential loop would see.
__device__ __forceinline__ double thin_cell(double r) { return r * (1.0 + 1.0 / 1048576.0); }
__device__ __forceinline__ u64 thin_pack(int64_t x, int64_t y, int64_t z) { return ((u64)x << 42) | ((u64)y << 21) | (u64)z; }
__device__ __forceinline__ int64_t thin_coord(double p, double lo, double h)
{
    const double f = floor((p - lo) / h);
    return !(f >= 0.0) ? 0 : (f > (double)THIN_MAXC ? THIN_MAXC : (int64_t)f);
}

__global__ void __launch_bounds__(256)
thin_keys(int64_t N, const double* __restrict__ pts, double r, u64* __restrict__ hdr, u64* __restrict__ keys, uint32_t* __restrict__ lo32, uint32_t* __restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double h = thin_cell(r);
    if (i == 0) {
        bool big = false;
        for (int c = 0; c < 3; c++) {
            const double lo = unordered64(hdr[c]), hi = unordered64(hdr[3 + c]);
            if (lo <= hi && !(floor((hi - lo) / h) <= (double)THIN_MAXC)) big = true;
        }
        if (big) atomicOr(&hdr[H_FLAGS], (u64)CLOUD_F_CELLS);
    }
    if (i >= N) return;
    int64_t c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) c[a] = thin_coord(pts[3 * i + a], unordered64(hdr[a]), h);
    const u64 key = thin_pack(c[0], c[1], c[2]);
    keys[i] = key;
    lo32[i] = (uint32_t)key;
    idx[i] = (uint32_t)i;
}
__global__ void __launch_bounds__(256)
thin_gather(int64_t N, const double* __restrict__ pts, const u64* __restrict__ keys, const uint32_t* __restrict__ idx,
            u64* __restrict__ skeys, double* __restrict__ spts, uint32_t* __restrict__ sorder, uint32_t* __restrict__ state)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const uint32_t i = idx[s];
    skeys[s] = keys[i];
    spts[3 * s] = pts[3 * (int64_t)i]; spts[3 * s + 1] = pts[3 * (int64_t)i + 1]; spts[3 * s + 2] = pts[3 * (int64_t)i + 2];
    sorder[s] = i;
    state[s] = ST_UNDECIDED;
}

// one round over the undecided (list == nullptr: all N points).  Still-undecided points are appended to list_out.
__global__ void __launch_bounds__(256)
thin_round(int64_t N, const uint32_t* __restrict__ list, const uint32_t* __restrict__ cnt_in, const u64* __restrict__ skeys,
           const double* __restrict__ spts, const uint32_t* __restrict__ sorder, uint32_t* __restrict__ state, uint32_t* __restrict__ list_out,
           uint32_t* __restrict__ cnt_out, double r2, u64* __restrict__ hdr)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = list ? (int64_t)min((int64_t)*cnt_in, N) : N;
    u64 evals = 0, scans = 0;
    if (t < n) {
        const int64_t s = list ? (int64_t)list[t] : t;
        if (s < N) {
            const uint32_t me = sorder[s];
            const u64 key = skeys[s];
            const int64_t cx = (int64_t)(key >> 42), cy = (int64_t)((key >> 21) & THIN_MAXC), cz = (int64_t)(key & THIN_MAXC);
            const double px = spts[3 * s], py = spts[3 * s + 1], pz = spts[3 * s + 2];
            bool removed = false, pending = false;
            for (int64_t x = max(cx - 1, (int64_t)0); x <= min(cx + 1, THIN_MAXC) && !removed; x++)
                for (int64_t y = max(cy - 1, (int64_t)0); y <= min(cy + 1, THIN_MAXC) && !removed; y++) {
                    const u64 klo = thin_pack(x, y, max(cz - 1, (int64_t)0)), khi = thin_pack(x, y, min(cz + 1, THIN_MAXC));
                    int64_t lo = 0, hi = N;                  // first position with skeys >= klo
                    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (skeys[mid] < klo) lo = mid + 1; else hi = mid; }
                    scans++;
                    for (int64_t q = lo; q < N && skeys[q] <= khi; q++) {
                        if (sorder[q] >= me) continue;
                        const uint32_t st = __hip_atomic_load(&state[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (st == ST_REMOVED) continue;      // (final: removed points never decide anything)
                        const double dx = spts[3 * q] - px, dy = spts[3 * q + 1] - py, dz = spts[3 * q + 2] - pz;
                        evals++;
                        if ((dx * dx + dy * dy) + dz * dz <= r2) {
                            if (st == ST_KEPT) { removed = true; break; }
                            pending = true;
                        }
                    }
                }
            if (removed) __hip_atomic_store(&state[s], ST_REMOVED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else if (!pending) __hip_atomic_store(&state[s], ST_KEPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else {
                const uint32_t slot = atomicAdd(cnt_out, 1u);
                if ((int64_t)slot < N) list_out[slot] = (uint32_t)s;
            }
        }
    }
    evals = wave_sum(evals);
    scans = wave_sum(scans);
    if ((threadIdx.x & 63) == 0 && evals) { atomicAdd(&hdr[H_CNT1], evals); atomicAdd(&hdr[H_CNT3], scans); }
}

__global__ void __launch_bounds__(256)
thin_finish(int64_t N, const uint32_t* __restrict__ sorder, const uint32_t* __restrict__ state, uint8_t* __restrict__ keep, u64* __restrict__ hdr)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    u64 k = 0;
    if (s < N) { k = state[s] == ST_KEPT ? 1u : 0u; keep[sorder[s]] = (uint8_t)k; }
    k = wave_sum(k);
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(&hdr[H_CNT0], k);
}

struct ThinWs { u64* hdr; uint32_t* cnt; u64* keys; u64* skeys; double* spts; uint32_t* sorder; uint32_t* state; Sort63Ws s; };
static size_t thin_layout(int64_t N, void* base, ThinWs* out)
{
    const size_t n = (size_t)(N < 1 ? 1 : N);
    Carver c{ static_cast<char*>(base), 0 };
    ThinWs w;
    w.hdr = c.take<u64>(HDR_WORDS);
    w.cnt = c.take<uint32_t>(THIN_BATCH_MAX + 2);
    w.keys = c.take<u64>(n);
    w.skeys = c.take<u64>(n);
    w.spts = c.take<double>(3 * n);
    w.sorder = c.take<uint32_t>(n);
    w.state = c.take<uint32_t>(n);
    sort63_carve(c, n, w.s);
    w.s.tmp = c.take<uint32_t>(rs_tmp_words(n));
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// (c) nearest neighbour between two clouds
// =====================================================================================================================================
typedef Box3<double> NnBox;

// 30-bit Morton code in the bounding box hdr[0..5] (points outside it -- queries -- are clamped: the order only affects the speed)
__global__ void __launch_bounds__(256)
nn_morton(int64_t N, const double* __restrict__ pts, const u64* __restrict__ box_hdr, uint32_t* __restrict__ codes, uint32_t* __restrict__ idx,
          u64* __restrict__ flag_hdr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    uint32_t code = 0;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!finite3(x, y, z)) atomicOr(&flag_hdr[H_FLAGS], (u64)CLOUD_F_NONFINITE);
    const double p[3] = { x, y, z };
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double lo = unordered64(box_hdr[c]), hi = unordered64(box_hdr[3 + c]);
        const double ext = hi - lo;
        const double cell = ext > 0.0 ? ((p[c] - lo) / ext) * 1023.0 : 0.0;
        code |= morton_spread10((uint32_t)fmin(fmax(cell, 0.0), 1023.0)) << c;
    }
    codes[i] = code;
    idx[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(BOX_POINTS)
nn_gather_boxes(int64_t N, const double* __restrict__ pts, const uint32_t* __restrict__ order, const uint32_t* __restrict__ codes,
                double* __restrict__ sorted, uint32_t* __restrict__ sidx, uint32_t* __restrict__ scodes, NnBox* __restrict__ boxes)
{
    const int64_t i = (int64_t)blockIdx.x * BOX_POINTS + threadIdx.x;
    NnBox b = box_empty<double>();
    if (i < N) {
        const int64_t s = order[i];
#pragma unroll
        for (int c = 0; c < 3; c++) { const double v = pts[3 * s + c]; sorted[3 * i + c] = v; b.lo[c] = b.hi[c] = v; }
        sidx[i] = (uint32_t)s;
        scodes[i] = codes[i];
    }
    __shared__ double s_lo[3][BOX_POINTS / 64], s_hi[3][BOX_POINTS / 64];
    b = block_box(b.lo, b.hi, s_lo, s_hi);
    if (threadIdx.x == 0) boxes[blockIdx.x] = b;
}

__global__ void __launch_bounds__(64)
nn_group_boxes(int64_t num_boxes, const NnBox* __restrict__ boxes, NnBox* __restrict__ groups)
{
    const NnBox r = group_box(num_boxes, boxes, (int64_t)blockIdx.x);
    if (threadIdx.x == 0) groups[blockIdx.x] = r;
}

__device__ __forceinline__ void nn_update(double px, double py, double pz, double cx, double cy, double cz, uint32_t ci, double& best, uint32_t& besti)
{
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    const double d = (dx * dx + dy * dy) + dz * dz;
    if (d < best || (d == best && ci < besti)) { best = d; besti = ci; }
}

__global__ void __launch_bounds__(BOX_POINTS)
nn_search(int64_t NQ, const double* __restrict__ query, const uint32_t* __restrict__ qorder, const uint32_t* __restrict__ qcodes,
          int64_t NS, const double* __restrict__ sorted, const uint32_t* __restrict__ sidx, const uint32_t* __restrict__ scodes,
          const NnBox* __restrict__ boxes, const NnBox* __restrict__ groups, int64_t num_boxes, int64_t num_groups,
          double* __restrict__ dist, int32_t* __restrict__ nearest, u64* __restrict__ hdr)
{
    __shared__ double s_pts[BOX_POINTS * 3];
    __shared__ uint32_t s_idx[BOX_POINTS];
    const int64_t i = (int64_t)blockIdx.x * BOX_POINTS + threadIdx.x;
    const bool valid = i < NQ;
    int64_t qi = 0;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    double best = __builtin_huge_val();
    uint32_t besti = 0xFFFFFFFFu;
    u64 scanned = 0, staged = 0, evals = 0;
    if (valid) {
        qi = qorder[i];
        qx = query[3 * qi]; qy = query[3 * qi + 1]; qz = query[3 * qi + 2];
        // a first bound: the query's neighbours in the Morton order of the reference cloud
        const uint32_t code = qcodes[i];
        int64_t lo = 0, hi = NS;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (scodes[mid] < code) lo = mid + 1; else hi = mid; }
        for (int64_t p = max(lo - 2, (int64_t)0); p < min(lo + 2, NS); p++) {
            nn_update(qx, qy, qz, sorted[3 * p], sorted[3 * p + 1], sorted[3 * p + 2], sidx[p], best, besti);
            evals++;
        }
    }
    for (int64_t g = 0; g < num_groups; g++) {
        const bool need_g = valid && !(box_dist(groups[g], qx, qy, qz) > best);
        if (!__syncthreads_or(need_g)) continue;
        const int64_t b1 = min(num_boxes, (g + 1) * BOX_GROUP);
        for (int64_t b = g * BOX_GROUP; b < b1; b++) {
            const bool need = valid && !(box_dist(boxes[b], qx, qy, qz) > best);
            if (!__syncthreads_or(need)) continue;                     // (also the barrier before restaging)
            const int64_t j0 = b * BOX_POINTS;
            const int cnt = (int)min((int64_t)BOX_POINTS, NS - j0);
            if ((int)threadIdx.x < cnt) {
                const int64_t j = j0 + threadIdx.x;
                s_pts[3 * threadIdx.x] = sorted[3 * j]; s_pts[3 * threadIdx.x + 1] = sorted[3 * j + 1]; s_pts[3 * threadIdx.x + 2] = sorted[3 * j + 2];
                s_idx[threadIdx.x] = sidx[j];
            }
            __syncthreads();
            if (threadIdx.x == 0) staged++;
            if (need) {
                for (int j = 0; j < cnt; j++) nn_update(qx, qy, qz, s_pts[3 * j], s_pts[3 * j + 1], s_pts[3 * j + 2], s_idx[j], best, besti);
                scanned++;
                evals += (u64)cnt;
            }
        }
    }
    if (valid) { dist[qi] = sqrt(best); nearest[qi] = (int32_t)besti; }
    scanned = wave_sum(scanned); staged = wave_sum(staged); evals = wave_sum(evals);
    if ((threadIdx.x & 63) == 0) {
        if (scanned) atomicAdd(&hdr[H_CNT0], scanned);
        if (staged) atomicAdd(&hdr[H_CNT1], staged);
        if (evals) atomicAdd(&hdr[H_CNT2], evals);
    }
}
__global__ void __launch_bounds__(256)
nn_fill_empty(int64_t NQ, double* __restrict__ dist, int32_t* __restrict__ nearest)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NQ) { dist[i] = __builtin_huge_val(); nearest[i] = -1; }
}

struct NnIndex { u64* hdr; double* sorted; uint32_t* sidx; uint32_t* scodes; NnBox* boxes; NnBox* groups; uint32_t *ka, *kb, *va, *vb, *tmp; };
static size_t nn_index_layout(int64_t NS, void* base, NnIndex* out)
{
    const size_t n = (size_t)(NS < 1 ? 1 : NS);
    const int64_t nb = box_count((int64_t)n), ng = group_count(nb);
    Carver c{ static_cast<char*>(base), 0 };
    NnIndex w;
    w.hdr = c.take<u64>(HDR_WORDS);
    w.sorted = c.take<double>(3 * n);
    w.sidx = c.take<uint32_t>(n);
    w.scodes = c.take<uint32_t>(n);
    w.boxes = c.take<NnBox>(nb);
    w.groups = c.take<NnBox>(ng);
    w.ka = c.take<uint32_t>(n); w.kb = c.take<uint32_t>(n); w.va = c.take<uint32_t>(n); w.vb = c.take<uint32_t>(n);
    w.tmp = c.take<uint32_t>(rs_tmp_words(n));
    if (out) *out = w;
    return c.total();
}
struct NnQueryWs { u64* hdr; uint32_t *ka, *kb, *va, *vb, *tmp; };
static size_t nn_query_layout(int64_t NQ, void* base, NnQueryWs* out)
{
    const size_t n = (size_t)(NQ < 1 ? 1 : NQ);
    Carver c{ static_cast<char*>(base), 0 };
    NnQueryWs w;
    w.hdr = c.take<u64>(HDR_WORDS);
    w.ka = c.take<uint32_t>(n); w.kb = c.take<uint32_t>(n); w.va = c.take<uint32_t>(n); w.vb = c.take<uint32_t>(n);
    w.tmp = c.take<uint32_t>(rs_tmp_words(n));
    if (out) *out = w;
    return c.total();
}

static int flags_error(u64 flags, const char* who)
{
    if (flags & CLOUD_F_NONFINITE) { set_error("%s: a coordinate is not finite", who); return GOF_E_INVALID; }
    if (flags & CLOUD_F_INDEX) { set_error("%s: a triangle names a vertex outside [0, num_vertices)", who); return GOF_E_INVALID; }
    if (flags & CLOUD_F_CELLS) { set_error("%s: the cloud spans more than 2^21 - 1 cells of edge r per axis", who); return GOF_E_INVALID; }
    return GOF_OK;
}

} // namespace gof

using namespace gof;

extern "C" {

size_t gof_cloud_sample_ws_bytes(int64_t NT) { return sample_layout(NT, nullptr, nullptr); }

int gof_cloud_sample_count(int64_t NV, const double* V, int64_t NT, const int32_t* T, double thresh, void* ws, size_t ws_bytes,
                           int64_t* num_samples, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_samples) { set_error("cloud_sample: num_samples is NULL"); return GOF_E_INVALID; }
    *num_samples = 0;
    if (bad_count(NV) || bad_count(NT)) { set_error("cloud_sample: bad counts (%lld vertices, %lld triangles)", (long long)NV, (long long)NT); return GOF_E_INVALID; }
    if (!(thresh > 0.0) || !(thresh <= DBL_MAX)) { set_error("cloud_sample: thresh must be positive and finite"); return GOF_E_INVALID; }
    if ((NV && !V) || (NT && !T) || !ws) { set_error("cloud_sample: vertices / triangles / workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_cloud_sample_ws_bytes(NT)) { set_error("cloud_sample: workspace too small"); return GOF_E_WORKSPACE; }
    SampleWs w;
    sample_layout(NT, ws_aligned(ws), &w);
    GOF_PROFILE("cloud_sample_count", stream);
    hipLaunchKernelGGL(cloud_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    const int64_t n = (NT + 1 > NV ? NT + 1 : NV);
    hipLaunchKernelGGL(cloud_sample_count, grid_of(n), dim3(256), 0, stream, NV, V, NT, T, thresh, w.counts, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.counts, nullptr, w.counts, (size_t)NT + 1, false, w.tmp, nullptr, stream));
    u64 h[2];
    GOF_HIP_CHECK(hipMemcpyAsync(h, w.hdr + H_FLAGS, sizeof(h), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (int e = flags_error(h[0], "cloud_sample")) return e;
    if (h[1] >= (1ull << 31)) { set_error("cloud_sample: %llu samples or a lattice finer than 2^30 steps (at most 2^31 - 1 samples)", h[1]); return GOF_E_CAPACITY; }
    *num_samples = (int64_t)h[1];
    return GOF_OK;
}

int gof_cloud_sample_emit(int64_t NV, const double* V, int64_t NT, const int32_t* T, double thresh, void* ws, size_t ws_bytes,
                          int64_t num_samples, double* points, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NV) || bad_count(NT) || bad_count(num_samples)) { set_error("cloud_sample: bad counts"); return GOF_E_INVALID; }
    if (num_samples == 0) return GOF_OK;
    if (!V || !T || !ws || !points || NT == 0) { set_error("cloud_sample: vertices / triangles / workspace / points is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_cloud_sample_ws_bytes(NT)) { set_error("cloud_sample: workspace too small"); return GOF_E_WORKSPACE; }
    SampleWs w;
    sample_layout(NT, ws_aligned(ws), &w);
    GOF_PROFILE("cloud_sample_emit", stream);
    const int64_t waves = (num_samples + CLOUD_SLICE - 1) / CLOUD_SLICE;
    hipLaunchKernelGGL(cloud_sample_emit, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, NV, V, NT, T, thresh, w.counts, num_samples, points);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

size_t gof_cloud_thin_ws_bytes(int64_t N) { return thin_layout(N, nullptr, nullptr); }

int gof_cloud_thin(int64_t N, const double* points, double r, uint8_t* keep, void* ws, size_t ws_bytes, int64_t* num_kept, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_kept) { set_error("cloud_thin: num_kept is NULL"); return GOF_E_INVALID; }
    *num_kept = 0;
    if (bad_count(N)) { set_error("cloud_thin: bad number of points (%lld)", (long long)N); return GOF_E_INVALID; }
    if (!(r > 0.0) || !(r <= DBL_MAX) || !(r * r <= DBL_MAX)) { set_error("cloud_thin: r must be positive and finite"); return GOF_E_INVALID; }
    if (!ws) { set_error("cloud_thin: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_cloud_thin_ws_bytes(N)) { set_error("cloud_thin: workspace too small"); return GOF_E_WORKSPACE; }
    ThinWs w;
    thin_layout(N, ws_aligned(ws), &w);
    hipLaunchKernelGGL(cloud_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    if (N == 0) return GOF_OK;
    if (!points || !keep) { set_error("cloud_thin: points / keep is NULL"); return GOF_E_INVALID; }
    GOF_PROFILE("cloud_thin", stream);
    hipLaunchKernelGGL(cloud_bbox, dim3((unsigned)min((int64_t)2048, (N + 255) / 256)), dim3(256), 0, stream, N, points, w.hdr);
    hipLaunchKernelGGL(thin_keys, grid_of(N), dim3(256), 0, stream, N, points, r, w.hdr, w.keys, w.s.lo[0], w.s.idx[0]);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t* order = nullptr;
    GOF_HIP_CHECK(sort_keys63(w.keys, (size_t)N, w.s, &order, stream));
    hipLaunchKernelGGL(thin_gather, grid_of(N), dim3(256), 0, stream, N, points, w.keys, order, w.skeys, w.spts, w.sorder, w.state);
    GOF_LAUNCH_CHECK(stream, 0);
    // the sort's buffers are dead now: the two lists of the undecided live in its key buffers
    uint32_t* lists[2] = { w.s.lo[0], w.s.lo[1] };
    const double r2 = r * r;
    int64_t count = N, rounds = 0, readbacks = 0;
    int batch = 4;
    while (count > 0) {
        GOF_HIP_CHECK(hipMemsetAsync(w.cnt + 1, 0, (size_t)batch * sizeof(uint32_t), stream));
        for (int b = 0; b < batch; b++, rounds++) {
            hipLaunchKernelGGL(thin_round, grid_of(count), dim3(256), 0, stream, N, rounds == 0 ? (const uint32_t*)nullptr : lists[rounds & 1],
                               w.cnt + b, w.skeys, w.spts, w.sorder, w.state, lists[(rounds + 1) & 1], w.cnt + b + 1, r2, w.hdr);
        }
        GOF_LAUNCH_CHECK(stream, 0);
        uint32_t left = 0;
        u64 flags = 0;
        GOF_HIP_CHECK(hipMemcpyAsync(&left, w.cnt + batch, 4, hipMemcpyDeviceToHost, stream));
        GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr + H_FLAGS, 8, hipMemcpyDeviceToHost, stream));
        GOF_HIP_CHECK(hipStreamSynchronize(stream));
        readbacks++;
        if (int e = flags_error(flags, "cloud_thin")) return e;
        if ((int64_t)left > count) { set_error("cloud_thin: inconsistent undecided count"); return GOF_E_DEVICE; }
        count = left;
        hipLaunchKernelGGL(cloud_set_u32, dim3(1), dim3(64), 0, stream, w.cnt, left);
        if (batch < THIN_BATCH_MAX) batch *= 2;
    }
    hipLaunchKernelGGL(thin_finish, grid_of(N), dim3(256), 0, stream, N, w.sorder, w.state, keep, w.hdr);
    hipLaunchKernelGGL(cloud_set_words, dim3(1), dim3(64), 0, stream, w.hdr + 11, (u64)rounds, (u64)readbacks);
    GOF_LAUNCH_CHECK(stream, 0);
    u64 kept = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&kept, w.hdr + H_CNT0, 8, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    *num_kept = (int64_t)kept;
    return GOF_OK;
}

int gof_cloud_thin_stats(const void* ws, int64_t* stats, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!ws || !stats) { set_error("cloud_thin_stats: NULL argument"); return GOF_E_INVALID; }
    const u64* hdr = static_cast<const u64*>(ws_aligned(ws));
    u64 h[HDR_WORDS];
    GOF_HIP_CHECK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    stats[0] = (int64_t)h[11]; stats[1] = (int64_t)h[H_CNT1]; stats[2] = (int64_t)h[12]; stats[3] = (int64_t)h[H_CNT3];
    return GOF_OK;
}

size_t gof_cloud_nn_index_bytes(int64_t NS) { return nn_index_layout(NS, nullptr, nullptr); }
size_t gof_cloud_nn_query_ws_bytes(int64_t NQ) { return nn_query_layout(NQ, nullptr, nullptr); }

int gof_cloud_nn_build(int64_t NS, const double* ref, void* index, size_t index_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NS)) { set_error("cloud_nn: bad number of reference points (%lld)", (long long)NS); return GOF_E_INVALID; }
    if (!index || (NS && !ref)) { set_error("cloud_nn: ref / index is NULL"); return GOF_E_INVALID; }
    if (index_bytes < gof_cloud_nn_index_bytes(NS)) { set_error("cloud_nn: index buffer too small"); return GOF_E_WORKSPACE; }
    NnIndex w;
    nn_index_layout(NS, ws_aligned(index), &w);
    hipLaunchKernelGGL(cloud_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    if (NS == 0) return GOF_OK;
    GOF_PROFILE("cloud_nn_build", stream);
    const int64_t nb = box_count(NS), ng = group_count(nb);
    hipLaunchKernelGGL(cloud_bbox, dim3((unsigned)min((int64_t)2048, (NS + 255) / 256)), dim3(256), 0, stream, NS, ref, w.hdr);
    hipLaunchKernelGGL(nn_morton, grid_of(NS), dim3(256), 0, stream, NS, ref, w.hdr, w.ka, w.va, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t *kr = nullptr, *vr = nullptr;
    GOF_HIP_CHECK(radix_sort_pairs_u32(w.ka, w.va, w.kb, w.vb, (size_t)NS, 30, w.tmp, &kr, &vr, stream));
    hipLaunchKernelGGL(nn_gather_boxes, dim3((unsigned)nb), dim3(BOX_POINTS), 0, stream, NS, ref, vr, kr, w.sorted, w.sidx, w.scodes, w.boxes);
    hipLaunchKernelGGL(nn_group_boxes, dim3((unsigned)ng), dim3(64), 0, stream, nb, w.boxes, w.groups);
    GOF_LAUNCH_CHECK(stream, 0);
    u64 flags = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr + H_FLAGS, 8, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    return flags_error(flags, "cloud_nn (reference cloud)");
}

int gof_cloud_nn_query(int64_t NS, const void* index, size_t index_bytes, int64_t NQ, const double* query, double* dist, int32_t* nearest,
                       void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NS) || bad_count(NQ)) { set_error("cloud_nn: bad counts (%lld reference, %lld query points)", (long long)NS, (long long)NQ); return GOF_E_INVALID; }
    if (!index || !ws) { set_error("cloud_nn: index / workspace is NULL"); return GOF_E_INVALID; }
    if (index_bytes < gof_cloud_nn_index_bytes(NS) || ws_bytes < gof_cloud_nn_query_ws_bytes(NQ)) { set_error("cloud_nn: index or workspace too small"); return GOF_E_WORKSPACE; }
    NnIndex x;
    nn_index_layout(NS, const_cast<void*>(ws_aligned(index)), &x);
    NnQueryWs w;
    nn_query_layout(NQ, ws_aligned(ws), &w);
    hipLaunchKernelGGL(cloud_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    if (NQ == 0) return GOF_OK;
    if (!query || !dist || !nearest) { set_error("cloud_nn: query / dist / nearest is NULL"); return GOF_E_INVALID; }
    GOF_PROFILE("cloud_nn_query", stream);
    hipLaunchKernelGGL(cloud_set_words, dim3(1), dim3(64), 0, stream, w.hdr + 11, (u64)NQ, (u64)NS);
    if (NS == 0) {
        hipLaunchKernelGGL(nn_fill_empty, grid_of(NQ), dim3(256), 0, stream, NQ, dist, nearest);
        GOF_LAUNCH_CHECK(stream, 0);
        return GOF_OK;
    }
    const int64_t nb = box_count(NS), ng = group_count(nb);
    hipLaunchKernelGGL(nn_morton, grid_of(NQ), dim3(256), 0, stream, NQ, query, x.hdr, w.ka, w.va, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t *kr = nullptr, *vr = nullptr;
    GOF_HIP_CHECK(radix_sort_pairs_u32(w.ka, w.va, w.kb, w.vb, (size_t)NQ, 30, w.tmp, &kr, &vr, stream));
    hipLaunchKernelGGL(nn_search, dim3((unsigned)box_count(NQ)), dim3(BOX_POINTS), 0, stream, NQ, query, vr, kr, NS, x.sorted, x.sidx,
                       x.scodes, x.boxes, x.groups, nb, ng, dist, nearest, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    u64 flags = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr + H_FLAGS, 8, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    return flags_error(flags, "cloud_nn (query cloud)");
}

int gof_cloud_nn_stats(const void* ws, int64_t* stats, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!ws || !stats) { set_error("cloud_nn_stats: NULL argument"); return GOF_E_INVALID; }
    const u64* hdr = static_cast<const u64*>(ws_aligned(ws));
    u64 h[HDR_WORDS];
    GOF_HIP_CHECK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    stats[0] = (int64_t)h[H_CNT0]; stats[1] = (int64_t)h[H_CNT1]; stats[2] = (int64_t)h[H_CNT2]; stats[3] = (int64_t)h[11];
    return GOF_OK;
}

} // extern "C"
