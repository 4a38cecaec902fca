// knn.hip -- mean squared distance to the 3 nearest neighbours (replaces reference submodules/simple-knn/simple_knn.cu).
//
// Same idea as the reference (Morton order -> boxes -> conservative pruning -> exact 3-NN), laid out for wave64 / LDS:
//   1. bounding box of the points AND the origin (the reference reduces with init = {0,0,0}, simple_knn.cu:191-199) with
//      order-preserving integer atomics; no host read-back (the reference copies min/max to the host twice);
//   2. 30-bit Morton codes (simple_knn.cu:39-57), stable radix sort (the library's own, 4 passes);
//   3. the points are GATHERED into Morton order once (float4), boxes of 256 consecutive points (one workgroup) and groups
//      of 32 boxes get their min/max (box_index.h, shared with cloud.hip's nearest search);
//   4. one workgroup per box: every thread owns one query point; the workgroup walks the group boxes, then the boxes of the
//      groups some thread still needs (__syncthreads_or), stages the 256 candidates of a box in LDS (coalesced float4) and
//      every thread that needs the box scans them from LDS (same-address broadcasts).  The reference lets every thread walk
//      all boxes alone and gather candidates through an index array (uncoalesced, divergent).
// Pruning is exact in floating point (box_dist, box_index.h): a box is skipped only if its distance exceeds the current 3rd best
// (simple_knn.cu:171-173), ties are visited.
#include <hip/hip_runtime.h>
#include <cfloat>
#include "../../include/gof_hip.h"
#include "../../include/gof_knn_hip.h"
#include "gof_common.h"
#include "radix.h"
#include "box_index.h"

namespace gof {

typedef Box3<float> KnnBox;

__global__ void __launch_bounds__(256)
knn_minmax(int64_t N, const float* __restrict__ pts, uint32_t* __restrict__ mm)   // mm[0..2] = min, mm[3..5] = max (ordered encoding)
{
    float lo[3] = { 0.f, 0.f, 0.f }, hi[3] = { 0.f, 0.f, 0.f };                  // init = origin (simple_knn.cu:191)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256)
#pragma unroll
        for (int c = 0; c < 3; c++) { const float v = pts[3 * i + c]; lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v); }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        for (int o = 32; o > 0; o >>= 1) { lo[c] = fminf(lo[c], __shfl_xor(lo[c], o)); hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o)); }
        if ((threadIdx.x & 63) == 0) { atomicMin(&mm[c], ordered32(lo[c])); atomicMax(&mm[3 + c], ordered32(hi[c])); }
    }
}

__global__ void __launch_bounds__(256)
knn_morton(int64_t N, const float* __restrict__ pts, const uint32_t* __restrict__ mm, uint32_t* __restrict__ codes, uint32_t* __restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    uint32_t code = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float lo = unordered32(mm[c]), hi = unordered32(mm[3 + c]);
        // simple_knn.cu:50-52; a degenerate axis (hi == lo) maps to cell 0 instead of converting a NaN (the order only
        // affects the pruning efficiency, never the result)
        const float ext = hi - lo;
        const float cell = ext > 0.f ? ((pts[3 * i + c] - lo) / ext) * (float)((1 << 10) - 1) : 0.f;
        code |= morton_spread10((uint32_t)fminf(fmaxf(cell, 0.f), 1023.f)) << c;
    }
    codes[i] = code;
    idx[i] = (uint32_t)i;
}

// gather into Morton order + box bounds; one workgroup per box
__global__ void __launch_bounds__(BOX_POINTS)
knn_gather_boxes(int64_t N, const float* __restrict__ pts, const uint32_t* __restrict__ order, float4* __restrict__ sorted, KnnBox* __restrict__ boxes)
{
    const int64_t i = (int64_t)blockIdx.x * BOX_POINTS + threadIdx.x;
    KnnBox b = box_empty<float>();
    if (i < N) {
        const size_t s = order[i];
        const float x = pts[3 * s], y = pts[3 * s + 1], z = pts[3 * s + 2];
        sorted[i] = make_float4(x, y, z, 0.f);
        b.lo[0] = b.hi[0] = x; b.lo[1] = b.hi[1] = y; b.lo[2] = b.hi[2] = z;
    }
    __shared__ float s_lo[3][BOX_POINTS / 64], s_hi[3][BOX_POINTS / 64];
    b = block_box(b.lo, b.hi, s_lo, s_hi);
    if (threadIdx.x == 0) boxes[blockIdx.x] = b;
}

__global__ void __launch_bounds__(64)
knn_group_boxes(int64_t num_boxes, const KnnBox* __restrict__ boxes, KnnBox* __restrict__ groups)
{
    const KnnBox r = group_box(num_boxes, boxes, (int64_t)blockIdx.x);
    if (threadIdx.x == 0) groups[blockIdx.x] = r;
}

__device__ __forceinline__ void update3(float px, float py, float pz, float4 c, float best[3])    // updateKBest<3>, simple_knn.cu:139-153
{
    const float dx = c.x - px, dy = c.y - py, dz = c.z - pz;
    float dist = dx * dx + dy * dy + dz * dz;
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (best[j] > dist) { const float t = best[j]; best[j] = dist; dist = t; }
}

__global__ void __launch_bounds__(BOX_POINTS)
knn_search(int64_t N, const float4* __restrict__ sorted, const uint32_t* __restrict__ order, const KnnBox* __restrict__ boxes,
           const KnnBox* __restrict__ groups, int64_t num_boxes, int64_t num_groups, float* __restrict__ out)
{
    __shared__ float4 s_pts[BOX_POINTS];
    const int64_t mybox = blockIdx.x;
    const int64_t i = mybox * BOX_POINTS + threadIdx.x;
    const bool valid = i < N;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) q = sorted[i];
    float best[3] = { FLT_MAX, FLT_MAX, FLT_MAX };

    // own box first: its 255 other points give a tight bound before anything is pruned
    s_pts[threadIdx.x] = q;
    __syncthreads();
    {
        const int cnt = (int)min((int64_t)BOX_POINTS, N - mybox * BOX_POINTS);
        if (valid)
            for (int j = 0; j < cnt; j++)
                if (j != (int)threadIdx.x) update3(q.x, q.y, q.z, s_pts[j], best);      // skips SELF by position only (simple_knn.cu:176-177)
    }
    for (int64_t g = 0; g < num_groups; g++) {
        const bool need_g = valid && !(box_dist(groups[g], q.x, q.y, q.z) > best[2]);
        if (!__syncthreads_or(need_g)) continue;
        const int64_t b1 = min(num_boxes, (g + 1) * BOX_GROUP);
        for (int64_t b = g * BOX_GROUP; b < b1; b++) {
            if (b == mybox) continue;
            const bool need = valid && !(box_dist(boxes[b], q.x, q.y, q.z) > best[2]);     // simple_knn.cu:171-173
            if (!__syncthreads_or(need)) continue;                                                  // (also the barrier before restaging)
            const int64_t j0 = b * BOX_POINTS;
            const int cnt = (int)min((int64_t)BOX_POINTS, N - j0);
            if ((int)threadIdx.x < cnt) s_pts[threadIdx.x] = sorted[j0 + threadIdx.x];
            __syncthreads();
            if (need)
                for (int j = 0; j < cnt; j++) update3(q.x, q.y, q.z, s_pts[j], best);
        }
    }
    if (valid) out[order[i]] = (best[0] + best[1] + best[2]) / 3.0f;                               // simple_knn.cu:183
}

struct KnnWs { uint32_t* mm; uint32_t *ka, *kb, *va, *vb, *tmp; float4* sorted; KnnBox* boxes; KnnBox* groups; };
static size_t knn_layout(int64_t N, void* base, KnnWs* out)
{
    const size_t n = (size_t)(N < 1 ? 1 : N);
    const int64_t nb = box_count((int64_t)n), ng = group_count(nb);
    Carver c{ static_cast<char*>(base), 0 };
    KnnWs w;
    w.mm = c.take<uint32_t>(8);
    w.ka = c.take<uint32_t>(n); w.kb = c.take<uint32_t>(n); w.va = c.take<uint32_t>(n); w.vb = c.take<uint32_t>(n);
    w.tmp = c.take<uint32_t>(rs_tmp_words(n));
    w.sorted = c.take<float4>(n);
    w.boxes = c.take<KnnBox>(nb);
    w.groups = c.take<KnnBox>(ng);
    if (out) *out = w;
    return c.total();
}

__global__ void knn_init_mm(uint32_t* mm)
{
    if (threadIdx.x < 6) mm[threadIdx.x] = 0x80000000u;      // ordered(0.0f): the origin
}

} // namespace gof

using namespace gof;

extern "C" {

size_t gof_knn_ws_bytes(int64_t N) { return knn_layout(N, nullptr, nullptr); }

int gof_knn_mean_dist3(int64_t N, const float* points, float* mean_dists, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (N < 0 || N >= ((int64_t)1 << 31)) { set_error("bad number of points (%lld)", (long long)N); return GOF_E_INVALID; }
    if (N == 0) return GOF_OK;
    if (!points || !mean_dists || !ws) { set_error("points / mean_dists / workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_knn_ws_bytes(N)) { set_error("knn workspace too small"); return GOF_E_WORKSPACE; }
    KnnWs w;
    knn_layout(N, ws_aligned(ws), &w);
    const int64_t nb = box_count(N), ng = group_count(nb);
    GOF_PROFILE("knn_mean_dist3", stream);
    hipLaunchKernelGGL(knn_init_mm, dim3(1), dim3(64), 0, stream, w.mm);
    hipLaunchKernelGGL(knn_minmax, dim3((unsigned)min((int64_t)2048, (N + 255) / 256)), dim3(256), 0, stream, N, points, w.mm);
    hipLaunchKernelGGL(knn_morton, grid_of(N), dim3(256), 0, stream, N, points, w.mm, w.ka, w.va);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t *kr = nullptr, *vr = nullptr;
    GOF_HIP_CHECK(radix_sort_pairs_u32(w.ka, w.va, w.kb, w.vb, (size_t)N, 30, w.tmp, &kr, &vr, stream));
    hipLaunchKernelGGL(knn_gather_boxes, dim3((unsigned)nb), dim3(BOX_POINTS), 0, stream, N, points, vr, w.sorted, w.boxes);
    hipLaunchKernelGGL(knn_group_boxes, dim3((unsigned)ng), dim3(64), 0, stream, nb, w.boxes, w.groups);
    hipLaunchKernelGGL(knn_search, dim3((unsigned)nb), dim3(BOX_POINTS), 0, stream, N, w.sorted, vr, w.boxes, w.groups, nb, ng, mean_dists);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // extern "C"
