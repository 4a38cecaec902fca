// box_index.h -- the two-level box index over a Morton-ordered cloud that knn.hip (fp32, 3 nearest within one cloud) and cloud.hip
// part (c) (fp64, nearest between two clouds) search: boxes of BOX_POINTS consecutive points (one workgroup), groups of BOX_GROUP
// consecutive boxes, each with its min / max, and the conservative distance of a point to a box.  Device pieces are force-inlined
// templates over the coordinate type; the kernels, their gather halves and the two searches stay in the units.
#pragma once
#include <limits>
#include "gof_geom.h"

namespace gof {

constexpr int BOX_POINTS = 256;     // points per box = threads of the workgroup that builds or searches it
constexpr int BOX_GROUP = 32;       // boxes per group

template <class T> struct Box3 { T lo[3]; T hi[3]; };
template <> struct Box3<float> { float lo[3]; float hi[3]; float pad[2] = { 0.f, 0.f }; };     // 32 B; the pad is stored as zeros
static_assert(sizeof(Box3<float>) == 32 && sizeof(Box3<double>) == 48, "the workspace layouts carve arrays of these");

// ---- host --------------------------------------------------------------------------------------------------------------------------
static inline int64_t box_count(int64_t n) { return (n + BOX_POINTS - 1) / BOX_POINTS; }
static inline int64_t group_count(int64_t nb) { return (nb + BOX_GROUP - 1) / BOX_GROUP; }

// ---- device ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float box_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double box_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float box_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double box_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float box_abs(float a) { return fabsf(a); }
__device__ __forceinline__ double box_abs(double a) { return fabs(a); }

// the box of no points (simple_knn.cu:88-92)
template <class T> __device__ __forceinline__ Box3<T> box_empty()
{
    constexpr T M = std::numeric_limits<T>::max();
    Box3<T> b;
#pragma unroll
    for (int c = 0; c < 3; c++) { b.lo[c] = M; b.hi[c] = -M; }
    return b;
}

// the wave's min / max of one coordinate, then of three, in every lane (all 64 lanes must call)
template <class T> __device__ __forceinline__ void wave_minmax(T& lo, T& hi)
{
    for (int o = 32; o > 0; o >>= 1) { lo = box_min(lo, __shfl_xor(lo, o)); hi = box_max(hi, __shfl_xor(hi, o)); }
}
template <class T> __device__ __forceinline__ void wave_minmax3(T (&lo)[3], T (&hi)[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++) wave_minmax(lo[c], hi[c]);
}

// the min / max over a workgroup of BOX_POINTS threads (all must call; s_lo / s_hi: its LDS); the result is thread 0's only
template <class T> __device__ __forceinline__ Box3<T> block_box(T (&lo)[3], T (&hi)[3], T (&s_lo)[3][BOX_POINTS / 64], T (&s_hi)[3][BOX_POINTS / 64])
{
#pragma unroll
    for (int c = 0; c < 3; c++) {
        wave_minmax(lo[c], hi[c]);
        if ((threadIdx.x & 63) == 0) { s_lo[c][threadIdx.x >> 6] = lo[c]; s_hi[c][threadIdx.x >> 6] = hi[c]; }
    }
    __syncthreads();
    Box3<T> b;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            b.lo[c] = box_min(box_min(s_lo[c][0], s_lo[c][1]), box_min(s_lo[c][2], s_lo[c][3]));
            b.hi[c] = box_max(box_max(s_hi[c][0], s_hi[c][1]), box_max(s_hi[c][2], s_hi[c][3]));
        }
    }
    return b;
}

// the min / max of the boxes of group g, in every lane of a workgroup of one wave
template <class T> __device__ __forceinline__ Box3<T> group_box(int64_t num_boxes, const Box3<T>* __restrict__ boxes, int64_t g)
{
    const int64_t b = g * BOX_GROUP + (threadIdx.x & (BOX_GROUP - 1));
    Box3<T> r = box_empty<T>();
    if (b < num_boxes && threadIdx.x < BOX_GROUP) {
#pragma unroll
        for (int c = 0; c < 3; c++) { r.lo[c] = boxes[b].lo[c]; r.hi[c] = boxes[b].hi[c]; }
    }
    wave_minmax3(r.lo, r.hi);
    return r;
}

// Squared distance of a point to a box (simple_knn.cu:126-136), conservative IN FLOATING POINT: subtraction, fabs, min, squaring and
// the two additions of non-negative terms are each monotone in |difference| in any IEEE format, and a point inside the box is at least
// as far from p along every axis as the nearer face, so fl(this) <= fl(squared distance of p to any point of the box) when that is
// summed in the same order.  A search may therefore skip a box whose distance EXCEEDS its current bound and lose nothing; ties must
// be visited.
template <class T> __device__ __forceinline__ T box_dist(const Box3<T>& box, T px, T py, T pz)
{
    T dx = 0, dy = 0, dz = 0;
    if (px < box.lo[0] || px > box.hi[0]) dx = box_min(box_abs(px - box.lo[0]), box_abs(px - box.hi[0]));
    if (py < box.lo[1] || py > box.hi[1]) dy = box_min(box_abs(py - box.lo[1]), box_abs(py - box.hi[1]));
    if (pz < box.lo[2] || pz > box.hi[2]) dz = box_min(box_abs(pz - box.lo[2]), box_abs(pz - box.hi[2]));
    return (dx * dx + dy * dy) + dz * dz;
}

} // namespace gof
