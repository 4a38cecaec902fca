// gof_geom.h -- what the stand-alone geometry units (knn, tsdf, cloud, cloud_reg, mesh_cull, delaunay) share besides radix.h: the
// ordered encodings of fp32 / fp64 for integer atomics and sort keys, the 10-bit Morton spread, the 64-bit wave sum, and the host-side
// plumbing of a C-ABI entry point (count check, workspace alignment and carving, the launch grid of one thread per item, the buffers
// of radix.h's 63-bit key sort).  Included by those six units, box_index.h (knn and cloud) and radix.hip only -- neither gof_common.h
// nor radix.h includes it -- so an edit here cannot reach the units of the training step (tests/devtools/dev_same_isa.py watches the
// two headers they do include).
#pragma once
#include <cfloat>
#include <cmath>
#include "gof_common.h"

namespace gof {

typedef unsigned long long u64;

// ---- device ------------------------------------------------------------------------------------------------------------------------
// fp32 <-> u32 and fp64 <-> u64 whose unsigned order is the order of the floats (atomicMin / atomicMax on coordinates, sort keys)
__device__ __forceinline__ uint32_t ordered32(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float unordered32(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }
__device__ __forceinline__ u64 ordered64(double d) { const u64 b = (u64)__double_as_longlong(d); return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }
__device__ __forceinline__ double unordered64(u64 u) { return __longlong_as_double((long long)((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u)); }
__device__ __forceinline__ bool finite3(double x, double y, double z) { return fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX && fabs(z) <= DBL_MAX; }
// bits 0..9 of x to bits 0, 3, .., 27: one axis of a 30-bit Morton code (simple_knn.cu:39-46).  x < 1024: the caller masks or clamps
__device__ __forceinline__ uint32_t morton_spread10(uint32_t x)
{
    x = (x | (x << 16)) & 0x030000FF;
    x = (x | (x << 8)) & 0x0300F00F;
    x = (x | (x << 4)) & 0x030C30C3;
    x = (x | (x << 2)) & 0x09249249;
    return x;
}
// the wave's sum in every lane (all 64 lanes must call)
__device__ __forceinline__ u64 wave_sum(u64 v)
{
    for (int o = 32; o > 0; o >>= 1) v += ((u64)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o) << 32 | (uint32_t)__shfl_xor((int)(uint32_t)v, o));
    return v;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
// one thread per item in workgroups of 256; never an empty grid
static inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1)); }
// a caller's workspace pointer -> the first ALIGN-ed address in it (every *_ws_bytes query includes that slack)
static inline void* ws_aligned(void* ws) { return reinterpret_cast<void*>(align_up(reinterpret_cast<size_t>(ws))); }
static inline const void* ws_aligned(const void* ws) { return reinterpret_cast<const void*>(align_up(reinterpret_cast<size_t>(ws))); }
// an item count the 32-bit indices, scans and sorts cannot take
static inline bool bad_count(int64_t n, int64_t limit = (int64_t)1 << 31) { return n < 0 || n >= limit; }

// Carves a workspace into ALIGN-ed arrays.  base == nullptr sizes it: every pointer comes back null and only `off` moves.
struct Carver {
    char* base;
    size_t off;      // end of the last array taken (not padded)
    template <class T> T* take(size_t count)
    {
        off = align_up(off);
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return r;
    }
    size_t total() const { return align_up(off) + ALIGN; }      // + the slack ws_aligned may consume
};

// The buffers of sort_keys63 (radix.h): [n] each; tmp: at least rs_tmp_words(n) words, carved by the unit (it may share it with a scan)
struct Sort63Ws { uint32_t* lo[2]; uint32_t* idx[2]; uint32_t* hi[2]; uint32_t* tmp; };
inline void sort63_carve(Carver& c, size_t n, Sort63Ws& w)
{
    for (int k = 0; k < 2; k++) { w.lo[k] = c.take<uint32_t>(n); w.idx[k] = c.take<uint32_t>(n); w.hi[k] = c.take<uint32_t>(n); }
}

} // namespace gof
