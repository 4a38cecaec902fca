// mesh_simplify.hip -- mesh simplification by uniform vertex clustering with a quadric-error representative (Lindstrom's scheme): what
// every user of fusion/mesh_binary_search_7.ply does first in some other tool.  Contract: DESIGN.md 3.21, include/gof_mesh_hip.h (h).
//
// Cluster.  A vertex's cell i = floor((x - o) / h) per axis packs into the key ix 2^42 + iy 2^21 + iz (bit 63 clear), the keys go through
// radix.h's stable sort_keys63, so the first vertex of a run of equal keys is the smallest vertex index of its cell.  Those first
// vertices are flagged OVER THE VERTICES and scanned: a cell's number is the rank of its smallest vertex index.
// Solve.  Two stable sorts by cluster number (the vertices; the face corners e = 3 f + k by the cluster of their vertex) and, over each
// sorted sequence, the three levels of left-to-right sums of DESIGN.md 3.18 (tiles of 256 positions, blocks of 256 tiles, the blocks):
// one lane per tile / block, so one cluster of nearly all corners costs what 10^5 small ones cost.  A lane RECOMPUTES the item at a
// sorted position (the corner's quadric from faces and vertices: 10 doubles that are never stored per corner); only the first and the
// last open run of a tile (block) are stored.  Then one lane per cluster: mean, regularised 3 x 3 Cholesky solve, fallback to the mean;
// a cluster of one vertex keeps that vertex.
// Faces.  Every index through vertex_cluster; a face with a repeated cluster is dropped; three stable radix passes by the sorted
// triple's c, b, a bring equal triples together in ascending face index, and an entry that equals its predecessor is dropped.
// fp64, -ffp-contract=off and no fma() here: every operation is the IEEE operation numpy performs, in the order written.  No
// floating-point atomics, no cross-lane operation: nothing here depends on which lanes of a wave are active.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_mesh_hip.h"
#include "gof_common.h"
#include "radix.h"
#include "gof_geom.h"

namespace gof {

namespace meshsimp {

constexpr int HDR_WORDS = 8;                    // u32: [0..3], [6] one word per flag (lanes store 1 into them), [4..5] counters (integer atomics)
constexpr int H_INDEX = 0, H_FINITE = 1, H_RANGE = 2, H_CLUSTER = 3, H_COUNT0 = 4, H_COUNT1 = 5, H_SORT = 6;
constexpr uint32_t SUM_TILE = 256u, SUM_BLOCK = SUM_TILE * 256u;
constexpr double CELL_LIMIT = 2097152.0;                      // 2^21 cells per axis
constexpr int64_t MESH_MAX_COUNT = ((int64_t)1 << 31) - 1;    // as mesh_components.hip: the scans run over N + 1 flags

struct Grid { double ox, oy, oz, h; };

__global__ void sm_init_hdr(uint32_t* hdr)
{
    if (threadIdx.x < HDR_WORDS) hdr[threadIdx.x] = 0u;
}

// a pair sort's "gave up waiting for a predecessor" word lives in the sort's scratch, which the next sort clears: keep it in the header
__global__ void sm_keep_sort_error(const uint32_t* __restrict__ flag, uint32_t* __restrict__ hdr)
{
    if (threadIdx.x == 0 && *flag) hdr[H_SORT] = 1u;
}

__device__ __forceinline__ double cell_of(double x, double o, double h) { return floor((x - o) / h); }
__device__ __forceinline__ bool cell_ok(double i) { return i >= 0.0 && i < CELL_LIMIT; }                 // (false for NaN)
__device__ __forceinline__ double cell_centre(double i, double o, double h) { return o + (i + 0.5) * h; }

// every vertex finite and inside the grid
__global__ void __launch_bounds__(256)
sm_validate_vertices(uint32_t NV, const double* __restrict__ V, Grid g, uint32_t* __restrict__ hdr)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= NV) return;
    const double x = V[3 * (size_t)v], y = V[3 * (size_t)v + 1], z = V[3 * (size_t)v + 2];
    if (!finite3(x, y, z)) { hdr[H_FINITE] = 1u; return; }
    if (!cell_ok(cell_of(x, g.ox, g.h)) || !cell_ok(cell_of(y, g.oy, g.h)) || !cell_ok(cell_of(z, g.oz, g.h))) hdr[H_RANGE] = 1u;
}
// every index in [0, NV)
__global__ void __launch_bounds__(256)
sm_validate_faces(int64_t NV, uint32_t NE, const int32_t* __restrict__ faces, uint32_t* __restrict__ hdr)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= NE) return;
    const int32_t v = faces[e];
    if (v < 0 || (int64_t)v >= NV) hdr[H_INDEX] = 1u;
}
// every cluster number in [0, NC)
__global__ void __launch_bounds__(256)
sm_validate_clusters(uint32_t NV, const int32_t* __restrict__ vc, int64_t NC, uint32_t* __restrict__ hdr)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= NV) return;
    const int32_t c = vc[v];
    if (c < 0 || (int64_t)c >= NC) hdr[H_CLUSTER] = 1u;
}

// =====================================================================================================================================
// cluster
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
sc_keys(uint32_t NV, const double* __restrict__ V, Grid g, u64* __restrict__ keys, uint32_t* __restrict__ lo, uint32_t* __restrict__ idx)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= NV) return;
    const u64 ix = (u64)cell_of(V[3 * (size_t)v], g.ox, g.h), iy = (u64)cell_of(V[3 * (size_t)v + 1], g.oy, g.h), iz = (u64)cell_of(V[3 * (size_t)v + 2], g.oz, g.h);
    const u64 k = (ix << 42) + (iy << 21) + iz;
    keys[v] = k;
    lo[v] = (uint32_t)k;
    idx[v] = v;
}
// head[i] = the sorted position i starts a run of equal keys
__global__ void __launch_bounds__(256)
sc_heads(uint32_t NV, const u64* __restrict__ keys, const uint32_t* __restrict__ order, uint32_t* __restrict__ head)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= NV) return;
    head[i] = (i == 0u || keys[order[i]] != keys[order[i - 1]]) ? 1u : 0u;
}
// run[i] = the inclusive scan of head: the 1-based number of position i's run.  A run's first vertex (its smallest index: the sort is
// stable) is remembered per run and flagged over the vertices; first[NV] = 0 (the exclusive scan's last word = NC)
__global__ void __launch_bounds__(256)
sc_firsts(uint32_t NV, const uint32_t* __restrict__ order, const uint32_t* __restrict__ run, uint32_t* __restrict__ run_first, uint32_t* __restrict__ first)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > NV) return;
    if (i == NV) { first[NV] = 0u; return; }
    const uint32_t v = order[i], r = run[i];
    const bool head = i == 0u || run[i - 1] != r;
    first[v] = head ? 1u : 0u;                                   // (every vertex stands at exactly one position)
    if (head) run_first[r - 1u] = v;
}
__global__ void __launch_bounds__(256)
sc_number(uint32_t NV, const uint32_t* __restrict__ order, const uint32_t* __restrict__ run, const uint32_t* __restrict__ run_first,
          const uint32_t* __restrict__ rank, int32_t* __restrict__ vertex_cluster)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < NV) vertex_cluster[order[i]] = (int32_t)rank[run_first[run[i] - 1u]];
}

struct ClusterWs { uint32_t* hdr; u64* keys; Sort63Ws s; uint32_t* run; uint32_t* run_first; uint32_t* first; };
static size_t cluster_layout(int64_t NV, void* base, ClusterWs* out)
{
    const size_t nv = (size_t)(NV < 0 ? 0 : NV);
    Carver c{ static_cast<char*>(base), 0 };
    ClusterWs w{};
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    w.keys = c.take<u64>(nv);
    sort63_carve(c, nv, w.s);
    w.run = c.take<uint32_t>(nv);
    w.run_first = c.take<uint32_t>(nv);
    w.first = c.take<uint32_t>(nv + 1);
    size_t tw = scan_tmp_words(nv + 1);
    if (rs_tmp_words(nv) > tw) tw = rs_tmp_words(nv);
    w.s.tmp = c.take<uint32_t>(tw);
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// sums over the runs of a sorted sequence: DESIGN.md 3.18's three levels, for any item a lane can recompute from its sorted position
// =====================================================================================================================================
// what a cluster's vertices add up to: q = p - centre per axis and the colour channels (integers: exact, whatever the order)
struct VSum {
    double q[3]; u64 c[3];
    __device__ __forceinline__ void add(const VSum& o) { for (int a = 0; a < 3; a++) { q[a] = q[a] + o.q[a]; c[a] += o.c[a]; } }
    __device__ __forceinline__ void clear() { for (int a = 0; a < 3; a++) { q[a] = 0.0; c[a] = 0ull; } }
};
// what a cluster's corners add up to: A (xx xy xz yy yz zz), b, c
struct Quadric {
    double v[10];
    __device__ __forceinline__ void add(const Quadric& o) { for (int a = 0; a < 10; a++) v[a] = v[a] + o.v[a]; }
    __device__ __forceinline__ void clear() { for (int a = 0; a < 10; a++) v[a] = 0.0; }
};

// the item at sorted position i of the vertex sequence (vals[i] = the vertex, keys[i] = its cluster)
struct VertexItems {
    typedef VSum T;
    const double* V; const uint8_t* colors; const uint32_t* vals; const double* centre;
    __device__ __forceinline__ VSum load(uint32_t i, uint32_t cluster) const
    {
        const size_t v = vals[i];
        VSum s;
        for (int a = 0; a < 3; a++) { s.q[a] = V[3 * v + a] - centre[3 * (size_t)cluster + a]; s.c[a] = colors ? (u64)colors[4 * v + a] : 0ull; }
        return s;
    }
};
// the item at sorted position i of the corner sequence (vals[i] = e = 3 f + k, keys[i] = the cluster of the corner's vertex): the
// plane of face f, weighted by its area, in coordinates relative to that cluster's cell centre
struct CornerItems {
    typedef Quadric T;
    const double* V; const int32_t* faces; const uint32_t* vals; const double* centre;
    __device__ __forceinline__ Quadric load(uint32_t i, uint32_t cluster) const
    {
        const size_t f = vals[i] / 3u;
        const double* c = centre + 3 * (size_t)cluster;
        const size_t i0 = (size_t)faces[3 * f], i1 = (size_t)faces[3 * f + 1], i2 = (size_t)faces[3 * f + 2];
        const double q0x = V[3 * i0] - c[0], q0y = V[3 * i0 + 1] - c[1], q0z = V[3 * i0 + 2] - c[2];
        const double q1x = V[3 * i1] - c[0], q1y = V[3 * i1 + 1] - c[1], q1z = V[3 * i1 + 2] - c[2];
        const double q2x = V[3 * i2] - c[0], q2y = V[3 * i2 + 1] - c[1], q2z = V[3 * i2 + 2] - c[2];
        const double e1x = q1x - q0x, e1y = q1y - q0y, e1z = q1z - q0z;
        const double e2x = q2x - q0x, e2y = q2y - q0y, e2z = q2z - q0z;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const double L = sqrt((nx * nx + ny * ny) + nz * nz);
        Quadric s;
        if (L == 0.0) { s.clear(); return s; }
        const double w = 0.5 / L;
        const double d = -((nx * q0x + ny * q0y) + nz * q0z);
        const double wx = w * nx, wy = w * ny, wz = w * nz, wd = w * d;
        s.v[0] = wx * nx; s.v[1] = wx * ny; s.v[2] = wx * nz; s.v[3] = wy * ny; s.v[4] = wy * nz; s.v[5] = wz * nz;
        s.v[6] = wd * nx; s.v[7] = wd * ny; s.v[8] = wd * nz; s.v[9] = wd * d;
        return s;
    }
};

// One run of equal clusters inside a tile (block) is closed: first / last sums of the tile, and the cluster's sum where its whole
// segment [start[c], start[c + 1]) lies in [lo, hi) and (level 2) not already inside one tile.
template <class T>
struct RunOut {
    T* head; T* tail; T* sum; const uint32_t* start; uint32_t lo, hi; bool level2; bool first;
    __device__ __forceinline__ void close(uint32_t c, const T& s)
    {
        if (first) { *head = s; first = false; }
        *tail = s;
        const uint32_t b = start[c], e = start[c + 1];
        if (b >= lo && e <= hi && (!level2 || b / SUM_TILE != (e - 1u) / SUM_TILE)) sum[c] = s;
    }
};
// start[c] = the first sorted position whose cluster is >= c, for c in [0, NC]
__global__ void __launch_bounds__(256)
ss_starts(uint32_t N, const uint32_t* __restrict__ keys, int64_t NC, uint32_t* __restrict__ start)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > N) return;
    const int64_t prev = i == 0u ? -1 : (int64_t)keys[i - 1], cur = i == N ? NC : (int64_t)keys[i];
    for (int64_t c = prev + 1; c <= cur; c++) start[c] = i;
}
// a cluster without an item sums to zero
template <class T>
__global__ void __launch_bounds__(256)
ss_empty(int64_t NC, const uint32_t* __restrict__ start, T* __restrict__ sum)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < NC && start[c + 1] == start[c]) sum[c].clear();
}
// level 1: one lane per tile of SUM_TILE sorted positions
template <class Items>
__global__ void __launch_bounds__(256)
ss_tile_sums(uint32_t N, const uint32_t* __restrict__ keys, Items items, const uint32_t* __restrict__ start, typename Items::T* __restrict__ head,
             typename Items::T* __restrict__ tail, typename Items::T* __restrict__ sum)
{
    typedef typename Items::T T;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if ((u64)t * SUM_TILE >= (u64)N) return;
    const uint32_t lo = t * SUM_TILE;
    const uint32_t hi = N - lo < SUM_TILE ? N : lo + SUM_TILE;
    RunOut<T> out{ &head[t], &tail[t], sum, start, lo, hi, false, true };
    uint32_t c = keys[lo];
    T s = items.load(lo, c);
    for (uint32_t i = lo + 1u; i < hi; i++) {
        const uint32_t k = keys[i];
        if (k != c) { out.close(c, s); c = k; s = items.load(i, k); }
        else s.add(items.load(i, k));
    }
    out.close(c, s);
}
// level 2: one lane per block of 256 tiles; a tile contributes its first run and, where it is another cluster's, its last
template <class T>
__global__ void __launch_bounds__(256)
ss_block_sums(uint32_t N, uint32_t ntiles, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ start, const T* __restrict__ head1,
              const T* __restrict__ tail1, T* __restrict__ head2, T* __restrict__ tail2, T* __restrict__ sum)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if ((u64)u * 256u >= (u64)ntiles) return;
    const uint32_t t0 = u * 256u;
    const uint32_t t1 = ntiles - t0 < 256u ? ntiles : t0 + 256u;
    const uint32_t lo = u * SUM_BLOCK, hi = N - lo < SUM_BLOCK ? N : lo + SUM_BLOCK;
    RunOut<T> out{ &head2[u], &tail2[u], sum, start, lo, hi, true, true };
    uint32_t c = 0u;
    T s;
    s.clear();
    bool open = false;
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t p = t * SUM_TILE, q = N - p < SUM_TILE ? N - 1u : p + SUM_TILE - 1u;
        const uint32_t kf = keys[p], kl = keys[q];
        if (open && kf == c) s.add(head1[t]);
        else { if (open) out.close(c, s); c = kf; s = head1[t]; open = true; }
        if (kl != kf) { out.close(c, s); c = kl; s = tail1[t]; }
    }
    out.close(c, s);
}
// level 3: the lane of the block a segment starts in adds up the blocks it reaches into
template <class T>
__global__ void __launch_bounds__(256)
ss_top_sums(uint32_t nblocks, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ start, const T* __restrict__ head2,
            const T* __restrict__ tail2, T* __restrict__ sum)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u + 1u >= nblocks) return;                               // (the last block has nothing behind it)
    const uint32_t c = keys[(u + 1u) * SUM_BLOCK - 1u];          // the cluster of the block's last position
    const uint32_t b = start[c], e = start[c + 1];
    if (b / SUM_BLOCK != u || (e - 1u) / SUM_BLOCK == u) return;
    T s = tail2[u];
    for (uint32_t v = u + 1u; v <= (e - 1u) / SUM_BLOCK; v++) s.add(head2[v]);
    sum[c] = s;
}

template <class T> struct SumWs { T* head1; T* tail1; T* head2; T* tail2; };
template <class T> static void sum_carve(Carver& c, size_t n, SumWs<T>& w)
{
    const size_t ntiles = (n + SUM_TILE - 1) / SUM_TILE, nblocks = (n + SUM_BLOCK - 1) / SUM_BLOCK;
    w.head1 = c.take<T>(ntiles); w.tail1 = c.take<T>(ntiles);
    w.head2 = c.take<T>(nblocks); w.tail2 = c.take<T>(nblocks);
}
// sum[c] for every c in [0, NC) over the N sorted positions (keys = cluster numbers, ascending; start filled by ss_starts)
template <class Items>
static void segment_sums(uint32_t N, const uint32_t* keys, const Items& items, int64_t NC, const uint32_t* start, const SumWs<typename Items::T>& w,
                         typename Items::T* sum, hipStream_t stream)
{
    typedef typename Items::T T;
    hipLaunchKernelGGL(ss_empty<T>, grid_of(NC), dim3(256), 0, stream, NC, start, sum);
    if (!N) return;
    const uint32_t ntiles = (N + SUM_TILE - 1u) / SUM_TILE, nblocks = (N + SUM_BLOCK - 1u) / SUM_BLOCK;
    hipLaunchKernelGGL(ss_tile_sums<Items>, grid_of(ntiles), dim3(256), 0, stream, N, keys, items, start, w.head1, w.tail1, sum);
    hipLaunchKernelGGL(ss_block_sums<T>, grid_of(nblocks), dim3(256), 0, stream, N, ntiles, keys, start, w.head1, w.tail1, w.head2, w.tail2, sum);
    if (nblocks > 1u) hipLaunchKernelGGL(ss_top_sums<T>, grid_of(nblocks), dim3(256), 0, stream, nblocks, keys, start, w.head2, w.tail2, sum);
}

// =====================================================================================================================================
// solve
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
sv_vertex_pairs(uint32_t NV, const int32_t* __restrict__ vc, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < NV) { keys[v] = (uint32_t)vc[v]; vals[v] = v; }
}
__global__ void __launch_bounds__(256)
sv_corner_pairs(uint32_t NE, const int32_t* __restrict__ faces, const int32_t* __restrict__ vc, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e < NE) { keys[e] = (uint32_t)vc[faces[e]]; vals[e] = e; }
}
// the cell centre of a cluster: that of the cell of its first (smallest) vertex; count[c] = its number of vertices, first[c] = that vertex
__global__ void __launch_bounds__(256)
sv_centres(int64_t NC, const uint32_t* __restrict__ start, const uint32_t* __restrict__ vals, const double* __restrict__ V, Grid g,
           double* __restrict__ centre, uint32_t* __restrict__ count, uint32_t* __restrict__ first)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= NC) return;
    const uint32_t s = start[c], n = start[c + 1] - s;
    count[c] = n;
    first[c] = n ? vals[s] : 0u;
    if (!n) { centre[3 * c] = centre[3 * c + 1] = centre[3 * c + 2] = 0.0; return; }
    const size_t v = vals[s];
    centre[3 * c] = cell_centre(cell_of(V[3 * v], g.ox, g.h), g.ox, g.h);
    centre[3 * c + 1] = cell_centre(cell_of(V[3 * v + 1], g.oy, g.h), g.oy, g.h);
    centre[3 * c + 2] = cell_centre(cell_of(V[3 * v + 2], g.oz, g.h), g.oz, g.h);
}
// one lane per cluster: mean, colours, the regularised solve, the fallback (DESIGN.md 3.21 writes the order of the operations down)
__global__ void __launch_bounds__(256)
sv_solve(int64_t NC, const uint32_t* __restrict__ count, const uint32_t* __restrict__ first, const double* __restrict__ V, const double* __restrict__ centre,
         const VSum* __restrict__ vsum, const Quadric* __restrict__ quad, double h, double* __restrict__ out_pos, uint8_t* __restrict__ out_colors, uint8_t* __restrict__ used_mean, uint32_t* __restrict__ hdr)
{
    __shared__ uint32_t s_used;
    if (threadIdx.x == 0) s_used = 0u;
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < NC) {
        const uint32_t n = count[c];
        const VSum vs = vsum[c];
        const double dn = (double)n;
        double m[3] = { 0.0, 0.0, 0.0 };
        if (n) for (int a = 0; a < 3; a++) m[a] = vs.q[a] / dn;
        if (out_colors) {
            for (int a = 0; a < 3; a++) out_colors[4 * c + a] = n ? (uint8_t)((2ull * vs.c[a] + (u64)n) / (2ull * (u64)n)) : 0;
            out_colors[4 * c + 3] = 0;
        }
        const Quadric Q = quad[c];
        const double t = (Q.v[0] + Q.v[3]) + Q.v[5];
        double y[3] = { m[0], m[1], m[2] };
        bool mean = true;
        if (t != 0.0 && n != 1u) {
            const double lam = t * 0.0009765625;                 // 2^-10
            const double a00 = Q.v[0] + lam, a11 = Q.v[3] + lam, a22 = Q.v[5] + lam, a01 = Q.v[1], a02 = Q.v[2], a12 = Q.v[4];
            const double r0 = lam * m[0] - Q.v[6], r1 = lam * m[1] - Q.v[7], r2 = lam * m[2] - Q.v[8];
            const double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
            const double l11 = sqrt(a11 - l10 * l10), l21 = (a12 - l20 * l10) / l11;
            const double l22 = sqrt((a22 - l20 * l20) - l21 * l21);
            const double z0 = r0 / l00, z1 = (r1 - l10 * z0) / l11, z2 = ((r2 - l20 * z0) - l21 * z1) / l22;
            const double y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = ((z0 - l10 * y1) - l20 * y2) / l00;
            const double half = 0.5 * h;
            if (fabs(y0) <= half && fabs(y1) <= half && fabs(y2) <= half) { y[0] = y0; y[1] = y1; y[2] = y2; mean = false; }      // (false for NaN)
        }
        // a cluster of one vertex keeps that vertex, bit for bit: every plane of its quadric passes through it, so it IS the minimiser
        if (n == 1u) for (int a = 0; a < 3; a++) out_pos[3 * c + a] = V[3 * (size_t)first[c] + a];
        else for (int a = 0; a < 3; a++) out_pos[3 * c + a] = centre[3 * c + a] + y[a];
        used_mean[c] = mean ? 1 : 0;
        if (mean) atomicAdd(&s_used, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_used) atomicAdd(&hdr[H_COUNT0], s_used);
}

struct SolveWs {
    uint32_t* hdr; uint32_t* keys[2]; uint32_t* vals[2]; uint32_t* start; uint32_t* count; uint32_t* first; double* centre; VSum* vsum; Quadric* quad;
    SumWs<VSum> sv; SumWs<Quadric> sq; uint32_t* tmp;
};
static size_t solve_layout(int64_t NV, int64_t NF, int64_t NC, void* base, SolveWs* out)
{
    const size_t nv = (size_t)(NV < 0 ? 0 : NV), ne = 3 * (size_t)(NF < 0 ? 0 : NF), nc = (size_t)(NC < 0 ? 0 : NC);
    const size_t n = nv > ne ? nv : ne;
    Carver c{ static_cast<char*>(base), 0 };
    SolveWs w{};
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    for (int k = 0; k < 2; k++) { w.keys[k] = c.take<uint32_t>(n); w.vals[k] = c.take<uint32_t>(n); }
    w.start = c.take<uint32_t>(nc + 1);
    w.count = c.take<uint32_t>(nc);
    w.first = c.take<uint32_t>(nc);
    w.centre = c.take<double>(3 * nc);
    w.vsum = c.take<VSum>(nc);
    w.quad = c.take<Quadric>(nc);
    sum_carve(c, nv, w.sv);
    sum_carve(c, ne, w.sq);
    w.tmp = c.take<uint32_t>(rs_tmp_words(n));
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// faces
// =====================================================================================================================================
__device__ __forceinline__ void sorted_triple(const int32_t* __restrict__ t, uint32_t& a, uint32_t& b, uint32_t& c)
{
    uint32_t x = (uint32_t)t[0], y = (uint32_t)t[1], z = (uint32_t)t[2], s;
    if (x > y) { s = x; x = y; y = s; }
    if (y > z) { s = y; y = z; z = s; }
    if (x > y) { s = x; x = y; y = s; }
    a = x; b = y; c = z;
}
// out_faces[f] = the clusters of the face's vertices; face_keep[f] = they are pairwise distinct; the first sort's pairs (c, f)
__global__ void __launch_bounds__(256)
sf_remap(uint32_t NF, const int32_t* __restrict__ faces, const int32_t* __restrict__ vc, int32_t* __restrict__ out_faces, uint8_t* __restrict__ face_keep,
         uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ hdr)
{
    __shared__ uint32_t s_drop;
    if (threadIdx.x == 0) s_drop = 0u;
    __syncthreads();
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < NF) {
        const int32_t a = vc[faces[3 * (size_t)f]], b = vc[faces[3 * (size_t)f + 1]], c = vc[faces[3 * (size_t)f + 2]];
        out_faces[3 * (size_t)f] = a; out_faces[3 * (size_t)f + 1] = b; out_faces[3 * (size_t)f + 2] = c;
        const bool keep = a != b && b != c && a != c;
        face_keep[f] = keep ? 1 : 0;
        if (!keep) atomicAdd(&s_drop, 1u);
        if (keys) { keys[f] = (uint32_t)(a > b ? (a > c ? a : c) : (b > c ? b : c)); vals[f] = f; }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_drop) atomicAdd(&hdr[H_COUNT0], s_drop);
}
// the next pass's keys in the order the last pass left: which = 1: b, 0: a of the sorted triple
__global__ void __launch_bounds__(256)
sf_keys(uint32_t NF, const int32_t* __restrict__ out_faces, const uint32_t* __restrict__ vals, int which, uint32_t* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= NF) return;
    uint32_t a, b, c;
    sorted_triple(out_faces + 3 * (size_t)vals[i], a, b, c);
    keys[i] = which ? b : a;
}
// an entry with three distinct clusters whose sorted triple equals its predecessor's is a duplicate of a face with a smaller index
__global__ void __launch_bounds__(256)
sf_dedupe(uint32_t NF, const int32_t* __restrict__ out_faces, const uint32_t* __restrict__ vals, uint8_t* __restrict__ face_keep, uint32_t* __restrict__ hdr)
{
    __shared__ uint32_t s_drop;
    if (threadIdx.x == 0) s_drop = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > 0u && i < NF) {
        uint32_t a, b, c, a0, b0, c0;
        const uint32_t f = vals[i];
        sorted_triple(out_faces + 3 * (size_t)f, a, b, c);
        sorted_triple(out_faces + 3 * (size_t)vals[i - 1], a0, b0, c0);
        if (a != b && b != c && a == a0 && b == b0 && c == c0) { face_keep[f] = 0; atomicAdd(&s_drop, 1u); }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_drop) atomicAdd(&hdr[H_COUNT1], s_drop);
}

struct FacesWs { uint32_t* hdr; uint32_t* keys[2]; uint32_t* vals[2]; uint32_t* tmp; };
static size_t faces_layout(int64_t NF, void* base, FacesWs* out)
{
    const size_t nf = (size_t)(NF < 0 ? 0 : NF);
    Carver c{ static_cast<char*>(base), 0 };
    FacesWs w{};
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    for (int k = 0; k < 2; k++) { w.keys[k] = c.take<uint32_t>(nf); w.vals[k] = c.take<uint32_t>(nf); }
    w.tmp = c.take<uint32_t>(rs_tmp_words(nf));
    if (out) *out = w;
    return c.total();
}

static bool bad_faces(int64_t NF) { return NF < 0 || 3 * NF >= ((int64_t)1 << 31); }
static bool bad_grid(const double* origin, double h)
{
    return !origin || !(fabs(origin[0]) <= DBL_MAX && fabs(origin[1]) <= DBL_MAX && fabs(origin[2]) <= DBL_MAX) || !(h > 0.0 && h <= DBL_MAX);
}
static int bits_for(int64_t n)
{
    int bits = 0;
    while (bits < 31 && ((int64_t)1 << bits) < n) bits++;
    return bits;
}

} // namespace meshsimp
} // namespace gof

using namespace gof;
using namespace gof::meshsimp;

extern "C" {

int gof_mesh_simplify_abi_version(void) { return 5; }

void gof_mesh_simplify_tiling(int64_t* out)
{
    size_t scan_tile = 1;
    while (scan_tmp_words(scan_tile + 1) == scan_tmp_words(1)) scan_tile++;
    out[0] = (int64_t)rs_block_items();
    out[1] = (int64_t)scan_tile;
    out[2] = (int64_t)SUM_TILE;
    out[3] = (int64_t)SUM_BLOCK;
}

size_t gof_mesh_cluster_ws_bytes(int64_t NV) { return cluster_layout(bad_count(NV, MESH_MAX_COUNT) ? 0 : NV, nullptr, nullptr); }

int gof_mesh_cluster(int64_t NV, const double* vertices, const double* origin, double h, int32_t* vertex_cluster, int64_t* num_clusters,
                     void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_clusters) { set_error("mesh_cluster: num_clusters is NULL"); return GOF_E_INVALID; }
    *num_clusters = 0;
    if (bad_count(NV, MESH_MAX_COUNT)) { set_error("mesh_cluster: bad number of vertices (%lld)", (long long)NV); return GOF_E_INVALID; }
    if (bad_grid(origin, h)) { set_error("mesh_cluster: the origin must be finite and the cell size finite and above 0"); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_cluster: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_cluster_ws_bytes(NV)) { set_error("mesh_cluster: workspace too small"); return GOF_E_WORKSPACE; }
    if (NV == 0) return GOF_OK;
    if (!vertices) { set_error("mesh_cluster: vertices is NULL"); return GOF_E_INVALID; }
    ClusterWs w;
    cluster_layout(NV, ws_aligned(ws), &w);
    const uint32_t nv = (uint32_t)NV;
    const Grid g{ origin[0], origin[1], origin[2], h };
    uint32_t hd[HDR_WORDS];
    GOF_PROFILE("mesh_cluster", stream);
    // the vertices, before anything is written into an output
    hipLaunchKernelGGL(sm_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(sm_validate_vertices, grid_of(NV), dim3(256), 0, stream, nv, vertices, g, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(hipMemcpyAsync(hd, w.hdr, sizeof(hd), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (hd[H_FINITE]) { set_error("mesh_cluster: a vertex is not finite"); return GOF_E_INVALID; }
    if (hd[H_RANGE]) { set_error("mesh_cluster: a cell coordinate lies outside [0, 2^21): the cell size is too small for the mesh, or the origin is not its corner"); return GOF_E_INVALID; }
    // key, sort, number
    uint32_t* order = nullptr;
    uint32_t sort_failed = 0;
    hipLaunchKernelGGL(sc_keys, grid_of(NV), dim3(256), 0, stream, nv, vertices, g, w.keys, w.s.lo[0], w.s.idx[0]);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(sort_keys63(w.keys, (size_t)nv, w.s, &order, stream));
    const uint32_t* sort_err = radix_sort_error_flag(w.s.tmp, (size_t)nv, 31);
    if (sort_err) GOF_HIP_CHECK(hipMemcpyAsync(&sort_failed, sort_err, 4, hipMemcpyDeviceToHost, stream));      // (read before the scan reuses tmp)
    hipLaunchKernelGGL(sc_heads, grid_of(NV), dim3(256), 0, stream, nv, w.keys, order, w.run);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.run, nullptr, w.run, (size_t)nv, true, w.s.tmp, nullptr, stream));
    uint32_t NC = 0;
    if (vertex_cluster) {
        hipLaunchKernelGGL(sc_firsts, grid_of(NV + 1), dim3(256), 0, stream, nv, order, w.run, w.run_first, w.first);
        GOF_LAUNCH_CHECK(stream, 0);
        GOF_HIP_CHECK(device_scan_u32(w.first, nullptr, w.first, (size_t)nv + 1, false, w.s.tmp, nullptr, stream));
        GOF_HIP_CHECK(hipMemcpyAsync(&NC, w.run + (nv - 1u), 4, hipMemcpyDeviceToHost, stream));
        GOF_HIP_CHECK(hipStreamSynchronize(stream));
        if (sort_failed) { set_error("mesh_cluster: the key sort gave up waiting for a predecessor"); return GOF_E_DEVICE; }
        hipLaunchKernelGGL(sc_number, grid_of(NV), dim3(256), 0, stream, nv, order, w.run, w.run_first, w.first, vertex_cluster);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    else {
        GOF_HIP_CHECK(hipMemcpyAsync(&NC, w.run + (nv - 1u), 4, hipMemcpyDeviceToHost, stream));
        GOF_HIP_CHECK(hipStreamSynchronize(stream));
        if (sort_failed) { set_error("mesh_cluster: the key sort gave up waiting for a predecessor"); return GOF_E_DEVICE; }
    }
    *num_clusters = (int64_t)NC;
    return GOF_OK;
}

size_t gof_mesh_cluster_solve_ws_bytes(int64_t NV, int64_t NF, int64_t NC)
{
    return solve_layout(bad_count(NV, MESH_MAX_COUNT) ? 0 : NV, bad_faces(NF) ? 0 : NF, bad_count(NC) ? 0 : NC, nullptr, nullptr);
}

int gof_mesh_cluster_solve(int64_t NV, int64_t NF, const double* vertices, const int32_t* faces, const uint8_t* colors, const int32_t* vertex_cluster,
                           int64_t NC, const double* origin, double h, double* out_vertices, uint8_t* out_colors, uint8_t* used_mean,
                           int64_t* used_mean_count, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (used_mean_count) *used_mean_count = 0;
    if (bad_count(NV, MESH_MAX_COUNT)) { set_error("mesh_cluster_solve: bad number of vertices (%lld)", (long long)NV); return GOF_E_INVALID; }
    if (bad_faces(NF)) { set_error("mesh_cluster_solve: bad number of faces (%lld): 3 * faces must be below 2^31", (long long)NF); return GOF_E_INVALID; }
    if (bad_count(NC) || NC > NV) { set_error("mesh_cluster_solve: bad number of clusters (%lld for %lld vertices)", (long long)NC, (long long)NV); return GOF_E_INVALID; }
    if (bad_grid(origin, h)) { set_error("mesh_cluster_solve: the origin must be finite and the cell size finite and above 0"); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_cluster_solve: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_cluster_solve_ws_bytes(NV, NF, NC)) { set_error("mesh_cluster_solve: workspace too small"); return GOF_E_WORKSPACE; }
    if (NV == 0 && NF == 0) return GOF_OK;
    if (NV == 0) { set_error("mesh_cluster_solve: %lld faces and no vertex", (long long)NF); return GOF_E_INVALID; }
    if (NC == 0) { set_error("mesh_cluster_solve: %lld vertices and no cluster", (long long)NV); return GOF_E_INVALID; }
    if (!vertices || !vertex_cluster || !out_vertices || !used_mean || (NF && !faces) || ((colors != nullptr) != (out_colors != nullptr))) {
        set_error("mesh_cluster_solve: vertices / faces / vertex_cluster / an output is NULL, or colours on one side only");
        return GOF_E_INVALID;
    }
    SolveWs w;
    solve_layout(NV, NF, NC, ws_aligned(ws), &w);
    const uint32_t nv = (uint32_t)NV, ne = 3u * (uint32_t)NF;
    const Grid g{ origin[0], origin[1], origin[2], h };
    const int bits = bits_for(NC);
    uint32_t hd[HDR_WORDS];
    GOF_PROFILE("mesh_cluster_solve", stream);
    // the input, before anything is read through an index or written into an output
    hipLaunchKernelGGL(sm_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(sm_validate_vertices, grid_of(NV), dim3(256), 0, stream, nv, vertices, g, w.hdr);
    hipLaunchKernelGGL(sm_validate_clusters, grid_of(NV), dim3(256), 0, stream, nv, vertex_cluster, NC, w.hdr);
    if (ne) hipLaunchKernelGGL(sm_validate_faces, grid_of(ne), dim3(256), 0, stream, NV, ne, faces, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(hipMemcpyAsync(hd, w.hdr, sizeof(hd), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (hd[H_INDEX]) { set_error("mesh_cluster_solve: a face index lies outside [0, %lld)", (long long)NV); return GOF_E_INVALID; }
    if (hd[H_FINITE]) { set_error("mesh_cluster_solve: a vertex is not finite"); return GOF_E_INVALID; }
    if (hd[H_RANGE]) { set_error("mesh_cluster_solve: a cell coordinate lies outside [0, 2^21)"); return GOF_E_INVALID; }
    if (hd[H_CLUSTER]) { set_error("mesh_cluster_solve: a cluster number lies outside [0, %lld)", (long long)NC); return GOF_E_INVALID; }
    // the vertices by cluster: centres, counts, sums
    uint32_t *keys = nullptr, *vals = nullptr;
    hipLaunchKernelGGL(sv_vertex_pairs, grid_of(NV), dim3(256), 0, stream, nv, vertex_cluster, w.keys[0], w.vals[0]);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(radix_sort_pairs_u32(w.keys[0], w.vals[0], w.keys[1], w.vals[1], (size_t)nv, bits, w.tmp, &keys, &vals, stream, nullptr));
    if (const uint32_t* err = radix_sort_error_flag(w.tmp, (size_t)nv, bits)) hipLaunchKernelGGL(sm_keep_sort_error, dim3(1), dim3(64), 0, stream, err, w.hdr);
    hipLaunchKernelGGL(ss_starts, grid_of(NV + 1), dim3(256), 0, stream, nv, keys, NC, w.start);
    hipLaunchKernelGGL(sv_centres, grid_of(NC), dim3(256), 0, stream, NC, w.start, vals, vertices, g, w.centre, w.count, w.first);
    segment_sums(nv, keys, VertexItems{ vertices, colors, vals, w.centre }, NC, w.start, w.sv, w.vsum, stream);
    GOF_LAUNCH_CHECK(stream, 0);
    // the corners by cluster: quadrics
    keys = w.keys[0];
    vals = w.vals[0];
    if (ne) {
        hipLaunchKernelGGL(sv_corner_pairs, grid_of(ne), dim3(256), 0, stream, ne, faces, vertex_cluster, w.keys[0], w.vals[0]);
        GOF_LAUNCH_CHECK(stream, 0);
        GOF_HIP_CHECK(radix_sort_pairs_u32(w.keys[0], w.vals[0], w.keys[1], w.vals[1], (size_t)ne, bits, w.tmp, &keys, &vals, stream, nullptr));
        if (const uint32_t* err = radix_sort_error_flag(w.tmp, (size_t)ne, bits)) hipLaunchKernelGGL(sm_keep_sort_error, dim3(1), dim3(64), 0, stream, err, w.hdr);
    }
    hipLaunchKernelGGL(ss_starts, grid_of((int64_t)ne + 1), dim3(256), 0, stream, ne, keys, NC, w.start);
    segment_sums(ne, keys, CornerItems{ vertices, faces, vals, w.centre }, NC, w.start, w.sq, w.quad, stream);
    hipLaunchKernelGGL(sv_solve, grid_of(NC), dim3(256), 0, stream, NC, w.count, w.first, vertices, w.centre, w.vsum, w.quad, h, out_vertices, out_colors, used_mean, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(hipMemcpyAsync(hd, w.hdr, sizeof(hd), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (hd[H_SORT]) { set_error("mesh_cluster_solve: a sort gave up waiting for a predecessor"); return GOF_E_DEVICE; }
    if (used_mean_count) *used_mean_count = (int64_t)hd[H_COUNT0];
    return GOF_OK;
}

size_t gof_mesh_cluster_faces_ws_bytes(int64_t NF) { return faces_layout(bad_faces(NF) ? 0 : NF, nullptr, nullptr); }

int gof_mesh_cluster_faces(int64_t NV, int64_t NF, const int32_t* faces, const int32_t* vertex_cluster, int64_t NC, int32_t dedupe, int32_t* out_faces,
                           uint8_t* face_keep, int64_t* counts, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (counts) counts[0] = counts[1] = 0;
    if (bad_count(NV, MESH_MAX_COUNT)) { set_error("mesh_cluster_faces: bad number of vertices (%lld)", (long long)NV); return GOF_E_INVALID; }
    if (bad_faces(NF)) { set_error("mesh_cluster_faces: bad number of faces (%lld): 3 * faces must be below 2^31", (long long)NF); return GOF_E_INVALID; }
    if (bad_count(NC) || NC > NV) { set_error("mesh_cluster_faces: bad number of clusters (%lld for %lld vertices)", (long long)NC, (long long)NV); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_cluster_faces: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_cluster_faces_ws_bytes(NF)) { set_error("mesh_cluster_faces: workspace too small"); return GOF_E_WORKSPACE; }
    if (NF == 0) return GOF_OK;
    if (!faces || !vertex_cluster || !out_faces || !face_keep) { set_error("mesh_cluster_faces: faces / vertex_cluster / out_faces / face_keep is NULL"); return GOF_E_INVALID; }
    FacesWs w;
    faces_layout(NF, ws_aligned(ws), &w);
    const uint32_t nf = (uint32_t)NF;
    uint32_t hd[HDR_WORDS];
    GOF_PROFILE("mesh_cluster_faces", stream);
    hipLaunchKernelGGL(sm_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(sm_validate_faces, grid_of(3 * NF), dim3(256), 0, stream, NV, 3u * nf, faces, w.hdr);
    if (NV) hipLaunchKernelGGL(sm_validate_clusters, grid_of(NV), dim3(256), 0, stream, (uint32_t)NV, vertex_cluster, NC, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(hipMemcpyAsync(hd, w.hdr, sizeof(hd), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (hd[H_INDEX]) { set_error("mesh_cluster_faces: a face index lies outside [0, %lld)", (long long)NV); return GOF_E_INVALID; }
    if (hd[H_CLUSTER]) { set_error("mesh_cluster_faces: a cluster number lies outside [0, %lld)", (long long)NC); return GOF_E_INVALID; }
    hipLaunchKernelGGL(sf_remap, grid_of(NF), dim3(256), 0, stream, nf, faces, vertex_cluster, out_faces, face_keep, dedupe ? w.keys[0] : (uint32_t*)nullptr,
                       w.vals[0], w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    if (dedupe) {
        const int bits = bits_for(NC);
        int cur = 0;                                             // the pair of buffers the last pass ended in
        for (int pass = 0; pass < 3; pass++) {                   // by c, then b, then a: stable, so equal triples end in ascending face index
            uint32_t *kres = nullptr, *vres = nullptr;
            if (pass) hipLaunchKernelGGL(sf_keys, grid_of(NF), dim3(256), 0, stream, nf, out_faces, w.vals[cur], pass == 1 ? 1 : 0, w.keys[cur]);
            GOF_HIP_CHECK(radix_sort_pairs_u32(w.keys[cur], w.vals[cur], w.keys[1 - cur], w.vals[1 - cur], (size_t)nf, bits, w.tmp, &kres, &vres, stream, nullptr));
            if (const uint32_t* err = radix_sort_error_flag(w.tmp, (size_t)nf, bits)) hipLaunchKernelGGL(sm_keep_sort_error, dim3(1), dim3(64), 0, stream, err, w.hdr);
            cur = vres == w.vals[0] ? 0 : 1;
        }
        hipLaunchKernelGGL(sf_dedupe, grid_of(NF), dim3(256), 0, stream, nf, out_faces, w.vals[cur], face_keep, w.hdr);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    GOF_HIP_CHECK(hipMemcpyAsync(hd, w.hdr, sizeof(hd), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (hd[H_SORT]) { set_error("mesh_cluster_faces: a sort gave up waiting for a predecessor"); return GOF_E_DEVICE; }
    if (counts) { counts[0] = (int64_t)hd[H_COUNT0]; counts[1] = (int64_t)hd[H_COUNT1]; }
    return GOF_OK;
}

} // extern "C"
