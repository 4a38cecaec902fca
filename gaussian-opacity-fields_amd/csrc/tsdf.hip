// tsdf.hip -- TSDF fusion of rendered depth / colour into a sparse volume of voxel blocks, and its marching-cubes mesh (replaces the
// Open3D VoxelBlockGrid of the reference's extract_mesh_tsdf.py).  The contract is DESIGN.md "TSDF fusion"; the float64 restatement
// the tests hold this file to is tests/tsdf_restatement.py.
//
// Volume: an open-addressing hash table (64-bit packed block key -> storage slot) over block storage of 5 fp32 planes of 16^3
// (tsdf, weight, r, g, b).  Per view:
//   touch:      one thread per pixel walks the blocks its truncation segment passes through (3-D DDA) and inserts their keys into a
//               frame-local hash set (64-bit atomicCAS on the key alone); the set is compacted with device_scan_u32 (radix.hip), and
//               the frame's keys the volume does not hold are counted -- the one read-back of a view;
//   activate:   one thread per frame key finds or inserts it in the volume's table; the thread that inserts a key takes a storage
//               slot (atomicAdd) and stores it.  The keys of one launch are unique, so no thread reads a value another thread of the
//               same launch wrote: values are read by later launches only (workgroups do not see each other's stores in-launch);
//   integrate:  one workgroup per frame block, 256 threads x 16 voxels, plane by plane so that every read-modify-write is coalesced;
//               each voxel has exactly one writer per frame.
// Mesh:  active keys sorted (radix.h's sort_keys63); a cube pass flags the edges emitted cubes use at
//        their owner voxel (atomicOr; read by the next launch); per-block vertex / triangle counts and their scans (the two totals
//        are the extraction's read-back); then the vertex and the triangle writes, a triangle finding its vertices through a per-voxel
//        index map.  Scratch is indexed by storage slot, the output ordered by key.
#include "gof_common.h"
#include "radix.h"
#include "gof_geom.h"
#include "../../include/gof_tsdf_hip.h"
#include "tsdf_tables.h"

namespace gof {

constexpr int TR = 16;                       // block resolution
constexpr int TR3 = TR * TR * TR;
constexpr size_t TBLOCK = 5 * (size_t)TR3;   // floats per block
constexpr uint64_t TK_EMPTY = ~0ull;
constexpr int32_t TK_BIAS = 1 << 20;         // block coordinates in [-2^20, 2^20), 21 bits each
constexpr uint32_t TSET_PROBES = 256;        // longest probe run of the frame set before the frame is redone with a larger one
constexpr uint32_t TSLOT_NONE = 0xFFFFFFFFu;

// cube corner offsets and the edges' owner voxel offset + axis (Lorensen-Cline / Bourke numbering, tsdf_tables.h)
__constant__ int8_t TSDF_CORNER[8][3] = { {0,0,0},{1,0,0},{1,1,0},{0,1,0},{0,0,1},{1,0,1},{1,1,1},{0,1,1} };
__constant__ int8_t TSDF_EDGE_OWNER[12][4] = { {0,0,0,0},{1,0,0,1},{0,1,0,0},{0,0,0,1},{0,0,1,0},{1,0,1,1},
                                               {0,1,1,0},{0,0,1,1},{0,0,0,2},{1,0,0,2},{1,1,0,2},{0,1,0,2} };

__device__ __forceinline__ uint64_t tk_hash(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}
__device__ __forceinline__ bool tk_in_range(int x, int y, int z)
{
    return x >= -TK_BIAS && x < TK_BIAS && y >= -TK_BIAS && y < TK_BIAS && z >= -TK_BIAS && z < TK_BIAS;
}
__device__ __forceinline__ uint64_t tk_pack(int x, int y, int z)
{
    return (uint64_t)(uint32_t)(x + TK_BIAS) | ((uint64_t)(uint32_t)(y + TK_BIAS) << 21) | ((uint64_t)(uint32_t)(z + TK_BIAS) << 42);
}
__device__ __forceinline__ void tk_unpack(uint64_t k, int& x, int& y, int& z)
{
    x = (int)(k & 0x1FFFFF) - TK_BIAS;
    y = (int)((k >> 21) & 0x1FFFFF) - TK_BIAS;
    z = (int)((k >> 42) & 0x1FFFFF) - TK_BIAS;
}
// storage slot of `key` in a table written by EARLIER launches, or -1
__device__ __forceinline__ int64_t tk_lookup(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint64_t mask, uint64_t key)
{
    uint64_t s = tk_hash(key) & mask;
    for (uint64_t n = 0; n <= mask; n++, s = (s + 1) & mask) {
        const uint64_t k = keys[s];
        if (k == key) return vals[s];
        if (k == TK_EMPTY) return -1;
    }
    return -1;
}
__device__ __forceinline__ int64_t tk_lookup_xyz(const GofTsdfVolume& vol, int x, int y, int z)
{
    if (!tk_in_range(x, y, z)) return -1;
    return tk_lookup(vol.table_keys, vol.table_vals, (uint64_t)vol.table_capacity - 1, tk_pack(x, y, z));
}

struct TsdfCam { float fx, fy, cx, cy, r[9], t[3]; };
__device__ __forceinline__ TsdfCam load_cam(const float* __restrict__ K, const float* __restrict__ E)
{
    TsdfCam c;
    c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) c.r[3 * i + j] = E[4 * i + j];
        c.t[i] = E[4 * i + 3];
    }
    return c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// touch
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool set_insert(uint64_t* __restrict__ set, uint32_t mask, uint64_t key)
{
    uint32_t s = (uint32_t)tk_hash(key) & mask;
    for (uint32_t n = 0; n < TSET_PROBES && n <= mask; n++, s = (s + 1) & mask) {
        // plain read first: within this launch a slot only goes from empty to its final key, so a stale read is empty
        unsigned long long k = set[s];
        if (k == key) return true;
        if (k == TK_EMPTY) {
            k = atomicCAS((unsigned long long*)&set[s], (unsigned long long)TK_EMPTY, (unsigned long long)key);
            if (k == TK_EMPTY || k == key) return true;
        }
    }
    return false;
}

// cnt: [2] |= 1 when the set overflowed, [3] |= 1 for a block coordinate out of range
__global__ void __launch_bounds__(256)
tsdf_touch(const float* __restrict__ depth, int H, int W, const float* __restrict__ K, const float* __restrict__ E, float depth_scale,
           float depth_max, float trunc, float block_size, uint64_t* __restrict__ set, uint32_t set_mask, uint32_t* __restrict__ cnt)
{
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)H * W) return;
    const float d = depth[pix] / depth_scale;
    if (!(d > 0.f && d <= depth_max)) return;
    const int u = (int)(pix % W), v = (int)(pix / W);
    const TsdfCam c = load_cam(K, E);
    const float dcx = ((float)u - c.cx) / c.fx, dcy = ((float)v - c.cy) / c.fy;
    const float t0 = fmaxf(d - trunc, 0.f), t1 = fminf(d + trunc, depth_max);
    float p0[3], p1[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float dw = c.r[i] * dcx + c.r[3 + i] * dcy + c.r[6 + i];           // R^T (dcx, dcy, 1)
        const float C = -(c.r[i] * c.t[0] + c.r[3 + i] * c.t[1] + c.r[6 + i] * c.t[2]);
        p0[i] = (C + t0 * dw) / block_size;
        p1[i] = (C + t1 * dw) / block_size;
    }
    int cell[3], rem[3], step[3];
    float tmax[3], tdel[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float lim = (float)TK_BIAS;
        if (!(p0[i] >= -lim && p0[i] < lim && p1[i] >= -lim && p1[i] < lim)) { atomicOr(&cnt[3], 1u); return; }
        cell[i] = (int)floorf(p0[i]);
        const int e = (int)floorf(p1[i]);
        step[i] = e > cell[i] ? 1 : -1;
        rem[i] = e > cell[i] ? e - cell[i] : cell[i] - e;
        const float dd = p1[i] - p0[i];
        tmax[i] = rem[i] ? ((float)(cell[i] + (step[i] > 0 ? 1 : 0)) - p0[i]) / dd : INFINITY;
        tdel[i] = rem[i] ? 1.f / fabsf(dd) : INFINITY;
    }
    if (!set_insert(set, set_mask, tk_pack(cell[0], cell[1], cell[2]))) { atomicOr(&cnt[2], 1u); return; }
    for (int n = rem[0] + rem[1] + rem[2]; n > 0; n--) {
        int a = -1;
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (rem[i] && (a < 0 || tmax[i] < tmax[a])) a = i;
        cell[a] += step[a];
        rem[a]--;
        tmax[a] += tdel[a];
        if (!set_insert(set, set_mask, tk_pack(cell[0], cell[1], cell[2]))) { atomicOr(&cnt[2], 1u); return; }
    }
}

__global__ void __launch_bounds__(256)
tsdf_set_flags(const uint64_t* __restrict__ set, uint32_t S, uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i <= S) flags[i] = (i < S && set[i] != TK_EMPTY) ? 1u : 0u;
}

// pos: exclusive scan of the flags.  cnt[0] = frame blocks, [1] = new ones; [4], [5] = the volume's counter words 0, 1
__global__ void __launch_bounds__(256)
tsdf_compact(const uint64_t* __restrict__ set, uint32_t S, const uint32_t* __restrict__ pos, GofTsdfVolume vol,
             uint64_t* __restrict__ fkeys, uint32_t* __restrict__ cnt)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == S) { cnt[0] = pos[S]; cnt[4] = vol.counter[0]; cnt[5] = vol.counter[1]; }
    if (i >= S) return;
    const uint64_t key = set[i];
    if (key == TK_EMPTY) return;
    fkeys[pos[i]] = key;
    if (tk_lookup(vol.table_keys, vol.table_vals, (uint64_t)vol.table_capacity - 1, key) < 0) atomicAdd(&cnt[1], 1u);
}

// ---------------------------------------------------------------------------------------------------------------------------
// activate + integrate
// ---------------------------------------------------------------------------------------------------------------------------
// insert `key` (unique in this launch) with a fresh storage slot, or find the slot an earlier launch gave it
__device__ __forceinline__ uint32_t table_find_or_insert(const GofTsdfVolume& vol, uint64_t key, bool take_slot, uint32_t given)
{
    const uint64_t mask = (uint64_t)vol.table_capacity - 1;
    uint64_t s = tk_hash(key) & mask;
    for (uint64_t n = 0; n <= mask; n++, s = (s + 1) & mask) {
        unsigned long long k = vol.table_keys[s];
        if (k == key) return vol.table_vals[s];
        if (k == TK_EMPTY) {
            k = atomicCAS((unsigned long long*)&vol.table_keys[s], (unsigned long long)TK_EMPTY, (unsigned long long)key);
            if (k == TK_EMPTY) {
                const uint32_t slot = take_slot ? atomicAdd(&vol.counter[0], 1u) : given;
                if (slot >= (uint64_t)vol.block_capacity) { atomicOr(&vol.counter[1], 1u); return TSLOT_NONE; }
                vol.table_vals[s] = slot;
                if (take_slot) vol.block_keys[slot] = key;
                return slot;
            }
            if (k == key) { atomicOr(&vol.counter[1], 2u); return TSLOT_NONE; }    // a duplicate key in one launch: never by construction
        }
    }
    atomicOr(&vol.counter[1], 4u);
    return TSLOT_NONE;
}

__global__ void __launch_bounds__(256)
tsdf_activate(GofTsdfVolume vol, uint32_t nf, const uint64_t* __restrict__ fkeys, uint32_t* __restrict__ fslots)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < nf) fslots[i] = table_find_or_insert(vol, fkeys[i], true, 0);
}

__global__ void __launch_bounds__(256)
tsdf_rehash(GofTsdfVolume vol, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) table_find_or_insert(vol, vol.block_keys[i], false, i);
}

__global__ void tsdf_set_counter(uint32_t* counter, uint32_t n)
{
    if (threadIdx.x < 4) counter[threadIdx.x] = threadIdx.x == 0 ? n : 0u;
}

__global__ void __launch_bounds__(256)
tsdf_integrate(GofTsdfVolume vol, const uint64_t* __restrict__ fkeys, const uint32_t* __restrict__ fslots, const float* __restrict__ depth,
               const float* __restrict__ color, int H, int W, const float* __restrict__ K, const float* __restrict__ E, float depth_scale,
               float depth_max)
{
    const uint32_t slot = fslots[blockIdx.x];
    if (slot == TSLOT_NONE) return;
    int bx, by, bz;
    tk_unpack(fkeys[blockIdx.x], bx, by, bz);
    const TsdfCam c = load_cam(K, E);
    const float v = vol.voxel_size, trunc = vol.trunc;
    const size_t HW = (size_t)H * W;
    float* __restrict__ base = vol.block_data + (size_t)slot * TBLOCK;
#pragma unroll 4
    for (int j = 0; j < TR3 / 256; j++) {
        const int l = threadIdx.x + 256 * j;
        const float px = v * (float)(bx * TR + (l & 15)), py = v * (float)(by * TR + ((l >> 4) & 15)), pz = v * (float)(bz * TR + (l >> 8));
        const float xc = c.r[0] * px + c.r[1] * py + c.r[2] * pz + c.t[0];
        const float yc = c.r[3] * px + c.r[4] * py + c.r[5] * pz + c.t[1];
        const float zc = c.r[6] * px + c.r[7] * py + c.r[8] * pz + c.t[2];
        if (!(zc > 0.f)) continue;
        const float u = c.fx * xc / zc + c.cx, vv = c.fy * yc / zc + c.cy;
        if (!(u >= 0.f && u <= (float)(W - 1) && vv >= 0.f && vv <= (float)(H - 1))) continue;
        const size_t pix = (size_t)(int)vv * W + (size_t)(int)u;           // truncation (both are >= 0)
        const float d = depth[pix] / depth_scale;
        if (!(d > 0.f && d <= depth_max)) continue;
        const float sdf = d - zc;
        if (sdf < -trunc) continue;
        const float s = fminf(sdf, trunc) / trunc;
        const float w = base[TR3 + l], w1 = w + 1.f;
        base[l] = (w * base[l] + s) / w1;
        base[TR3 + l] = w1;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) base[(2 + ch) * TR3 + l] = (w * base[(2 + ch) * TR3 + l] + color[ch * HW + pix]) / w1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// extraction
// ---------------------------------------------------------------------------------------------------------------------------
// slots of the blocks at offsets {lo..1}^3 of the workgroup's block (-1 = not active), threads [0, (2-lo)^3)
template <int LO>
__device__ __forceinline__ void load_neighbours(const GofTsdfVolume& vol, uint32_t slot, int* __restrict__ s_nb)
{
    constexpr int D = 2 - LO;
    if (threadIdx.x < D * D * D) {
        int bx, by, bz;
        tk_unpack(vol.block_keys[slot], bx, by, bz);
        const int t = threadIdx.x;
        const int dx = t % D + LO, dy = (t / D) % D + LO, dz = t / (D * D) + LO;
        s_nb[t] = (dx | dy | dz) == 0 ? (int)slot : (int)tk_lookup_xyz(vol, bx + dx, by + dy, bz + dz);
    }
    __syncthreads();
}
// (X, Y, Z) in [LO*16, 32) voxel coordinates relative to the block -> index into the neighbour slots and the voxel's linear index
template <int LO>
__device__ __forceinline__ int nb_slot(const int* __restrict__ s_nb, int X, int Y, int Z, int& lin)
{
    constexpr int D = 2 - LO;
    lin = (X & 15) + TR * (Y & 15) + TR * TR * (Z & 15);
    return s_nb[((X >> 4) - LO) + D * ((Y >> 4) - LO) + D * D * ((Z >> 4) - LO)];
}

__global__ void __launch_bounds__(256)
tsdf_cubes(GofTsdfVolume vol, const uint32_t* __restrict__ order, float tau, uint32_t* __restrict__ flags, uint8_t* __restrict__ cases)
{
    __shared__ int s_nb[8];
    const uint32_t slot = order[blockIdx.x];
    load_neighbours<0>(vol, slot, s_nb);
    const float* __restrict__ data = vol.block_data;
    for (int j = 0; j < TR3 / 256; j++) {
        const int l = threadIdx.x + 256 * j;
        const int x = l & 15, y = (l >> 4) & 15, z = l >> 8;
        int cs = 0;
        bool ok = true;
        for (int q = 0; q < 8 && ok; q++) {
            int lin;
            const int s = nb_slot<0>(s_nb, x + TSDF_CORNER[q][0], y + TSDF_CORNER[q][1], z + TSDF_CORNER[q][2], lin);
            if (s < 0) { ok = false; break; }
            const float* b = data + (size_t)s * TBLOCK;
            if (!(b[TR3 + lin] >= tau)) { ok = false; break; }
            cs |= (b[lin] < 0.f ? 1 : 0) << q;
        }
        if (!ok || TSDF_MC_NTRI[cs] == 0) { cases[(size_t)slot * TR3 + l] = 0; continue; }
        cases[(size_t)slot * TR3 + l] = (uint8_t)cs;
        const uint32_t em = TSDF_MC_EDGES[cs];
        for (int e = 0; e < 12; e++) {
            if (!((em >> e) & 1)) continue;
            int lin;
            const int s = nb_slot<0>(s_nb, x + TSDF_EDGE_OWNER[e][0], y + TSDF_EDGE_OWNER[e][1], z + TSDF_EDGE_OWNER[e][2], lin);
            atomicOr(&flags[(size_t)s * TR3 + lin], 1u << TSDF_EDGE_OWNER[e][3]);
        }
    }
}

__device__ __forceinline__ uint32_t block_sum_256(uint32_t v, uint32_t* __restrict__ s)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    const uint32_t r = s[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ uint32_t block_exclusive_256(uint32_t v, uint32_t* __restrict__ s)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t a = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0u;
        __syncthreads();
        s[threadIdx.x] += a;
        __syncthreads();
    }
    const uint32_t r = s[threadIdx.x] - v;
    __syncthreads();
    return r;
}

// per block (key order): vertices and triangles; entry n of both stays 0 so that their exclusive scans end with the totals
__global__ void __launch_bounds__(256)
tsdf_counts(const uint32_t* __restrict__ order, uint32_t n, const uint32_t* __restrict__ flags, const uint8_t* __restrict__ cases,
            uint32_t* __restrict__ bv, uint32_t* __restrict__ bt)
{
    __shared__ uint32_t s_red[256];
    const uint32_t slot = order[blockIdx.x];
    uint32_t nv = 0, nt = 0;
    for (int j = 0; j < TR3 / 256; j++) {
        const size_t l = (size_t)slot * TR3 + threadIdx.x + 256 * j;
        nv += __popc(flags[l] & 7u);
        nt += TSDF_MC_NTRI[cases[l]];
    }
    nv = block_sum_256(nv, s_red);
    nt = block_sum_256(nt, s_red);
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = nv;
        bt[blockIdx.x] = nt;
        if (blockIdx.x == 0) { bv[n] = 0; bt[n] = 0; }
    }
}

// value of `plane` at voxel (X, Y, Z) relative to the block, X.. in [-1, 32); false where the voxel's block is not active
__device__ __forceinline__ bool voxel_at(const float* __restrict__ data, const int* __restrict__ s_nb, int X, int Y, int Z, int plane, float& out)
{
    int lin;
    const int s = nb_slot<-1>(s_nb, X, Y, Z, lin);
    if (s < 0) return false;
    out = data[(size_t)s * TBLOCK + (size_t)plane * TR3 + lin];
    return true;
}
__device__ __forceinline__ void tsdf_gradient(const float* __restrict__ data, const int* __restrict__ s_nb, int X, int Y, int Z, float t0, float g[3])
{
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float tp = 0.f, tm = 0.f;
        const bool p = voxel_at(data, s_nb, X + (a == 0), Y + (a == 1), Z + (a == 2), 0, tp);
        const bool m = voxel_at(data, s_nb, X - (a == 0), Y - (a == 1), Z - (a == 2), 0, tm);
        g[a] = (p && m) ? 0.5f * (tp - tm) : p ? tp - t0 : m ? t0 - tm : 0.f;
    }
}

// thread t owns voxels [16 t, 16 t + 16) of the block: vertices in (voxel linear index, axis) order
__global__ void __launch_bounds__(256)
tsdf_vertices(GofTsdfVolume vol, const uint32_t* __restrict__ order, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ bv,
              uint32_t V, int32_t* __restrict__ vmap, float* __restrict__ verts, float* __restrict__ colors, float* __restrict__ normals)
{
    __shared__ int s_nb[27];
    __shared__ uint32_t s_scan[256];
    const uint32_t slot = order[blockIdx.x];
    load_neighbours<-1>(vol, slot, s_nb);
    const float* __restrict__ data = vol.block_data;
    const uint32_t* __restrict__ fl = flags + (size_t)slot * TR3 + 16 * threadIdx.x;
    uint32_t mine = 0;
    for (int j = 0; j < 16; j++) mine += __popc(fl[j] & 7u);
    uint32_t g = bv[blockIdx.x] + block_exclusive_256(mine, s_scan);
    int bx, by, bz;
    tk_unpack(vol.block_keys[slot], bx, by, bz);
    const float v = vol.voxel_size;
    for (int j = 0; j < 16; j++) {
        const uint32_t f = fl[j] & 7u;
        if (!f) continue;
        const int l = 16 * threadIdx.x + j;
        const int x = l & 15, y = (l >> 4) & 15, z = l >> 8;
        float ta, ga[3];
        voxel_at(data, s_nb, x, y, z, 0, ta);
        tsdf_gradient(data, s_nb, x, y, z, ta, ga);
        for (int a = 0; a < 3; a++) {
            if (!((f >> a) & 1)) continue;
            const int X = x + (a == 0), Y = y + (a == 1), Z = z + (a == 2);
            float tb = 0.f, gb[3];
            voxel_at(data, s_nb, X, Y, Z, 0, tb);
            tsdf_gradient(data, s_nb, X, Y, Z, tb, gb);
            const float r = ta / (ta - tb);
            if (g < V) {
                float p[3] = { v * (float)(bx * TR + x), v * (float)(by * TR + y), v * (float)(bz * TR + z) };
                p[a] = p[a] + r * v;
                float n[3], nn = 0.f;
                for (int k = 0; k < 3; k++) {
                    float ca = 0.f, cb = 0.f;
                    voxel_at(data, s_nb, x, y, z, 2 + k, ca);
                    voxel_at(data, s_nb, X, Y, Z, 2 + k, cb);
                    verts[3 * (size_t)g + k] = p[k];
                    colors[3 * (size_t)g + k] = ca + r * (cb - ca);
                    n[k] = (1.f - r) * ga[k] + r * gb[k];
                    nn += n[k] * n[k];
                }
                nn = sqrtf(nn);
                for (int k = 0; k < 3; k++) normals[3 * (size_t)g + k] = nn > 0.f ? n[k] / nn : 0.f;
            }
            vmap[((size_t)slot * TR3 + l) * 3 + a] = (int32_t)g;
            g++;
        }
    }
}

__global__ void __launch_bounds__(256)
tsdf_triangles(GofTsdfVolume vol, const uint32_t* __restrict__ order, const uint8_t* __restrict__ cases, const uint32_t* __restrict__ bt,
               uint32_t F, const int32_t* __restrict__ vmap, int32_t* __restrict__ tris)
{
    __shared__ int s_nb[8];
    __shared__ uint32_t s_scan[256];
    const uint32_t slot = order[blockIdx.x];
    load_neighbours<0>(vol, slot, s_nb);
    const uint8_t* __restrict__ cs = cases + (size_t)slot * TR3 + 16 * threadIdx.x;
    uint32_t mine = 0;
    for (int j = 0; j < 16; j++) mine += TSDF_MC_NTRI[cs[j]];
    uint32_t g = bt[blockIdx.x] + block_exclusive_256(mine, s_scan);
    for (int j = 0; j < 16; j++) {
        const int c = cs[j];
        const int nt = TSDF_MC_NTRI[c];
        if (!nt) continue;
        const int l = 16 * threadIdx.x + j;
        const int x = l & 15, y = (l >> 4) & 15, z = l >> 8;
        for (int t = 0; t < nt; t++, g++) {
            if (g >= F) continue;
            for (int k = 0; k < 3; k++) {
                const int e = TSDF_MC_TRI[c][3 * t + k];
                int lin;
                const int s = nb_slot<0>(s_nb, x + TSDF_EDGE_OWNER[e][0], y + TSDF_EDGE_OWNER[e][1], z + TSDF_EDGE_OWNER[e][2], lin);
                tris[3 * (size_t)g + k] = vmap[((size_t)s * TR3 + lin) * 3 + TSDF_EDGE_OWNER[e][3]];
            }
        }
    }
}

__global__ void __launch_bounds__(256)
tsdf_decode(const uint64_t* __restrict__ bkeys, uint32_t n, int32_t* __restrict__ coords)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x, y, z;
    tk_unpack(bkeys[i], x, y, z);
    coords[3 * (size_t)i] = x; coords[3 * (size_t)i + 1] = y; coords[3 * (size_t)i + 2] = z;
}

// ---------------------------------------------------------------------------------------------------------------------------
// workspaces
// ---------------------------------------------------------------------------------------------------------------------------
// (both layouts end at the last array's unpadded end, c.off, not at Carver::total(): the sizes the ABI has always reported)
struct FrameWs {
    uint64_t* set;       // [S] frame hash set
    uint32_t* pos;       // [S+1] flags -> their exclusive scan
    uint32_t* tmp;       // scan scratch
    uint64_t* fkeys;     // [S] compacted frame keys
    uint32_t* fslots;    // [S] their storage slots
    uint32_t* cnt;       // [8] see tsdf_touch / tsdf_compact
};
static size_t frame_layout(int64_t S, void* base, FrameWs* w)
{
    FrameWs tmp;
    FrameWs& o = w ? *w : tmp;
    Carver c{ static_cast<char*>(base), 0 };
    const size_t n = (size_t)S;
    o.set = c.take<uint64_t>(n);
    o.pos = c.take<uint32_t>(n + 1);
    o.tmp = c.take<uint32_t>(scan_tmp_words(n + 1));
    o.fkeys = c.take<uint64_t>(n);
    o.fslots = c.take<uint32_t>(n);
    o.cnt = c.take<uint32_t>(8);
    return c.off + ALIGN;
}

struct ExtractWs {
    Sort63Ws s;                         // sort buffers
    uint32_t* order;                    // [n] storage slot of every block in key order
    uint32_t* flags;                    // [n * 4096] used edges (bit = axis) at their owner voxel
    uint8_t* cases;                     // [n * 4096] cube case of emitting cubes, else 0
    int32_t* vmap;                      // [n * 4096 * 3] vertex index per voxel and axis
    uint32_t *bv, *bt;                  // [n + 1] per-block counts -> exclusive scans
    uint32_t* scan_tmp;
};
static size_t extract_layout(int64_t nb, void* base, ExtractWs* w)
{
    ExtractWs tmp;
    ExtractWs& o = w ? *w : tmp;
    Carver c{ static_cast<char*>(base), 0 };
    const size_t n = (size_t)nb;
    sort63_carve(c, n, o.s);
    o.order = c.take<uint32_t>(n);
    o.s.tmp = c.take<uint32_t>(rs_tmp_words(n));
    o.flags = c.take<uint32_t>(n * TR3);
    o.cases = c.take<uint8_t>(n * TR3);
    o.vmap = c.take<int32_t>(n * TR3 * 3);
    o.bv = c.take<uint32_t>(n + 1);
    o.bt = c.take<uint32_t>(n + 1);
    o.scan_tmp = c.take<uint32_t>(scan_tmp_words(n + 1));
    return c.off + ALIGN;
}

static int check_volume(const GofTsdfVolume* vol)
{
    if (!vol) { set_error("tsdf: volume is NULL"); return GOF_E_INVALID; }
    if (vol->block_resolution != TR) { set_error("tsdf: block_resolution must be 16 (got %d)", (int)vol->block_resolution); return GOF_E_INVALID; }
    if (!(vol->voxel_size > 0.f) || !(vol->trunc > 0.f)) { set_error("tsdf: voxel_size and trunc must be > 0"); return GOF_E_INVALID; }
    const int64_t tc = vol->table_capacity, bc = vol->block_capacity;
    if (bc < 1 || bc >= (1ll << 31) || tc < 2 * bc || (tc & (tc - 1)) != 0) {
        set_error("tsdf: table capacity %lld must be a power of two >= 2 * block capacity %lld (< 2^31)", (long long)tc, (long long)bc);
        return GOF_E_INVALID;
    }
    if (!vol->table_keys || !vol->table_vals || !vol->block_keys || !vol->block_data || !vol->counter) { set_error("tsdf: NULL volume buffer"); return GOF_E_INVALID; }
    return GOF_OK;
}

static int check_frame(int32_t H, int32_t W, const float* depth, const float* K, const float* E, int64_t S, const void* ws, size_t ws_bytes)
{
    if (H <= 0 || W <= 0 || !depth || !K || !E) { set_error("tsdf: bad image size or NULL depth / camera"); return GOF_E_INVALID; }
    if (S < 64 || S > (1ll << 30) || (S & (S - 1)) != 0) { set_error("tsdf: set capacity %lld must be a power of two in [64, 2^30]", (long long)S); return GOF_E_INVALID; }
    if (!ws || ws_bytes < gof_tsdf_frame_ws_bytes(S)) { set_error("tsdf: frame workspace too small"); return GOF_E_WORKSPACE; }
    return GOF_OK;
}

} // namespace gof

using namespace gof;

extern "C" {

size_t gof_tsdf_frame_ws_bytes(int64_t set_capacity) { return frame_layout(set_capacity < 0 ? 0 : set_capacity, nullptr, nullptr) + ALIGN; }
size_t gof_tsdf_extract_ws_bytes(int64_t num_blocks) { return extract_layout(num_blocks < 0 ? 0 : num_blocks, nullptr, nullptr) + ALIGN; }

int gof_tsdf_grow(const GofTsdfVolume* dst, const GofTsdfVolume* src, int64_t n, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = check_volume(dst)) return e;
    if (src) { if (int e = check_volume(src)) return e; }
    if (n < 0 || n > dst->block_capacity || (src ? n > src->block_capacity : n != 0)) { set_error("tsdf: %lld blocks do not fit", (long long)n); return GOF_E_INVALID; }
    GOF_HIP_CHECK(hipMemsetAsync(dst->table_keys, 0xFF, (size_t)dst->table_capacity * sizeof(uint64_t), stream));
    if (n > 0) {
        GOF_HIP_CHECK(hipMemcpyAsync(dst->block_keys, src->block_keys, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
        GOF_HIP_CHECK(hipMemcpyAsync(dst->block_data, src->block_data, (size_t)n * TBLOCK * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    GOF_HIP_CHECK(hipMemsetAsync(dst->block_data + (size_t)n * TBLOCK, 0, (size_t)(dst->block_capacity - n) * TBLOCK * sizeof(float), stream));
    hipLaunchKernelGGL(tsdf_set_counter, dim3(1), dim3(64), 0, stream, dst->counter, (uint32_t)n);
    GOF_LAUNCH_CHECK(stream, 0);
    if (n > 0) {
        hipLaunchKernelGGL(tsdf_rehash, grid_of(n), dim3(256), 0, stream, *dst, (uint32_t)n);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    return GOF_OK;
}

int gof_tsdf_touch(const GofTsdfVolume* vol, const float* depth, int32_t H, int32_t W, const float* K, const float* E, float depth_scale,
                   float depth_max, void* frame_ws, size_t frame_ws_bytes, int64_t S, int64_t* num_frame_blocks, int64_t* num_new_blocks,
                   void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_frame_blocks || !num_new_blocks) { set_error("tsdf: output pointers are NULL"); return GOF_E_INVALID; }
    *num_frame_blocks = 0; *num_new_blocks = 0;
    if (int e = check_volume(vol)) return e;
    if (int e = check_frame(H, W, depth, K, E, S, frame_ws, frame_ws_bytes)) return e;
    if (!(depth_scale > 0.f)) { set_error("tsdf: depth_scale must be > 0"); return GOF_E_INVALID; }
    FrameWs w;
    frame_layout(S, ws_aligned(frame_ws), &w);
    GOF_HIP_CHECK(hipMemsetAsync(w.set, 0xFF, (size_t)S * sizeof(uint64_t), stream));
    GOF_HIP_CHECK(hipMemsetAsync(w.cnt, 0, 8 * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(tsdf_touch, grid_of((int64_t)H * W), dim3(256), 0, stream, depth, (int)H, (int)W, K, E, depth_scale, depth_max,
                       vol->trunc, vol->voxel_size * TR, w.set, (uint32_t)(S - 1), w.cnt);
    GOF_LAUNCH_CHECK(stream, 0);
    hipLaunchKernelGGL(tsdf_set_flags, grid_of(S + 1), dim3(256), 0, stream, w.set, (uint32_t)S, w.pos);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.pos, nullptr, w.pos, (size_t)S + 1, false, w.tmp, nullptr, stream));
    hipLaunchKernelGGL(tsdf_compact, grid_of(S + 1), dim3(256), 0, stream, w.set, (uint32_t)S, w.pos, *vol, w.fkeys, w.cnt);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t cnt[8];
    GOF_HIP_CHECK(hipMemcpyAsync(cnt, w.cnt, sizeof(cnt), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (cnt[5]) { set_error("tsdf: the volume's table or storage was inconsistent in an earlier integrate (flags 0x%x)", cnt[5]); return GOF_E_DEVICE; }
    if (cnt[3]) { set_error("tsdf: a block coordinate lies outside [-2^20, 2^20)"); return GOF_E_INVALID; }
    if (cnt[2]) { set_error("tsdf: the frame needs more than %lld block-set slots", (long long)S); return GOF_E_CAPACITY; }
    *num_frame_blocks = cnt[0];
    *num_new_blocks = cnt[1];
    return GOF_OK;
}

int gof_tsdf_integrate(const GofTsdfVolume* vol, int64_t num_blocks, const float* depth, const float* color, int32_t H, int32_t W,
                       const float* K, const float* E, float depth_scale, float depth_max, void* frame_ws, size_t frame_ws_bytes,
                       int64_t S, int64_t nf, int64_t nn, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = check_volume(vol)) return e;
    if (int e = check_frame(H, W, depth, K, E, S, frame_ws, frame_ws_bytes)) return e;
    if (!color) { set_error("tsdf: colour is NULL"); return GOF_E_INVALID; }
    if (nf < 0 || nf > S || nn < 0 || nn > nf || num_blocks < 0) { set_error("tsdf: bad frame counts"); return GOF_E_INVALID; }
    if (num_blocks + nn > vol->block_capacity) {
        set_error("tsdf: %lld + %lld blocks exceed the block capacity %lld (gof_tsdf_grow first)", (long long)num_blocks, (long long)nn, (long long)vol->block_capacity);
        return GOF_E_CAPACITY;
    }
    if (nf == 0) return GOF_OK;
    FrameWs w;
    frame_layout(S, ws_aligned(frame_ws), &w);
    hipLaunchKernelGGL(tsdf_activate, grid_of(nf), dim3(256), 0, stream, *vol, (uint32_t)nf, w.fkeys, w.fslots);
    GOF_LAUNCH_CHECK(stream, 0);
    hipLaunchKernelGGL(tsdf_integrate, dim3((unsigned)nf), dim3(256), 0, stream, *vol, w.fkeys, w.fslots, depth, color, (int)H, (int)W, K, E,
                       depth_scale, depth_max);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_tsdf_extract_count(const GofTsdfVolume* vol, int64_t n, float tau, void* ws, size_t ws_bytes, int64_t* num_vertices,
                           int64_t* num_triangles, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_vertices || !num_triangles) { set_error("tsdf: output pointers are NULL"); return GOF_E_INVALID; }
    *num_vertices = 0; *num_triangles = 0;
    if (int e = check_volume(vol)) return e;
    if (n < 0 || n > vol->block_capacity) { set_error("tsdf: bad block count"); return GOF_E_INVALID; }
    if (n == 0) return GOF_OK;
    if (!ws || ws_bytes < gof_tsdf_extract_ws_bytes(n)) { set_error("tsdf: extraction workspace too small"); return GOF_E_WORKSPACE; }
    ExtractWs w;
    extract_layout(n, ws_aligned(ws), &w);
    // ascending 63-bit key (tk_pack leaves bit 63 clear)
    const u64* keys = reinterpret_cast<const u64*>(vol->block_keys);
    uint32_t* sorted = nullptr;
    GOF_HIP_CHECK(sort63_keys_lo(keys, (size_t)n, w.s, stream));
    GOF_HIP_CHECK(sort_keys63(keys, (size_t)n, w.s, &sorted, stream));
    GOF_HIP_CHECK(hipMemcpyAsync(w.order, sorted, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    GOF_HIP_CHECK(hipMemsetAsync(w.flags, 0, (size_t)n * TR3 * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(tsdf_cubes, dim3((unsigned)n), dim3(256), 0, stream, *vol, w.order, tau, w.flags, w.cases);
    GOF_LAUNCH_CHECK(stream, 0);
    hipLaunchKernelGGL(tsdf_counts, dim3((unsigned)n), dim3(256), 0, stream, w.order, (uint32_t)n, w.flags, w.cases, w.bv, w.bt);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.bv, nullptr, w.bv, (size_t)n + 1, false, w.scan_tmp, nullptr, stream));
    GOF_HIP_CHECK(device_scan_u32(w.bt, nullptr, w.bt, (size_t)n + 1, false, w.scan_tmp, nullptr, stream));
    uint32_t tot[2], vc[2];
    GOF_HIP_CHECK(hipMemcpyAsync(&tot[0], w.bv + n, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipMemcpyAsync(&tot[1], w.bt + n, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipMemcpyAsync(vc, vol->counter, sizeof(vc), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    // the volume's own slot count and error flags (an integrate given a wrong num_blocks, or a table that ran out of slots): a mesh
    // extracted from such a volume would read blocks nobody wrote
    if (vc[1]) { set_error("tsdf: the volume's table or storage was inconsistent in an earlier integrate (flags 0x%x)", vc[1]); return GOF_E_DEVICE; }
    if ((int64_t)vc[0] != n) { set_error("tsdf: num_blocks %lld differs from the volume's %u active blocks", (long long)n, vc[0]); return GOF_E_INVALID; }
    *num_vertices = tot[0];
    *num_triangles = tot[1];
    return GOF_OK;
}

int gof_tsdf_extract_emit(const GofTsdfVolume* vol, int64_t n, float tau, void* ws, size_t ws_bytes, int64_t V, int64_t F, float* vertices,
                          int32_t* triangles, float* colors, float* normals, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    (void)tau;
    if (int e = check_volume(vol)) return e;
    if (n < 0 || n > vol->block_capacity || V < 0 || F < 0 || V >= (1ll << 31) || F >= (1ll << 32)) { set_error("tsdf: bad counts"); return GOF_E_INVALID; }
    if (n == 0 || (V == 0 && F == 0)) return GOF_OK;
    if (!ws || ws_bytes < gof_tsdf_extract_ws_bytes(n)) { set_error("tsdf: extraction workspace too small"); return GOF_E_WORKSPACE; }
    if (!vertices || !triangles || !colors || !normals) { set_error("tsdf: NULL output"); return GOF_E_INVALID; }
    ExtractWs w;
    extract_layout(n, ws_aligned(ws), &w);
    hipLaunchKernelGGL(tsdf_vertices, dim3((unsigned)n), dim3(256), 0, stream, *vol, w.order, w.flags, w.bv, (uint32_t)V, w.vmap, vertices, colors, normals);
    GOF_LAUNCH_CHECK(stream, 0);
    hipLaunchKernelGGL(tsdf_triangles, dim3((unsigned)n), dim3(256), 0, stream, *vol, w.order, w.cases, w.bt, (uint32_t)F, w.vmap, triangles);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_tsdf_block_coords(const GofTsdfVolume* vol, int64_t n, int32_t* coords, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = check_volume(vol)) return e;
    if (n < 0 || n > vol->block_capacity) { set_error("tsdf: bad block count"); return GOF_E_INVALID; }
    if (n == 0) return GOF_OK;
    if (!coords) { set_error("tsdf: NULL output"); return GOF_E_INVALID; }
    hipLaunchKernelGGL(tsdf_decode, grid_of(n), dim3(256), 0, stream, vol->block_keys, (uint32_t)n, coords);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // extern "C"
