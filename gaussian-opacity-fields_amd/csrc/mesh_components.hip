// mesh_components.hip -- connected components of a triangle mesh over its faces: labels, per-component measures and the masks the
// selection needs (what the reference leaves to trimesh's split(): evaluate_dtu_mesh.py:132-138, eval_tnt/cull_mesh.py:186-201).
// Contract: DESIGN.md 3.18, include/gof_mesh_hip.h (d).
//
// Labels.  parent[] over the faces starts as the identity (it IS the face_label output).  A union walks both faces to their roots and
// hooks the LARGER root under the smaller with a device-scope atomicCAS on the root's own slot; a failed CAS returns the slot's
// value, an ancestor, and the walk goes on from there.  Parents only ever decrease, so whatever a load returns (every load of parent[]
// inside the linking launch is a relaxed device-scope atomic load: no L1 copy is trusted) is an ancestor, and only the CAS decides.
// The root of a component is therefore its smallest face index whatever the order of the unions.  No workgroup waits for another.
//   edge mode:   three keys min * 2^31 + max per face, written straight into the buffers of radix.h's sort_keys63 with value 3 f + k;
//                every sorted position whose key equals its predecessor's unites the two faces (a run of n equal keys: n - 1 unions).
//   vertex mode: owner[v] = the smallest face on v (atomicMin), then every face unites with the owners of its vertices.  No sort.
// Then launches of pointer jumping (up to JUMP_HOPS hops per face and launch) until a launch finds every face at its root, a launch
// that checks the labelling (every united pair has equal labels, label[label[f]] == label[f] <= f), and the numbering: root flags
// through the library's scan.
//
// Measures.  Faces sorted by component with the library's stable radix sort (ascending face index inside a component), the areas
// written in that order, then three levels of left-to-right sums over aligned tiles of 256 positions, blocks of 256 tiles and the
// blocks: one lane per tile / block, so one component of nearly all faces costs what 10^5 small ones cost.  A segment that lies inside
// one tile (one block) gets its area at that level; at most two segments per tile (block) stay open, its first and its last.
// fp64, -ffp-contract=off and no fma() here: every operation is the IEEE operation numpy performs, in the order written.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_mesh_hip.h"
#include "gof_common.h"
#include "radix.h"
#include "gof_geom.h"

namespace gof {

namespace meshcc {

constexpr int HDR_WORDS = 8;                    // u32: one word per flag (lanes store 1 into them: no atomic, no contention)
constexpr int H_INDEX = 0, H_CHECK = 1, H_COMP = 2, H_MORE = 3;
constexpr int JUMP_HOPS = 32, JUMP_MAX_ROUNDS = 64;          // 32^64 > any depth
constexpr uint32_t NO_FACE = 0xFFFFFFFFu;
constexpr uint32_t SUM_TILE = 256u, SUM_BLOCK = SUM_TILE * 256u;
constexpr int64_t MESH_MAX_COUNT = ((int64_t)1 << 31) - 1;    // as mesh_cull.hip: the compaction behind this unit scans N + 1 flags

__global__ void cc_init_hdr(uint32_t* hdr)
{
    if (threadIdx.x < HDR_WORDS) hdr[threadIdx.x] = 0u;
}
__global__ void cc_clear_word(uint32_t* word)
{
    if (threadIdx.x == 0) *word = 0u;
}

__device__ __forceinline__ bool index_ok(int32_t v, int64_t NV) { return v >= 0 && (int64_t)v < NV; }

// every index in [0, NV) (and, with face_comp, every component number in [0, C))
__global__ void __launch_bounds__(256)
cc_validate(int64_t NV, uint32_t NF, const int32_t* __restrict__ faces, const int32_t* __restrict__ face_comp, int64_t C, uint32_t* __restrict__ hdr)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= NF) return;
    if (!index_ok(faces[3 * (size_t)f], NV) || !index_ok(faces[3 * (size_t)f + 1], NV) || !index_ok(faces[3 * (size_t)f + 2], NV)) hdr[H_INDEX] = 1u;
    if (face_comp) { const int32_t c = face_comp[f]; if (c < 0 || (int64_t)c >= C) hdr[H_COMP] = 1u; }
}

// =====================================================================================================================================
// union-find over the faces
// =====================================================================================================================================
__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t uf_find(const uint32_t* parent, uint32_t x)
{
    uint32_t p = uf_load(&parent[x]);
    while (p != x) { x = p; p = uf_load(&parent[x]); }          // (strictly decreasing: ends)
    return x;
}

__device__ __forceinline__ void uf_union(uint32_t* parent, uint32_t a0, uint32_t b0)
{
    if (a0 == b0) return;
    uint32_t a = uf_find(parent, a0), b = uf_find(parent, b0);
    while (a != b) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicCAS(&parent[a], a, b);        // a was a root when looked at; it still is iff the slot holds a
        if (old == a) break;
        a = uf_find(parent, old);                                // someone hooked it first: go on from where it hangs now
        b = uf_find(parent, b);
    }
    // both faces hang below b now (b = a if they already hung together): shorten their paths.  atomicMin keeps "parents only decrease",
    // and b is an ancestor of both, so the forest stays the same set of trees.
    if (b < uf_load(&parent[a0])) atomicMin(&parent[a0], b);
    if (b < uf_load(&parent[b0])) atomicMin(&parent[b0], b);
}

// ---- edge mode ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 edge_key(int32_t a, int32_t b)
{
    const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
    return ((u64)lo << 31) + (u64)hi;                            // min * 2^31 + max < 2^62
}
__global__ void __launch_bounds__(256)
cc_edge_keys(uint32_t NF, const int32_t* __restrict__ faces, u64* __restrict__ keys, uint32_t* __restrict__ lo, uint32_t* __restrict__ idx,
             uint32_t* __restrict__ parent)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= NF) return;
    const int32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    const u64 k[3] = { edge_key(a, b), edge_key(b, c), edge_key(c, a) };
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const uint32_t e = 3u * f + (uint32_t)j;
        keys[e] = k[j];
        lo[e] = (uint32_t)k[j];
        idx[e] = e;
    }
    parent[f] = f;
}
// CHECK = false: unite; true: the united pairs must carry equal labels
template <bool CHECK>
__global__ void __launch_bounds__(256)
cc_edge_link(uint32_t NE, const u64* __restrict__ keys, const uint32_t* __restrict__ order, uint32_t* parent, uint32_t* __restrict__ hdr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0u || i >= NE) return;
    const uint32_t e = order[i], e0 = order[i - 1];
    if (keys[e] != keys[e0]) return;
    if (CHECK) { if (parent[e / 3u] != parent[e0 / 3u]) hdr[H_CHECK] = 1u; }
    else uf_union(parent, e / 3u, e0 / 3u);
}

// ---- vertex mode --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
cc_fill_u32(uint32_t n, uint32_t* __restrict__ out, uint32_t value, bool iota)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = iota ? i : value;
}
__global__ void __launch_bounds__(256)
cc_vertex_owner(uint32_t NF, const int32_t* __restrict__ faces, uint32_t* __restrict__ owner)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= NF) return;
#pragma unroll
    for (int j = 0; j < 3; j++) atomicMin(&owner[faces[3 * (size_t)f + j]], f);
}
template <bool CHECK>
__global__ void __launch_bounds__(256)
cc_vertex_link(uint32_t NF, const int32_t* __restrict__ faces, const uint32_t* __restrict__ owner, uint32_t* parent, uint32_t* __restrict__ hdr)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= NF) return;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const uint32_t o = owner[faces[3 * (size_t)f + j]];      // (<= f: this face took part in the minimum)
        if (CHECK) { if (o >= NF || parent[o] != parent[f]) hdr[H_CHECK] = 1u; }
        else if (o < NF) uf_union(parent, f, o);
    }
}

// ---- flatten, check, number ---------------------------------------------------------------------------------------------------------
// up to JUMP_HOPS hops from the face's parent; hdr[H_MORE] is set where the walk did not end at a root.  Nothing hooks any more: the
// roots are fixed, a face writes only its own slot, and every value a slot ever holds is an ancestor of the face.
__global__ void __launch_bounds__(256)
cc_jump(uint32_t NF, uint32_t* parent, uint32_t* __restrict__ hdr)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= NF) return;
    const uint32_t p = uf_load(&parent[f]);
    uint32_t x = p;
    bool root = false;
    for (int h = 0; h < JUMP_HOPS; h++) {
        const uint32_t q = uf_load(&parent[x]);
        if (q == x) { root = true; break; }
        x = q;
    }
    if (!root) hdr[H_MORE] = 1u;
    if (x != p) __hip_atomic_store(&parent[f], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// label[label[f]] == label[f] <= f; flags[f] = f is a root, flags[NF] = 0 (the exclusive scan's last word = C)
__global__ void __launch_bounds__(256)
cc_root_flags(uint32_t NF, const uint32_t* __restrict__ label, uint32_t* __restrict__ flags, uint32_t* __restrict__ hdr)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f > NF) return;
    if (f == NF) { flags[f] = 0u; return; }
    const uint32_t l = label[f];
    if (l > f || label[l] != l) hdr[H_CHECK] = 1u;
    flags[f] = l == f ? 1u : 0u;
}
__global__ void __launch_bounds__(256)
cc_number(uint32_t NF, const uint32_t* __restrict__ label, const uint32_t* __restrict__ rank, int32_t* __restrict__ face_comp)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < NF) { const uint32_t l = label[f]; face_comp[f] = (int32_t)rank[l <= f ? l : f]; }      // (l > f: the check has failed the call)
}

struct CcWs { uint32_t* hdr; u64* keys; Sort63Ws s; uint32_t* owner; uint32_t* flags; uint32_t* tmp; };
static size_t cc_layout(int64_t NV, int64_t NF, int mode, void* base, CcWs* out)
{
    const size_t nv = (size_t)(NV < 0 ? 0 : NV), nf = (size_t)(NF < 0 ? 0 : NF), ne = 3 * nf;
    Carver c{ static_cast<char*>(base), 0 };
    CcWs w{};
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    w.flags = c.take<uint32_t>(nf + 1);
    size_t tw = scan_tmp_words(nf + 1);
    if (mode == GOF_MESH_CONN_EDGE) {
        w.keys = c.take<u64>(ne);
        sort63_carve(c, ne, w.s);
        if (rs_tmp_words(ne) > tw) tw = rs_tmp_words(ne);
    }
    else w.owner = c.take<uint32_t>(nv);
    w.tmp = w.s.tmp = c.take<uint32_t>(tw);
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// measures
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
cs_fill(uint32_t NF, const int32_t* __restrict__ face_comp, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f < NF) { keys[f] = (uint32_t)face_comp[f]; vals[f] = f; }
}
// start[c] = the first sorted position whose component is >= c, for c in [0, C]: position i writes the components in
// (key[i - 1], key[i]] (key[-1] = -1, key[NF] = C).  Components without a face are a caller's doing; the loop is one step otherwise.
__global__ void __launch_bounds__(256)
cs_starts(uint32_t NF, const uint32_t* __restrict__ keys, int64_t C, uint32_t* __restrict__ start)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > NF) return;
    const int64_t prev = i == 0u ? -1 : (int64_t)keys[i - 1], cur = i == NF ? C : (int64_t)keys[i];
    for (int64_t c = prev + 1; c <= cur; c++) start[c] = i;
}
__global__ void __launch_bounds__(256)
cs_counts(int64_t C, const uint32_t* __restrict__ start, const uint32_t* __restrict__ vals, int64_t* __restrict__ comp_faces,
          int32_t* __restrict__ comp_first, double* __restrict__ comp_area)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const uint32_t s = start[c], n = start[c + 1] - s;
    comp_faces[c] = (int64_t)n;
    comp_first[c] = n ? (int32_t)vals[s] : -1;
    if (n == 0u) comp_area[c] = 0.0;
}
// area[i] = the area of the face at sorted position i
__global__ void __launch_bounds__(256)
cs_areas(uint32_t NF, const double* __restrict__ V, const int32_t* __restrict__ faces, const uint32_t* __restrict__ vals, double* __restrict__ area)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= NF) return;
    const size_t f = vals[i];
    const size_t a = (size_t)faces[3 * f], b = (size_t)faces[3 * f + 1], c = (size_t)faces[3 * f + 2];
    const double e1x = V[3 * b] - V[3 * a], e1y = V[3 * b + 1] - V[3 * a + 1], e1z = V[3 * b + 2] - V[3 * a + 2];
    const double e2x = V[3 * c] - V[3 * a], e2y = V[3 * c + 1] - V[3 * a + 1], e2z = V[3 * c + 2] - V[3 * a + 2];
    const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    area[i] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// One run of equal components inside a tile (block) is closed: first / last sums of the tile, and the component's area where its
// whole segment [start[c], start[c + 1]) lies in [lo, hi) and (level 2) not already inside one tile.
struct RunOut {
    double* head; double* tail; double* comp_area; const uint32_t* start; uint32_t lo, hi; bool level2; bool first;
    __device__ __forceinline__ void close(uint32_t c, double s)
    {
        if (first) { *head = s; first = false; }
        *tail = s;
        const uint32_t b = start[c], e = start[c + 1];
        if (b >= lo && e <= hi && (!level2 || b / SUM_TILE != (e - 1u) / SUM_TILE)) comp_area[c] = s;
    }
};
// level 1: one lane per tile of SUM_TILE sorted positions
__global__ void __launch_bounds__(256)
cs_tile_sums(uint32_t NF, const uint32_t* __restrict__ keys, const double* __restrict__ area, const uint32_t* __restrict__ start,
             double* __restrict__ head, double* __restrict__ tail, double* __restrict__ comp_area)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lo = t * SUM_TILE;
    if (lo >= NF) return;
    const uint32_t hi = NF - lo < SUM_TILE ? NF : lo + SUM_TILE;
    RunOut out{ &head[t], &tail[t], comp_area, start, lo, hi, false, true };
    uint32_t c = keys[lo];
    double s = area[lo];
    for (uint32_t i = lo + 1u; i < hi; i++) {
        const uint32_t k = keys[i];
        if (k != c) { out.close(c, s); c = k; s = area[i]; }
        else s = s + area[i];
    }
    out.close(c, s);
}
// level 2: one lane per block of 256 tiles; a tile contributes its first run and, where it is another component's, its last
__global__ void __launch_bounds__(256)
cs_block_sums(uint32_t NF, uint32_t ntiles, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ start, const double* __restrict__ head1,
              const double* __restrict__ tail1, double* __restrict__ head2, double* __restrict__ tail2, double* __restrict__ comp_area)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    const uint32_t t0 = u * 256u;
    if (t0 >= ntiles) return;
    const uint32_t t1 = ntiles - t0 < 256u ? ntiles : t0 + 256u;
    const uint32_t lo = u * SUM_BLOCK, hi = NF - lo < SUM_BLOCK ? NF : lo + SUM_BLOCK;
    RunOut out{ &head2[u], &tail2[u], comp_area, start, lo, hi, true, true };
    uint32_t c = 0u;
    double s = 0.0;
    bool open = false;
    for (uint32_t t = t0; t < t1; t++) {
        const uint32_t p = t * SUM_TILE, q = NF - p < SUM_TILE ? NF - 1u : p + SUM_TILE - 1u;
        const uint32_t kf = keys[p], kl = keys[q];
        if (open && kf == c) s = s + head1[t];
        else { if (open) out.close(c, s); c = kf; s = head1[t]; open = true; }
        if (kl != kf) { out.close(c, s); c = kl; s = tail1[t]; }
    }
    out.close(c, s);
}
// level 3: the lane of the block a segment starts in adds up the blocks it reaches into
__global__ void __launch_bounds__(256)
cs_top_sums(uint32_t NF, uint32_t nblocks, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ start, const double* __restrict__ head2,
            const double* __restrict__ tail2, double* __restrict__ comp_area)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u + 1u >= nblocks) return;                               // (the last block has nothing behind it)
    const uint32_t c = keys[(u + 1u) * SUM_BLOCK - 1u];          // the component of the block's last position
    const uint32_t b = start[c], e = start[c + 1];
    if (b / SUM_BLOCK != u || (e - 1u) / SUM_BLOCK == u) return;
    double s = tail2[u];
    for (uint32_t v = u + 1u; v <= (e - 1u) / SUM_BLOCK; v++) s = s + head2[v];
    comp_area[c] = s;
}

struct CsWs { uint32_t* hdr; uint32_t* keys[2]; uint32_t* vals[2]; uint32_t* start; double* area; double* head1; double* tail1; double* head2; double* tail2; uint32_t* tmp; };
static size_t cs_layout(int64_t NF, int64_t C, void* base, CsWs* out)
{
    const size_t nf = (size_t)(NF < 0 ? 0 : NF), nc = (size_t)(C < 0 ? 0 : C);
    const size_t ntiles = (nf + SUM_TILE - 1) / SUM_TILE, nblocks = (nf + SUM_BLOCK - 1) / SUM_BLOCK;
    Carver c{ static_cast<char*>(base), 0 };
    CsWs w{};
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    for (int k = 0; k < 2; k++) { w.keys[k] = c.take<uint32_t>(nf); w.vals[k] = c.take<uint32_t>(nf); }
    w.start = c.take<uint32_t>(nc + 1);
    w.area = c.take<double>(nf);
    w.head1 = c.take<double>(ntiles); w.tail1 = c.take<double>(ntiles);
    w.head2 = c.take<double>(nblocks); w.tail2 = c.take<double>(nblocks);
    w.tmp = c.take<uint32_t>(rs_tmp_words(nf));
    if (out) *out = w;
    return c.total();
}

// =====================================================================================================================================
// masks
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
cm_component_mask(uint32_t NF, const int32_t* __restrict__ face_comp, int64_t C, const uint8_t* __restrict__ comp_keep, uint8_t* __restrict__ face_keep)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= NF) return;
    const int32_t c = face_comp[f];
    face_keep[f] = (c >= 0 && (int64_t)c < C && comp_keep[c]) ? 1 : 0;
}
__global__ void __launch_bounds__(256)
cm_clear_bytes(int64_t n, uint8_t* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0;
}
__global__ void __launch_bounds__(256)
cm_mark_referenced(int64_t NV, uint32_t NF, const int32_t* __restrict__ faces, const uint8_t* __restrict__ face_keep, uint8_t* __restrict__ vert_keep)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= NF || (face_keep && !face_keep[f])) return;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int32_t v = faces[3 * (size_t)f + j];
        if (index_ok(v, NV)) vert_keep[v] = 1;                   // (every writer stores the same byte)
    }
}

static bool bad_faces(int64_t NF) { return NF < 0 || 3 * NF >= ((int64_t)1 << 31); }

} // namespace meshcc
} // namespace gof

using namespace gof;
using namespace gof::meshcc;

extern "C" {

int gof_mesh_abi_version(void) { return 2; }

void gof_mesh_components_tiling(int64_t* out)
{
    size_t scan_tile = 1;
    while (scan_tmp_words(scan_tile + 1) == scan_tmp_words(1)) scan_tile++;
    out[0] = (int64_t)rs_block_items();
    out[1] = (int64_t)scan_tile;
    out[2] = (int64_t)SUM_TILE;
    out[3] = (int64_t)SUM_BLOCK;
}

size_t gof_mesh_components_ws_bytes(int64_t NV, int64_t NF, int32_t mode) { return cc_layout(NV, bad_faces(NF) ? 0 : NF, mode, nullptr, nullptr); }

int gof_mesh_components(int64_t NV, int64_t NF, const int32_t* faces, int32_t mode, int32_t* face_label, int32_t* face_comp,
                        int64_t* num_components, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!num_components) { set_error("mesh_components: num_components is NULL"); return GOF_E_INVALID; }
    *num_components = 0;
    if (mode != GOF_MESH_CONN_EDGE && mode != GOF_MESH_CONN_VERTEX) { set_error("mesh_components: unknown connectivity mode %d", mode); return GOF_E_INVALID; }
    if (bad_count(NV, MESH_MAX_COUNT)) { set_error("mesh_components: bad number of vertices (%lld)", (long long)NV); return GOF_E_INVALID; }
    if (bad_faces(NF)) { set_error("mesh_components: bad number of faces (%lld): 3 * faces must be below 2^31", (long long)NF); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_components: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_components_ws_bytes(NV, NF, mode)) { set_error("mesh_components: workspace too small"); return GOF_E_WORKSPACE; }
    if (NF == 0) return GOF_OK;
    if (!faces || !face_label || !face_comp) { set_error("mesh_components: faces / face_label / face_comp is NULL"); return GOF_E_INVALID; }
    CcWs w;
    cc_layout(NV, NF, mode, ws_aligned(ws), &w);
    const uint32_t nf = (uint32_t)NF, ne = 3u * nf;
    uint32_t* parent = reinterpret_cast<uint32_t*>(face_label);
    uint32_t h[HDR_WORDS];
    GOF_PROFILE("mesh_components", stream);
    // the indices, before anything is written through them or into an output
    hipLaunchKernelGGL(cc_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(cc_validate, grid_of(NF), dim3(256), 0, stream, NV, nf, faces, (const int32_t*)nullptr, (int64_t)0, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(hipMemcpyAsync(h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (h[H_INDEX]) { set_error("mesh_components: a face index lies outside [0, %lld)", (long long)NV); return GOF_E_INVALID; }
    // link
    uint32_t* order = nullptr;
    const uint32_t* sort_err = nullptr;
    if (mode == GOF_MESH_CONN_EDGE) {
        hipLaunchKernelGGL(cc_edge_keys, grid_of(NF), dim3(256), 0, stream, nf, faces, w.keys, w.s.lo[0], w.s.idx[0], parent);
        GOF_LAUNCH_CHECK(stream, 0);
        GOF_HIP_CHECK(sort_keys63(w.keys, (size_t)ne, w.s, &order, stream));
        sort_err = radix_sort_error_flag(w.s.tmp, (size_t)ne, 31);
        if (sort_err) GOF_HIP_CHECK(hipMemcpyAsync(&h[H_COMP], sort_err, 4, hipMemcpyDeviceToHost, stream));      // (read before the scan reuses tmp)
        hipLaunchKernelGGL(cc_edge_link<false>, grid_of(ne), dim3(256), 0, stream, ne, w.keys, order, parent, w.hdr);
    }
    else {
        hipLaunchKernelGGL(cc_fill_u32, grid_of(NF), dim3(256), 0, stream, nf, parent, 0u, true);
        hipLaunchKernelGGL(cc_fill_u32, grid_of(NV), dim3(256), 0, stream, (uint32_t)NV, w.owner, NO_FACE, false);
        hipLaunchKernelGGL(cc_vertex_owner, grid_of(NF), dim3(256), 0, stream, nf, faces, w.owner);
        hipLaunchKernelGGL(cc_vertex_link<false>, grid_of(NF), dim3(256), 0, stream, nf, faces, w.owner, parent, w.hdr);
    }
    GOF_LAUNCH_CHECK(stream, 0);
    // flatten
    int rounds = 0;
    for (;; rounds++) {
        if (rounds == JUMP_MAX_ROUNDS) { set_error("mesh_components: the labels did not become flat in %d rounds", rounds); return GOF_E_DEVICE; }
        hipLaunchKernelGGL(cc_clear_word, dim3(1), dim3(64), 0, stream, w.hdr + H_MORE);
        hipLaunchKernelGGL(cc_jump, grid_of(NF), dim3(256), 0, stream, nf, parent, w.hdr);
        GOF_LAUNCH_CHECK(stream, 0);
        uint32_t more = 0;
        GOF_HIP_CHECK(hipMemcpyAsync(&more, w.hdr + H_MORE, 4, hipMemcpyDeviceToHost, stream));
        GOF_HIP_CHECK(hipStreamSynchronize(stream));
        if (!more) break;
    }
    if (sort_err && h[H_COMP]) { set_error("mesh_components: the edge sort gave up waiting for a predecessor"); return GOF_E_DEVICE; }
    // check, number
    if (mode == GOF_MESH_CONN_EDGE) hipLaunchKernelGGL(cc_edge_link<true>, grid_of(ne), dim3(256), 0, stream, ne, w.keys, order, parent, w.hdr);
    else hipLaunchKernelGGL(cc_vertex_link<true>, grid_of(NF), dim3(256), 0, stream, nf, faces, w.owner, parent, w.hdr);
    hipLaunchKernelGGL(cc_root_flags, grid_of(NF + 1), dim3(256), 0, stream, nf, parent, w.flags, w.hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.flags, nullptr, w.flags, (size_t)NF + 1, false, w.tmp, nullptr, stream));
    hipLaunchKernelGGL(cc_number, grid_of(NF), dim3(256), 0, stream, nf, parent, w.flags, face_comp);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t C = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipMemcpyAsync(&C, w.flags + NF, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (h[H_CHECK]) { set_error("mesh_components: the labelling failed its check (a united pair with different labels, or a label that is not a root)"); return GOF_E_DEVICE; }
    *num_components = (int64_t)C;
    return GOF_OK;
}

size_t gof_mesh_component_stats_ws_bytes(int64_t NF, int64_t C) { return cs_layout(bad_faces(NF) ? 0 : NF, bad_count(C) ? 0 : C, nullptr, nullptr); }

int gof_mesh_component_stats(int64_t NV, int64_t NF, const double* vertices, const int32_t* faces, const int32_t* face_comp, int64_t C,
                             int64_t* comp_faces, int32_t* comp_first, double* comp_area, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NV, MESH_MAX_COUNT)) { set_error("mesh_component_stats: bad number of vertices (%lld)", (long long)NV); return GOF_E_INVALID; }
    if (bad_faces(NF)) { set_error("mesh_component_stats: bad number of faces (%lld): 3 * faces must be below 2^31", (long long)NF); return GOF_E_INVALID; }
    if (bad_count(C)) { set_error("mesh_component_stats: bad number of components (%lld)", (long long)C); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_component_stats: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_component_stats_ws_bytes(NF, C)) { set_error("mesh_component_stats: workspace too small"); return GOF_E_WORKSPACE; }
    if (C == 0 && NF == 0) return GOF_OK;
    if (C == 0) { set_error("mesh_component_stats: %lld faces and no component", (long long)NF); return GOF_E_INVALID; }
    if (!comp_faces || !comp_first || !comp_area) { set_error("mesh_component_stats: an output is NULL"); return GOF_E_INVALID; }
    if (NF && (!vertices || !faces || !face_comp)) { set_error("mesh_component_stats: vertices / faces / face_comp is NULL"); return GOF_E_INVALID; }
    CsWs w;
    cs_layout(NF, C, ws_aligned(ws), &w);
    const uint32_t nf = (uint32_t)NF;
    GOF_PROFILE("mesh_component_stats", stream);
    uint32_t* keys = w.keys[0];
    uint32_t* vals = w.vals[0];
    if (NF) {
        uint32_t h[HDR_WORDS];
        hipLaunchKernelGGL(cc_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
        hipLaunchKernelGGL(cc_validate, grid_of(NF), dim3(256), 0, stream, NV, nf, faces, face_comp, C, w.hdr);
        GOF_LAUNCH_CHECK(stream, 0);
        GOF_HIP_CHECK(hipMemcpyAsync(h, w.hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
        GOF_HIP_CHECK(hipStreamSynchronize(stream));
        if (h[H_INDEX]) { set_error("mesh_component_stats: a face index lies outside [0, %lld)", (long long)NV); return GOF_E_INVALID; }
        if (h[H_COMP]) { set_error("mesh_component_stats: a component number lies outside [0, %lld)", (long long)C); return GOF_E_INVALID; }
        hipLaunchKernelGGL(cs_fill, grid_of(NF), dim3(256), 0, stream, nf, face_comp, w.keys[0], w.vals[0]);
        GOF_LAUNCH_CHECK(stream, 0);
        int bits = 0;
        while (bits < 31 && ((int64_t)1 << bits) < C) bits++;
        GOF_HIP_CHECK(radix_sort_pairs_u32(w.keys[0], w.vals[0], w.keys[1], w.vals[1], (size_t)NF, bits, w.tmp, &keys, &vals, stream, nullptr));
    }
    hipLaunchKernelGGL(cs_starts, grid_of(NF + 1), dim3(256), 0, stream, nf, keys, C, w.start);
    hipLaunchKernelGGL(cs_counts, grid_of(C), dim3(256), 0, stream, C, w.start, vals, comp_faces, comp_first, comp_area);
    if (NF) {
        const uint32_t ntiles = (nf + SUM_TILE - 1u) / SUM_TILE, nblocks = (nf + SUM_BLOCK - 1u) / SUM_BLOCK;
        hipLaunchKernelGGL(cs_areas, grid_of(NF), dim3(256), 0, stream, nf, vertices, faces, vals, w.area);
        hipLaunchKernelGGL(cs_tile_sums, grid_of(ntiles), dim3(256), 0, stream, nf, keys, w.area, w.start, w.head1, w.tail1, comp_area);
        hipLaunchKernelGGL(cs_block_sums, grid_of(nblocks), dim3(256), 0, stream, nf, ntiles, keys, w.start, w.head1, w.tail1, w.head2, w.tail2, comp_area);
        if (nblocks > 1u) hipLaunchKernelGGL(cs_top_sums, grid_of(nblocks), dim3(256), 0, stream, nf, nblocks, keys, w.start, w.head2, w.tail2, comp_area);
    }
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_mesh_component_mask(int64_t NF, const int32_t* face_comp, int64_t C, const uint8_t* comp_keep, uint8_t* face_keep, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_faces(NF) || bad_count(C)) { set_error("mesh_component_mask: bad counts (%lld faces, %lld components)", (long long)NF, (long long)C); return GOF_E_INVALID; }
    if (NF == 0) return GOF_OK;
    if (!face_comp || !face_keep || (C && !comp_keep)) { set_error("mesh_component_mask: face_comp / comp_keep / face_keep is NULL"); return GOF_E_INVALID; }
    hipLaunchKernelGGL(cm_component_mask, grid_of(NF), dim3(256), 0, stream, (uint32_t)NF, face_comp, C, comp_keep, face_keep);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_mesh_mark_referenced(int64_t NV, int64_t NF, const int32_t* faces, const uint8_t* face_keep, uint8_t* vert_keep, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NV, MESH_MAX_COUNT) || bad_faces(NF)) { set_error("mesh_mark_referenced: bad counts (%lld vertices, %lld faces)", (long long)NV, (long long)NF); return GOF_E_INVALID; }
    if (NV == 0) return GOF_OK;
    if (!vert_keep || (NF && !faces)) { set_error("mesh_mark_referenced: faces / vert_keep is NULL"); return GOF_E_INVALID; }
    hipLaunchKernelGGL(cm_clear_bytes, grid_of(NV), dim3(256), 0, stream, NV, vert_keep);
    if (NF) hipLaunchKernelGGL(cm_mark_referenced, grid_of(NF), dim3(256), 0, stream, NV, (uint32_t)NF, faces, face_keep, vert_keep);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // extern "C"
