// mesh_cull.hip -- mesh culling of the DTU evaluation (replaces what the reference's evaluate_dtu_mesh.py:77-131 asks of
// scikit-image, torch GEMMs + grid_sample and trimesh): (a) disk dilation of an object mask into a bit-packed image, (b) the test of
// every vertex against every view's dilated mask, (c) compaction of the mesh.  Contract: DESIGN.md 3.10, include/gof_mesh_hip.h.
//
// Arithmetic: (a) and (c) are integer work; (b) is fp64, compiled with -ffp-contract=off like the whole library and no fma() is
// written here, so every operation is the IEEE operation numpy performs on the host, in the order written.
//
// (a) one workgroup per tile of 16 rows x 16 words (1024 pixels) of the output.  The tile's input with a halo of r rows and one word
//     (r <= 31 < 64) is packed into LDS, one ballot per 64 pixels (a wave reads 64 consecutive pixels: coalesced).  The disk is the
//     union over the column offset s of the rows |dy| <= D(s) = floor(sqrt(r*r - s*s)) shifted by s: walking s from r down to 0 the
//     set of rows only grows, so V = OR of the rows |dy| <= D(s) is kept incrementally (2r + 1 three-word ORs in all) and every s
//     costs two funnel shifts of V: ~10 (2r + 1) operations per output word instead of (2r + 1)^2.
// (b) one lane per vertex, the loop over the views leaves at the first view that drops the vertex; the view record's address is
//     wave-uniform (scalar loads), the mask bit is one 8-byte load.
// (c) flags -> the library's scan -> ranks: kept vertices' rows, then the faces filtered and renumbered over the vertex ranks.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_mesh_hip.h"
#include "gof_common.h"
#include "radix.h"
#include "gof_geom.h"

namespace gof {

namespace mesh {

constexpr int DIL_ROWS = 16, DIL_WORDS = 16;                          // the output tile
constexpr int DIL_LDS_ROWS = DIL_ROWS + 2 * GOF_MESH_MAX_RADIUS;      // 78
constexpr int DIL_LDS_WORDS = DIL_WORDS + 2;                          // 18
constexpr uint32_t F_RECORD = 1u, F_INDEX = 2u;
constexpr int HDR_WORDS = 8;                                          // u32: [0] flags

// one less than the other units take (they accept N = 2^31 - 1): the compaction scans and launches over N + 1 flags, and this unit
// keeps that count below 2^31 as well
constexpr int64_t MESH_MAX_COUNT = ((int64_t)1 << 31) - 1;

__global__ void mesh_init_hdr(uint32_t* hdr)
{
    if (threadIdx.x < HDR_WORDS) hdr[threadIdx.x] = 0u;
}

// =====================================================================================================================================
// (a) disk dilation
// =====================================================================================================================================
template <typename T> __device__ __forceinline__ bool pixel_set(T m) { return (float)m / 256.0f != 0.0f; }

template <typename T>
__global__ void __launch_bounds__(256)
mesh_dilate(int W, int H, const T* __restrict__ mask, int r, int nw, u64* __restrict__ out)
{
    __shared__ u64 s_in[DIL_LDS_ROWS * DIL_LDS_WORDS];
    const int y0 = (int)blockIdx.y * DIL_ROWS, w0 = (int)blockIdx.x * DIL_WORDS;
    const int rows = DIL_ROWS + 2 * r;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // pack: LDS word (j, k) = pixels [64 (w0 - 1 + k), + 64) of row y0 - r + j; outside the image: unset
    for (int e = wave; e < rows * DIL_LDS_WORDS; e += 4) {
        const int j = e / DIL_LDS_WORDS, k = e - j * DIL_LDS_WORDS;
        const int y = y0 - r + j, wx = w0 - 1 + k;
        const int64_t x = (int64_t)wx * 64 + lane;
        bool set = false;
        if (y >= 0 && y < H && wx >= 0 && x < W) set = pixel_set<T>(mask[(int64_t)y * W + x]);
        const u64 word = __ballot(set);
        if (lane == 0) s_in[e] = word;
    }
    __syncthreads();
    const int i = threadIdx.x / DIL_WORDS, k = threadIdx.x % DIL_WORDS;      // output row / word of the tile
    const int y = y0 + i, wx = w0 + k;
    if (y >= H || wx >= nw) return;
    const u64* c = &s_in[(i + r) * DIL_LDS_WORDS + k + 1];                   // the centre word of the row dy = 0
    u64 VL = 0, VC = 0, VR = 0, res = 0;
    int d = -1;                                                              // rows |dy| <= d are in V
    for (int s = r; s >= 0; s--) {
        while ((d + 1) * (d + 1) + s * s <= r * r) {
            d++;
            const u64* a = c + d * DIL_LDS_WORDS;
            const u64* b = c - d * DIL_LDS_WORDS;
            VL |= a[-1] | b[-1]; VC |= a[0] | b[0]; VR |= a[1] | b[1];
        }
        // (d >= 0 from the first s on: 0 + r*r <= r*r)
        if (s == 0) res |= VC;
        else res |= (VC << s) | (VL >> (64 - s)) | (VC >> s) | (VR << (64 - s));
    }
    const int tail = W - wx * 64;                                            // pixels of the image in this word (>= 1)
    if (tail < 64) res &= (1ull << tail) - 1ull;
    out[(int64_t)y * nw + wx] = res;
}

// =====================================================================================================================================
// (b) vertex culling
// =====================================================================================================================================
__global__ void __launch_bounds__(256)
mesh_cull_kernel(int64_t NV, const float* __restrict__ vertices, int num_views, const GofCullView* __restrict__ views,
                 const u64* __restrict__ masks, int64_t mask_words, uint8_t* __restrict__ keep, uint32_t* __restrict__ hdr)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NV) return;
    const double vx = (double)vertices[3 * i], vy = (double)vertices[3 * i + 1], vz = (double)vertices[3 * i + 2];
    bool kept = true;
    for (int v = 0; v < num_views && kept; v++) {
        const GofCullView& V = views[v];
        const int W = V.W, H = V.H;
        const int64_t off = V.mask_offset, rw = V.row_words;
        // the record's mask must lie inside `masks` (in this order: no product before its factors are known to be small)
        if (W < 1 || H < 1 || rw < ((int64_t)W + 63) / 64 || rw > mask_words || off < 0 || off > mask_words || (int64_t)H > (mask_words - off) / rw) {
            atomicOr(&hdr[0], F_RECORD);
            continue;
        }
        const double x = ((V.m[0] * vx + V.m[1] * vy) + V.m[2] * vz) + V.m[3];
        const double y = ((V.m[4] * vx + V.m[5] * vy) + V.m[6] * vz) + V.m[7];
        const double z = ((V.m[8] * vx + V.m[9] * vy) + V.m[10] * vz) + V.m[11];
        const double d = z + 1e-6;
        const double w1 = (double)(W - 1), h1 = (double)(H - 1);
        const double px = ((x / d) / w1 - 0.5) * 2.0;
        const double py = ((y / d) / h1 - 0.5) * 2.0;
        const bool valid = px > -1.0 && px < 1.0 && py > -1.0 && py < 1.0;
        if (!valid) continue;
        const double fx = rint((px + 1.0) / 2.0 * w1), fy = rint((py + 1.0) / 2.0 * h1);
        bool in = false;
        if (fx >= 0.0 && fx <= w1 && fy >= 0.0 && fy <= h1) {
            const int64_t ix = (int64_t)fx, iy = (int64_t)fy;
            in = (masks[off + iy * rw + (ix >> 6)] >> (ix & 63)) & 1ull;
        }
        kept = in;
    }
    keep[i] = kept ? 1 : 0;
}

// =====================================================================================================================================
// (c) compaction
// =====================================================================================================================================
// flags[i] = keep[i] != 0, flags[N] = 0 (the exclusive scan's last word = the total)
__global__ void __launch_bounds__(256)
mesh_vertex_flags(int64_t NV, const uint8_t* __restrict__ keep, uint32_t* __restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= NV) flags[i] = (i < NV && keep[i]) ? 1u : 0u;
}
__global__ void __launch_bounds__(256)
mesh_vertex_rows(int64_t NV, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ rank, int32_t* __restrict__ out_rows)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NV && keep[i]) out_rows[rank[i]] = (int32_t)i;
}
__global__ void __launch_bounds__(256)
mesh_face_flags(int64_t NV, const uint8_t* __restrict__ keep, int64_t NF, const int32_t* __restrict__ faces, int drop, uint32_t* __restrict__ flags,
                uint8_t* __restrict__ face_keep, uint32_t* __restrict__ hdr)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j == NF) flags[j] = 0u;
    if (j >= NF) return;
    const int64_t a = faces[3 * j], b = faces[3 * j + 1], c = faces[3 * j + 2];
    bool all = false;
    if (a < 0 || a >= NV || b < 0 || b >= NV || c < 0 || c >= NV) atomicOr(&hdr[0], F_INDEX);
    else all = keep[a] && keep[b] && keep[c];
    if (face_keep) face_keep[j] = all ? 1 : 0;
    flags[j] = (drop ? all : true) ? 1u : 0u;
}
// pos = exclusive scan of the flags over NF + 1 words: face j is written iff pos[j + 1] > pos[j], to row pos[j]
__global__ void __launch_bounds__(256)
mesh_face_emit(int64_t NV, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ rank, int64_t NF, const int32_t* __restrict__ faces,
               const uint32_t* __restrict__ pos, int32_t* __restrict__ out_faces)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= NF) return;
    const uint32_t p = pos[j];
    if (pos[j + 1] == p) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int64_t v = faces[3 * j + c];
        const bool ok = v >= 0 && v < NV && keep[v];                         // (an index out of range: the call fails; nothing is read through it)
        out_faces[3 * (int64_t)p + c] = ok ? (int32_t)rank[v] : 0;
    }
}

struct CompactWs { uint32_t* hdr; uint32_t* vflags; uint32_t* fflags; uint32_t* tmp; };
static size_t compact_layout(int64_t NV, int64_t NF, void* base, CompactWs* out)
{
    const size_t nv = (size_t)(NV < 0 ? 0 : NV) + 1, nf = (size_t)(NF < 0 ? 0 : NF) + 1;
    Carver c{ static_cast<char*>(base), 0 };
    CompactWs w;
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    w.vflags = c.take<uint32_t>(nv);
    w.fflags = c.take<uint32_t>(nf);
    const size_t t1 = scan_tmp_words(nv), t2 = scan_tmp_words(nf);
    w.tmp = c.take<uint32_t>(t1 > t2 ? t1 : t2);
    if (out) *out = w;
    return c.total();
}

} // namespace mesh
} // namespace gof

using namespace gof;
using namespace gof::mesh;

extern "C" {

int64_t gof_mesh_mask_row_words(int32_t W) { return W < 1 ? 0 : ((int64_t)W + 63) / 64; }

int gof_mesh_dilate(int32_t W, int32_t H, const void* mask, int32_t is_u8, int32_t r, uint64_t* out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (W < 1 || H < 1) { set_error("mesh_dilate: bad image size (%d x %d)", W, H); return GOF_E_INVALID; }
    if (r < 0 || r > GOF_MESH_MAX_RADIUS) { set_error("mesh_dilate: the radius must lie in [0, %d], got %d", GOF_MESH_MAX_RADIUS, r); return GOF_E_INVALID; }
    if (!mask || !out) { set_error("mesh_dilate: mask / out is NULL"); return GOF_E_INVALID; }
    const int nw = (int)gof_mesh_mask_row_words(W);
    const dim3 grid((unsigned)((nw + DIL_WORDS - 1) / DIL_WORDS), (unsigned)((H + DIL_ROWS - 1) / DIL_ROWS));
    if (grid.y > 65535u) { set_error("mesh_dilate: more than %d rows", 65535 * DIL_ROWS); return GOF_E_CAPACITY; }
    GOF_PROFILE("mesh_dilate", stream);
    if (is_u8) hipLaunchKernelGGL(mesh_dilate<uint8_t>, grid, dim3(256), 0, stream, (int)W, (int)H, static_cast<const uint8_t*>(mask), (int)r, nw, reinterpret_cast<u64*>(out));
    else hipLaunchKernelGGL(mesh_dilate<float>, grid, dim3(256), 0, stream, (int)W, (int)H, static_cast<const float*>(mask), (int)r, nw, reinterpret_cast<u64*>(out));
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

size_t gof_mesh_cull_ws_bytes(int64_t) { return align_up(HDR_WORDS * 4) + ALIGN; }

int gof_mesh_cull(int64_t NV, const float* vertices, int32_t num_views, const GofCullView* views, const uint64_t* masks, int64_t mask_words,
                  uint8_t* keep, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NV, MESH_MAX_COUNT)) { set_error("mesh_cull: bad number of vertices (%lld)", (long long)NV); return GOF_E_INVALID; }
    if (num_views < 0 || mask_words < 0) { set_error("mesh_cull: bad number of views (%d) / mask words (%lld)", num_views, (long long)mask_words); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_cull: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_cull_ws_bytes(NV)) { set_error("mesh_cull: workspace too small"); return GOF_E_WORKSPACE; }
    if (num_views && (!views || !masks)) { set_error("mesh_cull: views / masks is NULL"); return GOF_E_INVALID; }
    if (NV == 0) return GOF_OK;
    if (!vertices || !keep) { set_error("mesh_cull: vertices / keep is NULL"); return GOF_E_INVALID; }
    uint32_t* hdr = static_cast<uint32_t*>(ws_aligned(ws));
    GOF_PROFILE("mesh_cull", stream);
    hipLaunchKernelGGL(mesh_init_hdr, dim3(1), dim3(64), 0, stream, hdr);
    hipLaunchKernelGGL(mesh_cull_kernel, grid_of(NV), dim3(256), 0, stream, NV, vertices, (int)num_views, views, reinterpret_cast<const u64*>(masks), mask_words, keep, hdr);
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t flags = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, hdr, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (flags & F_RECORD) { set_error("mesh_cull: a view record has a bad size or a mask that does not lie inside the %lld mask words", (long long)mask_words); return GOF_E_INVALID; }
    return GOF_OK;
}

size_t gof_mesh_compact_ws_bytes(int64_t NV, int64_t NF) { return compact_layout(NV, NF, nullptr, nullptr); }

int gof_mesh_compact(int64_t NV, const uint8_t* keep, int64_t NF, const int32_t* faces, int32_t drop_faces, int32_t* out_rows, int32_t* out_faces,
                     uint8_t* face_keep, void* ws, size_t ws_bytes, int64_t* counts, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!counts) { set_error("mesh_compact: counts is NULL"); return GOF_E_INVALID; }
    counts[0] = counts[1] = 0;
    if (bad_count(NV, MESH_MAX_COUNT) || bad_count(NF, MESH_MAX_COUNT)) { set_error("mesh_compact: bad counts (%lld vertices, %lld faces)", (long long)NV, (long long)NF); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_compact: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_compact_ws_bytes(NV, NF)) { set_error("mesh_compact: workspace too small"); return GOF_E_WORKSPACE; }
    if (NV && (!keep || !out_rows)) { set_error("mesh_compact: keep / out_rows is NULL"); return GOF_E_INVALID; }
    if (NF && (!faces || !out_faces)) { set_error("mesh_compact: faces / out_faces is NULL"); return GOF_E_INVALID; }
    if (NV == 0 && NF == 0) return GOF_OK;
    CompactWs w;
    compact_layout(NV, NF, ws_aligned(ws), &w);
    GOF_PROFILE("mesh_compact", stream);
    hipLaunchKernelGGL(mesh_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr);
    hipLaunchKernelGGL(mesh_vertex_flags, grid_of(NV + 1), dim3(256), 0, stream, NV, keep, w.vflags);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.vflags, nullptr, w.vflags, (size_t)NV + 1, false, w.tmp, nullptr, stream));
    if (NV) hipLaunchKernelGGL(mesh_vertex_rows, grid_of(NV), dim3(256), 0, stream, NV, keep, w.vflags, out_rows);
    if (NF) {
        hipLaunchKernelGGL(mesh_face_flags, grid_of(NF + 1), dim3(256), 0, stream, NV, keep, NF, faces, (int)(drop_faces != 0), w.fflags, face_keep, w.hdr);
        GOF_LAUNCH_CHECK(stream, 0);
        GOF_HIP_CHECK(device_scan_u32(w.fflags, nullptr, w.fflags, (size_t)NF + 1, false, w.tmp, nullptr, stream));
        hipLaunchKernelGGL(mesh_face_emit, grid_of(NF), dim3(256), 0, stream, NV, keep, w.vflags, NF, faces, w.fflags, out_faces);
    }
    GOF_LAUNCH_CHECK(stream, 0);
    uint32_t flags = 0, nv = 0, nf = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&flags, w.hdr, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipMemcpyAsync(&nv, w.vflags + NV, 4, hipMemcpyDeviceToHost, stream));
    if (NF) GOF_HIP_CHECK(hipMemcpyAsync(&nf, w.fflags + NF, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if (flags & F_INDEX) { set_error("mesh_compact: a face index lies outside [0, %lld)", (long long)NV); return GOF_E_INVALID; }
    counts[0] = nv;
    counts[1] = nf;
    return GOF_OK;
}

} // extern "C"
