// model_io.hip -- the model file's row transpose on HIP (C ABI in include/gof_model_io_hip.h).
//
// GaussianModel.save_ply / save_fused_ply / load_ply (reference scene/gaussian_model.py:374-430, 486-530) move the model between seven
// structure-of-arrays tensors and the rows of a PLY file: x y z | nx ny nz | f_dc | f_rest (channel-major) | opacity | scale | rot |
// filter_3D.  Two kernels, one workgroup of 256 threads per tile of 64 rows:
//
//   model_pack:   each tensor's slice of the tile is contiguous in memory: it is read coalesced, word by word, and placed at its
//                 column of the tile's image in LDS (the tile as it lies in the file: 64 rows of C words); the image then leaves as ONE
//                 contiguous run, 16 bytes per lane where the output is 16-byte aligned (a tile is 256 C bytes, so every tile start is).
//                 The LDS pitch is C itself so that the image needs no second index computation: at C = 63 (degree 3) the pitch is odd
//                 and the transposing writes of f_rest (lane stride K = 15 words inside a row, 63 between rows) spread over the 32
//                 write banks; at the even C of degrees 0, 2 and 4 they meet 2-way conflicts, on a kernel that waits for HBM.
//                 Values travel as 32-bit words (NaN payloads, -0.0 and denormals survive by construction); only the FUSED mode's
//                 four columns are computed, by the activations' own device functions (gof_activations.h) and logf.
//   model_unpack: the inverse, driven by a column table (byte offset and type per model channel) passed as a kernel argument: a
//                 thread per destination element, destinations written coalesced, sources read through the cache (the 64 rows of a
//                 tile are 64 * pitch contiguous bytes).  A value that is not 4-byte aligned is assembled from bytes; float64 is
//                 rounded to the nearest float32.
// Both are bound by HBM: 2 x 4 (18 + 3K) bytes moved per Gaussian and no arithmetic in RAW mode.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/gof_hip.h"
#include "../../include/gof_model_io_hip.h"
#include "gof_common.h"
#include "gof_activations.h"

namespace gof {
namespace model_io {

constexpr int TILE_ROWS = 64;
constexpr int THREADS = 256;
constexpr int MAX_C = 18 + 3 * GOF_MODEL_MAX_K;                 // words per row of the widest file
constexpr int MAX_CHANNELS = 15 + 3 * GOF_MODEL_MAX_K;
constexpr int NSEG = 7;
constexpr int64_t MAX_P = 0x7FFFFFFF;
constexpr int64_t MAX_PITCH = (int64_t)1 << 30;

enum Seg { S_XYZ = 0, S_DC = 1, S_REST = 2, S_OPACITY = 3, S_SCALING = 4, S_ROTATION = 5, S_FILTER = 6 };

// words per Gaussian of tensor s
__host__ __device__ __forceinline__ int seg_width(int s, int K)
{
    return s == S_REST ? 3 * K : (s == S_OPACITY || s == S_FILTER) ? 1 : s == S_ROTATION ? 4 : 3;
}
// the RAW file column of word e of tensor s's row (the FUSED file has the same columns without the last)
__host__ __device__ __forceinline__ int seg_column(int s, int e, int K)
{
    switch (s) {
    case S_XYZ: return e;
    case S_DC: return 6 + e;
    case S_REST: { const int k = e / 3, c = e - 3 * k; return 9 + c * K + k; }      // f_rest_j, j = c K + k, holds f_rest[p, k, c]
    case S_OPACITY: return 9 + 3 * K;
    case S_SCALING: return 10 + 3 * K + e;
    case S_ROTATION: return 13 + 3 * K + e;
    default: return 17 + 3 * K;
    }
}

struct PackSrc { const uint32_t* t[NSEG]; };
struct UnpackDst { uint32_t* t[NSEG]; };
// per model channel: byte offset inside a source row (< 2^30), bit 31 = the value is a float64
struct ColTable { uint32_t w[MAX_CHANNELS]; };

__global__ void __launch_bounds__(THREADS)
model_pack(int64_t first, int64_t count, int K, int fused, PackSrc src, uint32_t* __restrict__ out, int vec)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[TILE_ROWS * MAX_C];
    const int C = 18 + 3 * K - (fused ? 1 : 0);
    const int64_t tile0 = (int64_t)blockIdx.x * TILE_ROWS;
    const int rows = (int)(count - tile0 < TILE_ROWS ? count - tile0 : TILE_ROWS);
    const int tid = threadIdx.x;
    for (int s = 0; s < NSEG; s++) {
        if (fused && (s == S_OPACITY || s == S_SCALING || s == S_FILTER)) continue;
        const int w = seg_width(s, K);
        if (w == 0) continue;
        const uint32_t* __restrict__ base = src.t[s] + (first + tile0) * w;
        const int n = rows * w;
        for (int i = tid; i < n; i += THREADS) {
            const int r = i / w, e = i - r * w;
            s_tile[r * C + seg_column(s, e, K)] = base[i];
        }
    }
    for (int i = tid; i < rows * 3; i += THREADS) {             // nx ny nz: +0.0
        const int r = i / 3, e = i - 3 * r;
        s_tile[r * C + 3 + e] = 0u;
    }
    if (fused && tid < rows) {
        const int64_t p = first + tile0 + tid;
        const float f = __uint_as_float(src.t[S_FILTER][p]), ff = f * f;
        const float r0 = __uint_as_float(src.t[S_SCALING][3 * p]), r1 = __uint_as_float(src.t[S_SCALING][3 * p + 1]),
                    r2 = __uint_as_float(src.t[S_SCALING][3 * p + 2]);
        const float o = act_opacity_value(__uint_as_float(src.t[S_OPACITY][p]), r0, r1, r2, ff);
        uint32_t* row = s_tile + tid * C;
        row[9 + 3 * K] = __float_as_uint(logf(o / (1.0f - o)));                     // inverse_sigmoid (utils/general_utils.py)
        row[10 + 3 * K] = __float_as_uint(logf(act_scaling_value(r0, ff)));
        row[11 + 3 * K] = __float_as_uint(logf(act_scaling_value(r1, ff)));
        row[12 + 3 * K] = __float_as_uint(logf(act_scaling_value(r2, ff)));
    }
    __syncthreads();
    const int n = rows * C;
    uint32_t* __restrict__ dst = out + tile0 * C;
    int done = 0;
    if (vec) {
        const int n4 = n >> 2;
        const uint4* s4 = reinterpret_cast<const uint4*>(s_tile);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (int i = tid; i < n4; i += THREADS) d4[i] = s4[i];
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += THREADS) dst[i] = s_tile[i];
}

// the 32-bit little-endian word at p, whatever p's alignment
__device__ __forceinline__ uint32_t load_word(const uint8_t* p)
{
    if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ void __launch_bounds__(THREADS)
model_unpack(int64_t first, int64_t count, int K, const uint8_t* __restrict__ rows_, int64_t pitch, ColTable tab, UnpackDst dst)
{
    __shared__ uint32_t s_tab[MAX_CHANNELS];
    const int tid = threadIdx.x;
    const int nch = 15 + 3 * K;
    for (int i = tid; i < nch; i += THREADS) s_tab[i] = tab.w[i];
    __syncthreads();
    const int64_t tile0 = (int64_t)blockIdx.x * TILE_ROWS;
    const int rows = (int)(count - tile0 < TILE_ROWS ? count - tile0 : TILE_ROWS);
    const uint8_t* tile = rows_ + tile0 * pitch;
    for (int s = 0; s < NSEG; s++) {
        const int w = seg_width(s, K);
        if (w == 0) continue;
        uint32_t* __restrict__ base = dst.t[s] + (first + tile0) * w;
        const int n = rows * w;
        for (int i = tid; i < n; i += THREADS) {
            const int r = i / w, e = i - r * w;
            const int column = seg_column(s, e, K);
            const uint32_t col = s_tab[column < 3 ? column : column - 3];          // (the model has no channel for nx ny nz)
            const uint8_t* p = tile + (int64_t)r * pitch + (col & 0x7FFFFFFFu);
            uint32_t v = load_word(p);
            if (col >> 31) {
                const uint64_t bits = (uint64_t)v | ((uint64_t)load_word(p + 4) << 32);
                v = __float_as_uint((float)__builtin_bit_cast(double, bits));       // round to nearest even
            }
            base[i] = v;
        }
    }
}

static bool bad_range(int64_t P, int64_t first, int64_t count)
{
    return P < 0 || P > MAX_P || first < 0 || count < 0 || first > P || count > P - first;
}

} // namespace model_io
} // namespace gof

using namespace gof;
using namespace gof::model_io;

extern "C" {

int64_t gof_model_row_floats(int32_t K, int32_t mode)
{
    if (K < 0 || K > GOF_MODEL_MAX_K || (mode != GOF_MODEL_RAW && mode != GOF_MODEL_FUSED)) return -1;
    return 18 + 3 * (int64_t)K - (mode == GOF_MODEL_FUSED ? 1 : 0);
}

int64_t gof_model_channels(int32_t K)
{
    return (K < 0 || K > GOF_MODEL_MAX_K) ? -1 : 15 + 3 * (int64_t)K;
}

int gof_model_pack(int64_t P, int32_t K, int64_t first, int64_t count, const float* xyz, const float* f_dc, const float* f_rest,
                   const float* opacity, const float* scaling, const float* rotation, const float* filter_3D, int32_t mode,
                   float* out_rows, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (gof_model_row_floats(K, mode) < 0) { set_error("model_pack: bad K (%d, at most %d) or mode (%d)", K, GOF_MODEL_MAX_K, mode); return GOF_E_INVALID; }
    if (bad_range(P, first, count)) { set_error("model_pack: rows [%lld, %lld + %lld) do not lie inside a model of %lld", (long long)first, (long long)first, (long long)count, (long long)P); return GOF_E_INVALID; }
    if (count == 0) return GOF_OK;
    if (!xyz || !f_dc || (K && !f_rest) || !opacity || !scaling || !rotation || !filter_3D || !out_rows) { set_error("model_pack: a pointer is NULL"); return GOF_E_INVALID; }
    PackSrc src;
    const float* t[NSEG] = { xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D };
    for (int s = 0; s < NSEG; s++) src.t[s] = reinterpret_cast<const uint32_t*>(t[s]);
    const int vec = (reinterpret_cast<uintptr_t>(out_rows) & 15u) == 0 ? 1 : 0;
    GOF_PROFILE("model_pack", stream);
    hipLaunchKernelGGL(model_pack, dim3((unsigned)((count + TILE_ROWS - 1) / TILE_ROWS)), dim3(THREADS), 0, stream, first, count, (int)K,
                       mode == GOF_MODEL_FUSED ? 1 : 0, src, reinterpret_cast<uint32_t*>(out_rows), vec);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_model_unpack(int64_t P, int32_t K, int64_t first, int64_t count, const void* rows, int64_t pitch, const GofModelColumn* columns,
                     float* xyz, float* f_dc, float* f_rest, float* opacity, float* scaling, float* rotation, float* filter_3D,
                     void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t nch = gof_model_channels(K);
    if (nch < 0) { set_error("model_unpack: bad K (%d, at most %d)", K, GOF_MODEL_MAX_K); return GOF_E_INVALID; }
    if (bad_range(P, first, count)) { set_error("model_unpack: rows [%lld, %lld + %lld) do not lie inside a model of %lld", (long long)first, (long long)first, (long long)count, (long long)P); return GOF_E_INVALID; }
    if (pitch < 1 || pitch >= MAX_PITCH) { set_error("model_unpack: bad row pitch (%lld bytes)", (long long)pitch); return GOF_E_INVALID; }
    if (!columns) { set_error("model_unpack: the column table is NULL"); return GOF_E_INVALID; }
    ColTable tab;
    for (int64_t c = 0; c < nch; c++) {
        const GofModelColumn& col = columns[c];
        if (col.type != GOF_PLY_FLOAT32 && col.type != GOF_PLY_FLOAT64) {
            set_error("model_unpack: channel %lld has an integer type (%d): a model channel must be float32 or float64", (long long)c, col.type);
            return GOF_E_INVALID;
        }
        const int64_t size = col.type == GOF_PLY_FLOAT64 ? 8 : 4;
        if (col.offset < 0 || col.offset > pitch - size) {
            set_error("model_unpack: channel %lld (%lld bytes at offset %lld) does not lie inside a row of %lld bytes", (long long)c, (long long)size, (long long)col.offset, (long long)pitch);
            return GOF_E_INVALID;
        }
        tab.w[c] = (uint32_t)col.offset | (col.type == GOF_PLY_FLOAT64 ? 0x80000000u : 0u);
    }
    for (int64_t c = nch; c < MAX_CHANNELS; c++) tab.w[c] = 0u;
    if (count == 0) return GOF_OK;
    if (!rows || !xyz || !f_dc || (K && !f_rest) || !opacity || !scaling || !rotation || !filter_3D) { set_error("model_unpack: a pointer is NULL"); return GOF_E_INVALID; }
    UnpackDst dst;
    float* t[NSEG] = { xyz, f_dc, f_rest, opacity, scaling, rotation, filter_3D };
    for (int s = 0; s < NSEG; s++) dst.t[s] = reinterpret_cast<uint32_t*>(t[s]);
    GOF_PROFILE("model_unpack", stream);
    hipLaunchKernelGGL(model_unpack, dim3((unsigned)((count + TILE_ROWS - 1) / TILE_ROWS)), dim3(THREADS), 0, stream, first, count, (int)K,
                       static_cast<const uint8_t*>(rows), pitch, tab, dst);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // extern "C"
