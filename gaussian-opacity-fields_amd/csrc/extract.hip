// extract.hip -- the mesh extraction's own steps (replaces what the reference's extract_mesh.py:36-120 and
// scene/gaussian_model.py:31-72, 433-463 ask of torch einsums, boolean-mask assignments and trimesh): (a) the tetra points -- 9
// candidates per Gaussian tested against every view, the seen ones compacted in order, (b) one round of the bisection in one launch,
// (c) the edge length filter.  Contract: DESIGN.md 3.11, include/gof_extract_hip.h.
//
// Arithmetic: compiled with -ffp-contract=off like the whole library and no fma() is written here; the point values are fp32 and the
// keep decisions fp64, every operation the IEEE operation numpy performs on the host, in the order written.
//
// (a) one lane per candidate, the loop over the views leaves at the first view that sees the candidate; the view record's address is
//     wave-uniform (scalar loads).  Flags -> the library's scan -> a second pass that recomputes the point and writes it to its rank:
//     no buffer of views x points, 4 bytes of workspace per candidate besides the scan's scratch.
// (b), (c) elementwise, one lane per edge.
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gof_hip.h"
#include "../../include/gof_extract_hip.h"
#include "gof_common.h"
#include "radix.h"
#include "gof_geom.h"

namespace gof {

namespace extract {

// the scan runs over 9 P + 1 flags, and that count stays below 2^31
constexpr int64_t MAX_GAUSSIANS = (((int64_t)1 << 31) - 2) / 9;

// candidate i of 9 P -> its point and scale (fp32, in the order of DESIGN.md 3.11)
__device__ __forceinline__ void candidate(int64_t i, int64_t P, const float* __restrict__ xyz, const float* __restrict__ scaling,
                                          const float* __restrict__ rotation, float p[3], float& scale)
{
    const bool corner = i < 8 * P;
    const int64_t g = corner ? i / 8 : i - 8 * P;
    const float s0 = scaling[3 * g] * 3.0f, s1 = scaling[3 * g + 1] * 3.0f, s2 = scaling[3 * g + 2] * 3.0f;
    scale = s0;                                                              // the maximum as torch / numpy take it: a NaN stays
    scale = (s1 > scale || s1 != s1) ? s1 : scale;
    scale = (s2 > scale || s2 != s2) ? s2 : scale;
    const float c0 = xyz[3 * g], c1 = xyz[3 * g + 1], c2 = xyz[3 * g + 2];
    if (!corner) { p[0] = c0; p[1] = c1; p[2] = c2; return; }
    const float q0 = rotation[4 * g], q1 = rotation[4 * g + 1], q2 = rotation[4 * g + 2], q3 = rotation[4 * g + 3];
    const float n = sqrtf(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const float r = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
    const int c = (int)(i & 7);
    const float a0 = (c & 4) ? s0 : -s0, a1 = (c & 2) ? s1 : -s1, a2 = (c & 1) ? s2 : -s2;
    const float R00 = 1.0f - 2.0f * (y * y + z * z), R01 = 2.0f * (x * y - r * z), R02 = 2.0f * (x * z + r * y);
    const float R10 = 2.0f * (x * y + r * z), R11 = 1.0f - 2.0f * (x * x + z * z), R12 = 2.0f * (y * z - r * x);
    const float R20 = 2.0f * (x * z - r * y), R21 = 2.0f * (y * z + r * x), R22 = 1.0f - 2.0f * (x * x + y * y);
    p[0] = ((R00 * a0 + R01 * a1) + R02 * a2) + c0;
    p[1] = ((R10 * a0 + R11 * a1) + R12 * a2) + c1;
    p[2] = ((R20 * a0 + R21 * a1) + R22 * a2) + c2;
}

// flags[i] = some view sees candidate i; flags[N] = 0 (the exclusive scan's last word = the total)
__global__ void __launch_bounds__(256)
tetra_flags(int64_t P, const float* __restrict__ xyz, const float* __restrict__ scaling, const float* __restrict__ rotation, int num_views,
            const GofFrustumView* __restrict__ views, double cx, double cy, double umax, double vmax, double near_plane, double far_plane,
            uint32_t* __restrict__ flags)
{
    const int64_t N = 9 * P;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    if (i == N) { flags[i] = 0u; return; }
    float p[3], scale;
    candidate(i, P, xyz, scaling, rotation, p, scale);
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
    bool seen = false;
    for (int v = 0; v < num_views && !seen; v++) {
        const GofFrustumView& V = views[v];
        const double X = ((V.m[0] * px + V.m[1] * py) + V.m[2] * pz) + V.m[3];
        const double Y = ((V.m[4] * px + V.m[5] * py) + V.m[6] * pz) + V.m[7];
        const double Z = ((V.m[8] * px + V.m[9] * py) + V.m[10] * pz) + V.m[11];
        const double u = (V.fx * X + cx * Z) / Z;
        const double w = (V.fy * Y + cy * Z) / Z;
        seen = Z >= near_plane && Z <= far_plane && u >= 0.0 && u <= umax && w >= 0.0 && w <= vmax;
    }
    flags[i] = seen ? 1u : 0u;
}

// pos = exclusive scan of the flags over N + 1 words: candidate i is written iff pos[i + 1] > pos[i], to row pos[i] (< count)
__global__ void __launch_bounds__(256)
tetra_emit(int64_t P, const float* __restrict__ xyz, const float* __restrict__ scaling, const float* __restrict__ rotation,
           const uint32_t* __restrict__ pos, int64_t count, float* __restrict__ out_points, float* __restrict__ out_scales)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * P) return;
    const int64_t r = pos[i];
    if (pos[i + 1] == (uint32_t)r || r >= count) return;
    float p[3], scale;
    candidate(i, P, xyz, scaling, rotation, p, scale);
    out_points[3 * r] = p[0];
    out_points[3 * r + 1] = p[1];
    out_points[3 * r + 2] = p[2];
    out_scales[r] = scale;
}

__global__ void __launch_bounds__(256)
bisect_step(int64_t E, float* __restrict__ left_pts, float* __restrict__ right_pts, float* __restrict__ left_sdf, float* __restrict__ right_sdf,
            const float* __restrict__ value, int mode, float* __restrict__ mid_out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float l[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { l[k] = left_pts[3 * e + k]; r[k] = right_pts[3 * e + k]; }
    if (mode != GOF_BISECT_FIRST) {
        const float alpha = mode == GOF_BISECT_ALPHA ? value[e] : 1.0f - value[e];
        float mid_sdf = alpha - 0.5f;
        if (mid_sdf != mid_sdf) mid_sdf = __uint_as_float(0x7FC00000u);      // a NaN result's sign and payload are open in IEEE 754 (and to the compiler): the canonical NaN is stored
        const float ls = left_sdf[e];
        const bool low = (mid_sdf < 0.0f && ls < 0.0f) || (mid_sdf > 0.0f && ls > 0.0f);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float mid = (l[k] + r[k]) / 2.0f;
            if (low) { l[k] = mid; left_pts[3 * e + k] = mid; }
            else { r[k] = mid; right_pts[3 * e + k] = mid; }
        }
        if (low) left_sdf[e] = mid_sdf;
        else right_sdf[e] = mid_sdf;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) mid_out[3 * e + k] = (l[k] + r[k]) / 2.0f;
}

__global__ void __launch_bounds__(256)
edge_filter(int64_t E, const float* __restrict__ end_points, const float* __restrict__ end_scales, uint8_t* __restrict__ keep)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float* a = end_points + 6 * e;
    const float dx = a[0] - a[3], dy = a[1] - a[4], dz = a[2] - a[5];
    const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
    keep[e] = d <= end_scales[2 * e] + end_scales[2 * e + 1] ? 1 : 0;
}

struct TetraWs { uint32_t* flags; uint32_t* tmp; };
static size_t tetra_layout(int64_t P, void* base, TetraWs* out)
{
    const size_t n = (size_t)(P < 0 ? 0 : P) * 9 + 1;
    Carver c{ static_cast<char*>(base), 0 };
    TetraWs w;
    w.flags = c.take<uint32_t>(n);
    w.tmp = c.take<uint32_t>(scan_tmp_words(n));
    if (out) *out = w;
    return c.total();
}

} // namespace extract
} // namespace gof

using namespace gof;
using namespace gof::extract;

extern "C" {

size_t gof_tetra_points_ws_bytes(int64_t P) { return tetra_layout(P > MAX_GAUSSIANS ? 0 : P, nullptr, nullptr); }

int gof_tetra_points_count(int64_t P, const float* xyz, const float* scaling, const float* rotation, int32_t num_views, const GofFrustumView* views,
                           int32_t W, int32_t H, double near_plane, double far_plane, void* ws, size_t ws_bytes, int64_t* count, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!count) { set_error("tetra_points_count: count is NULL"); return GOF_E_INVALID; }
    *count = 0;
    if (bad_count(P, MAX_GAUSSIANS + 1)) { set_error("tetra_points_count: bad number of Gaussians (%lld)", (long long)P); return GOF_E_INVALID; }
    if (num_views < 0) { set_error("tetra_points_count: bad number of views (%d)", num_views); return GOF_E_INVALID; }
    if (num_views && !views) { set_error("tetra_points_count: views is NULL"); return GOF_E_INVALID; }
    if (num_views && (W < 1 || H < 1)) { set_error("tetra_points_count: bad image size (%d x %d)", W, H); return GOF_E_INVALID; }
    if (!ws) { set_error("tetra_points_count: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_tetra_points_ws_bytes(P)) { set_error("tetra_points_count: workspace too small"); return GOF_E_WORKSPACE; }
    if (P && (!xyz || !scaling || !rotation)) { set_error("tetra_points_count: xyz / scaling / rotation is NULL"); return GOF_E_INVALID; }
    TetraWs w;
    tetra_layout(P, ws_aligned(ws), &w);
    const int64_t N = 9 * P;
    const double cx = (double)(float)((double)W / 2.0), cy = (double)(float)((double)H / 2.0);
    GOF_PROFILE("tetra_points_count", stream);
    hipLaunchKernelGGL(tetra_flags, grid_of(N + 1), dim3(256), 0, stream, P, xyz, scaling, rotation, (int)num_views, views, cx, cy,
                       (double)(W - 1), (double)(H - 1), near_plane, far_plane, w.flags);
    GOF_LAUNCH_CHECK(stream, 0);
    GOF_HIP_CHECK(device_scan_u32(w.flags, nullptr, w.flags, (size_t)N + 1, false, w.tmp, nullptr, stream));
    uint32_t total = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&total, w.flags + N, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    *count = total;
    return GOF_OK;
}

int gof_tetra_points_emit(int64_t P, const float* xyz, const float* scaling, const float* rotation, const void* ws, size_t ws_bytes, int64_t count,
                          float* out_points, float* out_scales, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(P, MAX_GAUSSIANS + 1)) { set_error("tetra_points_emit: bad number of Gaussians (%lld)", (long long)P); return GOF_E_INVALID; }
    if (count < 0 || count > 9 * P) { set_error("tetra_points_emit: bad count (%lld of %lld candidates)", (long long)count, (long long)(9 * P)); return GOF_E_INVALID; }
    if (!ws) { set_error("tetra_points_emit: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_tetra_points_ws_bytes(P)) { set_error("tetra_points_emit: workspace too small"); return GOF_E_WORKSPACE; }
    if (P && (!xyz || !scaling || !rotation)) { set_error("tetra_points_emit: xyz / scaling / rotation is NULL"); return GOF_E_INVALID; }
    if (count && (!out_points || !out_scales)) { set_error("tetra_points_emit: out_points / out_scales is NULL"); return GOF_E_INVALID; }
    TetraWs w;
    tetra_layout(P, const_cast<void*>(ws_aligned(ws)), &w);
    const int64_t N = 9 * P;
    uint32_t total = 0;
    GOF_HIP_CHECK(hipMemcpyAsync(&total, w.flags + N, 4, hipMemcpyDeviceToHost, stream));
    GOF_HIP_CHECK(hipStreamSynchronize(stream));
    if ((int64_t)total != count) { set_error("tetra_points_emit: count is %lld, the workspace holds %u (not the workspace of gof_tetra_points_count?)", (long long)count, total); return GOF_E_INVALID; }
    if (count == 0) return GOF_OK;
    GOF_PROFILE("tetra_points_emit", stream);
    hipLaunchKernelGGL(tetra_emit, grid_of(N), dim3(256), 0, stream, P, xyz, scaling, rotation, w.flags, count, out_points, out_scales);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_bisect_step(int64_t E, float* left_pts, float* right_pts, float* left_sdf, float* right_sdf, const float* value, int32_t mode,
                    float* mid_out, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(E)) { set_error("bisect_step: bad number of edges (%lld)", (long long)E); return GOF_E_INVALID; }
    if (mode != GOF_BISECT_FINAL_ALPHA && mode != GOF_BISECT_FIRST && mode != GOF_BISECT_ALPHA) { set_error("bisect_step: bad mode (%d)", mode); return GOF_E_INVALID; }
    if (E == 0) return GOF_OK;
    if (!left_pts || !right_pts || !mid_out) { set_error("bisect_step: left_pts / right_pts / mid_out is NULL"); return GOF_E_INVALID; }
    if (mode != GOF_BISECT_FIRST && (!left_sdf || !right_sdf || !value)) { set_error("bisect_step: left_sdf / right_sdf / value is NULL"); return GOF_E_INVALID; }
    GOF_PROFILE("bisect_step", stream);
    hipLaunchKernelGGL(bisect_step, grid_of(E), dim3(256), 0, stream, E, left_pts, right_pts, left_sdf, right_sdf, value, (int)mode, mid_out);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

int gof_edge_filter(int64_t E, const float* end_points, const float* end_scales, uint8_t* keep, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(E)) { set_error("edge_filter: bad number of edges (%lld)", (long long)E); return GOF_E_INVALID; }
    if (E == 0) return GOF_OK;
    if (!end_points || !end_scales || !keep) { set_error("edge_filter: end_points / end_scales / keep is NULL"); return GOF_E_INVALID; }
    GOF_PROFILE("edge_filter", stream);
    hipLaunchKernelGGL(edge_filter, grid_of(E), dim3(256), 0, stream, E, end_points, end_scales, keep);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // extern "C"
