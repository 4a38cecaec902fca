// mesh_raster.hip -- a triangle rasteriser with a z-buffer and the per-vertex visibility count over it: what the reference's
// eval_tnt/cull_mesh.py asks of pyrender (OpenGL depth render of the mesh from every camera, :17-66) and of torch (Mesher.point_masks,
// :117-175).  Contract: DESIGN.md 3.19, include/gof_mesh_hip.h (e), (f).
//
// Arithmetic: fp64 without contraction in the written order up to the snap to 1/256 pixel, integers from there to the coverage
// decision, fp64 again for the depth of a covered pixel; the z-buffer is an unsigned minimum over float bit patterns (positive floats
// order like their bits), so the image does not depend on the order of the faces.
//
// (e) raster_faces: one thread per (face, view of the batch): transform, clip, snap, fan.  A fan triangle whose box of pixel centres is
//     at most INLINE_MAX pixels wide and high is rasterised by its thread (an extracted mesh at 1920 x 1080: nearly all triangles are
//     below one pixel and cover no centre at all: no memory traffic).  A larger one goes to a list (one atomic on the list's cursor,
//     one 64-byte record); raster_large walks the list: an entry is shared by STRIPES workgroups of 4 waves, a wave takes every 4 *
//     STRIPES-th tile of TILE_W x TILE_H = 64 pixels of the box, a lane one pixel.  No wave ever walks a large box alone.  A full list
//     (more than the capacity the workspace was sized for) makes the thread rasterise its triangle itself: slower, the same bits.
//     A covered pixel first reads the buffer and issues the atomic only if its value is smaller: the buffer only ever decreases, so
//     a stale read can only cost an atomic that changes nothing.
//     raster_faces, raster_large and what they call live in mesh_raster_dev.h, shared with csrc/mesh_render.hip (3.20).
// (f) raster_count: one lane per vertex, a loop over the views of the batch (the record's address is wave-uniform).
#include "mesh_raster_dev.h"

namespace gof {

namespace raster {

// FINAL = false: every pixel of every view's image becomes EMPTY; true: EMPTY becomes 0.0f
template <bool FINAL>
__global__ void __launch_bounds__(256)
raster_images(const GofRasterView* __restrict__ views, int64_t view_stride, uint32_t* __restrict__ depth)
{
    const GofRasterView& V = views[blockIdx.y];
    const int64_t n = (int64_t)V.W * V.H;
    uint32_t* img = depth + (int64_t)blockIdx.y * view_stride;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (!FINAL) img[i] = EMPTY;
        else if (img[i] == EMPTY) img[i] = 0u;
    }
}

__global__ void __launch_bounds__(256)
raster_count(int64_t NV, const float* __restrict__ vertices, int num_views, const GofRasterView* __restrict__ views, int64_t view_stride,
             const float* __restrict__ depth, double eps, int32_t* __restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NV) return;
    const double vx = (double)vertices[3 * i], vy = (double)vertices[3 * i + 1], vz = (double)vertices[3 * i + 2];
    int32_t seen = 0;
    for (int v = 0; v < num_views; v++) {
        const GofRasterView& V = views[v];
        const int W = V.W, H = V.H;
        const double x = ((V.w2c[0] * vx + V.w2c[1] * vy) + V.w2c[2] * vz) + V.w2c[3];
        const double y = ((V.w2c[4] * vx + V.w2c[5] * vy) + V.w2c[6] * vz) + V.w2c[7];
        const double Z = ((V.w2c[8] * vx + V.w2c[9] * vy) + V.w2c[10] * vz) + V.w2c[11];
        const double X = V.fx * x + V.cx * Z, Y = V.fy * y + V.cy * Z;
        const double z = Z + 1e-8;
        const double u = X / z, w = Y / z;
        const double w1 = (double)(W - 1), h1 = (double)(H - 1);
        if (!(u >= 0.0 && u <= w1 && w >= 0.0 && w <= h1 && z > 0.0)) continue;
        const double fx0 = floor(u), fy0 = floor(w);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const double tx = u - fx0, ty = w - fy0;
        const float* img = depth + (int64_t)v * view_stride;
        const double d00 = (double)img[(int64_t)y0 * W + x0], d01 = (double)img[(int64_t)y0 * W + x1];
        const double d10 = (double)img[(int64_t)y1 * W + x0], d11 = (double)img[(int64_t)y1 * W + x1];
        const double ds = ((d00 * ((1.0 - tx) * (1.0 - ty)) + d01 * (tx * (1.0 - ty))) + d10 * ((1.0 - tx) * ty)) + d11 * (tx * ty);
        const bool front = ds > 0.0 ? z < ds + eps : true;
        if (front) seen++;
    }
    count[i] += seen;
}

__global__ void __launch_bounds__(256)
raster_keep(int64_t NV, const int32_t* __restrict__ count, int32_t min_views, uint8_t* __restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < NV) keep[i] = count[i] >= min_views ? 1 : 0;
}

__global__ void __launch_bounds__(256)
raster_zero(int64_t n, int32_t* __restrict__ p)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// fill, rasterise and finish `n` views' images (records views[0 .. n), image v at depth + v * view_stride); checked input
static int render_views(int64_t NV, const float* vertices, int64_t NF, const int32_t* faces, int n, const GofRasterView* views, int64_t view_stride,
                        uint32_t* depth, const RasterWs& w, bool stats, hipStream_t stream)
{
    if (n == 0) return GOF_OK;
    hipLaunchKernelGGL(raster_init_hdr, dim3(1), dim3(64), 0, stream, w.hdr, w.stats, 0);
    hipLaunchKernelGGL(raster_images<false>, dim3(image_blocks(view_stride), n), dim3(256), 0, stream, views, view_stride, depth);
    if (NF) {
        const dim3 grid(grid_of(NF).x, (unsigned)n), lgrid(LARGE_GROUPS * STRIPES);
        if (stats) {
            hipLaunchKernelGGL(raster_faces<M_STATS>, grid, dim3(256), 0, stream, NV, vertices, NF, faces, views, view_stride, depth, w.hdr, w.list, w.cap, w.stats);
            hipLaunchKernelGGL(raster_large<M_STATS>, lgrid, dim3(256), 0, stream, views, view_stride, depth, w.hdr, w.list, w.cap, w.stats);
        } else {
            hipLaunchKernelGGL(raster_faces<0>, grid, dim3(256), 0, stream, NV, vertices, NF, faces, views, view_stride, depth, w.hdr, w.list, w.cap, w.stats);
            hipLaunchKernelGGL(raster_large<0>, lgrid, dim3(256), 0, stream, views, view_stride, depth, w.hdr, w.list, w.cap, w.stats);
        }
    }
    hipLaunchKernelGGL(raster_images<true>, dim3(image_blocks(view_stride), n), dim3(256), 0, stream, views, view_stride, depth);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

} // namespace raster
} // namespace gof

using namespace gof;
using namespace gof::raster;

extern "C" {

int gof_mesh_raster_abi_version(void) { return 3; }

void gof_mesh_raster_tiling(int64_t* out)
{
    if (!out) return;
    out[0] = INLINE_MAX; out[1] = TILE_W; out[2] = TILE_H; out[3] = GUARD_PX; out[4] = MAX_SIDE; out[5] = DEFAULT_BATCH; out[6] = LIST_MIN; out[7] = STRIPES;
}

size_t gof_mesh_render_depth_ws_bytes(int64_t NF) { return raster_layout(NF, 0, nullptr, nullptr); }

int gof_mesh_render_depth(int64_t NV, const float* vertices, int64_t NF, const int32_t* faces, int32_t num_views, const GofRasterView* views,
                          int64_t view_stride, float* depth, int64_t* stats, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NV, RASTER_MAX_COUNT) || bad_count(NF, RASTER_MAX_COUNT / 3)) { set_error("mesh_render_depth: bad counts (%lld vertices, %lld faces; 3 * faces < 2^31)", (long long)NV, (long long)NF); return GOF_E_INVALID; }
    if (num_views < 0 || num_views > 65535 || view_stride < 0) { set_error("mesh_render_depth: bad number of views (%d; at most 65535 per call) / view stride (%lld)", num_views, (long long)view_stride); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_render_depth: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_render_depth_ws_bytes(NF)) { set_error("mesh_render_depth: workspace too small"); return GOF_E_WORKSPACE; }
    if (num_views && (!views || !depth)) { set_error("mesh_render_depth: views / depth is NULL"); return GOF_E_INVALID; }
    if (NF && (!faces || (NV && !vertices))) { set_error("mesh_render_depth: vertices / faces is NULL"); return GOF_E_INVALID; }
    RasterWs w;
    raster_layout(NF, 0, ws_aligned(ws), &w);
    GOF_PROFILE("mesh_render_depth", stream);
    int rc = raster_validate("mesh_render_depth", NV, NF, faces, num_views, views, view_stride, w, true, stream);
    if (rc) return rc;
    rc = render_views(NV, vertices, NF, faces, num_views, views, view_stride, reinterpret_cast<uint32_t*>(depth), w, stats != nullptr, stream);
    if (rc) return rc;
    return stats ? read_stats(w, stats, stream) : GOF_OK;
}

int gof_mesh_visible_count(int64_t NV, const float* vertices, int32_t num_views, const GofRasterView* views, int64_t view_stride, const float* depth,
                           double eps, int32_t* count, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_count(NV, RASTER_MAX_COUNT)) { set_error("mesh_visible_count: bad number of vertices (%lld)", (long long)NV); return GOF_E_INVALID; }
    if (num_views < 0 || view_stride < 0) { set_error("mesh_visible_count: bad number of views (%d) / view stride (%lld)", num_views, (long long)view_stride); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_visible_count: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_render_depth_ws_bytes(0)) { set_error("mesh_visible_count: workspace too small"); return GOF_E_WORKSPACE; }
    if (num_views && (!views || !depth)) { set_error("mesh_visible_count: views / depth is NULL"); return GOF_E_INVALID; }
    if (NV && (!vertices || !count)) { set_error("mesh_visible_count: vertices / count is NULL"); return GOF_E_INVALID; }
    RasterWs w;
    raster_layout(0, 0, ws_aligned(ws), &w);
    GOF_PROFILE("mesh_visible_count", stream);
    const int rc = raster_validate("mesh_visible_count", NV, 0, nullptr, num_views, views, view_stride, w, false, stream);
    if (rc) return rc;
    if (NV && num_views) hipLaunchKernelGGL(raster_count, grid_of(NV), dim3(256), 0, stream, NV, vertices, (int)num_views, views, view_stride, depth, eps, count);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

static int visibility_batch(int32_t batch) { return batch == 0 ? DEFAULT_BATCH : batch; }

size_t gof_mesh_visibility_ws_bytes(int64_t NF, int64_t view_stride, int32_t batch)
{
    const int b = visibility_batch(batch);
    if (b < 1 || b > MAX_BATCH || view_stride < 0 || view_stride > (int64_t)MAX_SIDE * MAX_SIDE) return 0;
    return raster_layout(NF, view_stride * b, nullptr, nullptr);
}

int gof_mesh_visibility(int64_t NV, const float* vertices, int64_t NF, const int32_t* faces, int32_t num_views, const GofRasterView* views,
                        int64_t view_stride, int32_t batch, double eps, int32_t min_views, int32_t* count, uint8_t* keep, int64_t* stats,
                        void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int b = visibility_batch(batch);
    if (bad_count(NV, RASTER_MAX_COUNT) || bad_count(NF, RASTER_MAX_COUNT / 3)) { set_error("mesh_visibility: bad counts (%lld vertices, %lld faces; 3 * faces < 2^31)", (long long)NV, (long long)NF); return GOF_E_INVALID; }
    if (num_views < 0 || b < 1 || b > MAX_BATCH || view_stride < 0 || view_stride > (int64_t)MAX_SIDE * MAX_SIDE) {
        set_error("mesh_visibility: bad number of views (%d) / batch (%d; 1 .. %d) / view stride (%lld)", num_views, batch, MAX_BATCH, (long long)view_stride);
        return GOF_E_INVALID;
    }
    if (!ws) { set_error("mesh_visibility: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_visibility_ws_bytes(NF, view_stride, batch)) { set_error("mesh_visibility: workspace too small"); return GOF_E_WORKSPACE; }
    if (num_views && !views) { set_error("mesh_visibility: views is NULL"); return GOF_E_INVALID; }
    if (NF && (!faces || (NV && !vertices))) { set_error("mesh_visibility: vertices / faces is NULL"); return GOF_E_INVALID; }
    if (NV && (!vertices || !count || !keep)) { set_error("mesh_visibility: vertices / count / keep is NULL"); return GOF_E_INVALID; }
    RasterWs w;
    raster_layout(NF, view_stride * b, ws_aligned(ws), &w);
    GOF_PROFILE("mesh_visibility", stream);
    int rc = raster_validate("mesh_visibility", NV, NF, faces, num_views, views, view_stride, w, true, stream);
    if (rc) return rc;
    if (NV) hipLaunchKernelGGL(raster_zero, grid_of(NV), dim3(256), 0, stream, NV, count);
    for (int v0 = 0; v0 < num_views; v0 += b) {
        const int n = num_views - v0 < b ? num_views - v0 : b;
        rc = render_views(NV, vertices, NF, faces, n, views + v0, view_stride, w.depth, w, stats != nullptr, stream);
        if (rc) return rc;
        if (NV) hipLaunchKernelGGL(raster_count, grid_of(NV), dim3(256), 0, stream, NV, vertices, n, views + v0, view_stride, reinterpret_cast<const float*>(w.depth), eps, count);
    }
    if (NV) hipLaunchKernelGGL(raster_keep, grid_of(NV), dim3(256), 0, stream, NV, count, min_views, keep);
    GOF_LAUNCH_CHECK(stream, 0);
    return stats ? read_stats(w, stats, stream) : GOF_OK;
}

} // extern "C"
