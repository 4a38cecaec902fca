// mesh_render.hip -- pictures of the surface: area-weighted vertex normals, a face buffer beside the depth image, and the pass that
// resolves the two into normal-shaded, coloured or lit images: what the reference's mesh_viewer.py asks of Open3D
// (compute_vertex_normals, :48) and of an OpenGL window.  Contract: DESIGN.md 3.20, include/gof_mesh_hip.h (g).
//
// Arithmetic: IEEE fp64 without contraction in the written order, integers for coverage (mesh_raster_dev.h); the z-buffer is an
// unsigned 64-bit minimum over (depth bits << 32) | face, so neither image depends on the order of the faces.
//
// (g1) vn_corners counts the corners per vertex (integer atomics) and writes the (vertex, corner) pairs and the fp64 face vectors;
//      device_scan_u32 turns the counts into segment starts; the stable radix sort by vertex leaves every segment in ascending corner
//      order; vn_walk: one lane per vertex adds its segment's face vectors one by one.  No floating-point atomics.
// (g2) raster_faces / raster_large of mesh_raster_dev.h with the 64-bit pixel word; faces_images fills the words and splits them.
// (g3) shade_pixels: one lane per pixel of the batch.
#include "mesh_raster_dev.h"
#include "radix.h"

namespace gof {
namespace raster {

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 cross3(const D3& a, const D3& b) { return D3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double dot3(const D3& u, const D3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ D3 unit3(const D3& n)
{
    const double len = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
    if (!(len > 0.0 && len <= DBL_MAX)) return D3{ 0.0, 0.0, 1.0 };
    return D3{ n.x / len, n.y / len, n.z / len };
}
__device__ __forceinline__ D3 vertex3(const float* __restrict__ vertices, int64_t v)
{
    return D3{ (double)vertices[3 * v], (double)vertices[3 * v + 1], (double)vertices[3 * v + 2] };
}
// Nf = cross(v1 - v0, v2 - v0) of face f (indices checked before)
__device__ __forceinline__ D3 face_vector(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t f)
{
    const D3 v0 = vertex3(vertices, faces[3 * f]), v1 = vertex3(vertices, faces[3 * f + 1]), v2 = vertex3(vertices, faces[3 * f + 2]);
    return cross3(D3{ v1.x - v0.x, v1.y - v0.y, v1.z - v0.z }, D3{ v2.x - v0.x, v2.y - v0.y, v2.z - v0.z });
}

// ---- (g1) ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vn_zero(int64_t n, uint32_t* __restrict__ p)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

__global__ void __launch_bounds__(256)
vn_corners(int64_t NF, const float* __restrict__ vertices, const int32_t* __restrict__ faces, uint32_t* __restrict__ count, uint32_t* __restrict__ keys,
           uint32_t* __restrict__ vals, double* __restrict__ fvec)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const D3 n = face_vector(vertices, faces, f);
    fvec[3 * f] = n.x; fvec[3 * f + 1] = n.y; fvec[3 * f + 2] = n.z;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint32_t v = (uint32_t)faces[3 * f + k];
        keys[3 * f + k] = v;
        vals[3 * f + k] = (uint32_t)(3 * f + k);
        atomicAdd(&count[v], 1u);
    }
}

__global__ void __launch_bounds__(256)
vn_walk(int64_t NV, const uint32_t* __restrict__ start, const uint32_t* __restrict__ corner, const double* __restrict__ fvec, float* __restrict__ normals)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= NV) return;
    D3 s = { 0.0, 0.0, 0.0 };
    for (uint32_t p = start[v], e = start[v + 1]; p < e; p++) {
        const uint32_t f = corner[p] / 3u;
        s.x = s.x + fvec[3 * (size_t)f]; s.y = s.y + fvec[3 * (size_t)f + 1]; s.z = s.z + fvec[3 * (size_t)f + 2];
    }
    const D3 n = unit3(s);
    normals[3 * v] = (float)n.x; normals[3 * v + 1] = (float)n.y; normals[3 * v + 2] = (float)n.z;
}

__global__ void __launch_bounds__(256)
fn_faces(int64_t NF, const float* __restrict__ vertices, const int32_t* __restrict__ faces, float* __restrict__ normals)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= NF) return;
    const D3 n = unit3(face_vector(vertices, faces, f));
    normals[3 * f] = (float)n.x; normals[3 * f + 1] = (float)n.y; normals[3 * f + 2] = (float)n.z;
}

struct NormalsWs { uint32_t* hdr; uint32_t* start; uint32_t* keys[2]; uint32_t* vals[2]; double* fvec; uint32_t* tmp; };
static size_t normals_layout(int64_t NV, int64_t NF, void* base, NormalsWs* out)
{
    const size_t nv = (size_t)(NV < 0 ? 0 : NV), nc = 3 * (size_t)(NF < 0 ? 0 : NF);
    Carver c{ static_cast<char*>(base), 0 };
    NormalsWs w;
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    w.start = c.take<uint32_t>(nv + 1);
    for (int k = 0; k < 2; k++) { w.keys[k] = c.take<uint32_t>(nc); w.vals[k] = c.take<uint32_t>(nc); }
    w.fvec = c.take<double>(nc);
    const size_t a = scan_tmp_words(nv + 1), b = rs_tmp_words(nc);
    w.tmp = c.take<uint32_t>(a > b ? a : b);
    if (out) *out = w;
    return c.total();
}

// the header alone: what an entry point needs for raster_validate
static size_t header_layout(void* base, RasterWs* out)
{
    Carver c{ static_cast<char*>(base), 0 };
    RasterWs w{};
    w.hdr = c.take<uint32_t>(HDR_WORDS);
    if (out) *out = w;
    return c.total();
}

// ---- (g2) ------------------------------------------------------------------------------------------------------------------------------
// FINAL = false: every pixel word of every view becomes EMPTY64; true: the words are split into depth (EMPTY64 -> 0.0f) and face (-> -1)
template <bool FINAL>
__global__ void __launch_bounds__(256)
faces_images(const GofRasterView* __restrict__ views, int64_t view_stride, u64* __restrict__ pix, uint32_t* __restrict__ depth, int32_t* __restrict__ face)
{
    const GofRasterView& V = views[blockIdx.y];
    const int64_t n = (int64_t)V.W * V.H, off = (int64_t)blockIdx.y * view_stride;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (!FINAL) pix[off + i] = EMPTY64;
        else {
            const u64 w = pix[off + i];
            depth[off + i] = w == EMPTY64 ? 0u : (uint32_t)(w >> 32);
            face[off + i] = w == EMPTY64 ? -1 : (int32_t)(uint32_t)w;
        }
    }
}

struct FacesWs { RasterWs r; u64* pix; };
static size_t faces_layout(int64_t NF, int64_t pixels, void* base, FacesWs* out)
{
    Carver c{ static_cast<char*>(base), 0 };
    FacesWs w{};
    char* sub = c.take<char>(raster_layout(NF, 0, nullptr, nullptr));
    if (base) raster_layout(NF, 0, ws_aligned(sub), &w.r);
    w.pix = c.take<u64>((size_t)(pixels < 0 ? 0 : pixels));
    if (out) *out = w;
    return c.total();
}

// ---- (g3) ------------------------------------------------------------------------------------------------------------------------------
struct ShadeArgs {
    const float* vertices; const int32_t* faces; const float* normals; const uint8_t* colors; const GofRasterView* views; const int32_t* face;
    float* image; float* bary;
    int64_t NF, view_stride;
    GofShadeParams p;
};

__device__ __forceinline__ double sum3(const double l[3], double q0, double q1, double q2) { return (l[0] * q0 + l[1] * q1) + l[2] * q2; }

__global__ void __launch_bounds__(256)
shade_pixels(ShadeArgs A)
{
    const int view = (int)blockIdx.y;
    const GofRasterView& V = A.views[view];
    const int W = V.W, H = V.H;
    const int64_t n = (int64_t)W * H, off = (int64_t)view * A.view_stride;
    float* img = A.image + 3 * off;
    float* bar = A.bary ? A.bary + 3 * off : nullptr;
    const int mode = A.p.mode;
    const bool flat = (A.p.flags & GOF_SHADE_FLAT) != 0, vbase = (A.p.flags & GOF_SHADE_VERTEX_BASE) != 0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
        const int64_t f = A.face[off + q];
        if (f < 0 || f >= A.NF) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                img[c * A.view_stride + q] = (float)A.p.background[c];
                if (bar) bar[c * A.view_stride + q] = 0.0f;
            }
            continue;
        }
        const int i = (int)(q % W), j = (int)(q / W);
        const int64_t vi[3] = { A.faces[3 * f], A.faces[3 * f + 1], A.faces[3 * f + 2] };
        D3 cam[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const D3 v = vertex3(A.vertices, vi[k]);
            cam[k].x = ((V.w2c[0] * v.x + V.w2c[1] * v.y) + V.w2c[2] * v.z) + V.w2c[3];
            cam[k].y = ((V.w2c[4] * v.x + V.w2c[5] * v.y) + V.w2c[6] * v.z) + V.w2c[7];
            cam[k].z = ((V.w2c[8] * v.x + V.w2c[9] * v.y) + V.w2c[10] * v.z) + V.w2c[11];
        }
        const D3 d = { (((double)i + 0.5) - V.cx) / V.fx, (((double)j + 0.5) - V.cy) / V.fy, 1.0 };
        const double m0 = dot3(d, cross3(cam[1], cam[2])), m1 = dot3(d, cross3(cam[2], cam[0])), m2 = dot3(d, cross3(cam[0], cam[1]));
        const double s = (m0 + m1) + m2;
        double l[3] = { m0 / s, m1 / s, m2 / s };
#pragma unroll
        for (int k = 0; k < 3; k++) l[k] = !(l[k] >= 0.0) ? 0.0 : (l[k] > 1.0 ? 1.0 : l[k]);      // (NaN and negatives: 0)
        const double t = (l[0] + l[1]) + l[2];
        if (t > 0.0) { l[0] = l[0] / t; l[1] = l[1] / t; l[2] = l[2] / t; }
        else l[0] = l[1] = l[2] = 1.0 / 3.0;
        if (bar) {
#pragma unroll
            for (int c = 0; c < 3; c++) bar[c * A.view_stride + q] = (float)l[c];
        }
        double out[3];
        double col[3] = { 0.0, 0.0, 0.0 };
        if (mode == GOF_SHADE_COLOR || (mode == GOF_SHADE_SHADED && vbase)) {
#pragma unroll
            for (int c = 0; c < 3; c++)
                col[c] = sum3(l, (double)A.colors[4 * vi[0] + c], (double)A.colors[4 * vi[1] + c], (double)A.colors[4 * vi[2] + c]) / 255.0;
        }
        if (mode == GOF_SHADE_COLOR) { out[0] = col[0]; out[1] = col[1]; out[2] = col[2]; }
        else {
            D3 nw;
            if (flat) nw = face_vector(A.vertices, A.faces, f);
            else {
                const float* N = A.normals;
                nw.x = sum3(l, (double)N[3 * vi[0]], (double)N[3 * vi[1]], (double)N[3 * vi[2]]);
                nw.y = sum3(l, (double)N[3 * vi[0] + 1], (double)N[3 * vi[1] + 1], (double)N[3 * vi[2] + 1]);
                nw.z = sum3(l, (double)N[3 * vi[0] + 2], (double)N[3 * vi[1] + 2], (double)N[3 * vi[2] + 2]);
            }
            const D3 nu = unit3(nw);
            if (mode == GOF_SHADE_NORMAL_WORLD) { out[0] = (nu.x + 1.0) / 2.0; out[1] = (nu.y + 1.0) / 2.0; out[2] = (nu.z + 1.0) / 2.0; }
            else {
                const D3 nc = { (V.w2c[0] * nu.x + V.w2c[1] * nu.y) + V.w2c[2] * nu.z, (V.w2c[4] * nu.x + V.w2c[5] * nu.y) + V.w2c[6] * nu.z,
                                (V.w2c[8] * nu.x + V.w2c[9] * nu.y) + V.w2c[10] * nu.z };
                if (mode == GOF_SHADE_NORMAL_CAMERA) { out[0] = (nc.x + 1.0) / 2.0; out[1] = (nc.y + 1.0) / 2.0; out[2] = (nc.z + 1.0) / 2.0; }
                else {
                    const D3 p = { sum3(l, cam[0].x, cam[1].x, cam[2].x), sum3(l, cam[0].y, cam[1].y, cam[2].y), sum3(l, cam[0].z, cam[1].z, cam[2].z) };
                    const D3 v = unit3(D3{ -p.x, -p.y, -p.z });
                    const double lit = fabs(dot3(nc, v));
                    const double k = A.p.ambient + (1.0 - A.p.ambient) * lit;
#pragma unroll
                    for (int c = 0; c < 3; c++) out[c] = (vbase ? col[c] : A.p.base[c]) * k;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; c++) img[c * A.view_stride + q] = (float)out[c];
    }
}

static bool bad_views(const char* who, int32_t num_views, int64_t view_stride)
{
    if (num_views < 0 || num_views > 65535 || view_stride < 0 || view_stride > (int64_t)MAX_SIDE * MAX_SIDE) {
        set_error("%s: bad number of views (%d; at most 65535 per call) / view stride (%lld)", who, num_views, (long long)view_stride);
        return true;
    }
    return false;
}
static bool bad_mesh(const char* who, int64_t NV, int64_t NF)
{
    if (bad_count(NV, RASTER_MAX_COUNT) || bad_count(NF, RASTER_MAX_COUNT / 3)) {
        set_error("%s: bad counts (%lld vertices, %lld faces; 3 * faces < 2^31)", who, (long long)NV, (long long)NF);
        return true;
    }
    return false;
}

} // namespace raster
} // namespace gof

using namespace gof;
using namespace gof::raster;

extern "C" {

int gof_mesh_render_abi_version(void) { return 4; }

size_t gof_mesh_vertex_normals_ws_bytes(int64_t NV, int64_t NF) { return normals_layout(NV, NF, nullptr, nullptr); }

int gof_mesh_vertex_normals(int64_t NV, const float* vertices, int64_t NF, const int32_t* faces, float* normals, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_mesh("mesh_vertex_normals", NV, NF)) return GOF_E_INVALID;
    if (!ws) { set_error("mesh_vertex_normals: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_vertex_normals_ws_bytes(NV, NF)) { set_error("mesh_vertex_normals: workspace too small"); return GOF_E_WORKSPACE; }
    if ((NF && (!faces || !vertices)) || (NV && (!vertices || !normals))) { set_error("mesh_vertex_normals: vertices / faces / normals is NULL"); return GOF_E_INVALID; }
    NormalsWs w;
    normals_layout(NV, NF, ws_aligned(ws), &w);
    GOF_PROFILE("mesh_vertex_normals", stream);
    RasterWs h{};
    h.hdr = w.hdr;
    const int rc = raster_validate("mesh_vertex_normals", NV, NF, faces, 0, nullptr, 0, h, false, stream);
    if (rc) return rc;
    if (NV == 0) return GOF_OK;
    const size_t nc = 3 * (size_t)NF;
    hipLaunchKernelGGL(vn_zero, grid_of(NV + 1), dim3(256), 0, stream, NV + 1, w.start);
    uint32_t *keys = w.keys[0], *corner = w.vals[0];
    if (NF) {
        hipLaunchKernelGGL(vn_corners, grid_of(NF), dim3(256), 0, stream, NF, vertices, faces, w.start, w.keys[0], w.vals[0], w.fvec);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    GOF_HIP_CHECK(device_scan_u32(w.start, nullptr, w.start, (size_t)NV + 1, false, w.tmp, nullptr, stream));
    if (NF) {
        int bits = 0;
        while (bits < 31 && ((int64_t)1 << bits) < NV) bits++;
        GOF_HIP_CHECK(radix_sort_pairs_u32(w.keys[0], w.vals[0], w.keys[1], w.vals[1], nc, bits, w.tmp, &keys, &corner, stream, nullptr));
    }
    hipLaunchKernelGGL(vn_walk, grid_of(NV), dim3(256), 0, stream, NV, w.start, corner, w.fvec, normals);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

size_t gof_mesh_face_normals_ws_bytes(void) { return header_layout(nullptr, nullptr); }

int gof_mesh_face_normals(int64_t NV, const float* vertices, int64_t NF, const int32_t* faces, float* normals, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_mesh("mesh_face_normals", NV, NF)) return GOF_E_INVALID;
    if (!ws) { set_error("mesh_face_normals: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_face_normals_ws_bytes()) { set_error("mesh_face_normals: workspace too small"); return GOF_E_WORKSPACE; }
    if (NF && (!faces || !vertices || !normals)) { set_error("mesh_face_normals: vertices / faces / normals is NULL"); return GOF_E_INVALID; }
    RasterWs h;
    header_layout(ws_aligned(ws), &h);
    GOF_PROFILE("mesh_face_normals", stream);
    const int rc = raster_validate("mesh_face_normals", NV, NF, faces, 0, nullptr, 0, h, false, stream);
    if (rc) return rc;
    if (NF) hipLaunchKernelGGL(fn_faces, grid_of(NF), dim3(256), 0, stream, NF, vertices, faces, normals);
    GOF_LAUNCH_CHECK(stream, 0);
    return GOF_OK;
}

size_t gof_mesh_render_faces_ws_bytes(int64_t NF, int32_t num_views, int64_t view_stride)
{
    if (num_views < 0 || num_views > 65535 || view_stride < 0 || view_stride > (int64_t)MAX_SIDE * MAX_SIDE) return 0;
    return faces_layout(NF, (int64_t)num_views * view_stride, nullptr, nullptr);
}

int gof_mesh_render_faces(int64_t NV, const float* vertices, int64_t NF, const int32_t* faces, int32_t num_views, const GofRasterView* views,
                          int64_t view_stride, float* depth, int32_t* face, int64_t* stats, void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_mesh("mesh_render_faces", NV, NF) || bad_views("mesh_render_faces", num_views, view_stride)) return GOF_E_INVALID;
    if (!ws) { set_error("mesh_render_faces: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_render_faces_ws_bytes(NF, num_views, view_stride)) { set_error("mesh_render_faces: workspace too small"); return GOF_E_WORKSPACE; }
    if (num_views && (!views || !depth || !face)) { set_error("mesh_render_faces: views / depth / face is NULL"); return GOF_E_INVALID; }
    if (NF && (!faces || (NV && !vertices))) { set_error("mesh_render_faces: vertices / faces is NULL"); return GOF_E_INVALID; }
    FacesWs w;
    faces_layout(NF, (int64_t)num_views * view_stride, ws_aligned(ws), &w);
    GOF_PROFILE("mesh_render_faces", stream);
    const int rc = raster_validate("mesh_render_faces", NV, NF, faces, num_views, views, view_stride, w.r, true, stream);
    if (rc) return rc;
    if (num_views) {
        const int n = num_views;
        const dim3 igrid(image_blocks(view_stride), n);
        hipLaunchKernelGGL(raster_init_hdr, dim3(1), dim3(64), 0, stream, w.r.hdr, w.r.stats, 0);
        hipLaunchKernelGGL(faces_images<false>, igrid, dim3(256), 0, stream, views, view_stride, w.pix, static_cast<uint32_t*>(nullptr), static_cast<int32_t*>(nullptr));
        if (NF) {
            const dim3 grid(grid_of(NF).x, (unsigned)n), lgrid(LARGE_GROUPS * STRIPES);
            if (stats) {
                hipLaunchKernelGGL(raster_faces<M_FACE | M_STATS>, grid, dim3(256), 0, stream, NV, vertices, NF, faces, views, view_stride, w.pix, w.r.hdr, w.r.list, w.r.cap, w.r.stats);
                hipLaunchKernelGGL(raster_large<M_FACE | M_STATS>, lgrid, dim3(256), 0, stream, views, view_stride, w.pix, w.r.hdr, w.r.list, w.r.cap, w.r.stats);
            } else {
                hipLaunchKernelGGL(raster_faces<M_FACE>, grid, dim3(256), 0, stream, NV, vertices, NF, faces, views, view_stride, w.pix, w.r.hdr, w.r.list, w.r.cap, w.r.stats);
                hipLaunchKernelGGL(raster_large<M_FACE>, lgrid, dim3(256), 0, stream, views, view_stride, w.pix, w.r.hdr, w.r.list, w.r.cap, w.r.stats);
            }
        }
        hipLaunchKernelGGL(faces_images<true>, igrid, dim3(256), 0, stream, views, view_stride, w.pix, reinterpret_cast<uint32_t*>(depth), face);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    return stats ? read_stats(w.r, stats, stream) : GOF_OK;
}

size_t gof_mesh_shade_ws_bytes(void) { return header_layout(nullptr, nullptr); }

int gof_mesh_shade(int64_t NV, const float* vertices, int64_t NF, const int32_t* faces, const float* normals, const uint8_t* colors, int32_t num_views,
                   const GofRasterView* views, int64_t view_stride, const int32_t* face, const GofShadeParams* params, float* image, float* bary,
                   void* ws, size_t ws_bytes, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (bad_mesh("mesh_shade", NV, NF) || bad_views("mesh_shade", num_views, view_stride)) return GOF_E_INVALID;
    if (!params) { set_error("mesh_shade: params is NULL"); return GOF_E_INVALID; }
    const GofShadeParams P = *params;
    if (P.mode < 0 || P.mode > GOF_SHADE_SHADED || (P.flags & ~(GOF_SHADE_FLAT | GOF_SHADE_VERTEX_BASE))) {
        set_error("mesh_shade: unknown mode (%d; 0 .. %d) or flags (%d)", P.mode, GOF_SHADE_SHADED, P.flags);
        return GOF_E_INVALID;
    }
    if (!std::isfinite(P.ambient)) { set_error("mesh_shade: the ambient term is not finite"); return GOF_E_INVALID; }
    const bool need_colors = P.mode == GOF_SHADE_COLOR || (P.mode == GOF_SHADE_SHADED && (P.flags & GOF_SHADE_VERTEX_BASE));
    const bool need_normals = P.mode != GOF_SHADE_COLOR && !(P.flags & GOF_SHADE_FLAT);
    if (need_colors && !colors) { set_error("mesh_shade: this mode needs vertex colours and the mesh has none"); return GOF_E_INVALID; }
    if (need_normals && !normals && NV) { set_error("mesh_shade: this mode needs vertex normals (or GOF_SHADE_FLAT)"); return GOF_E_INVALID; }
    if (!ws) { set_error("mesh_shade: workspace is NULL"); return GOF_E_INVALID; }
    if (ws_bytes < gof_mesh_shade_ws_bytes()) { set_error("mesh_shade: workspace too small"); return GOF_E_WORKSPACE; }
    if (num_views && (!views || !face || !image)) { set_error("mesh_shade: views / face / image is NULL"); return GOF_E_INVALID; }
    if (NF && (!faces || !vertices)) { set_error("mesh_shade: vertices / faces is NULL"); return GOF_E_INVALID; }
    RasterWs h;
    header_layout(ws_aligned(ws), &h);
    GOF_PROFILE("mesh_shade", stream);
    const int rc = raster_validate("mesh_shade", NV, NF, faces, num_views, views, view_stride, h, false, stream);
    if (rc) return rc;
    if (num_views) {
        ShadeArgs A = { vertices, faces, normals, colors, views, face, image, bary, NF, view_stride, P };
        hipLaunchKernelGGL(shade_pixels, dim3(image_blocks(view_stride), num_views), dim3(256), 0, stream, A);
        GOF_LAUNCH_CHECK(stream, 0);
    }
    return GOF_OK;
}

} // extern "C"
