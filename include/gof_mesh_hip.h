/*
 * gof_mesh_hip.h -- C ABI of the mesh culling of the DTU evaluation in libgof_hip.so.
 *
 * What the reference's evaluate_dtu_mesh.py:77-131 (cull_mesh) asks of scikit-image, torch GEMMs + grid_sample and trimesh:
 * (a) disk dilation of every view's object mask, (b) projection of every vertex into every view and the test against the dilated
 * masks, (c) compaction of the mesh to the kept vertices and the faces between them.  And what that script and
 * eval_tnt/cull_mesh.py:186-201 leave disabled for want of a split() that scales: (d) the connected components of the mesh, their
 * sizes, and the masks that drop the small ones (csrc/mesh_components.hip).  And what eval_tnt/cull_mesh.py asks of
 * pyrender and of its point_masks: (e) a depth image of the mesh per camera, (f) the number of views that see a vertex in front of it
 * (csrc/mesh_raster.hip).  And what mesh_viewer.py asks of Open3D and a window: (g) vertex normals, a face buffer and the
 * images resolved from it (csrc/mesh_render.hip).  And what the reference's README leaves to MeshLab: (h) a mesh with fewer
 * faces, by vertex clustering with a quadric-error representative (csrc/mesh_simplify.hip).
 *
 * Conventions as in gof_hip.h: extern "C", device pointers, caller-owned workspace with a *_bytes query whose contents do not
 * matter on entry, launches on `stream`, 0 = ok, negative = GOF_E_* with text in gof_last_error().  Every operation that decides
 * something is an integer operation or IEEE fp64 without contraction, in the order DESIGN.md 3.10 writes down, so results compare
 * bit for bit with numpy on the host.  Entry points that report a status or a count wait for the stream once.
 */
#ifndef GOF_MESH_HIP_H_INCLUDED
#define GOF_MESH_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (a) disk dilation of a mask -----------------------------------------------------------------------------------------------
 * mask [H,W] row-major, float32 (is_u8 = 0) or uint8 (is_u8 = 1); a pixel is set iff (float)m / 256.0f != 0.
 * out: H rows of gof_mesh_mask_row_words(W) = ceil(W / 64) 64-bit words, pixel x of a row = bit (x % 64) of word (x / 64); bit
 * (y, x) is set iff some set input pixel (y + dy, x + dx) inside the image has dx*dx + dy*dy <= r*r; the bits x >= W of a row's
 * last word are zero.  0 <= r <= 31; W, H >= 1.  No workspace. */
#define GOF_MESH_MAX_RADIUS 31
int64_t gof_mesh_mask_row_words(int32_t W);
int gof_mesh_dilate(int32_t W, int32_t H, const void* mask, int32_t is_u8, int32_t r, uint64_t* out, void* stream);

/* ---- (b) vertex culling --------------------------------------------------------------------------------------------------------
 * One record per view, in device memory: m = rows 0..2 of K * W2C (row-major 3 x 4, fp64), the image size, and where the view's
 * dilated mask lies in `masks`: mask_offset (in 64-bit words) and row_words (>= ceil(W / 64)).
 * vertices [NV,3] float32, keep [NV] uint8.  Per vertex (vx, vy, vz widened to fp64) and view:
 *   x = ((m0 vx + m1 vy) + m2 vz) + m3, y and z from rows 1 and 2;  d = z + 1e-6;
 *   px = ((x / d) / (W - 1) - 0.5) * 2,  py = ((y / d) / (H - 1) - 0.5) * 2;
 *   valid = px > -1 && px < 1 && py > -1 && py < 1 (false for NaN); a view that is not valid keeps the vertex;
 *   otherwise ix = rint((px + 1) / 2 * (W - 1)), iy = rint((py + 1) / 2 * (H - 1)) (ties to even) and the view keeps the vertex
 *   iff 0 <= ix < W, 0 <= iy < H and bit (iy, ix) of its mask is set.
 * keep = AND over the views (num_views = 0: every vertex is kept).  A record with W or H < 1, row_words < ceil(W / 64) or a mask
 * that does not lie inside [0, mask_words) is GOF_E_INVALID (nothing outside `masks` is read). */
typedef struct GofCullView {
    double m[12];
    int32_t W, H;
    int64_t mask_offset;
    int64_t row_words;
} GofCullView;

size_t gof_mesh_cull_ws_bytes(int64_t num_vertices);
int gof_mesh_cull(int64_t num_vertices, const float* vertices, int32_t num_views, const GofCullView* views, const uint64_t* masks,
                  int64_t mask_words, uint8_t* keep, void* ws, size_t ws_bytes, void* stream);

/* ---- (c) mesh compaction -------------------------------------------------------------------------------------------------------
 * keep [NV] uint8, faces [NF,3] int32.  out_rows [NV]: the indices of the kept vertices in ascending order (counts[0] of them;
 * gather attribute rows with gof_rows_gather).  face_keep [NF] (may be NULL): 1 iff all three vertices of the face are kept.
 * out_faces [NF,3]: drop_faces != 0: the faces with face_keep = 1, in order, every index replaced by its vertex's new row
 * (counts[1] of them); drop_faces = 0: every face (counts[1] = NF), the index of a removed vertex replaced by 0.
 * counts [2] (host).  An index outside [0, NV) is GOF_E_INVALID. */
size_t gof_mesh_compact_ws_bytes(int64_t num_vertices, int64_t num_faces);
int gof_mesh_compact(int64_t num_vertices, const uint8_t* keep, int64_t num_faces, const int32_t* faces, int32_t drop_faces,
                     int32_t* out_rows, int32_t* out_faces, uint8_t* face_keep, void* ws, size_t ws_bytes, int64_t* counts,
                     void* stream);

/* ---- (d) connected components (csrc/mesh_components.hip) -----------------------------------------------------------
 * faces [NF,3] int32 with indices in [0, NV), 3 * NF < 2^31.  mode GOF_MESH_CONN_EDGE: two faces are adjacent iff they share an
 * unordered pair of vertex indices (however many faces lie on that pair); GOF_MESH_CONN_VERTEX: iff they share a vertex index.  A face
 * with a repeated index takes part like any other; vertices are never merged by position.
 * face_label [NF] int32: the smallest face index of the face's component.  face_comp [NF] int32: the rank of that index among all
 * roots (components numbered 0 .. C-1 in the order of their first face).  *num_components (host) = C.  Both arrays are functions of
 * `faces` alone.  An index outside [0, NV), 3 * NF >= 2^31 or an unknown mode is GOF_E_INVALID and nothing is written (the indices are
 * checked by a launch of their own before any output is touched); a labelling that fails its own check (a united pair with different
 * labels, a label that is not its own label) is GOF_E_DEVICE.  NF = 0 gives C = 0.  Waits for the stream (once for the index check,
 * once per round of pointer jumping, once for C). */
#define GOF_MESH_CONN_EDGE 0
#define GOF_MESH_CONN_VERTEX 1
int gof_mesh_abi_version(void);        /* 2: (a)-(c) were 1 */
/* the sizes at which this unit changes its path, for tests: out[0] items per block of the radix sort, out[1] items per tile of the
 * scan, out[2] positions per tile and out[3] per block of the area sums */
void gof_mesh_components_tiling(int64_t* out);
size_t gof_mesh_components_ws_bytes(int64_t num_vertices, int64_t num_faces, int32_t mode);
int gof_mesh_components(int64_t num_vertices, int64_t num_faces, const int32_t* faces, int32_t mode, int32_t* face_label,
                        int32_t* face_comp, int64_t* num_components, void* ws, size_t ws_bytes, void* stream);

/* Per component c of face_comp [NF] (values in [0, C); a component without a face is allowed):
 * comp_faces [C] int64: its number of faces; comp_first [C] int32: its smallest face index (-1 without a face); comp_area [C] fp64.
 * The area of a face (vertices [NV,3] fp64), every operation IEEE fp64 in this order, nothing contracted:
 *   e1 = v1 - v0, e2 = v2 - v0;  cx = e1y e2z - e1z e2y, cy = e1z e2x - e1x e2z, cz = e1x e2y - e1y e2x;
 *   a = 0.5 * sqrt((cx cx + cy cy) + cz cz).
 * The sum of a component: the faces stably sorted by component (ascending face index inside a component) form one sequence; position p
 * of that sequence lies in tile p / 256 and in block p / 65536.  The areas of a component inside one tile are added from left to
 * right, starting from the first; the tile sums inside one block are added from left to right; the block sums are added from left to
 * right.  No floating-point atomics: the result has the same bits on every run.  A component without a face has area 0.
 * An index outside [0, NV) or a face_comp outside [0, C) is GOF_E_INVALID, checked before any output is written. */
size_t gof_mesh_component_stats_ws_bytes(int64_t num_faces, int64_t num_components);
int gof_mesh_component_stats(int64_t num_vertices, int64_t num_faces, const double* vertices, const int32_t* faces,
                             const int32_t* face_comp, int64_t num_components, int64_t* comp_faces, int32_t* comp_first,
                             double* comp_area, void* ws, size_t ws_bytes, void* stream);

/* face_keep [NF] uint8 = comp_keep[face_comp[f]] != 0 (comp_keep [C] uint8; a face_comp outside [0, C) gives 0).  No workspace. */
int gof_mesh_component_mask(int64_t num_faces, const int32_t* face_comp, int64_t num_components, const uint8_t* comp_keep,
                            uint8_t* face_keep, void* stream);

/* vert_keep [NV] uint8 = 1 iff some face f with face_keep[f] != 0 (face_keep = NULL: every face) has the vertex among its indices.
 * Indices outside [0, NV) mark nothing (gof_mesh_compact refuses them).  No workspace, no wait. */
int gof_mesh_mark_referenced(int64_t num_vertices, int64_t num_faces, const int32_t* faces, const uint8_t* face_keep,
                             uint8_t* vert_keep, void* stream);

/* ---- (e) depth rasteriser, (f) visibility count (csrc/mesh_raster.hip) ----------------------------------------------
 * What eval_tnt/cull_mesh.py asks of pyrender (a depth image of the mesh per camera, :17-66) and of Mesher.point_masks (:117-175).
 * This part of the header is version 3 of the mesh ABI: gof_mesh_raster_abi_version() = 3.  gof_mesh_abi_version() keeps answering 2:
 * (a)-(d) are unchanged and their callers compare that number.
 *
 * One record per view, in device memory: w2c = rows 0..2 of world-to-camera (row-major 3 x 4, fp64; OpenCV convention: +x right, +y
 * down, +z forward), the intrinsics and the depth range in fp64, the image size.  Image v of a call lies at depth + v * view_stride
 * (in elements; W * H <= view_stride for every record).  1 <= W, H <= 16384, znear > 0, zfar > znear, else GOF_E_INVALID; so is a
 * face index outside [0, NV).  Both are checked by a launch of their own before any output is written; that check waits for the
 * stream once.  3 * NF < 2^31.
 *
 * (e) gof_mesh_render_depth: vertices [NV,3] float32 (widened to fp64), faces [NF,3] int32 -> depth: per view H x W float32, row 0
 * at the top, pixel (i, j) = column i of row j with its centre at (i + 0.5, j + 0.5); both orientations of a face are drawn.  Per face
 * and view, every operation IEEE fp64 in this order, nothing contracted:
 *   camera coordinates of a vertex: x = ((w2c[0] vx + w2c[1] vy) + w2c[2] vz) + w2c[3], y and z from rows 1 and 2; a face with a
 *   non-finite vertex coordinate or camera coordinate is skipped;
 *   Sutherland-Hodgman against z >= znear, walking the edges v0v1, v1v2, v2v0: an inside vertex is emitted, then, if the edge crosses,
 *   the point p = a + t (b - a) with t = (znear - za) / (zb - za), a the INSIDE endpoint and b the outside one, for x and y, and
 *   z = znear itself;
 *   projection of every vertex of that polygon: sx = fx (x / z) + cx, sy = fy (y / z) + cy, w = 1 / z; a non-finite sx or sy skips
 *   the face;
 *   the same clip, with the same rule for a and b and all of sx, sy, w interpolated by t except the clipped coordinate, which is the
 *   bound itself, against sx >= -G, sx <= W + G, sy >= -G, sy <= H + G in this order, G = 4096 pixels;
 *   the polygon q0 .. q(n-1) is fanned: (q0, qk, qk+1), k = 1 .. n - 2.  Per triangle (A, B, C): X = (int) rint(sx * 256), Y likewise;
 *   area = (Bx - Ax)(Cy - Ay) - (By - Ay)(Cx - Ax) in integers; 0: skipped; negative: B and C change places and area = -area.
 *   Pixel (i, j), P = (256 i + 128, 256 j + 128): e0 = (Cx - Bx)(Py - By) - (Cy - By)(Px - Bx), e1 the same from C to A, e2 from A to
 *   B; covered iff each ek > 0 or ek = 0 and its edge (dx, dy) = end - start has dy < 0 or (dy = 0 and dx > 0) (top-left rule);
 *   z = (double) area / (((double) e0 wA + (double) e1 wB) + (double) e2 wC); kept iff z > 0 and z <= zfar; d = (float) z.
 * A pixel holds the minimum of its d (an unsigned integer minimum over the floats' bit patterns: no floating-point atomics, the same
 * bits whatever the order of the faces and on every run), 0.0f where nothing is kept.  All |X|, |Y| < 2^23, so an edge function is
 * below 2^49 and exact in int64 and in fp64.
 * stats (host, may be NULL; 8 words): [0] fan triangles with a non-empty pixel box, [1] of them walked through the list, [2] refused by
 * a full list and drawn by their own thread, [3] atomics issued, [4] pixels covered and in range.  Collecting them costs time. */
typedef struct GofRasterView {
    double w2c[12];
    double fx, fy, cx, cy, znear, zfar;
    int32_t W, H;
} GofRasterView;

int gof_mesh_raster_abi_version(void); /* 3 */
/* for tests: out[0] the largest side, in pixels, of a triangle's box of pixel centres that its own thread draws (larger: the list),
 * out[1], out[2] width and height of the tile a wave walks the list's triangles with, out[3] G, out[4] the largest W or H, out[5] the
 * views per batch of gof_mesh_visibility with batch = 0, out[6] list entries the workspace holds besides NF / 8, out[7] workgroups
 * that share one list entry */
void gof_mesh_raster_tiling(int64_t* out);
size_t gof_mesh_render_depth_ws_bytes(int64_t num_faces);
int gof_mesh_render_depth(int64_t num_vertices, const float* vertices, int64_t num_faces, const int32_t* faces, int32_t num_views,
                          const GofRasterView* views, int64_t view_stride, float* depth, int64_t* stats, void* ws, size_t ws_bytes,
                          void* stream);

/* (f) count [NV] int32 += the number of views that see the vertex in front of their depth image (Mesher.point_masks in fp64).  Per
 * vertex and view: x, y, Z as in (e); X = fx x + cx Z, Y = fy y + cy Z; z = Z + 1e-8; u = X / z, v = Y / z;
 *   in_frustum = u >= 0 && u <= W - 1 && v >= 0 && v <= H - 1 && z > 0 (false for NaN); only then the image is read:
 *   x0 = floor(u), x1 = min(x0 + 1, W - 1), tx = u - x0, y likewise (grid_sample, bilinear, align_corners = True, border padding: the
 *   texel index is the coordinate); with dyx the texels widened to fp64:
 *   ds = ((d00 ((1 - tx)(1 - ty)) + d01 (tx (1 - ty))) + d10 ((1 - tx) ty)) + d11 (tx ty);
 *   front = ds > 0 ? z < ds + eps : true;  the view counts iff in_frustum && front.
 * The workspace is gof_mesh_render_depth_ws_bytes(0) bytes. */
int gof_mesh_visible_count(int64_t num_vertices, const float* vertices, int32_t num_views, const GofRasterView* views,
                           int64_t view_stride, const float* depth, double eps, int32_t* count, void* ws, size_t ws_bytes,
                           void* stream);

/* The two together: `batch` views (0: out[5] of the tiling query; at most 4096) are rendered into the workspace and counted, batch
 * after batch; the depth images of all views never exist at once.  count [NV] int32 (written, not added to), keep [NV] uint8 =
 * count >= min_views (min_views <= 0 keeps everything).  stats as in (e), summed over the batches. */
size_t gof_mesh_visibility_ws_bytes(int64_t num_faces, int64_t view_stride, int32_t batch);
int gof_mesh_visibility(int64_t num_vertices, const float* vertices, int64_t num_faces, const int32_t* faces, int32_t num_views,
                        const GofRasterView* views, int64_t view_stride, int32_t batch, double eps, int32_t min_views, int32_t* count,
                        uint8_t* keep, int64_t* stats, void* ws, size_t ws_bytes, void* stream);

/* ---- (g) pictures of the surface: vertex normals, face buffer, resolve (csrc/mesh_render.hip) ------------------------
 * What the reference's mesh_viewer.py asks of Open3D (compute_vertex_normals, then an OpenGL window).  Version 4 of the mesh ABI:
 * gof_mesh_render_abi_version() = 4; the three older numbers keep their values.  Every output is a pure function of the input, in
 * integers and IEEE fp64 without contraction in the written order; with
 *   cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx),  dot(u, v) = (ux vx + uy vy) + uz vz,
 *   unit(n): len = sqrt((nx nx + ny ny) + nz nz); n / len per component if len is finite and > 0, else (0, 0, 1).
 * Refused input (a face index outside [0, NV), a bad view record, a bad mode, ...) is GOF_E_INVALID with no output written; the
 * indices and records are checked by a launch of their own, which waits for the stream once.  3 * NF < 2^31.
 *
 * (g1) normals.  vertices [NV,3] float32 widened to fp64.  Face vector Nf = cross(v1 - v0, v2 - v0), not normalised (area weights).
 * gof_mesh_face_normals: out [NF,3] float32 = (float) unit(Nf).  gof_mesh_vertex_normals: out [NV,3] float32 = (float) unit(S), S = the
 * sum of Nf over the vertex's incident corners in ascending 3 * face + corner order, one addition per corner, starting from 0 (a
 * vertex without a face, or with S = 0 or not finite: (0, 0, 1)).  No floating-point atomics: the corners are counted per vertex,
 * the counts scanned, the (vertex, corner) pairs sorted stably by vertex, and one lane per vertex walks its segment. */
int gof_mesh_render_abi_version(void); /* 4 */
size_t gof_mesh_vertex_normals_ws_bytes(int64_t num_vertices, int64_t num_faces);
int gof_mesh_vertex_normals(int64_t num_vertices, const float* vertices, int64_t num_faces, const int32_t* faces, float* normals,
                            void* ws, size_t ws_bytes, void* stream);
size_t gof_mesh_face_normals_ws_bytes(void);
int gof_mesh_face_normals(int64_t num_vertices, const float* vertices, int64_t num_faces, const int32_t* faces, float* normals,
                          void* ws, size_t ws_bytes, void* stream);

/* (g2) face buffer.  The inputs of gof_mesh_render_depth; geometry and coverage are those of (e).  A pixel keeps the minimum of the
 * 64-bit word (bits(d) << 32) | face over everything that covers it (one unsigned 64-bit atomic minimum): the smallest depth and,
 * among equal depth bits, the smallest face index.  depth: per view H x W float32, bit-equal to (e)'s; face: per view H x W int32, -1
 * where nothing is seen; image v of both at + v * view_stride elements.  The workspace holds 8 bytes per pixel of the call
 * (num_views * view_stride words) besides (e)'s; the tiling query of (e) describes this entry as well.  stats as in (e).  The size
 * query answers 0 for num_views outside [0, 65535] or view_stride outside [0, 16384^2]. */
size_t gof_mesh_render_faces_ws_bytes(int64_t num_faces, int32_t num_views, int64_t view_stride);
int gof_mesh_render_faces(int64_t num_vertices, const float* vertices, int64_t num_faces, const int32_t* faces, int32_t num_views,
                          const GofRasterView* views, int64_t view_stride, float* depth, int32_t* face, int64_t* stats, void* ws,
                          size_t ws_bytes, void* stream);

/* (g3) resolve: one lane per pixel reads `face` (as (g2) wrote it; a value outside [0, NF) is background).  For pixel (i, j) with
 * face f: a, b, c = the camera coordinates of the face's ORIGINAL three vertices as in (e); d = (((i + 0.5) - cx) / fx,
 * ((j + 0.5) - cy) / fy, 1);  m0 = dot(d, cross(b, c)), m1 = dot(d, cross(c, a)), m2 = dot(d, cross(a, b));  s = (m0 + m1) + m2,
 * lk = mk / s;  each lk that is NaN or < 0 becomes 0, each > 1 becomes 1;  t = (l0 + l1) + l2;  lk /= t if t > 0, else all three are
 * 1/3: the perspective-correct barycentric coordinates of the ray through the pixel centre (a clipped face gives what an unclipped
 * one gives).  sum3(q) = (l0 q0 + l1 q1) + l2 q2 per component.
 * image: per view three planes of view_stride float32 (plane c of view v at (3 v + c) * view_stride), bary (may be NULL) likewise =
 * (float) lk.  Background pixels get (float) background[c] and a bary of 0.  Modes:
 *   NORMAL_WORLD   n = unit(sum3(N)) with N the vertex normals widened (normals [NV,3] float32); with GOF_SHADE_FLAT n = unit(Nf) of
 *                  (g1) instead and `normals` is not read;  out = (float)((n + 1) / 2).
 *   NORMAL_CAMERA  nc = ((w2c[4r] nx + w2c[4r+1] ny) + w2c[4r+2] nz), r = 0, 1, 2;  out = (float)((nc + 1) / 2).
 *   COLOR          out = (float)(sum3(C) / 255), C the vertex colours (colors [NV,4] uint8: red green blue and a pad byte).
 *   SHADED         p = sum3 of (a, b, c); v = unit(-p); l = |dot(nc, v)| (a two-sided headlight); out = (float)(base (amb + (1 - amb) l));
 *                  base = sum3(C) / 255 with GOF_SHADE_VERTEX_BASE, else the record's base.
 * GOF_E_INVALID besides the above: a mode above the last, flags beyond the two, an ambient that is not finite, colours needed and
 * NULL, normals needed and NULL.  The workspace is a few words. */
#define GOF_SHADE_NORMAL_WORLD 0
#define GOF_SHADE_NORMAL_CAMERA 1
#define GOF_SHADE_COLOR 2
#define GOF_SHADE_SHADED 3
#define GOF_SHADE_FLAT 1
#define GOF_SHADE_VERTEX_BASE 2
typedef struct GofShadeParams {
    int32_t mode, flags;
    double base[3], background[3], ambient;
} GofShadeParams;
size_t gof_mesh_shade_ws_bytes(void);
int gof_mesh_shade(int64_t num_vertices, const float* vertices, int64_t num_faces, const int32_t* faces, const float* normals,
                   const uint8_t* colors, int32_t num_views, const GofRasterView* views, int64_t view_stride, const int32_t* face,
                   const GofShadeParams* params, float* image, float* bary, void* ws, size_t ws_bytes, void* stream);

/* ---- (h) simplification: uniform vertex clustering with a quadric-error representative (csrc/mesh_simplify.hip) ----
 * What every user of fusion/mesh_binary_search_7.ply does first in some other tool.  Version 5 of the mesh ABI:
 * gof_mesh_simplify_abi_version() = 5; the four older numbers keep their values.  vertices [NV,3] fp64, faces [NF,3] int32 with indices
 * in [0, NV), 3 * NF < 2^31, origin: 3 doubles ON THE HOST, h the cell size.  Refused with GOF_E_INVALID and nothing written (the
 * inputs are checked by a launch of their own, which waits for the stream once): an index outside [0, NV), a cluster number outside
 * [0, NC), a vertex / origin / h that is not finite, h <= 0, a cell coordinate outside [0, 2^21).  Every operation below is an integer
 * operation or IEEE fp64 without contraction in the written order; no floating-point atomics; the bits depend neither on the run nor
 * on the workspace.
 *
 * gof_mesh_cluster.  Cell of a vertex: i_a = floor((x_a - o_a) / h) per axis; key = ix 2^42 + iy 2^21 + iz.  A cluster is a cell with a
 * vertex; the clusters are numbered 0 .. NC-1 in the order of their smallest vertex index.  vertex_cluster [NV] int32 (NULL: the
 * clusters are only counted), *num_clusters (host) = NC. */
int gof_mesh_simplify_abi_version(void); /* 5 */
/* the sizes at which this unit changes its path, for tests: out[0] items per block of the radix sort, out[1] items per tile of the
 * scan, out[2] positions per tile and out[3] per block of the sums */
void gof_mesh_simplify_tiling(int64_t* out);
size_t gof_mesh_cluster_ws_bytes(int64_t num_vertices);
int gof_mesh_cluster(int64_t num_vertices, const double* vertices, const double* origin, double h, int32_t* vertex_cluster,
                     int64_t* num_clusters, void* ws, size_t ws_bytes, void* stream);

/* gof_mesh_cluster_solve.  Per cluster (vertex_cluster [NV] as above, or any numbering with values in [0, NC)): its cell is that of
 * its smallest vertex, centre_a = o_a + (i_a + 0.5) h.  With q = p - centre per component:
 *   mean m = (sum of its vertices' q) / n;  colour channel = (2 S + n) / (2 n) in integers, S the sum of the channel, pad byte 0;
 *   quadric: over the corners e = 3 f + k whose vertex lies in the cluster, with q0, q1, q2 the face's three vertices:
 *     e1 = q1 - q0, e2 = q2 - q0;  n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);  L = sqrt((nx nx + ny ny) + nz nz);
 *     L == 0: ten zeros; else w = 0.5 / L, d = -((nx q0x + ny q0y) + nz q0z), wn = w n per component, wd = w d and
 *     A = (wnx nx, wnx ny, wnx nz, wny ny, wny nz, wnz nz), b = (wd nx, wd ny, wd nz), c = wd d.
 *   Both sums run over the items stably sorted by cluster (ascending vertex index, ascending e) in the order of (d): inside a tile of
 *   256 sorted positions from left to right starting from the first, the tile sums inside a block of 65536 positions from left to
 *   right, the block sums from left to right.
 *   t = (Axx + Ayy) + Azz.  t == 0: y = m.  Else lambda = t * 2^-10, M = A + lambda I, r = lambda m - b and
 *     l00 = sqrt(M00), l10 = M01 / l00, l20 = M02 / l00, l11 = sqrt(M11 - l10 l10), l21 = (M12 - l20 l10) / l11,
 *     l22 = sqrt((M22 - l20 l20) - l21 l21);  z0 = r0 / l00, z1 = (r1 - l10 z0) / l11, z2 = ((r2 - l20 z0) - l21 z1) / l22;
 *     y2 = z2 / l22, y1 = (z1 - l21 y2) / l11, y0 = ((z0 - l10 y1) - l20 y2) / l00;  unless every |y_a| <= 0.5 h: y = m.
 *   A cluster of ONE vertex skips the solve: y = m and its output is that vertex's own three doubles, bit for bit (every plane of its
 *   quadric passes through the vertex, so the vertex is the minimiser; centre + (p - centre) need not reproduce p).
 * out_vertices [NC,3] fp64 = centre + y (one vertex: the vertex); out_colors [NC,4] uint8 (NULL iff colors is NULL); used_mean [NC] uint8 = y is m;
 * *used_mean_count (host, may be NULL) = their number.  Waits for the stream once more at its end (the sorts' status; GOF_E_DEVICE if one gave up).  A cluster without a vertex (a caller's numbering)
 * gets the origin-independent position 0 + 0 and used_mean = 1. */
size_t gof_mesh_cluster_solve_ws_bytes(int64_t num_vertices, int64_t num_faces, int64_t num_clusters);
int gof_mesh_cluster_solve(int64_t num_vertices, int64_t num_faces, const double* vertices, const int32_t* faces, const uint8_t* colors,
                           const int32_t* vertex_cluster, int64_t num_clusters, const double* origin, double h, double* out_vertices,
                           uint8_t* out_colors, uint8_t* used_mean, int64_t* used_mean_count, void* ws, size_t ws_bytes, void* stream);

/* gof_mesh_cluster_faces.  out_faces [NF,3] int32 = vertex_cluster of every index, in the face's order.  face_keep [NF] uint8: 0 for a
 * face whose three clusters are not pairwise distinct; with dedupe != 0 also 0 for a face whose unordered triple of clusters is that of
 * a kept face with a smaller index (the triples sorted to a < b < c go through three stable sorts by c, b, a; an entry that equals its
 * predecessor is dropped); 1 otherwise.  counts (host, may be NULL): [0] faces dropped as degenerate,
 * [1] as duplicates.  Waits for the stream once more at its end (the sorts' status; GOF_E_DEVICE if one gave up). */
size_t gof_mesh_cluster_faces_ws_bytes(int64_t num_faces);
int gof_mesh_cluster_faces(int64_t num_vertices, int64_t num_faces, const int32_t* faces, const int32_t* vertex_cluster,
                           int64_t num_clusters, int32_t dedupe, int32_t* out_faces, uint8_t* face_keep, int64_t* counts, void* ws,
                           size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
