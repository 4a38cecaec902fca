/*
 * gof_mesh_hip.h -- C ABI of the mesh culling of the DTU evaluation in libgof_hip.so.
 *
 * What the reference's evaluate_dtu_mesh.py:77-131 (cull_mesh) asks of scikit-image, torch GEMMs + grid_sample and trimesh:
 * (a) disk dilation of every view's object mask, (b) projection of every vertex into every view and the test against the dilated
 * masks, (c) compaction of the mesh to the kept vertices and the faces between them.
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

#ifdef __cplusplus
}
#endif
#endif
