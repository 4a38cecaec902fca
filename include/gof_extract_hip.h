/*
 * gof_extract_hip.h -- C ABI of the mesh extraction's own steps in libgof_hip.so.
 *
 * What the reference's extract_mesh.py:36-120 and scene/gaussian_model.py:31-72, 433-463 ask of torch einsums, boolean-mask
 * assignments and trimesh: (a) the tetrahedralization's input points -- 9 candidates per Gaussian, each tested against every training
 * view, the seen ones compacted in order; (b) one round of the bisection along the crossing edges; (c) the edge length filter of
 * --filter_mesh.
 *
 * Conventions as in gof_mesh_hip.h: extern "C", device pointers, caller-owned workspace with a *_ws_bytes query whose contents do not
 * matter on entry (outputs likewise), launches on `stream`, 0 = ok, negative = GOF_E_* with text in gof_last_error().  The point
 * values are fp32 and the deciding operations IEEE fp64, both without contraction, in the order DESIGN.md 3.11 writes down, so results
 * compare bit for bit with numpy on the host.  Entry points that report a count wait for the stream once.
 */
#ifndef GOF_EXTRACT_HIP_H_INCLUDED
#define GOF_EXTRACT_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (a) tetra points ----------------------------------------------------------------------------------------------------------
 * xyz [P,3], scaling [P,3] (the activated scale with the 3D filter), rotation [P,4] (the raw quaternion r, x, y, z), float32.
 * Candidate i of 9 P: i < 8 P: corner c = i % 8 of Gaussian g = i / 8, signs (cx, cy, cz) = bits (2, 1, 0) of c as -1 / +1;
 * i >= 8 P: the centre of Gaussian i - 8 P.  In fp32:
 *   n = sqrt(((r r + x x) + y y) + z z), the quaternion divided by n, R as utils/general_utils.py: build_rotation writes it
 *   (R00 = 1 - 2 (y y + z z), R01 = 2 (x y - r z), ...);  s = scaling * 3;
 *   p_k = ((R_k0 (cx s0) + R_k1 (cy s1)) + R_k2 (cz s2)) + xyz_k;  a centre is xyz itself;  the point's scale is max(s0, s1, s2).
 * One record per view, in device memory: m = rows 0..2 of the world-to-camera matrix (row-major 3 x 4), fx, fy, as doubles.  Per
 * candidate (p widened to fp64) and view, in fp64:
 *   X = ((m0 px + m1 py) + m2 pz) + m3, Y and Z from rows 1 and 2;  cx = (float)(W / 2.), cy = (float)(H / 2.);
 *   u = (fx X + cx Z) / Z,  v = (fy Y + cy Z) / Z;
 *   seen = Z >= near && Z <= far && u >= 0 && u <= W - 1 && v >= 0 && v <= H - 1   (false for NaN and for Z = 0).
 * A candidate is kept iff some view sees it (num_views = 0: none is).  W, H are one image size for all views.
 * gof_tetra_points_count leaves the candidates' ranks in the workspace and *count (host) = K, the number kept;
 * gof_tetra_points_emit, given the same inputs, that workspace and K, writes the kept points [K,3] and scales [K] in candidate
 * order (a `count` that is not the workspace's K is GOF_E_INVALID and nothing is written).
 * The workspace is 4 bytes per candidate, the scan's scratch and under 1 KiB of alignment pads: at most 8 bytes per candidate for
 * num_gaussians >= 113. */
typedef struct GofFrustumView {
    double m[12];
    double fx, fy;
} GofFrustumView;

size_t gof_tetra_points_ws_bytes(int64_t num_gaussians);
int gof_tetra_points_count(int64_t num_gaussians, const float* xyz, const float* scaling, const float* rotation, int32_t num_views,
                           const GofFrustumView* views, int32_t W, int32_t H, double near_plane, double far_plane, void* ws,
                           size_t ws_bytes, int64_t* count, void* stream);
int gof_tetra_points_emit(int64_t num_gaussians, const float* xyz, const float* scaling, const float* rotation, const void* ws,
                          size_t ws_bytes, int64_t count, float* out_points, float* out_scales, void* stream);

/* ---- (b) one round of the bisection --------------------------------------------------------------------------------------------
 * left_pts, right_pts [E,3], left_sdf, right_sdf [E], value [E], mid_out [E,3], float32; in place, one launch, no workspace.
 *   GOF_BISECT_FIRST: mid_out = (left + right) / 2 and nothing else (value, left_sdf, right_sdf are not read and may be NULL).
 *   GOF_BISECT_FINAL_ALPHA: value = the transmittance the view reduction left; alpha = 1 - value.  GOF_BISECT_ALPHA: alpha = value.
 *   mid = (left + right) / 2;  mid_sdf = alpha - 0.5, a NaN replaced by the canonical quiet NaN (bits 0x7FC00000);
 *   low = (mid_sdf < 0 && left_sdf < 0) || (mid_sdf > 0 && left_sdf > 0);
 *   low: left = mid, left_sdf = mid_sdf; otherwise (mid_sdf = +-0 and NaN included): right = mid, right_sdf = mid_sdf;
 *   mid_out = (left' + right') / 2, the next round's query points. */
#define GOF_BISECT_FINAL_ALPHA 0
#define GOF_BISECT_FIRST 1
#define GOF_BISECT_ALPHA 2
int gof_bisect_step(int64_t num_edges, float* left_pts, float* right_pts, float* left_sdf, float* right_sdf, const float* value,
                    int32_t mode, float* mid_out, void* stream);

/* ---- (c) the edge filter -------------------------------------------------------------------------------------------------------
 * end_points [E,2,3], end_scales [E,2], float32 -> keep [E] uint8: with d = end_points[e,0] - end_points[e,1],
 * keep = sqrt((dx dx + dy dy) + dz dz) <= end_scales[e,0] + end_scales[e,1]  (false for NaN).  No workspace. */
int gof_edge_filter(int64_t num_edges, const float* end_points, const float* end_scales, uint8_t* keep, void* stream);

#ifdef __cplusplus
}
#endif
#endif
