/*
 * gof_cloud_reg_hip.h -- C ABI of the registration primitives of the Tanks-and-Temples F-score evaluation in libgof_hip.so
 * (DESIGN.md 3.9).
 *
 * What the reference's eval_tnt/registration.py and evaluation.py ask of Open3D besides a nearest-neighbour search (that one is
 * gof_cloud_nn_build / gof_cloud_nn_query of gof_cloud_hip.h): rigid transformation + polygon-volume crop, voxel down-sampling and
 * the correspondence sums of one ICP iteration.
 *
 * Conventions as in gof_cloud_hip.h: extern "C", device pointers, caller-owned workspace with a *_bytes query, launches on `stream`,
 * 0 = ok, negative = GOF_E_* with text in gof_last_error().  Coordinates are fp64 [N,3] row-major, N < 2^31.  Every deciding
 * operation is IEEE fp64 without contraction in the order DESIGN.md 3.9 writes down; no floating-point atomics.  A non-finite
 * coordinate is GOF_E_INVALID.  Small parameters (a 4x4 matrix, means, result sums) are HOST pointers and say so; entry points that
 * return counts or sums wait for the stream once.
 */
#ifndef GOF_CLOUD_REG_HIP_H_INCLUDED
#define GOF_CLOUD_REG_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- transformation ------------------------------------------------------------------------------------------------------------
 * matrix: HOST, 16 values row-major (the last row is not read).  out[i][r] = ((m_r0 x + m_r1 y) + m_r2 z) + m_r3.  matrix = NULL
 * copies the points.  out may not alias points.  The workspace holds the status word only. */
size_t gof_cloud_transform_ws_bytes(int64_t num_points);
int gof_cloud_transform(int64_t num_points, const double* points, const double* matrix, double* out, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- (a) transformation + polygon-volume crop -----------------------------------------------------------------------------------
 * axis: 0 = X, 1 = Y, 2 = Z is the volume's orthogonal axis w; the polygon lives in the other two (u, v): X -> (y, z), Y -> (z, x),
 * Z -> (x, y).  polygon: DEVICE [K,3] fp64 (the vertices as the volume file gives them; their w is not read), K <= 4096 (more:
 * GOF_E_CAPACITY).  A transformed point p' is kept iff axis_min <= p'_w <= axis_max and the number of edges (P_i, P_j), j = i - 1
 * (mod K), with ((P_i.v < p'.v && P_j.v >= p'.v) || (P_j.v < p'.v && P_i.v >= p'.v)) and
 * P_i.u + (p'.v - P_i.v) / (P_j.v - P_i.v) * (P_j.u - P_i.u) < p'.u is odd.  out_points [N,3] / out_index [N] (capacity N): the kept
 * transformed points in input order and their input rows; *num_kept = how many. */
size_t gof_cloud_crop_ws_bytes(int64_t num_points);
int gof_cloud_crop(int64_t num_points, const double* points, const double* matrix, int axis, double axis_min, double axis_max,
                   int64_t num_polygon, const double* polygon, double* out_points, int32_t* out_index, void* ws, size_t ws_bytes,
                   int64_t* num_kept, void* stream);

/* ---- (b) voxel down-sampling ------------------------------------------------------------------------------------------------------
 * lo = per-axis minimum, o = lo - 0.5 v, cell = floor((p - o) / v) per axis (at most 2^21 - 1 per axis, else GOF_E_INVALID), key =
 * x 2^42 | y 2^21 | z.  out_points [N,3] / out_counts [N] (capacity N): one row per occupied voxel in ascending key order = the sum
 * of the voxel's points added left to right in input order, divided by their number; *num_voxels = how many.  v <= 0 or non-finite
 * is GOF_E_INVALID. */
size_t gof_cloud_voxel_ws_bytes(int64_t num_points);
int gof_cloud_voxel(int64_t num_points, const double* points, double voxel, double* out_points, int32_t* out_counts, void* ws,
                    size_t ws_bytes, int64_t* num_voxels, void* stream);

/* ---- (c) correspondence sums of one ICP iteration ----------------------------------------------------------------------------------
 * source [N,3]: the TRANSFORMED source points s'; target [NT,3]; dist [N], nearest [N]: what gof_cloud_nn_query returned for s'.
 * i is a correspondence iff dist[i] < threshold (and nearest[i] >= 0); a nearest[i] >= NT is GOF_E_INVALID, and so is a
 * correspondence whose coordinates, squared distance or products are not finite (the rows of non-correspondences are not read).
 * sums1: *n = number of correspondences, sums (HOST) [7] = sum s' (3), sum t (3), sum dist^2 (dist[i] * dist[i]).
 * sums2: means (HOST) [6] = mu_s (3), mu_t (3); sums (HOST) [10] = sum (t - mu_t)(s' - mu_s)^T row-major (9), sum |s' - mu_s|^2
 * (((dx dx + dy dy) + dz dz) per point).
 * Every sum is the balanced binary tree over the source points in index order, a non-correspondence contributing +0.0, padded with
 * +0.0 to the next power of two: the result does not depend on the launch shape and numpy restates it exactly. */
size_t gof_cloud_icp_sums_ws_bytes(int64_t num_source);
int gof_cloud_icp_sums1(int64_t num_source, const double* source, int64_t num_target, const double* target, const double* dist,
                        const int32_t* nearest, double threshold, void* ws, size_t ws_bytes, int64_t* n, double* sums, void* stream);
int gof_cloud_icp_sums2(int64_t num_source, const double* source, int64_t num_target, const double* target, const double* dist,
                        const int32_t* nearest, double threshold, const double* means, void* ws, size_t ws_bytes, double* sums,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
