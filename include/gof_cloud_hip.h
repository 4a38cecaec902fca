/*
 * gof_cloud_hip.h -- C ABI of the point-cloud primitives of the DTU Chamfer evaluation in libgof_hip.so.
 *
 * The three computations of the reference's dtu_eval/eval.py (lattice sampling of every triangle :50-71, greedy radius thinning
 * :86-94, nearest-neighbour distance between two clouds :119-134) without Open3D / scikit-learn.
 *
 * Conventions as in gof_hip.h: extern "C", device pointers, caller-owned workspace with a *_bytes query, launches on `stream`,
 * 0 = ok, negative = GOF_E_* with text in gof_last_error().  All coordinates are fp64 [N,3] row-major, N < 2^31.  Every operation
 * that decides something is IEEE fp64 without contraction, in the order DESIGN.md 3.8 writes down, so results compare bit for bit
 * with numpy on the host.  Entry points that return a count wait for the stream once (or once per batch of rounds: gof_cloud_thin).
 */
#ifndef GOF_CLOUD_HIP_H_INCLUDED
#define GOF_CLOUD_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (a) triangle sampling ---------------------------------------------------------------------------------------------------
 * vertices [NV,3] fp64, triangles [NT,3] int32.  count: per-triangle sample counts + their scan (left in ws), *num_samples = total.
 * emit (same arguments, same ws): points [num_samples,3] in triangle order, then (i, j).  A non-finite vertex or an index outside
 * [0, NV) is GOF_E_INVALID; 2^31 samples or more is GOF_E_CAPACITY. */
size_t gof_cloud_sample_ws_bytes(int64_t num_triangles);
int gof_cloud_sample_count(int64_t num_vertices, const double* vertices, int64_t num_triangles, const int32_t* triangles, double thresh,
                           void* ws, size_t ws_bytes, int64_t* num_samples, void* stream);
int gof_cloud_sample_emit(int64_t num_vertices, const double* vertices, int64_t num_triangles, const int32_t* triangles, double thresh,
                          void* ws, size_t ws_bytes, int64_t num_samples, double* points, void* stream);

/* ---- (b) greedy radius thinning ----------------------------------------------------------------------------------------------
 * points [N,3] in visiting order; keep[i] = 1 iff no kept j < i has (dx*dx + dy*dy) + dz*dz <= r*r.  *num_kept = sum(keep).
 * r <= 0, a non-finite coordinate or an extent of more than 2^21 - 1 cells of edge r is GOF_E_INVALID.
 * stats [4] (host): rounds, distance evaluations, read-backs, occupied-cell scans. */
size_t gof_cloud_thin_ws_bytes(int64_t num_points);
int gof_cloud_thin(int64_t num_points, const double* points, double r, uint8_t* keep, void* ws, size_t ws_bytes, int64_t* num_kept,
                   void* stream);
int gof_cloud_thin_stats(const void* ws, int64_t* stats, void* stream);

/* ---- (c) nearest neighbour between two clouds --------------------------------------------------------------------------------
 * build: the index over ref [NS,3] (Morton order, boxes of 256, groups of 32 boxes) in `index`.  query: for every query point
 * dist = sqrt(min_s ((dx*dx + dy*dy) + dz*dz)) and the index of the minimiser (the smallest on a tie); NS = 0 gives +inf and -1.
 * A non-finite coordinate is GOF_E_INVALID.  stats [4] (host): boxes scanned summed over the queries, boxes staged, distance
 * evaluations, queries. */
size_t gof_cloud_nn_index_bytes(int64_t num_ref);
int gof_cloud_nn_build(int64_t num_ref, const double* ref, void* index, size_t index_bytes, void* stream);
size_t gof_cloud_nn_query_ws_bytes(int64_t num_query);
int gof_cloud_nn_query(int64_t num_ref, const void* index, size_t index_bytes, int64_t num_query, const double* query, double* dist,
                       int32_t* nearest, void* ws, size_t ws_bytes, void* stream);
int gof_cloud_nn_stats(const void* ws, int64_t* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
