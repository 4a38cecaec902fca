/*
 * gof_delaunay_hip.h -- C ABI of the Delaunay tetrahedralization in libgof_hip.so (csrc/delaunay.hip): the finite cells of the
 * Delaunay tetrahedralization of a float32 point set (the reference's extract_mesh.py calls tetranerf's cpp.triangulate, CGAL's
 * Delaunay_triangulation_3).  The contract -- exact predicates, symbolic perturbation, duplicates, canonical order -- is in
 * DESIGN.md ("Delaunay tetrahedralization").
 *
 * Conventions as in gof_hip.h: extern "C", device pointers, a caller-owned workspace, 0 = ok, text of an error in gof_last_error().
 * gof_delaunay_build runs the insertion rounds from the host with small read-backs (one per round): it SYNCHRONISES `stream`.  It is
 * a mesh-extraction step, not part of the training loop.
 *
 *   ws = gof_delaunay_ws_bytes(n, cap)  ->  gof_delaunay_build(n, points, cap, ws, .., &m, stream)
 *        (GOF_E_CAPACITY: m holds a larger capacity; redo with it, nothing carries over)
 *   ->  gof_delaunay_emit(ws, m, tets, stream)   [m][4] int32 into `tets`
 */
#ifndef GOF_DELAUNAY_HIP_H_INCLUDED
#define GOF_DELAUNAY_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Workspace of a build of n points with room for tet_capacity cells (finite and infinite, live and not yet compacted; the
 * triangulation of n points in general position has about 6.5 n cells).  tet_capacity in [16, 2^30). */
size_t gof_delaunay_ws_bytes(int64_t n, int64_t tet_capacity);

/* Triangulates points [n][3] (fp32, device, n < 2^31).  *num_tets: the number of finite cells (0 for fewer than 4 distinct
 * points or a coplanar set).  GOF_E_INVALID for a non-finite coordinate, GOF_E_CAPACITY when the cell arena is too small (then
 * *num_tets is the capacity to redo the call with), GOF_E_DEVICE when a device-side check failed.  Synchronises `stream`. */
int gof_delaunay_build(int64_t n, const float* points, int64_t tet_capacity, void* ws, size_t ws_bytes, int64_t* num_tets, void* stream);

/* Writes the num_tets cells of the last build on `ws` into tets_out [num_tets][4] (int32 input indices): positively oriented,
 * each starting at its smallest index with the smallest of the other three second, sorted lexicographically. */
int gof_delaunay_emit(void* ws, int64_t num_tets, int32_t* tets_out, void* stream);

/* Statistics of the last build on `ws`: [0] rounds, [1] exact predicate evaluations, [2] peak arena cells, [3] slow-path
 * insertions, [4] points located by a global scan, [5] distinct points, [6] cell capacity, [7] live cells (finite and infinite). */
int gof_delaunay_stats(const void* ws, int64_t* stats, void* stream);

/* ---- test support (the debug family, like gof_debug_fetch): not part of the product's contract, may change with the tests ----
 *
 * Runs one of the build's own predicate functions on n_queries index tuples idx [n_queries][6] = (a, b, c, d, e, aux) into
 * xyz [n_points][3] (fp32), one thread per query, no workspace:
 *   op 0  orient(a, b, c, d)            sign det[b - a, c - a, d - a], fp64 filter first
 *   op 1  insphere(a, b, c, d, e)       > 0: e inside the sphere of the positive (a, b, c, d); 0: on it
 *   op 2  orient_exact, op 3 insphere_exact: the expansion arithmetic without the filter
 *   op 4  collinear(a, b, c)            1: collinear, 0: not
 *   op 5  insphere_perturbed(cell (a, b, c, d), p = e)         the cell positively oriented; never 0
 *   op 6  incircle_perturbed(fin = (a, b, c, d), dk = aux, p = e)   fin positive, aux in [0, 4) its vertex off the face, p in the
 *         face's plane; never 0
 * Every query fully writes sign[q], exact[q] (the exact evaluations it made) and err[q] (the DTE_* bits it raised: 1 = an
 * expansion outgrew its buffer, 32 = the perturbation did not decide).  All pointers are device pointers.  GOF_E_INVALID for a NULL
 * pointer, an unknown op, or a query whose indices -- those its op reads -- lie outside [0, n_points); nothing is read out of
 * range.  Synchronises `stream`. */
int gof_debug_delaunay_predicates(int64_t n_points, const float* xyz, int64_t n_queries, const int32_t* idx, int op, int32_t* sign,
                                  uint32_t* exact, uint32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif
