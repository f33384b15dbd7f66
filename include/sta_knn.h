/*
 * sta_knn.h - C ABI of libsta_knn.so: the k nearest reference points of every query on the uniform grid that sta_nn_build
 * (include/sta_cloud.h) wrote, and the moments of those neighbourhoods - mean neighbour distance, normal, surface variation - that the
 * cloud filters and estimate_normals of vista_slam_amd/cloud.py sit on.
 *
 * This is NOT part of the product ABI (include/sta_mi355.h) and not part of libsta_cloud.so: an eleventh library with its own
 * translation unit (vista_slam_amd/csrc/sta_knn.hip, kernels in csrc/knn.h, which includes sta_common.h alone), its own ctypes table
 * (_lib.KNN_SIGNATURES) and its own inventories (tests/test_knn_abi.py, tests/knn_stream_cases.py).  It READS the index of
 * sta_nn_build and includes no file of that library: sta_knn_grid below restates sta_nn_index field by field (same order, same
 * types; tests/test_knn_abi.py compares the two lists), so the caller passes the very struct sta_nn_build filled.
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name ends in _host; every buffer is the
 *     caller's (sta_knn_plan gives the byte counts).  NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_knn_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is
 *     contracted into an FMA.  tests/knn_cases.py restates all of it in numpy.
 *   - The only atomic is the integer OR of a status bit.
 */
#ifndef STA_KNN_H
#define STA_KNN_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_KNN_MAX_K 64         /* neighbours per query */
#define STA_KNN_MAX_RINGS 32     /* radius <= STA_KNN_MAX_RINGS * cell: STA_NN_MAX_RINGS of include/sta_cloud.h, restated */
#define STA_KNN_RECORD 8         /* doubles in a moments record */
#define STA_KNN_PLAN_SIZES 3     /* entries of sta_knn_plan's sizes_out */
#define STA_KNN_MIN_COUNT 3      /* the smallest min_count sta_knn_moments takes */
#define STA_KNN_STATUS_BOUND 1   /* status bit: a cell of the index named sorted positions outside [0, n_finite]: the walk was cut there */
#define STA_KNN_STATUS_ORDER 2   /* status bit: an entry of `order` outside [0, Q): that slot was skipped */

/* sta_nn_index of include/sta_cloud.h, restated: a HOST struct whose pointers point into the index buffer of sta_nn_build. */
typedef struct sta_knn_grid {
    const uint64_t* cell_key;   /* [C]      ascending keys of the occupied cells */
    const int32_t* cell_start;  /* [C + 1]  first sorted position of every occupied cell; cell_start[C] = n_finite */
    const float* sorted_pts;    /* [M, 3]   the reference coordinates in sorted order (the first n_finite rows are the grid) */
    const int32_t* sorted_idx;  /* [M]      original reference index of every sorted position; ascending inside a cell */
    int64_t lo[3];              /* smallest cell index per axis */
    int64_t ext[3];             /* cells per axis (0 when no reference point is finite) */
    double cell;
    int64_t M;                  /* reference points */
    int64_t n_finite;           /* ... of which all three coordinates are finite; the others are left out of the grid */
    int64_t C;                  /* occupied cells */
} sta_knn_grid;

/* Host only.  sizes_out[STA_KNN_PLAN_SIZES] = bytes of {d2_out of sta_knn_query (Q * k float64), idx_out (Q * k int32), work of
 * sta_knn_moments for Q queries}.  Refuses M or Q outside [1, 2^30) and k outside [1, STA_KNN_MAX_K], with the numbers in the
 * message. */
STA_API int sta_knn_plan(int64_t M, int64_t Q, int64_t k, int64_t* sizes_out);

/* For each query the k smallest reference points under the total order (d2, original reference index), among those with
 * d2 <= radius*radius (inclusive, as in sta_nn_query).
 *   d2 = (dx*dx + dy*dy) + dz*dz with dx = double(q_x) - double(p_x): sta_nn_query's formula on double(q).  There is no T.
 *   d2_out [Q,k] float64 and idx_out [Q,k] int32, ascending in that order; unused slots hold (+inf, -1).  count_out [Q] int32 is the
 *   number of filled slots.  Each of the three may be NULL.  A non-finite query gets count 0.  Non-finite reference points are not in
 *   the grid and are never found.
 *   self_base >= 0: query i skips the reference point whose original index is self_base + i - how a cloud is queried against
 *   itself, whole (self_base = 0) or in chunks (self_base = the chunk's first row).  A negative self_base skips nothing.
 *   order: a device permutation [Q] int32, or NULL.  Slot i of the launch processes query order[i] and writes row order[i]: it
 *   changes which lanes sit together (pass the grid's sorted_idx for a cloud against itself: a wave's queries then share cells),
 *   never a bit of the output.  An entry outside [0, Q) is skipped and sets STA_KNN_STATUS_ORDER.
 *   The search walks the rings of sta_nn_query: cells of growing Chebyshev distance j = 0, 1, .. from the query's cell (clamped in
 *   float64 to the grid plus the search margin, as there), with bound_j = (j*cell) * (1 - 2^-30).  It stops after ring j once the
 *   list is full and its k-th d2 < bound_j^2, or once bound_j > radius (at most ring 33).
 *   Why that is exact for the k-th element.  Without rounding, a cell not yet visited after ring j is j + 1 or more cells away
 *   on some axis, so every point in it is further than j*cell from the query on that axis alone, hence d2 > (j*cell)^2.  When the
 *   list holds k points with d2 < (j*cell)^2, an unvisited point is behind all k of them in (d2, index) order whatever its index is:
 *   the strict inequality leaves no tie to break.  With rounding, a point lies in the cell that the rounded division names to within
 *   2^-31 of a cell (the two roundings of floor(double(x) / cell) for |cell index| <= 2^21, include/sta_cloud.h), for the query and
 *   for the point: together at most 2^-30 of a cell, which the factor 1 - 2^-30 takes off the bound from ring 1 on (ring 0 has
 *   bound 0 and stops nothing).  The argument nowhere uses k: it is the argument of sta_nn_query with "the best" read as "the k-th".
 *   Refused: radius not finite, < 0 or > STA_KNN_MAX_RINGS * cell; k outside [1, STA_KNN_MAX_K]; Q outside [1, 2^30); a struct that
 *   is no index of sta_nn_build.
 *   status: one device int32 that the caller zeroed.  The walk is bounded by the index's own counts: a cell whose sorted positions
 *   leave [0, n_finite] is cut there and sets STA_KNN_STATUS_BOUND instead of reading beyond the buffers or spinning.
 *   Asynchronous.  grid_host is read during the call only. */
STA_API int sta_knn_query(const sta_knn_grid* grid_host, const float* qry, int64_t Q, const int32_t* order, int64_t self_base, int64_t k,
                          double radius, double* d2_out, int32_t* idx_out, int32_t* count_out, int32_t* status, void* stream);

/* The moments of every query's neighbourhood, from the lists of sta_knn_query: d2 [Q,k], idx [Q,k], count [Q], and ref [M,3] fp32 in
 * ORIGINAL order, read through idx.  c = count[i] clamped to [0, k]; an index outside [0, M) ends that query's list there (c = its slot).
 *   mean_dist_out [Q] float64 = (sum_j sqrt(d2_j)) / c, summed in list order; +inf for c = 0.
 *   For c >= min_count (the caller's value, at least STA_KNN_MIN_COUNT):
 *     m = (sum_j double(p_j)) / c per axis, summed in list order; the six sums a_xy = sum_j dx*dy with dx = double(p_j.x) - m_x are
 *     taken about m, in list order (a00 a01 a02 a11 a12 a22).  Then 8 cyclic Jacobi sweeps over (0,1), (0,2), (1,2), V starting at
 *     the identity, one rotation on (p, q) with r the third index being
 *         if a_pq != 0:  theta = (a_qq - a_pp) / (2 * a_pq);  h = sqrt(theta*theta + 1);  t = 1 / (|theta| + h), negated when theta < 0;
 *                        c = 1 / sqrt(t*t + 1);  s = t*c;  z = t*a_pq;  a_pp = a_pp - z;  a_qq = a_qq + z;  a_pq = 0;
 *                        (a_rp, a_rq) = (c*a_rp - s*a_rq, s*a_rp + c*a_rq);  likewise (V_kp, V_kq) for k = 0, 1, 2
 *     (the rotation of include/sta_simp.h, restated).  The eigenvalues are the diagonal, sorted l0 <= l1 <= l2 with the lowest column
 *     first among equals; n = the column of l0 divided by sqrt((x*x + y*y) + z*z) of itself.
 *     Orientation: with v = double(view[i]) (view: device [Q,3] fp32, each point's own camera centre) or, when view is NULL,
 *     v = view_host (3 doubles), n is negated when ((v_x - q_x)*n_x + (v_y - q_y)*n_y) + (v_z - q_z)*n_z < 0, q = double(qry[i]).  With
 *     neither, n is negated when its component of largest magnitude (the first among equals) is negative.  Negation is exact.
 *     normal_out [Q,3] fp32 = float(n), rounded once.  curv_out [Q] float64 = l0 / ((l0 + l1) + l2), or 0 when that sum is 0.
 *   Below min_count the normal and curv are NaN.
 *   record_out: STA_KNN_RECORD device doubles, reduced without floating-point atomics in an order that depends on Q alone (two calls
 *   are bit-identical; inputs whose float64 sums are exact give exact sums):
 *       [0] queries with c >= 1   [1] sum mean_dist over them   [2] sum mean_dist*mean_dist   [3] queries with c >= min_count   [4..7] 0.
 *   Any output may be NULL; record_out needs work (sizes_out[2] of sta_knn_plan), qry is needed only with view or view_host, d2 only
 *   with mean_dist_out or record_out.
 *   Refused: M or Q outside [1, 2^30), k outside [1, STA_KNN_MAX_K], min_count < STA_KNN_MIN_COUNT, a short or missing work.
 *   Asynchronous.  view_host is read during the call only. */
STA_API int sta_knn_moments(const float* ref, int64_t M, const float* qry, int64_t Q, const double* d2, const int32_t* idx, const int32_t* count,
                            int64_t k, const float* view, const double* view_host, int64_t min_count, float* normal_out, double* curv_out,
                            double* mean_dist_out, double* record_out, void* work, int64_t work_bytes, void* stream);

STA_API const char* sta_knn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
