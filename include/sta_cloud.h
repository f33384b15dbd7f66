/*
 * sta_cloud.h - C ABI of libsta_cloud.so: exact nearest neighbours between point clouds on a uniform grid, for the offline
 * metrics of a run (point-to-point ICP, accuracy / completeness / chamfer; vista_slam_amd/cloud.py and evaluate.py sit on top).
 *
 * This is NOT part of the product ABI (include/sta_mi355.h): it is a second library with its own translation unit
 * (vista_slam_amd/csrc/sta_cloud.hip, kernels in csrc/cloud.h), its own ctypes table (_lib.CLOUD_SIGNATURES) and its own
 * inventories (tests/test_cloud_abi.py, tests/cloud_stream_cases.py).
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name ends in _host; every workspace is the
 *     caller's (sta_nn_plan gives the byte counts); no call allocates.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_cloud_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is
 *     contracted into an FMA.  tests/cloud_cases.py restates all of it in numpy.
 *
 * The grid.  A point's cell on an axis is floor(double(x) / cell): a lattice anchored at 0.  lo[a] is the smallest cell index of the
 * finite reference points on axis a, ext[a] the number of cells from the smallest to the largest.  The cells of one build are
 * keyed ((iz - lo_z) << 42) | ((iy - lo_y) << 21) | (ix - lo_x), hence ext[a] <= 2^21.  The ring bound of sta_nn_query rests on a
 * point lying in the cell that the rounded division names to within 2^-30 of a cell, hence every cell index must be inside
 * [-2^21, 2^21] (|x| <= 2 097 152 * cell): the two roundings then reach at most 2^-31 of a cell, half the margin at k = 1.
 */
#ifndef STA_CLOUD_H
#define STA_CLOUD_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_NN_MAX_EXTENT (1 << 21)     /* cells per axis */
#define STA_NN_MAX_CELL_INDEX (1 << 21) /* |cell index| */
#define STA_NN_MAX_RINGS 32             /* radius <= STA_NN_MAX_RINGS * cell */
#define STA_NN_RECORD 24                /* doubles in a query record */

/* The index of one sta_nn_build: a HOST struct whose pointers point into the caller's index_buf (device memory). */
typedef struct sta_nn_index {
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
} sta_nn_index;

/* Host only.  sizes_out[3] = bytes of {index_buf of sta_nn_build for M reference points, work of sta_nn_build for M, work of
 * sta_nn_query for Q queries}.  Refuses M or Q outside [1, 2^30). */
STA_API int sta_nn_plan(int64_t M, int64_t Q, int64_t* sizes_out);

/* Uniform-grid index over ref [M,3] fp32.
 *   min / max of the finite points per axis and the number of non-finite ones come from a device reduction; lo and ext are derived
 *   on the device; (key, input index) is sorted with the stable LSD radix sort of csrc/voxel.h (eight 8-bit passes: the pass count
 *   does not wait for the extents), so inside a cell the points are in ascending input order; the sorted keys are compacted to
 *   cell_key / cell_start; the coordinates are copied in sorted order.
 *   The call SYNCHRONISES `stream` once, at its end, for the extent check and C: index_out_host is complete on return.
 *   Refused (nothing usable is left in index_buf): an extent above STA_NN_MAX_EXTENT cells on an axis or a cell index beyond
 *   +-STA_NN_MAX_CELL_INDEX, with the extents in the message; a cell that is not finite and > 0; buffers smaller than sta_nn_plan's.
 *   ref must stay unchanged only during the call: queries read the sorted copy. */
STA_API int sta_nn_build(const float* ref, int64_t M, double cell, void* index_buf, int64_t index_bytes, void* work, int64_t work_bytes,
                         sta_nn_index* index_out_host, void* stream);

/* For each query the exact nearest reference point within `radius`.
 *   T_host: 12 doubles, a row-major 3x4 matrix; NULL = the identity matrix (evaluated like any other).
 *       q'_x = ((T00*x + T01*y) + T02*z) + T03, likewise y and z, on double(x), double(y), double(z).
 *   d2 = (dx*dx + dy*dy) + dz*dz with dx = q'_x - double(p_x).
 *   A reference point qualifies when d2 <= radius*radius (inclusive: this contract's own rule); among equal d2 the lowest original
 *   reference index wins.
 *   d2_out [Q] float64, +inf when nothing qualifies; idx_out [Q] int32, -1 when nothing qualifies; either may be NULL.
 *   A query whose q' is not finite gives (+inf, -1) and is counted in record[19], not in record[0].
 *   Refused: radius not finite, < 0 or > STA_NN_MAX_RINGS * cell.
 *   The search visits the cells in rings of growing Chebyshev distance k = 0, 1, .. from the query's cell and stops after ring k
 *   once best d2 < (k*cell*(1 - 2^-30))^2, or once k*cell*(1 - 2^-30) > radius (at most ring 33: 67^3 cells for the worst query).
 *   A query's cell index is clamped in float64 to the grid plus that margin before it becomes an integer.
 *   record_out: STA_NN_RECORD device doubles (NULL = none; then work may be NULL), reduced without floating-point atomics in an
 *   order that depends on Q alone (two calls are bit-identical; inputs whose float64 sums are exact give exact sums):
 *       [0] finite queries   [1] matched queries   [2] sum d2 over matched   [3] sum min(d2, radius^2) over finite queries (an
 *       unmatched one contributes radius^2)   over matched pairs: [4..6] sum q'   [7..9] sum double(p)   [10..18] sum q' p^T
 *       (row-major, row = axis of q')   [19] non-finite queries   [20..23] 0.
 *   Asynchronous: no copy to the host, no synchronisation.  index_host is read during the call only. */
STA_API int sta_nn_query(const sta_nn_index* index_host, const float* qry, int64_t Q, const double* T_host, double radius, double* d2_out,
                         int32_t* idx_out, double* record_out, void* work, int64_t work_bytes, void* stream);

/* out [M,3] = float(q') of pts [M,3] (q' as in sta_nn_query, rounded to nearest once).  Non-finite input is not special: it goes
 * through the same arithmetic.  out may be pts.  Asynchronous. */
STA_API int sta_cloud_transform(const float* pts, int64_t M, const double* T_host, float* out, void* stream);

STA_API const char* sta_cloud_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
