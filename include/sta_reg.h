/*
 * sta_reg.h - C ABI of libsta_reg.so: registration of a cloud against a triangle mesh.  sta_reg_pass is ONE evaluation of an ICP
 * loop: every query is moved by T, its nearest point of the mesh is found - the BRUTE-FORCE minimum over all valid triangles, exactly
 * as sta_tri_query of include/sta_dist.h defines it, with the moved query q' in place of q -, the plane of the winning triangle gives a
 * signed residual r and a Jacobian row J, and the sums that a point-to-point step (Kabsch) and a point-to-plane step (Gauss-Newton,
 * H delta = -g) need are reduced into one record of 64 doubles.  Every per-query output is defined bit for bit by this header: float64
 * operations in a written order.  tests/reg_cases.py restates all of it in numpy; vista_slam_amd/meshdist.py (reg_plan,
 * TriIndex.register_pass, RegRecord, plane_step, icp) and evaluate.eval_mesh(refine=) sit on top.
 *
 * This is a tenth library with its own translation unit (vista_slam_amd/csrc/sta_reg.hip, kernels in csrc/reg.h, which includes
 * sta_common.h alone), its own ctypes table (_lib.REG_SIGNATURES) and its own inventories (tests/test_reg_abi.py,
 * tests/reg_stream_cases.py).  It READS the index that sta_tri_build of include/sta_dist.h wrote and neither rebuilds nor changes it; it
 * includes no file of that library: the index comes in as plain arguments and the three constants it needs are restated below
 * (tests/test_reg_abi.py holds them against sta_dist.h).  None of the other nine libraries includes or links any of this.
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name is sizes_out or ends in _host; every buffer,
 *     the workspace included, is the caller's; NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_reg_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is
 *     contracted into an FMA.  float(x) rounds a float64 to float32 once.  dot(x, y) = (x_0 * y_0 + x_1 * y_1) + x_2 * y_2 everywhere.
 *   - Every device loop carries a bound taken from the arguments or from the level count; no kernel waits for another lane's progress;
 *     there is no floating-point atomic.  The one atomic of the library is the integer OR into `status`.
 *
 * The index (sta_tri_index of include/sta_dist.h, field by field): tri [nt,9] float32, the corners A, B, C of the triangle at every
 * sorted position; src [nt] int32, its input index; boxes [nodes,6] float32, lo xyz, hi xyz of every node, a node without a valid
 * triangle having lo = +inf, hi = -inf; counters int32, of which entry STA_REG_N_VALID alone is read: the sorted positions
 * [0, N_VALID) are the VALID triangles, and only those are ever scored or returned.  Levels, counts and offsets follow from nt alone:
 * count[0] = ceil(nt / F), count[l + 1] = ceil(count[l] / F), levels = the first l + 1 with count[l] == 1, the nodes of level l begin
 * at the sum of the counts below it; level-0 node j covers the sorted positions [F j, F j + F), a node above the nodes [F j, F j + F)
 * of the level below.
 *
 * 1. The query.  x, y, z = the doubles of qry[i] (float32 [Q,3]); T = T_host, 12 host doubles, a row-major 3x4 matrix, NULL = the
 *    identity (evaluated like any other):
 *      q'_x = ((T00 * x + T01 * y) + T02 * z) + T03, likewise q'_y and q'_z      - the formula and order of sta_nn_query (sta_cloud.h).
 *    q' IS NOT ROUNDED TO FLOAT32: the search runs on the three doubles.  A q' with a coordinate that is not finite is a NON-FINITE
 *    query: it is unmatched and counted in record[19], not in record[0].
 *
 * 2. The search: sta_tri_query's contract (include/sta_dist.h) with q' in place of q.  For every VALID triangle with corners a, b, c
 *    (the doubles of its float32 coordinates):
 *      Closest point (Ericson, Real-Time Collision Detection, ClosestPtPointTriangle; the first rule that applies decides):
 *        ab = b - a, ac = c - a, ap = q' - a;  d1 = dot(ab, ap), d2 = dot(ac, ap)
 *          d1 <= 0 and d2 <= 0:                                    p = a
 *        bp = q' - b;  d3 = dot(ab, bp), d4 = dot(ac, bp)
 *          d3 >= 0 and d4 <= d3:                                   p = b
 *        vc = d1 * d4 - d3 * d2
 *          vc <= 0 and d1 >= 0 and d3 <= 0:   v = d1 / (d1 - d3);  p_k = a_k + ab_k * v
 *        cp = q' - c;  d5 = dot(ab, cp), d6 = dot(ac, cp)
 *          d6 >= 0 and d5 <= d6:                                   p = c
 *        vb = d5 * d2 - d1 * d6
 *          vb <= 0 and d2 >= 0 and d6 <= 0:   w = d2 / (d2 - d6);  p_k = a_k + ac_k * w
 *        va = d3 * d6 - d5 * d4;  e1 = d4 - d3, e2 = d5 - d6
 *          va <= 0 and e1 >= 0 and e2 >= 0:   w = e1 / (e1 + e2);  p_k = b_k + (c_k - b_k) * w
 *        otherwise:  denom = 1 / ((va + vb) + vc), v = vb * denom, w = vc * denom;  p_k = (a_k + ab_k * v) + ac_k * w
 *        (every comparison is false for NaN, so a NaN falls through to the last rule.)
 *      Clamp.  lo_k / hi_k = the min / max of a_k, b_k, c_k.  c_k = p_k if p_k >= lo_k, else lo_k; then c_k = hi_k unless c_k <= hi_k.
 *        THE CLAMP IS PART OF THE CONTRACT: it is what makes the search exact.
 *      Distance.  dx = q'_x - c_x, dy = q'_y - c_y, dz = q'_z - c_z;  d2 = (dx * dx + dy * dy) + dz * dz.
 *      Qualification and ties.  The triangle QUALIFIES iff d2 <= r2 with r2 = radius * radius (false for NaN; radius may be +inf).  The
 *        answer is the qualifying triangle of the smallest d2; among equal d2, the one of the lowest input index t.  A query with an
 *        answer has FOUND a triangle.
 *    Why the search equals the brute-force minimum: the no-margin argument of include/sta_dist.h.  A node's lower bound for q' is
 *        e_k = max(max(lo_k - q'_k, q'_k - hi_k), 0) per axis,  bound = (e_x * e_x + e_y * e_y) + e_z * e_z,
 *    the clamped c lies inside the float32 box of its triangle and of every node above it exactly, float64 subtraction, multiplication
 *    of non-negative numbers and addition are monotone, so the computed bound is <= the computed d2 of every triangle under the node.
 *    THAT ARGUMENT NOWHERE USES THAT q IS A FLOAT32 - only that the same three doubles enter the bound and d2 - so it carries over to
 *    q' as it stands: a node is skipped exactly when it is empty or bound > best (which starts at r2), a node whose bound equals
 *    the best is still visited, for the tie rule.
 *    The traversal is this library's own and does not show in the outputs.  One lane per query.  It first walks down from the root, at
 *    every level into the non-empty child of the smallest bound, among equal bounds the one whose box centre is nearest (<= levels
 *    steps), and scores that leaf.  Then it visits the nodes in depth-first index order WITHOUT A STACK: the node after (l, j) is
 *    (l, j + 1) when j + 1 is a sibling, else the node after its parent; the state is two integers.  The loop is bounded by
 *    nodes + 1 visits; a lane that reaches the bound ORs STA_REG_STATUS_BOUND into `status`, is unmatched, and leaves.  It never spins.
 *    tests/test_reg_gpu.py holds d2_out, tri_out and point_out with T = NULL against sta_tri_query of the same points by array_equal:
 *    the two statements of the search cannot drift apart.
 *
 * 3. The plane of the winning triangle, from the float32 corners A, B, C at its sorted position (doubles), as include/sta_dist.h
 *    writes w_t:
 *      u = B - A, v = C - A, n = (u_y * v_z - u_z * v_y, u_z * v_x - u_x * v_z, u_x * v_y - u_y * v_x),
 *      w = sqrt((n_x * n_x + n_y * n_y) + n_z * n_z)      (finite and > 0: the triangle is valid),      nhat_k = n_k / w.
 *      d = q' - c: the dx, dy, dz of d2.      r = dot(d, nhat)      - the signed distance to the plane THROUGH THE CLOSEST POINT; for a
 *      closest point inside the triangle |r| is the distance, on an edge or a corner it is smaller than sqrt(d2).
 *      x = q' - pivot, pivot = pivot_host, 3 host doubles, NULL = (0, 0, 0).
 *      J = (x_y * nhat_z - x_z * nhat_y, x_z * nhat_x - x_x * nhat_z, x_x * nhat_y - x_y * nhat_x, nhat_x, nhat_y, nhat_z)
 *      - the derivative of r under q' -> Exp(omega)(q' - pivot) + pivot + v at (omega, v) = 0, the closest point held fixed.
 *
 * 4. Normal agreement, optional: qnrm [Q,3] float32 or NULL.  With n_q = the doubles of qnrm[i] and R the 3x3 of T (T NULL: the
 *    identity), m_k = (R_k0 * n_q0 + R_k1 * n_q1) + R_k2 * n_q2.  A query that FOUND a triangle is REJECTED iff
 *      dot(m, nhat) < min_cos * sqrt(dot(m, m))
 *    (false for NaN: a NaN normal rejects nothing).  Rejection happens AFTER the search, as Open3D's correspondence checkers do: the
 *    nearest triangle is not replaced by a farther one that agrees.  A rejected query is counted in record[20], is not matched, and
 *    contributes r2 to record[3].  With qnrm == NULL nothing is rejected and min_cos is only checked.
 *    A query is MATCHED iff it found a triangle and was not rejected.
 *
 * 5. Per-query outputs (any may be NULL): d2_out [Q] float64 = d2, tri_out [Q] int32 = the input index t, point_out [Q,3] float32 =
 *    float(c), resid_out [Q] float64 = r - of the triangle FOUND, also for a rejected query; +inf, -1, three NaNs and NaN when no
 *    triangle qualifies or the query is non-finite.
 *
 * 6. The record.  record_out: STA_REG_RECORD = 64 device doubles (NULL = none; then work may be NULL).
 *      [0] finite queries   [1] matched queries   [2] sum d2 over matched   [3] sum min(d2, r2) over finite queries: a matched one
 *      contributes d2, an unmatched or rejected one r2
 *      over matched queries:  [4..6] sum q'   [7..9] sum c   [10..18] sum q' c^T (row-major, row = axis of q')
 *      [19] non-finite queries   [20] rejected queries
 *      over matched queries:  [21] sum r * r   [22] sum |r|   [23..28] g = sum J_k * r   [29..49] the upper triangle of
 *      H = sum J J^T, row-major: (0,0) (0,1) .. (0,5) (1,1) .. (5,5), each term J_a * J_b      [50..63] 0.
 *    Entries 0 .. 19 are laid out as the record of sta_nn_query (include/sta_cloud.h): cloud.kabsch takes it as it is.  c in the sums is
 *    the float64 closest point, not float(c).  Only matched queries contribute beyond entry 3.
 *    Reduction, without floating-point atomics, in an order that depends on Q alone (two calls are bit-identical; inputs whose float64
 *    sums are exact give exact sums): one lane per query, 256 queries per workgroup; per entry a xor butterfly over the 64 lanes of a
 *    wave (offsets 32, 16, .. 1, a + b on both sides), the four waves through LDS as ((w0 + w1) + w2) + w3: one partial row of 64
 *    doubles per workgroup in `work`.  A second launch of one workgroup of 256 threads folds the ceil(Q / 256) rows: thread t adds the
 *    rows t, t + 256, .. in ascending order, then the same butterfly and the same four waves.
 */
#ifndef STA_REG_H
#define STA_REG_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_REG_FANOUT 8                /* F: STA_DIST_FANOUT of the index */
#define STA_REG_MAX_LEVELS 9            /* STA_DIST_MAX_LEVELS: F^9 = 2^27 > nt */
#define STA_REG_N_VALID 0               /* STA_DIST_N_VALID: the entry of the index's counters that is read */
#define STA_REG_PLAN_SIZES 2
#define STA_REG_RECORD 64               /* doubles in a record and in a partial row */
#define STA_REG_STATUS_BOUND 1          /* bit 0 of status[0]: a traversal reached its bound of (number of nodes + 1) visits; cannot happen */

/* The layout of `sizes_out` of sta_reg_plan: STA_REG_PLAN_SIZES int64. */
typedef struct sta_reg_sizes {
    int64_t nodes;
    int64_t work_bytes;
} sta_reg_sizes;

/* Host only, no GPU.  sizes_out[0] = the number of nodes of the index of nt triangles, sizes_out[1] = bytes of `work` of
 * sta_reg_pass for Q queries: ceil(Q / 256) partial rows of STA_REG_RECORD doubles.
 * Refuses, with the numbers in the message: nt outside [1, 2^27); Q outside [1, 2^30). */
STA_API int sta_reg_plan(int64_t nt, int64_t Q, int64_t* sizes_out);

/* One pass: rules 1 to 6 for the queries qry[i], i < Q, under T_host about pivot_host.
 * T_host and pivot_host are HOST memory, read during the call only.  status [1] int32 belongs to the caller, who clears it; the call
 * only ever ORs STA_REG_STATUS_BOUND into it.  work: sizes_out[1] bytes of sta_reg_plan when record_out is given; its contents before
 * and after the call mean nothing.
 * Refused, with the numbers in the message: nt outside [1, 2^27); Q outside [1, 2^30); a radius that is < 0 or NaN (+inf is allowed);
 * a NaN min_cos; with record_out, a null work or work_bytes below the plan's; a null tri, src, boxes, counters, qry or status. */
STA_API int sta_reg_pass(const float* tri, const int32_t* src, const float* boxes, const int32_t* counters, int64_t nt, const float* qry,
                         const float* qnrm, int64_t Q, const double* T_host, const double* pivot_host, double radius, double min_cos,
                         double* d2_out, int32_t* tri_out, float* point_out, double* resid_out, double* record_out, void* work,
                         int64_t work_bytes, int32_t* status, void* stream);

STA_API const char* sta_reg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
