/*
 * sta_dist.h - C ABI of libsta_dist.so: the exact distance from a point to a triangle mesh.  sta_tri_build sorts the triangles along a
 * Morton curve and fits an implicit bounding-volume hierarchy over the sorted order; sta_tri_query returns, for every query point, the
 * nearest point of the mesh, its squared distance and its triangle - the BRUTE-FORCE minimum over all valid triangles, reached through the
 * hierarchy without any margin (the argument is below).  Keys, order and boxes are integers and float32 min / max; the closest point is
 * float64 operations in a written order: every output is defined bit for bit by this header.  tests/dist_cases.py restates all of it in
 * numpy; vista_slam_amd/meshdist.py (plan, TriIndex, point_to_mesh) and evaluate.eval_mesh(mode="surface") sit on top.
 *
 * This is an eighth library with its own translation unit (vista_slam_amd/csrc/sta_dist.hip, kernels in csrc/dist.h, which includes
 * voxel.h, select.h, elementwise.h and sta_common.h unchanged), its own ctypes table (_lib.DIST_SIGNATURES) and its own inventories
 * (tests/test_dist_abi.py, tests/dist_stream_cases.py).  None of the other seven libraries includes or links any of it.
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name is sizes_out, index_out_host or index_host;
 *     every buffer, the workspace included, is the caller's; NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_tri_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order on the doubles of the
 *     float32 inputs; nothing is contracted into an FMA.  float(x) rounds a float64 to float32 once.
 *     dot(x, y) = (x_0 * y_0 + x_1 * y_1) + x_2 * y_2 everywhere.
 *   - Every device loop carries a bound taken from the arguments or from the level count; no kernel waits for another lane's progress;
 *     there is no floating-point atomic.
 *   - verts [nv,3] float32, tris [nt,3] int32, qry [Q,3] float32.
 *
 * A triangle t = (i0, i1, i2) is VALID iff (1) its three indices are in [0, nv), (2) its nine coordinates are finite and (3) w_t, exactly
 * as include/sta_surf.h writes it (u = B - A, v = C - A, n = (u_y * v_z - u_z * v_y, u_z * v_x - u_x * v_z, u_x * v_y - u_y * v_x),
 * w_t = sqrt((n_x * n_x + n_y * n_y) + n_z * n_z)), is finite and > 0.  A triangle that fails (1) is a BAD-INDEX triangle, one that passes
 * (1) and fails (2) a NON-FINITE one, one that passes both and fails (3) one WITHOUT AREA.  Only valid triangles are ever returned.
 *
 * What it is not.  No signed distance (no inside / outside), no ray casting, no point-to-plane ICP against the mesh.  It was not compared
 * with Open3D's RaycastingScene.compute_closest_points or trimesh's closest_point: neither is available; tests/test_meshdist_cpu.py holds the
 * restatement against a second, independent statement in extended precision.
 */
#ifndef STA_DIST_H
#define STA_DIST_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_DIST_FANOUT 8               /* F: the sorted triangles of a level-0 node and the children of every node above */
#define STA_DIST_MAX_LEVELS 9           /* F^9 = 2^27 > nt */
#define STA_DIST_KEY_BITS 21            /* bits per axis of the Morton key */
#define STA_DIST_PLAN_SIZES 2
#define STA_DIST_COUNTERS 8
/* the layout of `counters` (int32) */
#define STA_DIST_N_VALID 0
#define STA_DIST_N_BAD_INDEX 1
#define STA_DIST_N_NON_FINITE 2
#define STA_DIST_N_NO_AREA 3
#define STA_DIST_STATUS 4               /* 0, or STA_DIST_STATUS_BOUND; entries 5 .. 7 are 0 */
#define STA_DIST_STATUS_BOUND 1         /* bit 0: a traversal reached its bound of (number of nodes + 1) visits; cannot happen, see below */

/* The layout of `sizes_out` of sta_tri_plan: STA_DIST_PLAN_SIZES int64. */
typedef struct sta_dist_sizes {
    int64_t index_bytes;
    int64_t build_work_bytes;
} sta_dist_sizes;

/* The index on the host: pointers into index_buf and the shape of the tree.  Everything but the base address follows from nt alone.
 *   level l has count[l] nodes: count[0] = ceil(nt / F), count[l + 1] = ceil(count[l] / F); levels = the first l + 1 with count[l] == 1.
 *   level_offset[0] = 0, level_offset[l + 1] = level_offset[l] + count[l]; level_offset[levels] = the number of nodes.
 *   The struct holds no device state: copying it is copying the index's address. */
typedef struct sta_tri_index {
    float* tri;                 /* [nt,9]  the coordinates A, B, C of the triangle at every sorted position (NaN for one that is not valid) */
    int32_t* src;               /* [nt]    the input index of the triangle at every sorted position */
    float* boxes;               /* [nodes,6] lo_x, lo_y, lo_z, hi_x, hi_y, hi_z of node level_offset[l] + j */
    int32_t* counters;          /* [STA_DIST_COUNTERS] the index's own copy of counters_out; queries read N_VALID and OR into STATUS here */
    int64_t nt;
    int32_t levels;
    int32_t reserved;
    int64_t level_offset[STA_DIST_MAX_LEVELS + 1];
} sta_tri_index;

/* Host only, no GPU.  sizes_out[0] = bytes of index_buf, sizes_out[1] = bytes of `work` of sta_tri_build (sort buffers, partial bounds;
 * every part rounded up to 256 bytes).  Q is only checked: a query takes no workspace.
 * Refuses, with the numbers in the message: nt outside [1, 2^27); Q outside [1, 2^30).  (nv is an argument of sta_tri_build, which refuses
 * it outside [1, 2^31).) */
STA_API int sta_tri_plan(int64_t nt, int64_t Q, int64_t* sizes_out);

/* Build.  The result is a function of verts and tris alone: not of scheduling, not of what index_buf or work held.
 *   counters_out [8] int32: N_VALID, N_BAD_INDEX, N_NON_FINITE, N_NO_AREA (their sum is nt), STATUS = 0, three zeros.
 *   Key.  For a valid triangle and per axis k: m_k = (double(min_k) + double(max_k)) * 0.5 with min_k / max_k over its three float32
 *     coordinates.  L_k / U_k = the min / max of m_k over all valid triangles (exact, order-free).
 *     g_k = floor(((m_k - L_k) / (U_k - L_k)) * 2097152.0), then 2^21 - 1 where it is larger and 0 where it is smaller; 0 where U_k == L_k.
 *     key = the Morton interleave: bit b of g_x is bit 3 b, of g_y bit 3 b + 1, of g_z bit 3 b + 2 (63 bits).
 *     A triangle that is not valid has the key 2^63.
 *   Order.  (key, t) through the stable LSD radix sort of csrc/voxel.h over all 64 bits: ascending key, equal keys in ascending t.  So the
 *     valid triangles are the sorted positions [0, N_VALID).  src[i] = the t at position i; tri[i] = its nine float32 coordinates, nine
 *     NaNs for a position >= N_VALID.
 *   Tree.  Implicit: level-0 node j covers the sorted positions [F j, F j + F) (below nt), a level-(l + 1) node j covers the level-l nodes
 *     [F j, F j + F) (below count[l]).  A node's box is the float32 min / max over the vertices of its valid triangles; a node without a
 *     valid triangle has the box lo = (+inf, +inf, +inf), hi = (-inf, -inf, -inf).  One launch per level: a lane per node reads its F
 *     children; no pointers, no arrival counters, no atomics.
 *   index_out_host: written on the host before the call returns (the addresses are a layout of index_buf, the rest follows from nt).
 * work: sizes_out[1] bytes of sta_tri_plan; its contents before and after the call mean nothing.
 * Refused, with the numbers in the message: nt outside [1, 2^27); nv outside [1, 2^31); index_bytes or work_bytes below the plan's; a
 * null pointer. */
STA_API int sta_tri_build(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, void* index_buf, int64_t index_bytes, void* work,
                          int64_t work_bytes, sta_tri_index* index_out_host, int32_t* counters_out, void* stream);

/* Query.  For query q = the doubles of qry[i] and every VALID triangle with corners a, b, c (doubles of its float32 coordinates):
 *   Closest point (Ericson, Real-Time Collision Detection, ClosestPtPointTriangle; the first rule that applies decides):
 *     ab = b - a, ac = c - a, ap = q - a;  d1 = dot(ab, ap), d2 = dot(ac, ap)
 *       d1 <= 0 and d2 <= 0:                                    p = a
 *     bp = q - b;  d3 = dot(ab, bp), d4 = dot(ac, bp)
 *       d3 >= 0 and d4 <= d3:                                   p = b
 *     vc = d1 * d4 - d3 * d2
 *       vc <= 0 and d1 >= 0 and d3 <= 0:   v = d1 / (d1 - d3);  p_k = a_k + ab_k * v
 *     cp = q - c;  d5 = dot(ab, cp), d6 = dot(ac, cp)
 *       d6 >= 0 and d5 <= d6:                                   p = c
 *     vb = d5 * d2 - d1 * d6
 *       vb <= 0 and d2 >= 0 and d6 <= 0:   w = d2 / (d2 - d6);  p_k = a_k + ac_k * w
 *     va = d3 * d6 - d5 * d4;  e1 = d4 - d3, e2 = d5 - d6
 *       va <= 0 and e1 >= 0 and e2 >= 0:   w = e1 / (e1 + e2);  p_k = b_k + (c_k - b_k) * w
 *     otherwise:  denom = 1 / ((va + vb) + vc), v = vb * denom, w = vc * denom;  p_k = (a_k + ab_k * v) + ac_k * w
 *     (every comparison is false for NaN, so a NaN falls through to the last rule.)
 *   Clamp.  lo_k / hi_k = the min / max of a_k, b_k, c_k.  c_k = p_k if p_k >= lo_k, else lo_k; then c_k = hi_k unless c_k <= hi_k.
 *     (So a NaN becomes lo_k: c always lies inside the triangle's box.)  THE CLAMP IS PART OF THE CONTRACT: it is what makes the search
 *     exact.
 *   Distance.  dx = q_x - c_x, dy = q_y - c_y, dz = q_z - c_z;  d2 = (dx * dx + dy * dy) + dz * dz.
 *   Qualification and ties.  The triangle QUALIFIES iff d2 <= r2 with r2 = radius * radius (false for NaN).  The answer is the qualifying
 *     triangle of the smallest d2; among equal d2, the one of the lowest input index t.
 *   Outputs (any of the three may be NULL): d2_out [Q] float64 = its d2, tri_out [Q] int32 = its t, point_out [Q,3] float32 = float(c).
 *     When nothing qualifies, or for a query with a coordinate that is not finite: +inf, -1 and three NaNs.
 *   radius may be +inf.  There is no limit tied to a cell size.
 *
 * Why the search equals the brute-force minimum.  A node's lower bound for q is
 *     e_k = max(max(lo_k - q_k, q_k - hi_k), 0) per axis,  bound = (e_x * e_x + e_y * e_y) + e_z * e_z     - the order of d2's sum.
 *   The clamped c of a triangle lies inside the triangle's box EXACTLY (the clamp compares against the very float32 values the box is the
 *   min / max of), and that box lies inside the box of every ancestor (min / max of float32 are exact).  So lo_k <= c_k <= hi_k for every
 *   node above the triangle, hence |q_k - c_k| >= e_k >= 0 in real numbers, and since float64 subtraction is monotone in each operand
 *   the COMPUTED |d_k| >= the COMPUTED e_k; float64 multiplication of non-negative numbers and float64 addition are monotone too, and the
 *   two sums have the same shape.  So the computed bound is <= the computed d2 of every triangle under the node, with no margin at all.
 *   A node may therefore be skipped exactly when bound > best, the best (d2) so far, which starts at r2: nothing under it can win or tie.
 *   A node whose bound EQUALS the best must still be visited, for the tie rule.  A node without a valid triangle is never entered (its
 *   bound is +inf; it is skipped by its empty box, so also when best is +inf).
 *   How the traversal runs does not show in the outputs.  One lane per query.  It first walks down from the root, at every level into
 *   the non-empty child of the smallest bound, among equal bounds the one whose box centre is nearest (<= levels steps), and scores that leaf: a good first `best`.  Then it visits the nodes in
 *   depth-first index order WITHOUT A STACK: the tree is implicit, so the node after (l, j) is (l, j + 1) when j + 1 is a sibling, else
 *   the node after its parent; the state is two integers.  Every node is visited at most once: the loop is bounded by nodes + 1 visits
 *   and a lane that reaches the bound sets STA_DIST_STATUS_BOUND in the index's counters and leaves.  It never spins.
 * Refused, with the numbers in the message: Q outside [1, 2^30); a radius that is < 0 or NaN; a null index_host or qry; an index whose
 * nt, levels or pointers are not those of a build. */
STA_API int sta_tri_query(const sta_tri_index* index_host, const float* qry, int64_t Q, double radius, double* d2_out, int32_t* tri_out,
                          float* point_out, void* stream);

STA_API const char* sta_tri_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
