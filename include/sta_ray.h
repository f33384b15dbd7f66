/*
 * sta_ray.h - C ABI of libsta_ray.so: rays against a triangle mesh.  sta_ray_cast returns, for every ray, the FIRST HIT - the
 * qualifying triangle of the smallest ray parameter, BRUTE FORCE over all valid triangles, reached through the hierarchy without any
 * margin (the argument is below); sta_ray_occluded says whether any triangle qualifies.  Every output is defined bit for bit by this
 * header: float64 operations in a written order on the doubles of the float32 inputs.  tests/ray_cases.py restates all of it in numpy;
 * vista_slam_amd/meshdist.py (TriIndex.cast, TriIndex.occluded, ray_cast, camera_rays, ray_depth, visible) and
 * evaluate.pointmap_range_error / mesh_depth_l1(method="rays") sit on top.
 *
 * This is a ninth library with its own translation unit (vista_slam_amd/csrc/sta_ray.hip, kernels in csrc/ray.h, which includes
 * sta_common.h alone), its own ctypes table (_lib.RAY_SIGNATURES) and its own inventories (tests/test_ray_abi.py,
 * tests/ray_stream_cases.py).  It READS the index that sta_tri_build of include/sta_dist.h wrote and neither rebuilds nor changes it; it
 * includes no file of that library: the index comes in as plain arguments and the three constants it needs are restated below
 * (tests/test_ray_abi.py holds them against sta_dist.h).  None of the other eight libraries includes or links any of this.
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name is sizes_out; every buffer is the caller's;
 *     NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES.  A cast takes no workspace.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_ray_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order on the doubles of the
 *     float32 inputs; nothing is contracted into an FMA.  float(x) rounds a float64 to float32 once.  max(a, b) below is
 *     `b > a ? b : a` and min(a, b) is `b < a ? b : a`, folded from the left.
 *   - Every device loop carries a bound taken from the arguments or from the level count; no kernel waits for another lane's progress;
 *     there is no floating-point atomic.  The one atomic of the library is the integer OR into `status`.
 *
 * The index (sta_tri_index of include/sta_dist.h, field by field): tri [nt,9] float32, the corners A, B, C of the triangle at every
 * sorted position; src [nt] int32, its input index; boxes [nodes,6] float32, lo xyz, hi xyz of every node, a node without a valid
 * triangle having lo = +inf, hi = -inf; counters int32, of which entry STA_RAY_N_VALID alone is read: the sorted positions
 * [0, N_VALID) are the VALID triangles, and only those are ever tested or returned.  Levels, counts and offsets follow from nt alone:
 * count[0] = ceil(nt / F), count[l + 1] = ceil(count[l] / F), levels = the first l + 1 with count[l] == 1, the nodes of level l begin
 * at the sum of the counts below it; level-0 node j covers the sorted positions [F j, F j + F), a node above the nodes [F j, F j + F)
 * of the level below.
 *
 * A ray is x(t) = o + t d with o = org[i], d = dir[i] as given - d is NOT normalised, so t is in units of |d|: a segment A -> B is
 * o = A, d = B - A, t in [0, 1]; with a d whose camera-space z is 1, t is the depth.
 *
 * 1. A usable ray.  Its six numbers are finite and d is not (0, 0, 0).  Any other ray is unmatched.
 *
 * 2. The slab interval of a box (lo, hi: float32) for a ray.  The box is widened by one float32 step outward:
 *      lo'_k = nextafterf(lo_k, -inf), hi'_k = nextafterf(hi_k, +inf).
 *    enter = t_min, exit = t_max; then for k = x, y, z in this order:
 *      d_k != 0:  inv_k = 1 / d_k;  (near, far) = (lo'_k, hi'_k) if d_k > 0, else (hi'_k, lo'_k);
 *                 tn_k = (near - o_k) * inv_k,  tf_k = (far - o_k) * inv_k;  enter = max(enter, tn_k),  exit = min(exit, tf_k)
 *      d_k == 0:  the axis passes iff lo'_k <= o_k and o_k <= hi'_k; it contributes no bound.
 *    The box PASSES iff every zero axis passes and enter <= exit.  A float32 d_k, even a subnormal one, has a finite non-zero float64
 *    reciprocal, and a widened bound is never NaN, so no NaN arises for a usable ray.
 *
 * 3. The triangle test: Woop, Benthin and Wald's sheared 2-D form (Watertight Ray/Triangle Intersection, JCGT 2013), not the 3-D triple
 *    product.  Per ray: kz = the first axis of the largest |d_k|, kx = (kz + 1) % 3, ky = (kz + 2) % 3;
 *      Sx = d_kx / d_kz,  Sy = d_ky / d_kz,  Sz = 1 / d_kz.
 *    Per vertex P (A, B and C alike), P' = P - o per component:
 *      Px = P'_kx - Sx * P'_kz,  Py = P'_ky - Sy * P'_kz,  Pz = Sz * P'_kz.
 *    Edge values:  U = Cx * By - Cy * Bx,  V = Ax * Cy - Ay * Cx,  W = Bx * Ay - By * Ax;  det = (U + V) + W.
 *    The test passes iff (U >= 0 and V >= 0 and W >= 0) or (U <= 0 and V <= 0 and W <= 0) - two-sided - and det != 0 (every comparison
 *    is false for NaN).  Then
 *      t = ((U * Az + V * Bz) + W * Cz) / det,   bary = (float(U / det), float(V / det), float(W / det)).
 *    A vertex gets ONE computed 2-D position per ray, whatever triangle names it, and an edge value is an exact negation under exchange
 *    of its two vertices: a ray cannot pass between two triangles that share an edge or a vertex.  A hit on a shared edge is accepted
 *    by both, and the tie rule picks one.
 *
 * 4. Qualification.  A VALID triangle qualifies iff
 *      (a) its own box passes rule 2 - own box: lo_k / hi_k = the float32 min / max of its three k coordinates, widened as there -
 *          with enter_own and exit_own,
 *      (b) rule 3 passes, and
 *      (c) t_min <= t and t <= t_max for the raw t (false for NaN).
 *    Its answer is t_c = min(max(t, enter_own), exit_own), i.e. `t >= enter_own ? t : enter_own`, then `<= exit_own ? that : exit_own`.
 *    THE OWN-BOX TEST AND THE CLAMP ARE PART OF THE CONTRACT: they are what makes the search exact.
 *
 * 5. Answer.  The qualifying triangle of the smallest t_c; among equal t_c, the one of the lowest input index.
 *    Outputs of sta_ray_cast (any of the three may be NULL): t_out [R] float64 = its t_c, tri_out [R] int32 = its input index,
 *    bary_out [R,3] float32 = its bary (the weights of A, B, C).  A ray without a qualifying triangle, or one that is not usable, gets
 *    +inf, -1 and three NaNs.  sta_ray_occluded writes occ_out [R] uint8 = 1 iff some triangle qualifies, else 0: the same kernel, leaving at the first
 *    qualifying triangle it meets.
 *
 * 6. Why the search equals brute force.  A node's float32 box contains the boxes of everything below it exactly (min / max of float32
 *    are exact), and nextafterf is monotone, so the same holds for the widened boxes.  Float64 subtraction is monotone in each operand
 *    and so is multiplication by a number of fixed sign: per axis, for d_k > 0, lo'_node <= lo'_own gives
 *    (lo'_node - o_k) * inv_k <= (lo'_own - o_k) * inv_k in the COMPUTED values, and for d_k < 0 hi'_node >= hi'_own gives the same
 *    after the multiplication by the negative inv_k; likewise tf_node >= tf_own.  A zero axis that passes for the own box passes for the
 *    node.  max and min are monotone, so
 *        enter_node <= enter_own <= t_c <= exit_own <= exit_node        for every node above a qualifying triangle,
 *    with no margin at all: such a node passes rule 2.  A node may therefore be skipped exactly when it is empty, or fails rule 2, or
 *    enter_node > best, the best t_c so far (+inf at the start): nothing under it can win or tie.  A node with enter_node == best must
 *    still be visited, for the tie rule.  How the traversal runs does not show in the outputs.  One lane per ray.  It first walks down
 *    from the root, at every level into the passing child of the smallest enter (the first among equals; <= levels steps), and tests
 *    that leaf: a good first `best`.  Then it visits the nodes in depth-first index order WITHOUT A STACK: the tree is implicit, so the
 *    node after (l, j) is (l, j + 1) when j + 1 is a sibling, else the node after its parent; the state is two integers.  Every node
 *    is visited at most once: the loop is bounded by nodes + 1 visits, and a lane that reaches the bound ORs STA_RAY_STATUS_BOUND into
 *    `status`, writes the unmatched answer and leaves.  It never spins.
 *
 * What it is not.  No signed distance and no crossing parity (a hit on a shared edge is accepted by both neighbours by design, so
 * counting hits does not count crossings), no all-hits list, no point-to-plane ICP against the mesh.  It was not compared with Open3D's
 * RaycastingScene.cast_rays / test_occlusions: they are not available; tests/test_ray_cpu.py holds the restatement against a second,
 * independent statement (Moeller-Trumbore in extended precision) and asserts the chain of rule 6 exactly.
 */
#ifndef STA_RAY_H
#define STA_RAY_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_RAY_FANOUT 8                /* F: STA_DIST_FANOUT of the index */
#define STA_RAY_MAX_LEVELS 9            /* STA_DIST_MAX_LEVELS: F^9 = 2^27 > nt */
#define STA_RAY_N_VALID 0               /* STA_DIST_N_VALID: the entry of the index's counters that is read */
#define STA_RAY_PLAN_SIZES 1
#define STA_RAY_STATUS_BOUND 1          /* bit 0 of status[0]: a traversal reached its bound of (number of nodes + 1) visits; cannot happen */

/* The layout of `sizes_out` of sta_ray_plan: STA_RAY_PLAN_SIZES int64. */
typedef struct sta_ray_sizes {
    int64_t nodes;
} sta_ray_sizes;

/* Host only, no GPU.  sizes_out[0] = the number of nodes of the index of nt triangles (a cast takes no workspace: there are no bytes
 * to report).  Refuses, with the numbers in the message: nt outside [1, 2^27); R outside [1, 2^30). */
STA_API int sta_ray_plan(int64_t nt, int64_t R, int64_t* sizes_out);

/* First hit of the rays (org[i], dir[i]), i < R, in [t_min, t_max] (both inclusive; t_max may be +inf): rules 1 to 6.
 * status [1] int32 belongs to the caller, who clears it; the call only ever ORs STA_RAY_STATUS_BOUND into it.
 * Refused, with the numbers in the message: nt outside [1, 2^27); R outside [1, 2^30); t_min < 0, t_min > t_max or a NaN among them;
 * a null tri, src, boxes, counters, org, dir or status. */
STA_API int sta_ray_cast(const float* tri, const int32_t* src, const float* boxes, const int32_t* counters, int64_t nt, const float* org,
                         const float* dir, int64_t R, double t_min, double t_max, double* t_out, int32_t* tri_out, float* bary_out,
                         int32_t* status, void* stream);

/* occ_out[i] = 1 iff some valid triangle qualifies for ray i in [t_min, t_max], else 0 (also for a ray that is not usable).  The
 * refusals of sta_ray_cast, and a null occ_out. */
STA_API int sta_ray_occluded(const float* tri, const int32_t* src, const float* boxes, const int32_t* counters, int64_t nt, const float* org,
                             const float* dir, int64_t R, double t_min, double t_max, uint8_t* occ_out, int32_t* status, void* stream);

STA_API const char* sta_ray_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
