/*
 * sta_surf.h - C ABI of libsta_surf.so: what a fused mesh needs before it is shown or scored.  sta_surf_components labels the connected
 * components of an indexed triangle mesh (so that floaters - small blobs and shell fragments in free space - can be dropped by size);
 * sta_surf_weights and sta_surf_sample draw points uniformly by area from its surface (so that a mesh can be scored the way the 7-Scenes
 * and Replica evaluations score one: samples against samples).  Labels and counts are integers; the sampler is a counter-based integer
 * generator plus float64 operations in a written order: every output is defined bit for bit by this header.  tests/surf_cases.py restates
 * all of it in numpy; vista_slam_amd/surface.py (components, clean_mesh, area, sample_surface) and vista_slam_amd/evaluate.py (eval_mesh)
 * sit on top.
 *
 * This is a sixth library with its own translation unit (vista_slam_amd/csrc/sta_surf.hip, kernels in csrc/surf.h, which includes
 * sta_common.h unchanged), its own ctypes table (_lib.SURF_SIGNATURES) and its own inventories (tests/test_surf_abi.py,
 * tests/surf_stream_cases.py).  None of the other five libraries includes or links any of it.
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name is sizes_out; every buffer, the workspace
 *     included, is the caller's; NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_surf_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is contracted
 *     into an FMA.  sqrt is the IEEE one; float(x) rounds a float64 to float32 once; double(i) of an integer below 2^53 is exact.
 *     uint64 arithmetic is modulo 2^64.
 *   - Every device loop carries a bound taken from the arguments; no kernel waits for another lane's progress.
 *   - verts [nv,3] float32, tris [nt,3] int32.  A triangle is VALID iff all three of its indices are in [0, nv).  Repeated indices are
 *     valid.
 *
 * What it is not (against Open3D's cluster_connected_triangles): two triangles are adjacent here when they share a VERTEX, not only when
 * they share an edge - two shells that touch in one vertex are one component here and two there.  Component areas are not computed.
 */
#ifndef STA_SURF_H
#define STA_SURF_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_SURF_CHUNK 1024             /* the triangles of one chunk of the prefix order of sta_surf_weights */
#define STA_SURF_STATUS_BOUND 1         /* bit 0 of `status`: a find or hooking loop reached its bound of nv + 1 steps */
#define STA_SURF_PLAN_SIZES 3

/* The layout of `sizes_out` of sta_surf_plan: STA_SURF_PLAN_SIZES int64. */
typedef struct sta_surf_sizes {
    int64_t components_work_bytes;
    int64_t weights_work_bytes;
    int64_t sample_work_bytes;      /* always 0 */
} sta_surf_sizes;

/* Host only, no GPU.  sizes_out[0] = bytes of `work` of sta_surf_components (one int32 parent per vertex), sizes_out[1] = bytes of `work`
 * of sta_surf_weights (the chunk sums S and the chunk offsets O), sizes_out[2] = 0: sta_surf_sample takes no workspace and ns is only
 * checked.  Refuses nt, nv or ns outside [0, 2^31), with the numbers in the message. */
STA_API int sta_surf_plan(int64_t nt, int64_t nv, int64_t ns, int64_t* sizes_out);

/* Connected components.  Two vertices are connected iff some valid triangle names both; components are the transitive closure (a
 * triangle with repeated indices still links the distinct vertices it names; a triangle (v, v, v) makes v a component of its own).
 *   vlabel [nv] int32   the smallest vertex index of v's component, or -1 for a vertex that no valid triangle names
 *   tlabel [nt] int32   vlabel[i0] for a valid triangle (i0 its first index), -1 otherwise
 *   tcount [nv] int32   at index r the number of valid triangles with tlabel == r; 0 at every index that is not a component's smallest
 *   status [1]  int32   0, or STA_SURF_STATUS_BOUND when a loop reached its bound (the three arrays then mean nothing)
 * The result is defined by the input alone: not by the order of the triangles, not by scheduling.  Two calls give the same bits.
 * Five launches, no host round trip: parents start as the identity; one lane per triangle unites (i0, i1) and (i0, i2) in a lock-free
 * union-find whose only link is an integer compare-and-swap of the LARGER root under the smaller, so a parent is never larger than its
 * child and the root of a finished component is its smallest index whatever the interleaving; finds halve their path with integer
 * atomic minima; one lane per vertex then finds its root; one lane per triangle writes tlabel and counts with integer atomics (one per
 * distinct label of a wavefront); one lane per vertex writes -1 where a root has no triangle.  A find takes at most nv + 1 steps, a
 * uniting at most nv + 1 retries; beyond that the lane sets status and leaves the loop.
 * work: sizes_out[0] bytes of sta_surf_plan; its contents before and after the call mean nothing.
 * Refused, with the numbers in the message: nt or nv outside [0, 2^31); work_bytes below the plan's; a null pointer that is needed.
 * nt == 0 and nv == 0 launches nothing. */
STA_API int sta_surf_components(const int32_t* tris, int64_t nt, int64_t nv, int32_t* vlabel, int32_t* tlabel, int32_t* tcount, int32_t* status,
                                void* work, int64_t work_bytes, void* stream);

/* Sampling weights and their inclusive prefix.  tri_keep [nt] uint8 or NULL (= every triangle).  Triangle t with indices i0, i1, i2:
 *   A, B, C = the doubles of verts[i0], verts[i1], verts[i2];  u = B - A, v = C - A,
 *   n = (u_y * v_z - u_z * v_y, u_z * v_x - u_x * v_z, u_x * v_y - u_y * v_x),  |n| = sqrt((n_x * n_x + n_y * n_y) + n_z * n_z)
 *   - exactly as include/sta_mesh.h writes them.  w_t = |n| (twice the area), and w_t = 0 for a triangle that is not valid, for one with
 *   tri_keep[t] == 0, and for a |n| that is not finite.
 * Prefix, in chunks of STA_SURF_CHUNK consecutive triangles (chunk c holds t = 1024 c .. 1024 c + 1023; nchunks = ceil(nt / 1024)):
 *   I[t] = the sequential sum, in ascending t, of the w of t's chunk up to and including t (starting from the first w, not from 0 + w)
 *   S[c] = I of the chunk's last element; the elements a last chunk lacks count as 0, so S[c] = I[nt - 1] there
 *   O[0] = 0,  O[c + 1] = O[c] + S[c], ascending
 *   P[t] = O[c] + I[t],   total = O[nchunks]
 * Since float64 addition of non-negative numbers is monotone in each operand, P is non-decreasing (also across a chunk boundary:
 * P[1024 c + 1023] = O[c] + S[c] = O[c + 1] <= O[c + 1] + I[t']), P[t] > P[t - 1] implies w_t > 0, and P[nt - 1] == total bit for bit.
 * Outputs: P [nt] float64, total [1] float64 (0 for nt == 0).
 * Three launches: one wavefront per chunk computes the w into shared memory, one lane sums them in order, all write I and S; one lane
 * sums the S (a loop of nchunks steps); one lane per triangle adds O.
 * work: sizes_out[1] bytes of sta_surf_plan.  Refused: nt or nv outside [0, 2^31); work_bytes below the plan's; a null pointer that is
 * needed. */
STA_API int sta_surf_weights(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, const uint8_t* tri_keep, double* P, double* total,
                             void* work, int64_t work_bytes, void* stream);

/* ns surface samples, stratified over the cumulative area, from P and total of sta_surf_weights OF THE SAME verts, tris AND tri_keep.
 * The generator is splitmix64 as a function of a counter i:
 *   z = seed + i * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
 *   (seed 0: i = 1, 2, 3 give e220a8397b1dcdaf, 6e789e6aa1b965f4, 06c45d188009454f).
 * Sample k, with u_j = double(z(3 k + j + 1) >> 11) * 2^-53 for j = 0, 1, 2 (each in [0, 1)):
 *   Triangle.  x = ((double(k) + u_0) / double(ns)) * total.  t = the smallest index with P[t] > x; if there is none, the smallest index
 *     with P[t] >= total.  Either way P[t] > P[t - 1] (or t == 0 and P[0] > 0), so w_t > 0: a triangle of weight 0 is never chosen.
 *   Position.  r = sqrt(u_1),  b0 = 1 - r,  b1 = r * (1 - u_2),  b2 = r * u_2  (all three >= 0);
 *     p = (b0 * A + b1 * B) + b2 * C per component on the doubles of the float32 vertices, points[k] = float(p).
 *   tri[k] = t.
 *   colors_out [ns,3] float32 (NULL = not wanted; colors [nv,3] float32 is then not read): the same combination of the three vertex
 *     colours.  normals_out [ns,3] float32 (NULL = not wanted): float(n_x / |n|), float(n_y / |n|), float(n_z / |n|) of triangle t.
 * `total` is on the device, so a bad one cannot be refused: unless total > 0 and total is finite every tri[k] is -1 and every float of
 * sample k is NaN.  The same holds for a single sample whose search finds no triangle or a triangle that is not valid - which cannot
 * happen with the P of the same mesh.
 * One launch, one lane per sample; the two searches are binary searches of at most 32 steps each.
 * Refused: nt, nv or ns outside [0, 2^31); colors_out without colors; a null pointer that is needed.  ns == 0 launches nothing. */
STA_API int sta_surf_sample(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, const double* P, const double* total, const float* colors,
                            int64_t ns, uint64_t seed, float* points, int32_t* tri, float* colors_out, float* normals_out, void* stream);

STA_API const char* sta_surf_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
