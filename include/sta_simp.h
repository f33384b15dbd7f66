/*
 * sta_simp.h - C ABI of libsta_simp.so: the step between a fused mesh and one that can be handed on.  Uniform-grid vertex clustering
 * (Rossignac-Borrel): every vertex goes to the cell of a lattice that holds it, every occupied cell that a surviving triangle names
 * becomes one output vertex, triangles whose corners fall into fewer than three cells collapse, triangles that name the same three
 * cells are merged.  The output vertex of a cell is the mean of the cell's vertices or the minimiser of the summed Garland-Heckbert
 * vertex quadrics of the cell (Lindstrom's out-of-core form): a 3x3 symmetric eigenproblem per cell.  Cells, ranks, triangles and maps
 * are integers; the placement is float64 operations in a written order: every output is defined bit for bit by this header.
 * tests/simp_cases.py restates all of it in numpy; vista_slam_amd/simplify.py (cells, cluster_triangles, simplify_mesh) sits on top.
 *
 * This is a seventh library with its own translation unit (vista_slam_amd/csrc/sta_simp.hip, kernels in csrc/simp.h, which includes
 * voxel.h, select.h, elementwise.h and sta_common.h unchanged), its own ctypes table (_lib.SIMP_SIGNATURES) and its own inventories
 * (tests/test_simp_abi.py, tests/simp_stream_cases.py).  None of the other six libraries includes or links any of it.
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name is sizes_out; every buffer, the workspace
 *     included, is the caller's; NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_simp_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is contracted
 *     into an FMA.  sqrt is the IEEE one; float(x) rounds a float64 to float32 once; double(i) of an integer below 2^53 is exact.
 *   - Every device loop carries a bound taken from the arguments; no kernel waits for another lane's progress; no floating-point atomic.
 *   - verts [nv,3] float32, tris [nt,3] int32, colors [nv,3] float32 or NULL.  cell > 0 and the origin (ox, oy, oz) are finite float64.
 *   - counters [STA_SIMP_COUNTERS] int64 on the device; each call sets the entries it owns and leaves the others alone.  The library never
 *     reads a count back: kernels read them from device memory, output buffers are sized by the caller for the worst case.
 *   - The three stages are separate calls so that each can be tested; sta_simp_triangles takes the vcell of sta_simp_cells, sta_simp_place
 *     the vcell and the cell_out of the two before it, with the same verts, tris, cell and origin.
 *
 * What it is not.  It is not iterative edge collapse, and there is no target triangle count: `cell` is the control.  There is no
 * guarantee of manifoldness: two sheets closer than a cell merge, a fan can fold onto an edge, thin features can vanish.  There are no
 * boundary or colour quadrics.  Normals are not preserved as an attribute; recompute them (sta_mesh_vertex_normals).  It was not compared
 * with Open3D's simplify_vertex_clustering or MeshLab.
 */
#ifndef STA_SIMP_H
#define STA_SIMP_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_SIMP_SWEEPS 8               /* the fixed number of cyclic Jacobi sweeps of sta_simp_place */
#define STA_SIMP_INDEX_BITS 21          /* a cell index per axis lies in [-2^20, 2^20) and is stored biased by 2^20 */
#define STA_SIMP_PLACE_MEAN 0
#define STA_SIMP_PLACE_QUADRIC 1
#define STA_SIMP_PLAN_SIZES 3
#define STA_SIMP_COUNTERS 8
/* the layout of `counters` */
#define STA_SIMP_N_CELLS 0              /* occupied cells                                                   (sta_simp_cells) */
#define STA_SIMP_N_VERTS 1              /* output vertices = used cells                                     (sta_simp_triangles) */
#define STA_SIMP_N_TRIS 2               /* output triangles                                                 (sta_simp_triangles) */
#define STA_SIMP_N_DROPPED 3            /* vertices that are not finite or beyond the index range           (sta_simp_cells) */
#define STA_SIMP_N_INVALID 4            /* triangles with an index outside [0, nv) or a dropped vertex      (sta_simp_triangles) */
#define STA_SIMP_N_COLLAPSED 5          /* valid triangles with two corners in one cell                     (sta_simp_triangles) */
#define STA_SIMP_N_DUPLICATE 6          /* triangles that lost to an earlier one of the same three cells    (sta_simp_triangles) */
#define STA_SIMP_N_FALLBACK 7           /* used cells whose quadric position was not accepted               (sta_simp_place) */

/* The layout of `sizes_out` of sta_simp_plan: STA_SIMP_PLAN_SIZES int64. */
typedef struct sta_simp_sizes {
    int64_t cells_work_bytes;
    int64_t triangles_work_bytes;
    int64_t place_work_bytes;
} sta_simp_sizes;

/* Host only, no GPU.  The bytes of `work` of the three stages (sort buffers, scan offsets, flags; every part rounded up to 256 bytes).
 * Refuses, with the numbers in the message: nv outside [0, 2^31); nt negative or 3 * nt not below 2^31. */
STA_API int sta_simp_plan(int64_t nt, int64_t nv, int64_t* sizes_out);

/* Stage 1, cells.  Vertex v = (p_x, p_y, p_z) has the cell index i_k = floor((double(p_k) - o_k) / cell) per axis: one subtraction, one
 * division.  v is KEPT iff its three coordinates are finite and every i_k lies in [-2^20, 2^20); otherwise it is dropped and counted -
 * nothing is refused for it and nothing waits for an extent.  key = ((i_z + 2^20) << 42) | ((i_y + 2^20) << 21) | (i_x + 2^20).
 * The occupied cells are ranked in ascending key order:
 *   vcell [nv] int32     the rank of v's cell, or -1 for a dropped vertex
 *   counters[STA_SIMP_N_CELLS] = the number of occupied cells, counters[STA_SIMP_N_DROPPED] = the number of dropped vertices
 * One key kernel, a stable LSD radix sort of (key, v) over 63 bits (the sort of csrc/voxel.h), heads of runs counted per workgroup,
 * one scan, one kernel that writes each vertex the number of heads at or before its sorted position minus one.
 * work: sizes_out[0] bytes of sta_simp_plan; its contents before and after the call mean nothing.
 * Refused, with the numbers in the message: nv outside [0, 2^31); cell not finite or not > 0; an origin that is not finite; work_bytes
 * below the plan's; a null pointer that is needed.  nv == 0 only sets the two counters to 0. */
STA_API int sta_simp_cells(const float* verts, int64_t nv, double cell, double ox, double oy, double oz, int32_t* vcell, int64_t* counters,
                           void* work, int64_t work_bytes, void* stream);

/* Stage 2, triangles.  vcell [nv] is stage 1's (a value outside [0, nv) is read as -1).  Triangle t = (i0, i1, i2) is VALID iff its three
 * indices are in [0, nv) and all three vertices are kept; its cluster triple is (a, b, c) = (vcell[i0], vcell[i1], vcell[i2]).  It
 * COLLAPSES iff two of the three are equal.  Among the valid triangles that do not collapse and have the same SET {a, b, c} (any
 * rotation, either winding) the one with the lowest t survives; the others are duplicates.
 *   tri_src  [nt] int32      tri_src[j] = the index t of output triangle j; the survivors come out in ascending t
 *   cell_out [nv] int32      a cell is USED iff a survivor names it; the used cells in ascending rank get the output indices 0, 1, ...;
 *                            cell_out[c] is that index, -1 for a cell that is not used and for every c at or beyond the number of cells
 *   tris_out [nt,3] int32    output triangle j = the triple of tri_src[j] rotated cyclically so that its smallest cluster comes first
 *                            (a smallest: (a, b, c); b smallest: (b, c, a); c smallest: (c, a, b) - the winding is kept), each cluster
 *                            replaced by its cell_out
 *   vmap     [nv] int32      cell_out[vcell[v]], or -1 for a dropped vertex
 *   rows j at and beyond the number of output triangles: tri_src[j] = -1 and tris_out[j] = (-1, -1, -1)
 *   counters[STA_SIMP_N_VERTS], [STA_SIMP_N_TRIS], [STA_SIMP_N_INVALID], [STA_SIMP_N_COLLAPSED], [STA_SIMP_N_DUPLICATE];
 *   nt = N_TRIS + N_INVALID + N_COLLAPSED + N_DUPLICATE.
 * How duplicates are found does not show in the outputs: the sorted triple s0 < s1 < s2 is sorted by s2, then by (s0, s1), both with the
 * stable sort, so that equal sets are adjacent in ascending t; a triangle is a duplicate iff its sorted predecessor has the same triple.
 * Survivors are compacted in order (ballot ranks, one scan), used cells are marked by integer stores and compacted the same way.
 * work: sizes_out[1] bytes of sta_simp_plan.  Refused: nv outside [0, 2^31); nt negative or 3 * nt not below 2^31; work_bytes below the
 * plan's; a null pointer that is needed. */
STA_API int sta_simp_triangles(const int32_t* tris, int64_t nt, int64_t nv, const int32_t* vcell, int32_t* tris_out, int32_t* tri_src,
                               int32_t* cell_out, int32_t* vmap, int64_t* counters, void* work, int64_t work_bytes, void* stream);

/* Stage 3, placement: one output vertex per used cell c, at row cell_out[c] of verts_out [nv,3] float32 (and of colors_out, when colors
 * and colors_out are given; both or neither).  Rows at and beyond the number of output vertices are not written.
 *   Mean.  s = the sequential float64 sum, starting from 0.0, of double(verts[v]) over the cell's kept vertices in ascending v, per
 *     component; m = s / double(count).  The colour is the same sum and division over colors, rounded once by float().
 *   placement == STA_SIMP_PLACE_MEAN: the position is float(m).
 *   placement == STA_SIMP_PLACE_QUADRIC: every (valid triangle t, corner j) pair contributes to the cell of that corner, in ascending
 *     3 t + j (a triangle with two corners in one cell contributes twice there: the sum of the Garland-Heckbert vertex quadrics).
 *       A, B, C = the doubles of verts[i0], verts[i1], verts[i2];  u = B - A, v = C - A,
 *       n = (u_y * v_z - u_z * v_y, u_z * v_x - u_x * v_z, u_x * v_y - u_y * v_x)       - as include/sta_surf.h and sta_mesh.h write them
 *       the pair is skipped when a component of n is not finite
 *       q00 += n_x * n_x, q01 += n_x * n_y, q02 += n_x * n_z, q11 += n_y * n_y, q12 += n_y * n_z, q22 += n_z * n_z
 *       d = (n_x * (m_x - A_x) + n_y * (m_y - A_y)) + n_z * (m_z - A_z);   g_k += n_k * d        (the gradient at m, relative to m)
 *     all nine sums start from 0.0.  Eigen-decomposition of Q by cyclic Jacobi: a = Q (a01 = q01 and so on; only the upper triangle is
 *     kept), V = the identity; STA_SIMP_SWEEPS sweeps, each the pairs (p, q) = (0, 1), (0, 2), (1, 2) in that order, r the third index:
 *       skipped when a_pq == 0 exactly; otherwise
 *       theta = (a_qq - a_pp) / (2 * a_pq);   h = sqrt(theta * theta + 1);   t = 1 / (|theta| + h), negated when theta < 0
 *         (sign(0) = +1; an overflowing theta * theta gives t = +-0, the right limit)
 *       c = 1 / sqrt(t * t + 1);   s = t * c;   z = t * a_pq
 *       a_pp = a_pp - z;   a_qq = a_qq + z;   a_pq = 0
 *       (a_rp, a_rq) = (c * a_rp - s * a_rq,  s * a_rp + c * a_rq)                         from the old a_rp, a_rq
 *       (V_kp, V_kq) = (c * V_kp - s * V_kq,  s * V_kp + c * V_kq)  for k = 0, 1, 2        from the old V_kp, V_kq
 *     l_i = a_ii, e_i = column i of V.  lmax = l_0; if l_1 > lmax: lmax = l_1; if l_2 > lmax: lmax = l_2.  thr = sv_ratio * lmax.
 *     y = (0, 0, 0); for i = 0, 1, 2 with l_i > thr:  w = ((V_0i * g_0 + V_1i * g_1) + V_2i * g_2) / l_i;   y_k = y_k + V_ki * w.
 *     x_k = m_k - y_k.
 *     x is accepted iff lmax > 0, every x_k is finite and lo_k <= x_k <= hi_k with lo_k = o_k + double(i_k) * cell and
 *     hi_k = o_k + double(i_k + 1) * cell (i_k the cell's index on axis k).  Otherwise x = m, counted in counters[STA_SIMP_N_FALLBACK]
 *     (set to 0 with STA_SIMP_PLACE_MEAN).  The position is float(x).
 * Two stable sorts - (vcell[v], v) and (cell of corner j of t, 3 t + j), a dropped vertex and a corner of a triangle that is not valid
 * behind every cell - then one lane per cell: it finds its two runs by binary search, sums in the written order, rotates and solves in
 * registers.  With STA_SIMP_PLACE_MEAN tris is not read and the pair sort is not run.
 * work: sizes_out[2] bytes of sta_simp_plan.  Refused: nv or nt as above; cell or origin as in sta_simp_cells; placement not 0 or 1;
 * sv_ratio outside [0, 1); exactly one of colors and colors_out; work_bytes below the plan's; a null pointer that is needed. */
STA_API int sta_simp_place(const float* verts, const float* colors, int64_t nv, const int32_t* tris, int64_t nt, const int32_t* vcell,
                           const int32_t* cell_out, double cell, double ox, double oy, double oz, int placement, double sv_ratio,
                           float* verts_out, float* colors_out, int64_t* counters, void* work, int64_t work_bytes, void* stream);

STA_API const char* sta_simp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
