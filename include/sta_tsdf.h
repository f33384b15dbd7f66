/*
 * sta_tsdf.h - C ABI of libsta_tsdf.so: volumetric fusion of the map.  Depth maps are folded into a sparse truncated signed distance
 * volume and the zero level set is extracted as a triangle mesh by marching tetrahedra.  Every output is defined bit for bit by this
 * header: tests/tsdf_cases.py restates all of it in numpy; vista_slam_amd/tsdf.py sits on top.
 *
 * This is NOT part of the product ABI (include/sta_mi355.h) nor of include/sta_cloud.h or include/sta_raster.h: it is a fourth library
 * with its own translation unit (vista_slam_amd/csrc/sta_tsdf.hip, kernels in csrc/tsdf.h), its own ctypes table (_lib.TSDF_SIGNATURES)
 * and its own inventories (tests/test_tsdf_abi.py, tests/tsdf_stream_cases.py).
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name ends in _host; every buffer is the caller's;
 *     no call allocates.  sta_tsdf_blocks and sta_tsdf_mesh synchronise their stream once, to return their counts; no other call copies
 *     to the host or synchronises.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_tsdf_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is contracted
 *     into an FMA.  floor is exact; float(x) rounds a float64 to float32 once, to nearest; double(x) widens a float32 or an integer.
 *     There are no floating-point atomics: the result does not depend on the order in which the hardware runs the threads.
 *
 * The volume.  Values live at lattice points: point i = (ix, iy, iz) sits at x_k = o_k + double(i_k) * voxel_size.  origin_host is three
 * doubles (NULL = 0, 0, 0), so that two volumes can share a lattice.  Storage is sparse in blocks of 8 x 8 x 8 lattice points: block
 * b = (bx, by, bz) holds the points 8 b .. 8 b + 7 per axis, the local index of a point is (lz * 8 + ly) * 8 + lx.  A block's key is
 *     ((bz + 2^20) << 42) | ((by + 2^20) << 21) | (bx + 2^20)                with every block index in [-2^20, 2^20)
 * keys [nb] uint64 is strictly ascending, a block's rank is its position in keys; tsdf [nb,512] float32, weight [nb,512] float32 and
 * optionally rgb [nb,512,3] float32 hold the values.  A neighbouring block is found by a binary search in keys; there is no hash table.
 *
 * A view.  depths [V,H,W] float32, scales [V] float32, K [V,4] float64 (fx, fy, cx, cy), c2w / w2c [V,12] float64 (row-major 3x4),
 * obs [V,H,W] float32 (the observation weight).  Pixel (v, iy, ix) is OBSERVED iff obs > 0 (false for NaN) and
 * D = double(depth) * double(scale) is finite with 0 < D <= depth_max.
 */
#ifndef STA_TSDF_H
#define STA_TSDF_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_TSDF_BLOCK 8                /* lattice points per block and axis */
#define STA_TSDF_BLOCK_POINTS 512
#define STA_TSDF_MAX_TRUNC_VOXELS 4     /* trunc <= 4 * voxel_size */
#define STA_TSDF_MAX_BLOCKS 16777216    /* max_blocks < 2^24 */
#define STA_TSDF_MAX_PIXELS 268435456   /* V * H * W < 2^28 */
#define STA_TSDF_BLOCK_BIAS 1048576     /* 2^20 */
#define STA_TSDF_KEY_SENTINEL 0xFFFFFFFFFFFFFFFFull
#define STA_TSDF_PLAN_SIZES 8
#define STA_TSDF_TABLE_ROW 7            /* the case table: [6][16][7] int8 */

/* The layout of counts_out_host of sta_tsdf_blocks (three int64) and of sta_tsdf_mesh (two). */
typedef struct sta_tsdf_block_counts {
    int64_t blocks;         /* nb */
    int64_t observed;       /* observed pixels */
    int64_t dropped;        /* observed pixels whose surface point does not fit the key's fields */
} sta_tsdf_block_counts;
typedef struct sta_tsdf_mesh_counts {
    int64_t vertices;
    int64_t triangles;
} sta_tsdf_mesh_counts;

/* Host only.  sizes_out[STA_TSDF_PLAN_SIZES] ={bytes of the workspace of sta_tsdf_blocks, bytes of keys, bytes of tsdf (= of weight),
 * bytes of rgb, bytes of the workspace of sta_tsdf_mesh, bytes of verts (= of cols), bytes of tris, key slots = 8 * V * H * W} for
 * max_blocks blocks, max_vertices vertices and max_triangles triangles.  Refused, with the numbers in the message: voxel_size or trunc
 * not finite or not > 0; trunc > STA_TSDF_MAX_TRUNC_VOXELS * voxel_size; V < 1, H < 1 or W < 1; V * H * W >= STA_TSDF_MAX_PIXELS;
 * max_blocks outside [1, STA_TSDF_MAX_BLOCKS); max_vertices or max_triangles outside [0, 2^31). */
STA_API int sta_tsdf_plan(int64_t V, int H, int W, double voxel_size, double trunc, int64_t max_blocks, int64_t max_vertices, int64_t max_triangles,
                          int64_t* sizes_out);

/* Host only.  table_out_host [6][16][STA_TSDF_TABLE_ROW] int8: for tetrahedron t and case m the number of triangles (0, 1 or 2) and then
 * six vertex codes, three per triangle in output order, -1 where unused.  A vertex code is 4 * i + j for the corner pair (v_i inside,
 * v_j outside).  See sta_tsdf_mesh for the rule that generates it. */
STA_API int sta_tsdf_table(int8_t* table_out_host);

/* Views -> the sorted block list.  The surface point of an observed pixel (v, iy, ix) is
 *     l = ((double(ix) - cx) / fx * D, (double(iy) - cy) / fy * D, D)
 *     P_x = ((R00*l_x + R01*l_y) + R02*l_z) + t_x, likewise y and z, with c2w = [R | t]
 * and it touches the blocks of its eight corners c = (P_x -+ trunc, P_y -+ trunc, P_z -+ trunc) (one subtraction or addition per axis):
 * per axis the voxel index is floor((c_k - o_k) / voxel_size) and the block index is that index arithmetically shifted right by 3.  A
 * point with a corner whose voxel index is not in [-2^23, 2^23) on some axis (a NaN or an infinity fails it) is dropped and counted.
 * keys_out [max_blocks] receives the distinct keys in ascending order.
 * counts_out_host [3] = {nb, n_observed, n_dropped}: the number of blocks, of observed pixels and of dropped points among them.
 * Implementation: eight key slots per pixel (STA_TSDF_KEY_SENTINEL for a pixel that is not observed, a dropped point and a corner whose
 * block repeats an earlier corner's of the same pixel), the stable LSD radix sort of csrc/voxel.h over all 64 bits, an ordered compaction
 * of the heads.  The call synchronises `stream` once.  nb > max_blocks is refused with nb in the message (counts_out_host is filled):
 * nothing is written past max_blocks keys.  Refused too: what sta_tsdf_plan refuses; depth_max not > 0 (+inf is allowed); an origin that
 * is not finite; work_bytes smaller than the plan's. */
STA_API int sta_tsdf_blocks(const float* depths, const float* scales, const double* K, const double* c2w, const float* obs, int64_t V, int H, int W,
                            double voxel_size, double trunc, const double* origin_host, double depth_max, uint64_t* keys_out, int64_t max_blocks,
                            void* work, int64_t work_bytes, int64_t* counts_out_host, void* stream);

/* tsdf = 1, weight = 0, rgb = 0 (rgb may be NULL) for nb blocks. */
STA_API int sta_tsdf_clear(float* tsdf, float* weight, float* rgb, int64_t nb, void* stream);

/* Folds the views v0 <= v < v1 into the volume, in ascending view order per lattice point.  imgs [V,3,H,W] float32 in [-1,1]; colour is
 * fused iff imgs and rgb are both given.  For the lattice point i of a block at x_k = o_k + double(i_k) * voxel_size and view v:
 *     pc_x = ((T00*x + T01*y) + T02*z) + T03, likewise y and z, with T = w2c[v]; skipped unless pc_z > 0
 *     u = fx * (pc_x / pc_z) + cx, px = floor(u + 0.5);  w = fy * (pc_y / pc_z) + cy, py = floor(w + 0.5)
 *     skipped unless 0 <= px <= W - 1 and 0 <= py <= H - 1 as float64 (a NaN fails); skipped unless the pixel (v, py, px) is observed
 *     sdf = D - pc_z; skipped if sdf < -trunc;  d = min(sdf / trunc, 1)
 *     with w = double(obs) and Wo = double(weight):   tsdf <- float((Wo * double(tsdf) + w * d) / (Wo + w))
 *     every rgb channel likewise with c = (double(img) + 1) * 0.5 in the place of d;  then weight <- float(min(Wo + w, max_weight))
 * Nearest pixel, no interpolation.  The call does not synchronise; calls over [0, a) and [a, V) give the bits of one call over [0, V).
 * A view that no lattice point of a block can project into may be skipped as a whole for that block: the output does not depend on it.
 * Refused: nb outside [0, STA_TSDF_MAX_BLOCKS); v0 / v1 not 0 <= v0 <= v1 <= V; max_weight not finite or not > 0; the rest as above. */
STA_API int sta_tsdf_integrate(const uint64_t* keys, int64_t nb, float* tsdf, float* weight, float* rgb, const float* depths, const float* scales,
                               const double* K, const double* w2c, const float* obs, const float* imgs, int64_t V, int H, int W, int64_t v0, int64_t v1,
                               double voxel_size, double trunc, const double* origin_host, double depth_max, double max_weight, void* stream);

/* Marching tetrahedra on the Freudenthal (Kuhn) split of every lattice cube.  A lattice point is KNOWN iff weight >= min_weight
 * (min_weight > 0; a point of a block that is not in keys is not known) and INSIDE iff it is known and tsdf < 0 (an exact 0 is outside).
 * The cube with base c has six tetrahedra; tetrahedron t is the t-th permutation (p0, p1, p2) of the axes in lexicographic order (012,
 * 021, 102, 120, 201, 210) with the corners v0 = c, v1 = v0 + e_p0, v2 = v1 + e_p1, v3 = c + (1,1,1).  A tetrahedron is emitted iff its
 * four corners are known; its case has bit k set iff v_k is inside.  Triangles as corner pairs (inside, outside):
 *     one inside corner a, outside o1 < o2 < o3:        (a,o1), (a,o2), (a,o3)
 *     three inside i1 < i2 < i3, one outside o:         (i1,o), (i2,o), (i3,o)
 *     two inside a < b, two outside c < d:              (a,c), (a,d), (b,d)   and   (a,c), (b,d), (b,c)
 * Orientation, in integers: with every vertex at the sum of its two corners (twice the midpoint), n = (p1 - p0) x (p2 - p0) and
 * s = n . (|in| * sum of the outside corners - |out| * sum of the inside corners); if s < 0 the last two vertices are swapped (s is never
 * 0): normals point into free space.
 * The vertex on the edge (v_i, v_j), i < j, is owned by the lattice point a = c + v_i; its type is dx + 2 dy + 4 dz - 1 of v_j - v_i
 * (0 .. 6).  With b the other end, da and db the doubles of the two float32 tsdf values:  t = da / (da - db); per axis the coordinate is
 * o_k + (double(a_k) + (dir_k ? t : 0)) * voxel_size; the colour is ca + t * (cb - ca) per channel; each is stored as float32.  A vertex
 * exists iff an emitted triangle references it.  Vertices are ordered by (rank of the owner's block, owner's local index, type),
 * triangles by (rank of c's block, c's local index, tetrahedron, position in the table).
 * verts_out [max_vertices,3] float32, cols_out [max_vertices,3] float32 (NULL, or rgb NULL: no colours), tris_out [max_triangles,3] int32.
 * counts_out_host [2] = {nv, nt}.  The call synchronises `stream` once.  verts_out == NULL and tris_out == NULL: it only counts.
 * nv > max_vertices or nt > max_triangles is refused with the numbers in the message (counts_out_host is filled) and nothing is written.
 * Refused too: nb outside [0, STA_TSDF_MAX_BLOCKS); min_weight not finite or not > 0; nv or nt >= 2^31; work_bytes smaller than the plan's. */
STA_API int sta_tsdf_mesh(const uint64_t* keys, int64_t nb, const float* tsdf, const float* weight, const float* rgb, double voxel_size,
                          const double* origin_host, double min_weight, float* verts_out, float* cols_out, int32_t* tris_out, int64_t max_vertices,
                          int64_t max_triangles, void* work, int64_t work_bytes, int64_t* counts_out_host, void* stream);

STA_API const char* sta_tsdf_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
