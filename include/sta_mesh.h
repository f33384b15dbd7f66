/*
 * sta_mesh.h - C ABI of libsta_mesh.so: triangles for the headless rasteriser, and vertex normals.  sta_mesh_triangles draws an indexed
 * triangle mesh into the key buffer of include/sta_raster.h - the same keys, the same camera, the same 64-bit atomic minimum - so that
 * triangles, points and lines share one canvas, occlude each other and may be issued in any order.  Coverage is exact integer
 * arithmetic on a fixed-point grid, everything else is float64 in a written order: an image is defined bit for bit by this header.
 * tests/mesh_cases.py restates all of it in numpy; vista_slam_amd/render.py (Canvas.mesh, render_mesh, mesh_depth) and
 * vista_slam_amd/tsdf.py (vertex_normals, visible_triangles) sit on top.
 *
 * This is a fifth library with its own translation unit (vista_slam_amd/csrc/sta_mesh.hip, kernels in csrc/mesh.h, which includes
 * raster.h and voxel.h unchanged), its own ctypes table (_lib.MESH_SIGNATURES) and its own inventories (tests/test_mesh_abi.py,
 * tests/mesh_stream_cases.py).  None of the other four libraries includes or links any of it.
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name ends in _host; every buffer, the workspace
 *     included, is the caller's; NO CALL ALLOCATES, COPIES TO THE HOST OR SYNCHRONISES.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_mesh_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is contracted
 *     into an FMA.  floor, rint and sqrt are the IEEE ones; float(x) rounds a float64 to float32 once; double(i) rounds an int64 to
 *     float64 once, to nearest.  "int64" arithmetic is exact: the limits below keep it from overflowing.
 *   - keys, H, W, ssaa, T_host, K_host, near, far, pc, us, vs, Hs, Ws: exactly as in include/sta_raster.h.
 *
 * What it is not (against a GL rasteriser): no far-plane and no 2-D polygon clipping - only the per-fragment far test and the 2^28
 * drop below; one flat light factor per face; square pixels whose centre is at the integer coordinate; fragments of equal float32
 * depth go to the smaller payload; no textures, no transparency, no smooth shading.
 */
#ifndef STA_MESH_H
#define STA_MESH_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_MESH_SUBPIXEL 256           /* snapped coordinates are in 1/256 of a key-buffer pixel */
#define STA_MESH_MAX_SNAP 268435456     /* 2^28: a piece with a snapped coordinate of larger magnitude is dropped and counted */
#define STA_MESH_PAYLOAD_ID 0
#define STA_MESH_PAYLOAD_COLOR 1
#define STA_MESH_PAYLOAD_NORMAL 2
#define STA_MESH_CULL_NONE 0
#define STA_MESH_CULL_BACK 1            /* back faces are not drawn */
#define STA_MESH_CULL_FRONT 2           /* front faces are not drawn */
#define STA_MESH_COUNTERS 8
#define STA_MESH_PLAN_SIZES 2

/* The layout of `counters` of sta_mesh_triangles: eight device uint64.  The first four count triangles, the last four count PIECES (a
 * triangle that is not clipped is one piece; a clipped one is one or two). */
typedef struct sta_mesh_counters {
    uint64_t seen;          /* triangles of the call */
    uint64_t bad;           /* dropped whole: an index outside [0, nv), or a camera coordinate of a vertex that is not finite */
    uint64_t behind;        /* dropped whole: all three pc_z < near */
    uint64_t clipped;       /* crossed z = near and was cut into one or two pieces (drawn, not dropped) */
    uint64_t too_large;     /* pieces dropped: a snapped coordinate is not finite or above STA_MESH_MAX_SNAP in magnitude */
    uint64_t degenerate;    /* pieces dropped: A2 == 0 */
    uint64_t culled;        /* pieces dropped by `cull` */
    uint64_t off_canvas;    /* pieces dropped: no pixel centre of the canvas inside the snapped bounding box */
} sta_mesh_counters;

/* Host only, no GPU.  sizes_out[0] = bytes of `work` of sta_mesh_triangles for nt triangles (the list of the pieces that take the
 * large path: two entries per triangle, so it cannot overflow, and its counter), sizes_out[1] = bytes of `work` of
 * sta_mesh_vertex_normals (the (vertex, triangle) pairs and the sort's buffers), or -1 when 3 * nt >= 2^31, which that call refuses.
 * Refuses nt or nv outside [0, 2^31), with the numbers in the message. */
STA_API int sta_mesh_plan(int64_t nt, int64_t nv, int64_t* sizes_out);

/* Accumulates nt triangles, verts [nv,3] float32 world coordinates, tris [nt,3] int32, into keys.  Triangle t with indices i0, i1, i2:
 *   counters[0] += 1.  Unless 0 <= i < nv for all three: counters[1] += 1, dropped.  V_k = pc(verts[i_k]); unless all nine camera
 *   coordinates are finite: counters[1] += 1, dropped.
 *   Near plane.  in_k = (V_k.z >= near).  None in: counters[2] += 1, dropped.  All in: one piece (V_0, V_1, V_2).  Otherwise
 *   counters[3] += 1 and the triangle is cut by z = near in camera space.  The point on a crossing edge is computed FROM THE END THAT
 *   IS IN towards the other:  P(in, out):  t = (near - in.z) / (out.z - in.z),  x = in.x + t * (out.x - in.x),  y likewise, z = near
 *   EXACTLY, and every vertex attribute c (a colour channel) likewise c = in.c + t * (out.c - in.c) - so two triangles that share the
 *   edge compute the same bits.  With (i, j, k) a cyclic rotation of (0, 1, 2):
 *     one in, V_i:        one piece   (V_i, P(V_i, V_j), P(V_i, V_k))
 *     one out, V_i:       two pieces  (V_j, V_k, Pk) and (V_j, Pk, Pj) with Pk = P(V_k, V_i), Pj = P(V_j, V_i): the diagonal of the
 *                         quad V_j V_k Pk Pj goes from V_j to Pk.
 *   Each piece (a, b, c), in this order:
 *   Projection and snap.  us, vs of each vertex as in sta_raster.h from its (x, y, z):  us = (fx * (x / z) + cx) * s + (s - 1) * 0.5.
 *     Xd = floor(us * 256 + 0.5), Yd = floor(vs * 256 + 0.5).  Unless all six satisfy |Xd| <= 2^28 (a NaN fails): counters[4] += 1,
 *     dropped.  X = int64(Xd), Y = int64(Yd).  With coordinates of at most 2^28 and pixel centres of at most 2^21, every difference
 *     below is at most 2^29 in magnitude, every product at most 2^58, every edge function a difference of two such products: it fits int64.
 *   Area and facing.  A2 = (Xb - Xa) * (Yc - Ya) - (Yb - Ya) * (Xc - Xa).  A2 == 0: counters[5] += 1, dropped.  The piece is
 *     FRONT-FACING iff A2 < 0: with x to the right, y down and z forward that is a triangle whose normal (B - A) x (C - A) points towards
 *     the camera, as the triangles of sta_tsdf_mesh (normals into free space) do when they are seen from free space.  cull ==
 *     STA_MESH_CULL_BACK and A2 > 0, or cull == STA_MESH_CULL_FRONT and A2 < 0: counters[6] += 1, dropped.
 *     If A2 < 0, b and c change places (with everything they carry) and A2 = -A2.
 *   Bounding box.  x0 = max(ceil(min X / 256), 0), x1 = min(floor(max X / 256), Ws - 1), y0, y1 likewise with Hs (integer ceil and
 *     floor).  x0 > x1 or y0 > y1: counters[7] += 1, dropped.  EVERY key write of the call is to a pixel of this clamped box.
 *   Coverage of the pixel (x, y) of the box, px = 256 * x, py = 256 * y, exact int64:
 *       e_a = (Xc - Xb) * (py - Yb) - (Yc - Yb) * (px - Xb)          (the edge b -> c, the weight of a)
 *       e_b = (Xa - Xc) * (py - Yc) - (Ya - Yc) * (px - Xc)          (the edge c -> a)
 *       e_c = (Xb - Xa) * (py - Ya) - (Yb - Ya) * (px - Xa)          (the edge a -> b)
 *     e_a + e_b + e_c == A2.  The pixel is covered iff each of the three is > 0, or == 0 on an edge that is TOP OR LEFT: an edge p -> q
 *     with (dx, dy) = (Xq - Xp, Yq - Yp) is top or left iff dy < 0, or dy == 0 and dx > 0.  (A pixel centre on an edge shared by two
 *     triangles belongs to exactly one of them; a vertex on a centre to exactly one of its fan.)
 *   Depth, perspective-correct.  w_k = 1 / z_k per vertex of the piece.
 *       w = ((double(e_a) * w_a + double(e_b) * w_b) + double(e_c) * w_c) / double(A2),    depth = 1 / w.
 *     Far plane, per fragment: unless depth <= far the fragment is not written (a NaN fails).
 *   Payload.
 *     STA_MESH_PAYLOAD_ID      uint32(id_base + t); the two pieces of a clipped triangle share it.
 *     STA_MESH_PAYLOAD_COLOR   colors [nv,3] float32: per channel q_k = double(colour of vertex k) * w_k (a cut point's colour is the c
 *                              above),  cw = ((double(e_a) * q_a + double(e_b) * q_b) + double(e_c) * q_c) / double(A2),  c = cw / w.
 *                              colors == NULL: c = color_host[channel] (three doubles), one colour for the whole call.
 *                              light_host != NULL (four doubles eye_x, eye_y, eye_z, ambient): c = c * L with the triangle's
 *                              two-sided factor L below.  Then channel = rint(min(max(c, 0), 1) * 255) with NaN -> 0 (the channel rule
 *                              of sta_raster_points), packed (r << 24) | (g << 16) | (b << 8) | 255.
 *     STA_MESH_PAYLOAD_NORMAL  per channel the same channel rule on (n_a / |n|) * 0.5 + 0.5; 128, 128, 128 unless |n| > 0.
 *     The face normal and the light factor are per TRIANGLE t (not per piece) on the double of the float32 world vertices
 *     A, B, C = verts[i0], verts[i1], verts[i2]:  u = B - A, v = C - A,  n = (u_y * v_z - u_z * v_y, u_z * v_x - u_x * v_z,
 *     u_x * v_y - u_y * v_x),  |n| = sqrt((n_x * n_x + n_y * n_y) + n_z * n_z);  d = eye - A, |d| likewise,
 *     dot = (n_x * d_x + n_y * d_y) + n_z * d_z;   L = ambient + (1 - ambient) * (|dot| / (|n| * |d|)), and L = ambient unless |n| > 0
 *     and |d| > 0.
 *   key = (uint64(bits of float(depth)) << 32) | payload, merged with a 64-bit atomic minimum (a plain load that skips the atomic when
 *   the stored key is already not larger is allowed: the result does not depend on it).
 * counters: STA_MESH_COUNTERS device uint64 (NULL = not counted), added with integer atomics; the caller zeroes them.
 * work: sizes_out[0] bytes of sta_mesh_plan; its contents before and after the call mean nothing.
 * Refused, with the numbers in the message: nt or nv outside [0, 2^31); what sta_raster_plan refuses; near / far outside the limits of
 * sta_raster.h; a T_host, K_host, color_host or light_host entry that is not finite; ambient outside [0, 1]; a payload_kind that does not
 * agree with its pointers (ID and NORMAL: colors, color_host and light_host all NULL; COLOR: exactly one of colors and color_host);
 * a cull outside 0 .. 2; id_base + nt > 2^32 - 1 with STA_MESH_PAYLOAD_ID (the id 2^32 - 1 is what sta_raster_resolve reports for an
 * empty pixel); work_bytes below the plan's.  nt == 0 launches nothing.
 * Two launches: one lane per triangle sets it up and draws every piece of a small box itself; a piece of a larger box is appended to a
 * list in `work` and drawn by a second launch, one wavefront per piece with the lanes over the box.  The list's order is not defined
 * and the image does not depend on it. */
STA_API int sta_mesh_triangles(uint64_t* keys, int H, int W, int ssaa, const float* verts, int64_t nv, const int32_t* tris, int64_t nt,
                               const float* colors, const double* color_host, const double* light_host, int payload_kind, int cull, int64_t id_base,
                               const double* T_host, const double* K_host, double near, double far, uint64_t* counters, void* work, int64_t work_bytes,
                               void* stream);

/* Area-weighted vertex normals: normals_out [nv,3] float32.  For vertex v:  S = (0, 0, 0); for every corner of every triangle that names
 * v, IN ASCENDING TRIANGLE INDEX (and corner index within a triangle), S = S + n with the un-normalised face normal n of that triangle as
 * above ((B - A) x (C - A): its length is twice the area).  A triangle with an index outside [0, nv) contributes to no vertex.
 *   len = sqrt((S_x * S_x + S_y * S_y) + S_z * S_z);  normals_out[v] = float(S / len) per component, or (0, 0, 0) unless len > 0 and
 *   len is finite (no triangle, a zero sum, a sum that is not finite).
 * No floating-point atomics: the 3 * nt (vertex, corner) pairs are sorted by vertex with a stable radix sort, one lane per vertex finds
 * its run by binary search and sums it in order.  Two calls give the same bits.
 * work: sizes_out[1] bytes of sta_mesh_plan.  Refused: nv outside [0, 2^31), nt outside [0, 2^31) or 3 * nt >= 2^31; work_bytes below the
 * plan's.  nv == 0 launches nothing. */
STA_API int sta_mesh_vertex_normals(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, float* normals_out, void* work,
                                    int64_t work_bytes, void* stream);

STA_API const char* sta_mesh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
