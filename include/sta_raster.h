/*
 * sta_raster.h - C ABI of libsta_raster.so: a headless rasteriser for the map.  Points and line segments are projected by a pinhole
 * camera and z-buffered into a buffer of 64-bit keys with integer atomic minima, so the image does not depend on the order in which
 * the hardware runs the threads: it is defined bit for bit by this header.  tests/render_cases.py restates all of it in numpy;
 * vista_slam_amd/render.py sits on top.
 *
 * This is NOT part of the product ABI (include/sta_mi355.h) nor of include/sta_cloud.h: it is a third library with its own translation
 * unit (vista_slam_amd/csrc/sta_raster.hip, kernels in csrc/raster.h), its own ctypes table (_lib.RASTER_SIGNATURES) and its own
 * inventories (tests/test_render_abi.py, tests/render_stream_cases.py).
 *
 * Conventions
 *   - No handle.  Every pointer is device memory of the CURRENT HIP device unless its name ends in _host; every buffer is the caller's;
 *     no call allocates, copies to the host or synchronises.
 *   - Work is enqueued on the caller's hipStream_t (`stream`, passed as void*).
 *   - Return value: 0 on success, negative on error; sta_raster_last_error() returns a thread-local message.
 *   - Arithmetic: every floating-point operation named below is ONE IEEE float64 operation in the written order; nothing is contracted
 *     into an FMA.  floor and rint (to nearest, ties to even) are exact; float(x) rounds a float64 to float32 once, to nearest.
 *
 * The key buffer.  keys [Hs, Ws] uint64 with Hs = H * ssaa, Ws = W * ssaa (ssaa 1, 2 or 4: the number of sub-pixels per output pixel and
 * axis).  A key is (uint64(bits of a float32 depth) << 32) | payload.  The depth is positive, so its bit pattern grows with it, and the
 * smallest key of a pixel is its nearest fragment; among fragments of equal float32 depth the smaller payload wins.  The all-ones key
 * (STA_RASTER_EMPTY) means empty: its depth field is no positive float.
 *
 * The camera.  T_host: 12 doubles, a row-major 3x4 world-to-camera matrix.  K_host: 4 doubles fx, fy, cx, cy in OUTPUT pixels.
 *     pc_x = ((T00*x + T01*y) + T02*z) + T03, likewise y and z, on double(x), double(y), double(z)           (as sta_nn_query does)
 *     u = fx * (pc_x / pc_z) + cx        v = fy * (pc_y / pc_z) + cy
 * A pixel's centre is at its integer coordinate.  On the key buffer, with s = ssaa:
 *     us = u * s + (s - 1) * 0.5         vs = v * s + (s - 1) * 0.5           ((s - 1) * 0.5 is exact; for s = 1 us is u)
 * near and far: STA_RASTER_MIN_NEAR <= near <= far <= STA_RASTER_MAX_FAR, so that float(depth) is a positive normal float.
 *
 * A footprint of size p (1 .. STA_RASTER_MAX_SIZE) around the pixel (cx, cy) is the columns cx - (p - 1) / 2 .. cx + p / 2 (integer
 * division) and the rows likewise, in key-buffer pixels.  Every footprint pixel inside [0, Ws) x [0, Hs) is written; the others are not.
 */
#ifndef STA_RASTER_H
#define STA_RASTER_H

#include <stdint.h>

#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define STA_RASTER_MAX_DIM 8192         /* H * ssaa and W * ssaa */
#define STA_RASTER_MAX_SIZE 8           /* point_size, line_width */
#define STA_RASTER_CLIP_MARGIN 8        /* key-buffer pixels by which the 2-D clip window of a segment is wider than the canvas */
#define STA_RASTER_MIN_NEAR 1e-30
#define STA_RASTER_MAX_FAR 1e30
#define STA_RASTER_MAX_COORD 1099511627776.0   /* 2^40: a segment with a projected end beyond it (in key-buffer pixels) is dropped */
#define STA_RASTER_EMPTY 0xFFFFFFFFFFFFFFFFull
#define STA_RASTER_COLOR_NONE 0         /* colors == NULL: the payload is the point's id */
#define STA_RASTER_COLOR_U8 1           /* colors [M,3] uint8 */
#define STA_RASTER_COLOR_F32 2          /* colors [M,3] float32 in [0, 1] */

/* The layout of `counters` of sta_raster_points: four device uint64. */
typedef struct sta_raster_counters {
    uint64_t seen;          /* points of the call */
    uint64_t non_finite;    /* dropped: a camera coordinate is not finite */
    uint64_t near_far;      /* dropped: pc_z outside [near, far] */
    uint64_t off_canvas;    /* dropped: no footprint pixel on the canvas */
} sta_raster_counters;

/* Host only.  sizes_out[3] = {bytes of the key buffer, Hs, Ws}.  Refuses H or W < 1, ssaa outside {1, 2, 4}, H * ssaa or W * ssaa above
 * STA_RASTER_MAX_DIM, with the numbers in the message. */
STA_API int sta_raster_plan(int H, int W, int ssaa, int64_t* sizes_out);

/* Every key = STA_RASTER_EMPTY. */
STA_API int sta_raster_clear(uint64_t* keys, int H, int W, int ssaa, void* stream);

/* Accumulates M points into keys.  Point i:
 *   counters[0] += 1.  pc as above; unless pc_x, pc_y and pc_z are all finite: counters[1] += 1, dropped.
 *   Unless near <= pc_z <= far: counters[2] += 1, dropped.
 *   ix = floor(us + 0.5), iy = floor(vs + 0.5), float64 values.  Unless ix + p / 2 >= 0 and ix - (p - 1) / 2 <= Ws - 1 and the same for iy
 *   and Hs (no footprint pixel is on the canvas; a NaN fails it too): counters[3] += 1, dropped.  Only then ix, iy become integers.
 *   payload: colors == NULL (color_kind STA_RASTER_COLOR_NONE): uint32(id_base + i).
 *            otherwise (r << 24) | (g << 16) | (b << 8) | 255 with r, g, b the uint8 values, or for float32 colours
 *            rint(min(max(double(c), 0), 1) * 255) per channel with NaN -> 0.
 *   key = (uint64(bits of float(pc_z)) << 32) | payload, written to every footprint pixel with a 64-bit atomic minimum (a plain load
 *   that skips the atomic when the stored key is already not larger is allowed: the result does not depend on it).
 * counters: 4 device uint64 (NULL = not counted), added with integer atomics; the caller zeroes them.
 * Refused: M outside [0, 2^31); point_size outside [1, STA_RASTER_MAX_SIZE]; near / far outside the limits above; a T_host or K_host entry
 * that is not finite; a color_kind that does not agree with colors; id_base + M > 2^32 - 1 with colors == NULL (the id 2^32 - 1 is what
 * sta_raster_resolve reports for an empty pixel); the refusals of sta_raster_plan.  M == 0 launches nothing. */
STA_API int sta_raster_points(uint64_t* keys, int H, int W, int ssaa, const float* pts, const void* colors, int color_kind, int64_t id_base,
                              int64_t M, const double* T_host, const double* K_host, double near, double far, int point_size,
                              uint64_t* counters, void* stream);

/* Accumulates S segments, segs [S,2,3] float32 world coordinates, colors [S,3] uint8, into keys.  Segment j with ends A, B:
 *   a = pc(A), b = pc(B); dropped unless all six are finite.  za = a_z, zb = b_z, dz = zb - za.
 *   Depth clip.  Dropped if za < near and zb < near, or za > far and zb > far.
 *     t0 = za < near ? (near - za) / dz : za > far ? (far - za) / dz : 0
 *     t1 = zb < near ? (near - za) / dz : zb > far ? (far - za) / dz : 1
 *     End 0 is a where t0 is the literal 0; else x = a_x + t0 * (b_x - a_x), y likewise, and z is EXACTLY the plane's value (near or far).
 *     End 1 is b where t1 is the literal 1; else the same with t1.
 *   Projection of both ends to (us, vs) as above, w = 1 / z.  Dropped unless the four coordinates are finite and of magnitude <=
 *   STA_RASTER_MAX_COORD.
 *   2-D clip (Liang-Barsky) to xmin = -0.5 - STA_RASTER_CLIP_MARGIN, xmax = (Ws - 0.5) + STA_RASTER_CLIP_MARGIN, ymin / ymax likewise:
 *     dx = us1 - us0, dy = vs1 - vs0, e0 = 0, e1 = 1; for (p, q) in (-dx, us0 - xmin), (dx, xmax - us0), (-dy, vs0 - ymin),
 *     (dy, ymax - vs0), in this order:  p == 0: dropped if q < 0.   p < 0: r = q / p; dropped if r > e1; e0 = r if r > e0.
 *     p > 0: r = q / p; dropped if r < e0; e1 = r if r < e1.
 *     End 0 stays (us0, vs0, w0) bit for bit where e0 is still the literal 0, else (us0 + e0 * dx, vs0 + e0 * dy, w0 + e0 * (w1 - w0));
 *     end 1 stays where e1 is still 1, else the same with e1.  Call the results (U0, V0, W0), (U1, V1, W1).
 *   DDA.  ax = floor(U0 + 0.5), ay, bx, by likewise (float64; the segment is dropped unless all four are in [-16, 8192 + 16), which the
 *   clip guarantees; then they become integers).  n = max(|bx - ax|, |by - ay|).  Step k = 0 .. n: t = double(k) / double(n) (t = 0 when
 *   n == 0), x = floor((U0 + t * (U1 - U0)) + 0.5), y = floor((V0 + t * (V1 - V0)) + 0.5), w = W0 + t * (W1 - W0),
 *   key = (uint64(bits of float(1 / w)) << 32) | the segment's packed colour, written with the footprint of line_width around (x, y).
 *   Every step is independent of the others (one wavefront per segment, lanes over k).
 * Lines and points share one key buffer: lines are occluded by the map and occlude it.
 * Refused: S outside [0, 2^24); line_width outside [1, STA_RASTER_MAX_SIZE]; the rest as sta_raster_points. */
STA_API int sta_raster_lines(uint64_t* keys, int H, int W, int ssaa, const float* segs, const uint8_t* colors, int64_t S, const double* T_host,
                             const double* K_host, double near, double far, int line_width, void* stream);

/* keys -> images of H x W output pixels; each output may be NULL.  background_host: 4 uint8 r, g, b, a.  With s = ssaa, the block of the
 * output pixel (y, x) is the s x s keys (y*s .. y*s + s - 1, x*s .. x*s + s - 1).
 *   rgba_out [H,W,4] uint8, 4-byte aligned.  s == 1: the payload's four bytes, most significant first (r, g, b, then 255 for a colour payload), or
 *       background where empty.  s > 1: per channel (sum over the block + s*s/2) / (s*s) in integers, where a covered sub-pixel gives
 *       its payload's r, g, b and the alpha 255, an empty one the background's four bytes.
 *   depth_out [H,W] float32: the depth of the block's smallest key, +inf when the whole block is empty.
 *   id_out [H,W] uint32: the payload of the block's smallest key, 0xFFFFFFFF when the whole block is empty. */
STA_API int sta_raster_resolve(const uint64_t* keys, int H, int W, int ssaa, const uint8_t* background_host, uint8_t* rgba_out, float* depth_out,
                               uint32_t* id_out, void* stream);

STA_API const char* sta_raster_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
