// libsta_raster.so: the C ABI of include/sta_raster.h.  A translation unit of its own - no handle, no workspace, no allocation: neither
// the product library (sta_api.hip) nor libsta_cloud.so includes or links any of this.  Static helpers carry the prefix rs_.
// The error buffer, REQUIRE, HIPCHK, the bump and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_raster.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "raster.h"

#include <cmath>
#include <cstring>

extern "C" const char* sta_raster_last_error(void) { return g_err; }

static int rs_check_canvas(const char* who, int H, int W, int ssaa) {
    REQUIRE(H >= 1 && W >= 1, "%s: H and W must be >= 1 (got %d x %d)", who, H, W);
    REQUIRE(ssaa == 1 || ssaa == 2 || ssaa == 4, "%s: ssaa must be 1, 2 or 4 (got %d)", who, ssaa);
    REQUIRE((long long)H * ssaa <= STA_RASTER_MAX_DIM && (long long)W * ssaa <= STA_RASTER_MAX_DIM,
            "%s: %d x %d at ssaa %d is a key buffer of %lld x %lld, at most %d per axis", who, H, W, ssaa, (long long)H * ssaa, (long long)W * ssaa,
            STA_RASTER_MAX_DIM);
    return 0;
}

extern "C" int sta_raster_plan(int H, int W, int ssaa, int64_t* sizes_out) {
    REQUIRE(sizes_out, "raster_plan: null argument");
    if (rs_check_canvas("raster_plan", H, W, ssaa)) return -1;
    sizes_out[1] = (int64_t)H * ssaa;
    sizes_out[2] = (int64_t)W * ssaa;
    sizes_out[0] = sizes_out[1] * sizes_out[2] * 8;
    return 0;
}

extern "C" int sta_raster_clear(uint64_t* keys, int H, int W, int ssaa, void* stream) {
    REQUIRE(keys, "raster_clear: null argument");
    if (rs_check_canvas("raster_clear", H, W, ssaa)) return -1;
    const long long n = (long long)H * ssaa * W * ssaa;
    hipLaunchKernelGGL(rs_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)keys, n);
    HIPCHK(hipGetLastError());
    return 0;
}

static int rs_camera_of(const char* who, int H, int W, int ssaa, const double* T_host, const double* K_host, double near, double far, RsCam* c) {
    if (rs_check_canvas(who, H, W, ssaa)) return -1;
    REQUIRE(T_host && K_host, "%s: null argument", who);
    for (int i = 0; i < 12; ++i) REQUIRE(std::isfinite(T_host[i]), "%s: T_host[%d] is not finite (%g)", who, i, T_host[i]);
    for (int i = 0; i < 4; ++i) REQUIRE(std::isfinite(K_host[i]), "%s: K_host[%d] is not finite (%g)", who, i, K_host[i]);
    REQUIRE(near >= STA_RASTER_MIN_NEAR && near <= far && far <= STA_RASTER_MAX_FAR, "%s: near / far must satisfy %g <= near <= far <= %g (got %g, %g)", who,
            STA_RASTER_MIN_NEAR, STA_RASTER_MAX_FAR, near, far);
    memcpy(c->T, T_host, sizeof(c->T));
    c->fx = K_host[0]; c->fy = K_host[1]; c->cx = K_host[2]; c->cy = K_host[3];
    c->near = near; c->far = far;
    c->s = (double)ssaa; c->off = (double)(ssaa - 1) * 0.5;
    c->Hs = H * ssaa; c->Ws = W * ssaa;
    return 0;
}

extern "C" int sta_raster_points(uint64_t* keys, int H, int W, int ssaa, const float* pts, const void* colors, int color_kind, int64_t id_base,
                                 int64_t M, const double* T_host, const double* K_host, double near, double far, int point_size,
                                 uint64_t* counters, void* stream) {
    RsCam c;
    if (rs_camera_of("raster_points", H, W, ssaa, T_host, K_host, near, far, &c)) return -1;
    REQUIRE(M >= 0 && M < (int64_t)1 << 31, "raster_points: M must be in [0, 2^31) (got %lld)", (long long)M);
    REQUIRE(point_size >= 1 && point_size <= STA_RASTER_MAX_SIZE, "raster_points: point_size must be in [1, %d] (got %d)", STA_RASTER_MAX_SIZE, point_size);
    REQUIRE((colors == nullptr) == (color_kind == STA_RASTER_COLOR_NONE) && color_kind >= STA_RASTER_COLOR_NONE && color_kind <= STA_RASTER_COLOR_F32,
            "raster_points: color_kind %d does not agree with colors (%s)", color_kind, colors ? "given" : "NULL");
    if (!colors)
        REQUIRE(id_base >= 0 && id_base + M <= 4294967295ll, "raster_points: ids %lld .. %lld + %lld would reach 2^32 - 1, the id of an empty pixel",
                (long long)id_base, (long long)id_base, (long long)M);
    if (M == 0) return 0;
    REQUIRE(keys && pts, "raster_points: null argument");
    hipLaunchKernelGGL(rs_points_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)keys, c, pts, colors,
                       color_kind, (unsigned)id_base, (long long)M, point_size, (unsigned long long*)counters);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_raster_lines(uint64_t* keys, int H, int W, int ssaa, const float* segs, const uint8_t* colors, int64_t S, const double* T_host,
                                const double* K_host, double near, double far, int line_width, void* stream) {
    RsCam c;
    if (rs_camera_of("raster_lines", H, W, ssaa, T_host, K_host, near, far, &c)) return -1;
    REQUIRE(S >= 0 && S < (int64_t)1 << 24, "raster_lines: S must be in [0, 2^24) (got %lld)", (long long)S);
    REQUIRE(line_width >= 1 && line_width <= STA_RASTER_MAX_SIZE, "raster_lines: line_width must be in [1, %d] (got %d)", STA_RASTER_MAX_SIZE, line_width);
    if (S == 0) return 0;
    REQUIRE(keys && segs && colors, "raster_lines: null argument");
    hipLaunchKernelGGL(rs_lines_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)keys, c, segs,
                       (const unsigned char*)colors, (long long)S, line_width);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_raster_resolve(const uint64_t* keys, int H, int W, int ssaa, const uint8_t* background_host, uint8_t* rgba_out, float* depth_out,
                                  uint32_t* id_out, void* stream) {
    if (rs_check_canvas("raster_resolve", H, W, ssaa)) return -1;
    REQUIRE(keys, "raster_resolve: null argument");
    REQUIRE(!rgba_out || background_host, "raster_resolve: rgba_out needs background_host");
    REQUIRE(((uintptr_t)rgba_out & 3) == 0, "raster_resolve: rgba_out must be 4-byte aligned");
    if (!rgba_out && !depth_out && !id_out) return 0;
    RsBackground bg{{0, 0, 0, 0}};
    if (background_host) memcpy(bg.v, background_host, 4);
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(rs_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)keys, H, W, ssaa, bg,
                       (unsigned char*)rgba_out, depth_out, (unsigned*)id_out);
    HIPCHK(hipGetLastError());
    return 0;
}
