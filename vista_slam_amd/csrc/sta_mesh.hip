// libsta_mesh.so: the C ABI of include/sta_mesh.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other four libraries includes or links any of this.  Static helpers carry the prefix ms_.
// The error buffer, REQUIRE, HIPCHK, the bump and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_mesh.h"
#include "../../include/sta_raster.h"     // the limits of the canvas and of near / far (declarations only: nothing of libsta_raster.so is linked)
#include "sta_common.h"
#include "sta_hostkit.h"
#include "elementwise.h"      // cloud_scan_kernel (voxel.h)
#include "select.h"           // sel_block_scan (voxel.h)
#include "voxel.h"            // the stable LSD radix sort
#include "raster.h"           // RsCam, rs_camera, rs_finite, rs_channel, rs_count
#include "mesh.h"

#include <algorithm>
#include <cmath>
#include <cstring>

extern "C" const char* sta_mesh_last_error(void) { return g_err; }

// One bump layout per workspace serves the plan and the call: what the plan reports is what the call takes.
struct MsListLayout { unsigned* count; unsigned* list; };

static int64_t ms_list_layout(void* buf, int64_t nt, MsListLayout* L) {
    PlanBump b{(char*)buf, 0};
    L->count = (unsigned*)b.take(4);
    L->list = (unsigned*)b.take(2 * nt * 4);
    return b.used;
}
static int64_t ms_sort_layout(void* buf, int64_t m, VoxSort* L) {
    PlanBump b{(char*)buf, 0};
    vox_take_sort(b, m, L);
    return b.used;
}

static int ms_check_counts(const char* who, int64_t nt, int64_t nv) {
    REQUIRE(nt >= 0 && nt < (int64_t)1 << 31, "%s: nt must be in [0, 2^31) (got %lld)", who, (long long)nt);
    REQUIRE(nv >= 0 && nv < (int64_t)1 << 31, "%s: nv must be in [0, 2^31) (got %lld)", who, (long long)nv);
    return 0;
}

extern "C" int sta_mesh_plan(int64_t nt, int64_t nv, int64_t* sizes_out) {
    REQUIRE(sizes_out, "mesh_plan: null argument");
    if (ms_check_counts("mesh_plan", nt, nv)) return -1;
    MsListLayout ll; VoxSort sl;
    sizes_out[0] = ms_list_layout(nullptr, nt, &ll);
    sizes_out[1] = 3 * nt < (int64_t)1 << 31 ? ms_sort_layout(nullptr, 3 * nt, &sl) : -1;
    return 0;
}

static int ms_check_canvas(const char* who, int H, int W, int ssaa) {
    REQUIRE(H >= 1 && W >= 1, "%s: H and W must be >= 1 (got %d x %d)", who, H, W);
    REQUIRE(ssaa == 1 || ssaa == 2 || ssaa == 4, "%s: ssaa must be 1, 2 or 4 (got %d)", who, ssaa);
    REQUIRE((long long)H * ssaa <= STA_RASTER_MAX_DIM && (long long)W * ssaa <= STA_RASTER_MAX_DIM,
            "%s: %d x %d at ssaa %d is a key buffer of %lld x %lld, at most %d per axis", who, H, W, ssaa, (long long)H * ssaa, (long long)W * ssaa,
            STA_RASTER_MAX_DIM);
    return 0;
}

extern "C" int sta_mesh_triangles(uint64_t* keys, int H, int W, int ssaa, const float* verts, int64_t nv, const int32_t* tris, int64_t nt,
                                  const float* colors, const double* color_host, const double* light_host, int payload_kind, int cull, int64_t id_base,
                                  const double* T_host, const double* K_host, double near, double far, uint64_t* counters, void* work, int64_t work_bytes,
                                  void* stream) {
    const char* who = "mesh_triangles";
    if (ms_check_canvas(who, H, W, ssaa) || ms_check_counts(who, nt, nv)) return -1;
    REQUIRE(T_host && K_host, "%s: null argument", who);
    for (int i = 0; i < 12; ++i) REQUIRE(std::isfinite(T_host[i]), "%s: T_host[%d] is not finite (%g)", who, i, T_host[i]);
    for (int i = 0; i < 4; ++i) REQUIRE(std::isfinite(K_host[i]), "%s: K_host[%d] is not finite (%g)", who, i, K_host[i]);
    REQUIRE(near >= STA_RASTER_MIN_NEAR && near <= far && far <= STA_RASTER_MAX_FAR, "%s: near / far must satisfy %g <= near <= far <= %g (got %g, %g)", who,
            STA_RASTER_MIN_NEAR, STA_RASTER_MAX_FAR, near, far);
    REQUIRE(payload_kind >= STA_MESH_PAYLOAD_ID && payload_kind <= STA_MESH_PAYLOAD_NORMAL, "%s: payload_kind must be 0, 1 or 2 (got %d)", who, payload_kind);
    if (payload_kind == STA_MESH_PAYLOAD_COLOR)
        REQUIRE((colors != nullptr) != (color_host != nullptr), "%s: payload_kind %d takes exactly one of colors (%s) and color_host (%s)", who, payload_kind,
                colors ? "given" : "NULL", color_host ? "given" : "NULL");
    else
        REQUIRE(!colors && !color_host && !light_host, "%s: payload_kind %d takes no colors (%s), color_host (%s) or light_host (%s)", who, payload_kind,
                colors ? "given" : "NULL", color_host ? "given" : "NULL", light_host ? "given" : "NULL");
    REQUIRE(cull >= STA_MESH_CULL_NONE && cull <= STA_MESH_CULL_FRONT, "%s: cull must be 0, 1 or 2 (got %d)", who, cull);
    if (color_host)
        for (int i = 0; i < 3; ++i) REQUIRE(std::isfinite(color_host[i]), "%s: color_host[%d] is not finite (%g)", who, i, color_host[i]);
    if (light_host) {
        for (int i = 0; i < 4; ++i) REQUIRE(std::isfinite(light_host[i]), "%s: light_host[%d] is not finite (%g)", who, i, light_host[i]);
        REQUIRE(light_host[3] >= 0.0 && light_host[3] <= 1.0, "%s: ambient must be in [0, 1] (got %g)", who, light_host[3]);
    }
    if (payload_kind == STA_MESH_PAYLOAD_ID)
        REQUIRE(id_base >= 0 && id_base + nt <= 4294967295ll, "%s: ids %lld .. %lld + %lld would reach 2^32 - 1, the id of an empty pixel", who,
                (long long)id_base, (long long)id_base, (long long)nt);
    MsListLayout L;
    const int64_t need = ms_list_layout(work, nt, &L);
    REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld triangles", who, (long long)work_bytes, (long long)need, (long long)nt);
    if (nt == 0) return 0;
    REQUIRE(keys && verts && tris && work, "%s: null argument", who);
    MsParams P;
    memcpy(P.cam.T, T_host, sizeof(P.cam.T));
    P.cam.fx = K_host[0]; P.cam.fy = K_host[1]; P.cam.cx = K_host[2]; P.cam.cy = K_host[3];
    P.cam.near = near; P.cam.far = far;
    P.cam.s = (double)ssaa; P.cam.off = (double)(ssaa - 1) * 0.5;
    P.cam.Hs = H * ssaa; P.cam.Ws = W * ssaa;
    P.verts = verts; P.tris = (const int*)tris; P.colors = colors;
    P.nv = nv; P.nt = nt;
    for (int i = 0; i < 3; ++i) { P.ucol[i] = color_host ? color_host[i] : 0.0; P.eye[i] = light_host ? light_host[i] : 0.0; }
    P.ambient = light_host ? light_host[3] : 1.0;
    P.kind = payload_kind; P.lit = light_host ? 1 : 0; P.cull = cull;
    P.id_base = (unsigned)id_base;
    P.keys = (unsigned long long*)keys; P.counters = (unsigned long long*)counters;
    P.list = L.list; P.list_n = L.count;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(L.count, 0, 4, st));
    hipLaunchKernelGGL(ms_setup_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, P);
    const int64_t waves = std::min<int64_t>((2 * nt + 3) / 4, MS_DRAIN_BLOCKS);
    hipLaunchKernelGGL(ms_drain_kernel, dim3((unsigned)waves), dim3(256), 0, st, P);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_mesh_vertex_normals(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, float* normals_out, void* work,
                                       int64_t work_bytes, void* stream) {
    const char* who = "mesh_vertex_normals";
    if (ms_check_counts(who, nt, nv)) return -1;
    REQUIRE(3 * nt < (int64_t)1 << 31, "%s: 3 * nt must be below 2^31 (got nt = %lld)", who, (long long)nt);
    const int64_t m64 = 3 * nt;
    VoxSort L;
    const int64_t need = ms_sort_layout(work, m64, &L);
    REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld triangles", who, (long long)work_bytes, (long long)need, (long long)nt);
    if (nv == 0) return 0;
    REQUIRE(verts && normals_out && (nt == 0 || (tris && work)), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    const int m = (int)m64;
    if (m > 0) {
        hipLaunchKernelGGL(ms_pair_kernel, dim3((unsigned)((m64 + 255) / 256)), dim3(256), 0, st, (const int*)tris, m, (long long)nv, L.key[0], L.idx[0]);
        // the digits that hold the largest key, nv; an even number of passes leaves the result in key[0] / idx[0]
        int passes = 1;
        while (passes < 4 && ((uint64_t)nv >> (8 * passes)) != 0) ++passes;
        passes += passes & 1;
        vox_sort(st, L, m, passes);
    }
    hipLaunchKernelGGL(ms_normal_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, verts, (const int*)tris, (long long)nv, m,
                       (const unsigned long long*)L.key[0], (const int*)L.idx[0], normals_out);
    HIPCHK(hipGetLastError());
    return 0;
}
