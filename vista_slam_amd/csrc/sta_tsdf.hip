// libsta_tsdf.so: the C ABI of include/sta_tsdf.h.  A translation unit of its own - no handle, no workspace of the library's, no
// allocation: none of the other three libraries includes or links any of this.  Static helpers carry the prefix ts_.
// The error buffer, REQUIRE, HIPCHK, the bump and blocks() are sta_hostkit.h's: one copy per library, none exported.
#pragma clang fp contract(off)
#include "../../include/sta_tsdf.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "elementwise.h"      // cloud_scan_kernel (voxel.h)
#include "select.h"           // sel_block_scan (voxel.h)
#include "voxel.h"            // the stable LSD radix sort, vox_block_count / vox_block_rank
#include "tsdf.h"

#include <cmath>
#include <cstring>

extern "C" const char* sta_tsdf_last_error(void) { return g_err; }

// One bump layout per workspace serves the plan and the call: what the plan reports is what the call takes.
struct TsBlocksLayout { VoxSort sort; VoxScan scan; unsigned long long* counters; };      // the sort's payload is carried, never read by this library
struct TsMeshLayout { unsigned char* mask; unsigned short* pre; int* vcnt; int* tcnt; int64_t* voff; int64_t* toff; };

static int64_t ts_blocks_layout(void* buf, int64_t n8, TsBlocksLayout* L) {
    PlanBump b{(char*)buf, 0};
    vox_take_sort(b, n8, &L->sort);
    vox_take_scan(b, (n8 + 255) / 256, &L->scan);
    L->counters = (unsigned long long*)b.take(16);
    return b.used;
}
static int64_t ts_mesh_layout(void* buf, int64_t nb, TsMeshLayout* L) {
    PlanBump b{(char*)buf, 0};
    L->mask = (unsigned char*)b.take(nb * 512);
    L->pre = (unsigned short*)b.take(nb * 512 * 2);
    L->vcnt = (int*)b.take(nb * 4);
    L->tcnt = (int*)b.take(nb * 4);
    L->voff = (int64_t*)b.take((nb + 1) * 8);
    L->toff = (int64_t*)b.take((nb + 1) * 8);
    return b.used;
}

static int ts_check_grid(const char* who, double voxel_size, double trunc) {
    REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0, "%s: voxel_size must be finite and > 0 (got %g)", who, voxel_size);
    REQUIRE(std::isfinite(trunc) && trunc > 0.0, "%s: trunc must be finite and > 0 (got %g)", who, trunc);
    REQUIRE(trunc <= STA_TSDF_MAX_TRUNC_VOXELS * voxel_size, "%s: trunc %g is more than %d voxels of %g", who, trunc, STA_TSDF_MAX_TRUNC_VOXELS, voxel_size);
    return 0;
}
static int ts_check_views(const char* who, int64_t V, int H, int W) {
    REQUIRE(H >= 1 && W >= 1, "%s: H and W must be >= 1 (got %d x %d)", who, H, W);
    REQUIRE(V >= 1, "%s: V must be >= 1 (got %lld)", who, (long long)V);
    REQUIRE(V < STA_TSDF_MAX_PIXELS && V * (int64_t)H < STA_TSDF_MAX_PIXELS && V * (int64_t)H * W < STA_TSDF_MAX_PIXELS,
            "%s: V * H * W must be below 2^28 (got %lld x %d x %d)", who, (long long)V, H, W);
    return 0;
}
static int ts_origin(const char* who, const double* origin_host, double* o) {
    for (int a = 0; a < 3; ++a) {
        o[a] = origin_host ? origin_host[a] : 0.0;
        REQUIRE(std::isfinite(o[a]), "%s: origin_host[%d] is not finite (%g)", who, a, o[a]);
    }
    return 0;
}

extern "C" int sta_tsdf_plan(int64_t V, int H, int W, double voxel_size, double trunc, int64_t max_blocks, int64_t max_vertices, int64_t max_triangles,
                             int64_t* sizes_out) {
    REQUIRE(sizes_out, "tsdf_plan: null argument");
    if (ts_check_grid("tsdf_plan", voxel_size, trunc) || ts_check_views("tsdf_plan", V, H, W)) return -1;
    REQUIRE(max_blocks >= 1 && max_blocks < STA_TSDF_MAX_BLOCKS, "tsdf_plan: max_blocks must be in [1, 2^24) (got %lld)", (long long)max_blocks);
    REQUIRE(max_vertices >= 0 && max_vertices < (int64_t)1 << 31 && max_triangles >= 0 && max_triangles < (int64_t)1 << 31,
            "tsdf_plan: max_vertices and max_triangles must be in [0, 2^31) (got %lld, %lld)", (long long)max_vertices, (long long)max_triangles);
    TsBlocksLayout bl; TsMeshLayout ml;
    const int64_t n8 = 8 * V * H * W;
    sizes_out[0] = ts_blocks_layout(nullptr, n8, &bl);
    sizes_out[1] = max_blocks * 8;
    sizes_out[2] = max_blocks * 512 * 4;
    sizes_out[3] = max_blocks * 512 * 12;
    sizes_out[4] = ts_mesh_layout(nullptr, max_blocks, &ml);
    sizes_out[5] = max_vertices * 12;
    sizes_out[6] = max_triangles * 12;
    sizes_out[7] = n8;
    return 0;
}

extern "C" int sta_tsdf_table(int8_t* table_out_host) {
    REQUIRE(table_out_host, "tsdf_table: null argument");
    static_assert(sizeof(ts_table_host.e) == 6 * 16 * STA_TSDF_TABLE_ROW, "the table is [6][16][7] int8");
    memcpy(table_out_host, ts_table_host.e, sizeof(ts_table_host.e));
    return 0;
}

extern "C" int sta_tsdf_blocks(const float* depths, const float* scales, const double* K, const double* c2w, const float* obs, int64_t V, int H, int W,
                               double voxel_size, double trunc, const double* origin_host, double depth_max, uint64_t* keys_out, int64_t max_blocks,
                               void* work, int64_t work_bytes, int64_t* counts_out_host, void* stream) {
    REQUIRE(depths && scales && K && c2w && obs && keys_out && work && counts_out_host, "tsdf_blocks: null argument");
    if (ts_check_grid("tsdf_blocks", voxel_size, trunc) || ts_check_views("tsdf_blocks", V, H, W)) return -1;
    REQUIRE(max_blocks >= 1 && max_blocks < STA_TSDF_MAX_BLOCKS, "tsdf_blocks: max_blocks must be in [1, 2^24) (got %lld)", (long long)max_blocks);
    REQUIRE(depth_max > 0.0, "tsdf_blocks: depth_max must be > 0 (got %g)", depth_max);
    TsGrid g;
    if (ts_origin("tsdf_blocks", origin_host, g.o)) return -1;
    g.vs = voxel_size; g.trunc = trunc; g.depth_max = depth_max;
    const int64_t n = V * H * W, n8 = 8 * n;
    TsBlocksLayout L;
    const int64_t need = ts_blocks_layout(work, n8, &L);
    REQUIRE(work_bytes >= need, "tsdf_blocks: work of %lld bytes, %lld needed for %lld x %d x %d", (long long)work_bytes, (long long)need, (long long)V, H, W);
    counts_out_host[0] = counts_out_host[1] = counts_out_host[2] = 0;
    hipStream_t st = (hipStream_t)stream;
    const int m = (int)n8, nb256 = (int)((n8 + 255) / 256);
    HIPCHK(hipMemsetAsync(L.counters, 0, 16, st));
    hipLaunchKernelGGL(ts_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, depths, scales, K, c2w, obs, (int)n, H * W, W, g, L.sort.key[0], L.counters);
    // all 64 key bits, so that the sentinel sorts behind every block; an even number of passes leaves the result in key[0]
    vox_sort(st, L.sort, m, 8);
    hipLaunchKernelGGL(ts_head_count_kernel, dim3(nb256), dim3(256), 0, st, (const unsigned long long*)L.sort.key[0], m, L.scan.counts);
    vox_scan(st, L.scan.counts, L.scan.offs, nb256);
    hipLaunchKernelGGL(ts_head_emit_kernel, dim3(nb256), dim3(256), 0, st, (const unsigned long long*)L.sort.key[0], m, (const int64_t*)L.scan.offs, (long long)max_blocks,
                       (unsigned long long*)keys_out);
    HIPCHK(hipGetLastError());
    // the call's one synchronisation: the three counts
    int64_t nb = 0; unsigned long long cnt[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&nb, L.scan.offs + nb256, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cnt, L.counters, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    counts_out_host[0] = nb; counts_out_host[1] = (int64_t)cnt[0]; counts_out_host[2] = (int64_t)cnt[1];
    REQUIRE(nb <= max_blocks, "tsdf_blocks: the views touch %lld blocks, max_blocks is %lld", (long long)nb, (long long)max_blocks);
    return 0;
}

extern "C" int sta_tsdf_clear(float* tsdf, float* weight, float* rgb, int64_t nb, void* stream) {
    REQUIRE(nb >= 0 && nb < STA_TSDF_MAX_BLOCKS, "tsdf_clear: nb must be in [0, 2^24) (got %lld)", (long long)nb);
    if (nb == 0) return 0;
    REQUIRE(tsdf && weight, "tsdf_clear: null argument");
    const long long n = (long long)nb * 512;
    hipLaunchKernelGGL(ts_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tsdf, weight, rgb, n);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_tsdf_integrate(const uint64_t* keys, int64_t nb, float* tsdf, float* weight, float* rgb, const float* depths, const float* scales,
                                  const double* K, const double* w2c, const float* obs, const float* imgs, int64_t V, int H, int W, int64_t v0, int64_t v1,
                                  double voxel_size, double trunc, const double* origin_host, double depth_max, double max_weight, void* stream) {
    if (ts_check_grid("tsdf_integrate", voxel_size, trunc) || ts_check_views("tsdf_integrate", V, H, W)) return -1;
    REQUIRE(nb >= 0 && nb < STA_TSDF_MAX_BLOCKS, "tsdf_integrate: nb must be in [0, 2^24) (got %lld)", (long long)nb);
    REQUIRE(0 <= v0 && v0 <= v1 && v1 <= V, "tsdf_integrate: views [%lld, %lld) of %lld", (long long)v0, (long long)v1, (long long)V);
    REQUIRE(depth_max > 0.0, "tsdf_integrate: depth_max must be > 0 (got %g)", depth_max);
    REQUIRE(std::isfinite(max_weight) && max_weight > 0.0, "tsdf_integrate: max_weight must be finite and > 0 (got %g)", max_weight);
    TsInt p;
    if (ts_origin("tsdf_integrate", origin_host, p.o)) return -1;
    if (nb == 0 || v0 == v1) return 0;
    REQUIRE(keys && tsdf && weight && depths && scales && K && w2c && obs, "tsdf_integrate: null argument");
    p.keys = (const unsigned long long*)keys; p.tsdf = tsdf; p.weight = weight; p.rgb = rgb;
    p.depths = depths; p.scales = scales; p.K = K; p.w2c = w2c; p.obs = obs; p.imgs = imgs;
    p.H = H; p.W = W; p.v0 = (int)v0; p.v1 = (int)v1;
    p.vs = voxel_size; p.trunc = trunc; p.depth_max = depth_max; p.max_weight = max_weight;
    hipLaunchKernelGGL(ts_integrate_kernel, dim3((unsigned)nb), dim3(512), 0, (hipStream_t)stream, p);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_tsdf_mesh(const uint64_t* keys, int64_t nb, const float* tsdf, const float* weight, const float* rgb, double voxel_size,
                             const double* origin_host, double min_weight, float* verts_out, float* cols_out, int32_t* tris_out, int64_t max_vertices,
                             int64_t max_triangles, void* work, int64_t work_bytes, int64_t* counts_out_host, void* stream) {
    REQUIRE(counts_out_host, "tsdf_mesh: null argument");
    REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0, "tsdf_mesh: voxel_size must be finite and > 0 (got %g)", voxel_size);
    REQUIRE(nb >= 0 && nb < STA_TSDF_MAX_BLOCKS, "tsdf_mesh: nb must be in [0, 2^24) (got %lld)", (long long)nb);
    REQUIRE(std::isfinite(min_weight) && min_weight > 0.0, "tsdf_mesh: min_weight must be finite and > 0 (got %g)", min_weight);
    REQUIRE(max_vertices >= 0 && max_vertices < (int64_t)1 << 31 && max_triangles >= 0 && max_triangles < (int64_t)1 << 31,
            "tsdf_mesh: max_vertices and max_triangles must be in [0, 2^31) (got %lld, %lld)", (long long)max_vertices, (long long)max_triangles);
    TsMesh p;
    if (ts_origin("tsdf_mesh", origin_host, p.o)) return -1;
    counts_out_host[0] = counts_out_host[1] = 0;
    if (nb == 0) return 0;
    REQUIRE(keys && tsdf && weight && work, "tsdf_mesh: null argument");
    TsMeshLayout L;
    const int64_t need = ts_mesh_layout(work, nb, &L);
    REQUIRE(work_bytes >= need, "tsdf_mesh: work of %lld bytes, %lld needed for %lld blocks", (long long)work_bytes, (long long)need, (long long)nb);
    p.keys = (const unsigned long long*)keys; p.nb = (int)nb; p.tsdf = tsdf; p.weight = weight; p.rgb = rgb;
    p.vs = voxel_size; p.min_weight = min_weight;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ts_mesh_mask_kernel, dim3((unsigned)nb), dim3(256), 0, st, p, L.mask, L.pre, L.vcnt, L.tcnt);
    vox_scan(st, L.vcnt, L.voff, (int)nb);
    vox_scan(st, L.tcnt, L.toff, (int)nb);
    HIPCHK(hipGetLastError());
    // the call's one synchronisation: the two counts, before anything is written to the outputs
    int64_t nv = 0, nt = 0;
    HIPCHK(hipMemcpyAsync(&nv, L.voff + nb, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nt, L.toff + nb, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    counts_out_host[0] = nv; counts_out_host[1] = nt;
    REQUIRE(nv < (int64_t)1 << 31 && nt < (int64_t)1 << 31, "tsdf_mesh: %lld vertices and %lld triangles do not fit int32 indices", (long long)nv, (long long)nt);
    if (!verts_out && !tris_out) return 0;
    REQUIRE(nv <= max_vertices && nt <= max_triangles, "tsdf_mesh: the mesh has %lld vertices and %lld triangles, the capacities are %lld and %lld",
            (long long)nv, (long long)nt, (long long)max_vertices, (long long)max_triangles);
    if (nv == 0) return 0;
    hipLaunchKernelGGL(ts_mesh_emit_kernel, dim3((unsigned)nb), dim3(256), 0, st, p, (const unsigned char*)L.mask, (const unsigned short*)L.pre,
                       (const int64_t*)L.voff, (const int64_t*)L.toff, verts_out, rgb ? cols_out : nullptr, tris_out);
    HIPCHK(hipGetLastError());
    return 0;
}
