// libsta_cloud.so: the C ABI of include/sta_cloud.h.  A translation unit of its own - no handle, no workspace of the library's, no
// allocation: the product library (sta_api.hip) neither includes nor links any of this.  Static helpers carry the prefix cl_.
// The error buffer, REQUIRE, HIPCHK, the bump and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_cloud.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "elementwise.h"      // cloud_scan_kernel, cloud_write_record (voxel.h)
#include "select.h"           // sel_block_scan (voxel.h)
#include "voxel.h"            // bounds, the stable LSD radix sort, the head compaction
#include "cloud.h"

#include <cmath>
#include <cstring>

extern "C" const char* sta_cloud_last_error(void) { return g_err; }

// One bump layout serves sta_nn_plan and sta_nn_build: what the plan reports is what the build takes.
struct ClIndexLayout { unsigned long long* cell_key; int* cell_start; float* spts; int* sidx; };
struct ClBuildLayout { float* bpart; float* bout; ClGrid* grid; VoxSort sort; VoxScan scan; };      // sort.idx[0] is the index's sidx

static int64_t cl_index_layout(void* buf, int64_t M, ClIndexLayout* L) {
    PlanBump b{(char*)buf, 0};
    L->cell_key = (unsigned long long*)b.take(M * 8);
    L->cell_start = (int*)b.take((M + 2) * 4);
    L->spts = (float*)b.take(M * 12);
    L->sidx = (int*)b.take(M * 4);
    return b.used;
}
static int64_t cl_build_layout(void* buf, int64_t M, ClBuildLayout* L) {
    PlanBump b{(char*)buf, 0};
    L->bpart = (float*)b.take(1024 * 32);
    L->bout = (float*)b.take(32);
    L->grid = (ClGrid*)b.take(sizeof(ClGrid));
    vox_take_sort(b, M, &L->sort, false);
    vox_take_scan(b, (M + 255) / 256, &L->scan);
    return b.used;
}
static int cl_query_blocks(int64_t Q) {
    const int64_t nb = (Q + 255) / 256;
    return (int)(nb < CL_MAX_QBLOCKS ? nb : CL_MAX_QBLOCKS);
}
static int64_t cl_query_bytes(int64_t Q) { return (((int64_t)cl_query_blocks(Q) * CL_RECORD * 8) + 255) & ~(int64_t)255; }

extern "C" int sta_nn_plan(int64_t M, int64_t Q, int64_t* sizes_out) {
    REQUIRE(sizes_out, "null argument");
    REQUIRE(M >= 1 && M < (int64_t)1 << 30, "nn_plan: M must be in [1, 2^30) (got %lld)", (long long)M);
    REQUIRE(Q >= 1 && Q < (int64_t)1 << 30, "nn_plan: Q must be in [1, 2^30) (got %lld)", (long long)Q);
    ClIndexLayout il; ClBuildLayout bl;
    sizes_out[0] = cl_index_layout(nullptr, M, &il);
    sizes_out[1] = cl_build_layout(nullptr, M, &bl);
    sizes_out[2] = cl_query_bytes(Q);
    return 0;
}

extern "C" int sta_nn_build(const float* ref, int64_t M, double cell, void* index_buf, int64_t index_bytes, void* work, int64_t work_bytes,
                            sta_nn_index* index_out_host, void* stream) {
    REQUIRE(ref && index_buf && work && index_out_host, "null argument");
    REQUIRE(M >= 1 && M < (int64_t)1 << 30, "nn_build: M must be in [1, 2^30) (got %lld)", (long long)M);
    REQUIRE(std::isfinite(cell) && cell > 0.0, "nn_build: cell must be finite and > 0 (got %g)", cell);
    ClIndexLayout il; ClBuildLayout bl;
    const int64_t need_i = cl_index_layout(index_buf, M, &il), need_w = cl_build_layout(work, M, &bl);
    REQUIRE(index_bytes >= need_i, "nn_build: index_buf of %lld bytes, %lld needed for M = %lld", (long long)index_bytes, (long long)need_i, (long long)M);
    REQUIRE(work_bytes >= need_w, "nn_build: work of %lld bytes, %lld needed for M = %lld", (long long)work_bytes, (long long)need_w, (long long)M);
    memset(index_out_host, 0, sizeof(*index_out_host));
    hipStream_t st = (hipStream_t)stream;
    const int m = (int)M;
    const int nb256 = (m + 255) / 256, nbb = nb256 < 1024 ? nb256 : 1024;
    // 1. bounds -> grid (on the device)  2. keys
    hipLaunchKernelGGL(vox_bounds_kernel, dim3(nbb), dim3(256), 0, st, ref, m, bl.bpart);
    hipLaunchKernelGGL(vox_bounds_final_kernel, dim3(1), dim3(256), 0, st, (const float*)bl.bpart, nbb, bl.bout);
    hipLaunchKernelGGL(cl_grid_kernel, dim3(1), dim3(64), 0, st, (const float*)bl.bout, cell, bl.grid);
    bl.sort.idx[0] = il.sidx;
    unsigned long long* const* key = bl.sort.key;
    hipLaunchKernelGGL(cl_key_kernel, dim3(nb256), dim3(256), 0, st, ref, m, cell, (const ClGrid*)bl.grid, key[0], il.sidx);
    // 3. sort: all 64 key bits, so that the all-ones key of a non-finite point sorts last whatever the extents are; an even
    // number of passes leaves the result in key[0] / idx[0] = the index's sorted_idx
    vox_sort(st, bl.sort, m, 8);
    // 4. heads over all M sorted positions: the non-finite points, if any, are one last "cell" that no query's key reaches
    hipLaunchKernelGGL(vox_head_count_kernel, dim3(nb256), dim3(256), 0, st, (const unsigned long long*)key[0], m, bl.scan.counts);
    vox_scan(st, bl.scan.counts, bl.scan.offs, nb256);
    hipLaunchKernelGGL(vox_head_emit_kernel, dim3(nb256), dim3(256), 0, st, (const unsigned long long*)key[0], m, (const int64_t*)bl.scan.offs, nb256, il.cell_start);
    hipLaunchKernelGGL(cl_finish_kernel, dim3(nb256), dim3(256), 0, st, ref, m, (const unsigned long long*)key[0], (const int*)il.sidx,
                       (const int*)il.cell_start, (const int64_t*)(bl.scan.offs + nb256), il.cell_key, il.spts);
    HIPCHK(hipGetLastError());
    // the call's one synchronisation: the grid and the number of cells
    ClGrid g; int64_t total = 0;
    HIPCHK(hipMemcpyAsync(&g, bl.grid, sizeof(g), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, bl.scan.offs + nb256, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t n = M - g.dropped;
    sta_nn_index* o = index_out_host;
    o->cell = cell; o->M = M; o->n_finite = n;
    if (n > 0) {
        for (int a = 0; a < 3; ++a) {
            const long long hi = g.lo[a] + g.ext[a] - 1;
            REQUIRE(g.lo[a] >= -(long long)STA_NN_MAX_CELL_INDEX && hi <= (long long)STA_NN_MAX_CELL_INDEX,
                    "nn_build: cell index outside +-2^21 on axis %d: [%lld, %lld] at cell %g (extents %lld x %lld x %lld)", a, g.lo[a], hi, cell,
                    g.ext[0], g.ext[1], g.ext[2]);
        }
        REQUIRE(g.ext[0] <= STA_NN_MAX_EXTENT && g.ext[1] <= STA_NN_MAX_EXTENT && g.ext[2] <= STA_NN_MAX_EXTENT,
                "nn_build: grid too wide: %lld x %lld x %lld cells at cell %g (at most %d per axis)", g.ext[0], g.ext[1], g.ext[2], cell,
                STA_NN_MAX_EXTENT);
        for (int a = 0; a < 3; ++a) { o->lo[a] = g.lo[a]; o->ext[a] = g.ext[a]; }
        o->C = total - (g.dropped > 0 ? 1 : 0);
    }
    o->cell_key = (const uint64_t*)il.cell_key; o->cell_start = il.cell_start; o->sorted_pts = il.spts; o->sorted_idx = il.sidx;
    return 0;
}

static void cl_matrix(const double* T_host, double* T) {
    static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(T, T_host ? T_host : eye, sizeof(eye));
}

extern "C" int sta_nn_query(const sta_nn_index* index_host, const float* qry, int64_t Q, const double* T_host, double radius, double* d2_out,
                            int32_t* idx_out, double* record_out, void* work, int64_t work_bytes, void* stream) {
    REQUIRE(index_host && qry, "null argument");
    const sta_nn_index& ix = *index_host;
    REQUIRE(Q >= 1 && Q < (int64_t)1 << 30, "nn_query: Q must be in [1, 2^30) (got %lld)", (long long)Q);
    REQUIRE(ix.cell_key && ix.cell_start && ix.sorted_pts && ix.sorted_idx && std::isfinite(ix.cell) && ix.cell > 0.0 && ix.C >= 0 &&
            ix.C <= ix.n_finite && ix.n_finite <= ix.M && ix.M < (int64_t)1 << 30, "nn_query: not an index of sta_nn_build");
    for (int a = 0; a < 3; ++a)
        REQUIRE(ix.ext[a] >= 0 && ix.ext[a] <= STA_NN_MAX_EXTENT && (ix.C == 0 || ix.ext[a] >= 1), "nn_query: not an index of sta_nn_build");
    REQUIRE(std::isfinite(radius) && radius >= 0.0, "nn_query: radius must be finite and >= 0 (got %g)", radius);
    REQUIRE(radius <= (double)STA_NN_MAX_RINGS * ix.cell, "nn_query: radius %.17g is more than %d cells of %.17g", radius, STA_NN_MAX_RINGS, ix.cell);
    const int nblk = cl_query_blocks(Q);
    if (record_out) {
        REQUIRE(work, "null argument");
        REQUIRE(work_bytes >= cl_query_bytes(Q), "nn_query: work of %lld bytes, %lld needed for Q = %lld", (long long)work_bytes,
                (long long)cl_query_bytes(Q), (long long)Q);
    }
    hipStream_t st = (hipStream_t)stream;
    ClQuery P;
    P.cell_key = (const unsigned long long*)ix.cell_key; P.cell_start = ix.cell_start; P.spts = ix.sorted_pts; P.sidx = ix.sorted_idx;
    for (int a = 0; a < 3; ++a) { P.lo[a] = (double)ix.lo[a]; P.ext[a] = (int)ix.ext[a]; }
    P.C = (int)ix.C; P.cell = ix.cell; P.qry = qry; P.Q = (int)Q;
    cl_matrix(T_host, P.T);
    {
#pragma clang fp contract(off)
        P.r2 = radius * radius;
        int k = 0;                                  // the first ring after which nothing further out can be inside the radius
        while (((double)k * ix.cell) * (1.0 - 9.313225746154785e-10) <= radius) ++k;
        P.kmax = k;                                 // <= STA_NN_MAX_RINGS + 1
    }
    P.d2_out = d2_out; P.idx_out = idx_out; P.part = record_out ? (double*)work : nullptr;
    hipLaunchKernelGGL(cl_query_kernel, dim3(nblk), dim3(256), 0, st, P);
    if (record_out) hipLaunchKernelGGL(cl_record_final_kernel, dim3(1), dim3(256), 0, st, (const double*)work, nblk, record_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_cloud_transform(const float* pts, int64_t M, const double* T_host, float* out, void* stream) {
    REQUIRE(M >= 0 && M < (int64_t)1 << 30, "cloud_transform takes fewer than 2^30 points (got %lld)", (long long)M);
    if (M == 0) return 0;
    REQUIRE(pts && out, "null argument");
    ClMat m;
    cl_matrix(T_host, m.T);
    hipLaunchKernelGGL(cl_transform_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, (long long)M, m, out);
    HIPCHK(hipGetLastError());
    return 0;
}
