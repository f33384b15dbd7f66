// libsta_dist.so: the C ABI of include/sta_dist.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other seven libraries includes or links any of this.  Static helpers carry the prefix ds_.
// The error buffer, REQUIRE, HIPCHK, the bump and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_dist.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "elementwise.h"      // cloud_scan_kernel (voxel.h)
#include "select.h"           // sel_block_scan (voxel.h)
#include "voxel.h"            // the stable LSD radix sort
#include "dist.h"

#include <cmath>

static_assert(DS_F == STA_DIST_FANOUT && DS_MAX_LEVELS == STA_DIST_MAX_LEVELS, "dist.h repeats the header's constants");
static_assert(DS_VALID == STA_DIST_N_VALID && DS_BAD_INDEX == STA_DIST_N_BAD_INDEX && DS_NON_FINITE == STA_DIST_N_NON_FINITE &&
              DS_NO_AREA == STA_DIST_N_NO_AREA && DS_STATUS == STA_DIST_STATUS && DS_STATUS_BOUND == STA_DIST_STATUS_BOUND && STA_DIST_COUNTERS == 8,
              "dist.h uses the counter layout by number");

extern "C" const char* sta_tri_last_error(void) { return g_err; }

// One bump layout per buffer serves the plan and the call: what the plan reports is what the call takes.
struct DsWork { VoxSort sort; double* part; double* lu; };

// levels, offsets: a function of nt alone
static void ds_tree(int64_t nt, DsTree* T) {
    T->nt = (int)nt;
    int64_t cnt = (nt + DS_F - 1) / DS_F, off = 0;
    int l = 0;
    for (int k = 0; k <= DS_MAX_LEVELS; ++k) T->off[k] = 0;
    for (;; ++l) {
        T->off[l] = (int)off;
        off += cnt;
        if (cnt == 1) break;
        cnt = (cnt + DS_F - 1) / DS_F;
    }
    T->levels = l + 1;
    for (int k = l + 1; k <= DS_MAX_LEVELS; ++k) T->off[k] = (int)off;        // off[levels] = the number of nodes, repeated behind it
}
static int64_t ds_index_layout(void* buf, int64_t nt, const DsTree& T, sta_tri_index* I) {
    PlanBump b{(char*)buf, 0};
    I->tri = (float*)b.take(nt * 36);
    I->src = (int32_t*)b.take(nt * 4);
    I->boxes = (float*)b.take((int64_t)T.off[T.levels] * 24);
    I->counters = (int32_t*)b.take(STA_DIST_COUNTERS * 4);
    I->nt = nt; I->levels = T.levels; I->reserved = 0;
    for (int k = 0; k <= STA_DIST_MAX_LEVELS; ++k) I->level_offset[k] = T.off[k];
    return b.used;
}
static int64_t ds_work_layout(void* buf, int64_t nt, DsWork* W) {
    PlanBump b{(char*)buf, 0};
    vox_take_sort(b, nt, &W->sort);
    W->part = (double*)b.take(DS_PARTS * 8 * 8);
    W->lu = (double*)b.take(8 * 8);
    return b.used;
}
static int ds_check_nt(const char* who, int64_t nt) {
    REQUIRE(nt >= 1 && nt < (int64_t)1 << 27, "%s: nt must be in [1, 2^27) (got %lld)", who, (long long)nt);
    return 0;
}
static int ds_check_q(const char* who, int64_t Q) {
    REQUIRE(Q >= 1 && Q < (int64_t)1 << 30, "%s: Q must be in [1, 2^30) (got %lld)", who, (long long)Q);
    return 0;
}

extern "C" int sta_tri_plan(int64_t nt, int64_t Q, int64_t* sizes_out) {
    const char* who = "tri_plan";
    REQUIRE(sizes_out, "%s: null argument", who);
    if (ds_check_nt(who, nt) || ds_check_q(who, Q)) return -1;
    DsTree T; sta_tri_index I; DsWork W;
    ds_tree(nt, &T);
    sizes_out[0] = ds_index_layout(nullptr, nt, T, &I);
    sizes_out[1] = ds_work_layout(nullptr, nt, &W);
    return 0;
}

extern "C" int sta_tri_build(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, void* index_buf, int64_t index_bytes, void* work,
                             int64_t work_bytes, sta_tri_index* index_out_host, int32_t* counters_out, void* stream) {
    const char* who = "tri_build";
    if (ds_check_nt(who, nt)) return -1;
    REQUIRE(nv >= 1 && nv < (int64_t)1 << 31, "%s: nv must be in [1, 2^31) (got %lld)", who, (long long)nv);
    REQUIRE(verts && tris && index_buf && work && index_out_host && counters_out, "%s: null argument", who);
    DsTree T; sta_tri_index I; DsWork W;
    ds_tree(nt, &T);
    const int64_t need_i = ds_index_layout(index_buf, nt, T, &I), need_w = ds_work_layout(work, nt, &W);
    REQUIRE(index_bytes >= need_i, "%s: index_buf of %lld bytes, %lld needed for %lld triangles", who, (long long)index_bytes, (long long)need_i, (long long)nt);
    REQUIRE(work_bytes >= need_w, "%s: work of %lld bytes, %lld needed for %lld triangles", who, (long long)work_bytes, (long long)need_w, (long long)nt);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)nt;
    const unsigned parts = blocks(nt) < DS_PARTS ? blocks(nt) : DS_PARTS;
    hipLaunchKernelGGL(ds_bounds_kernel, dim3(parts), dim3(256), 0, st, verts, (long long)nv, (const int*)tris, n, W.part);
    hipLaunchKernelGGL(ds_bounds_final_kernel, dim3(1), dim3(256), 0, st, (const double*)W.part, (int)parts, W.lu, (int*)I.counters, (int*)counters_out);
    hipLaunchKernelGGL(ds_key_kernel, dim3(blocks(nt)), dim3(256), 0, st, verts, (long long)nv, (const int*)tris, n, (const double*)W.lu, W.sort.key[0],
                       W.sort.idx[0]);
    const int r = vox_sort(st, W.sort, n, 8);          // all 64 key bits
    hipLaunchKernelGGL(ds_gather_kernel, dim3(blocks(nt)), dim3(256), 0, st, verts, (long long)nv, (const int*)tris, n,
                       (const unsigned long long*)W.sort.key[r], (const int*)W.sort.idx[r], I.tri, (int*)I.src);
    const int n0 = T.off[1] - T.off[0];
    hipLaunchKernelGGL(ds_leaf_kernel, dim3(blocks(n0)), dim3(256), 0, st, (const float*)I.tri, n, (const int*)I.counters, n0, I.boxes);
    for (int l = 1; l < T.levels; ++l) {          // one launch per level
        const int nc = T.off[l] - T.off[l - 1], nn = T.off[l + 1] - T.off[l];
        hipLaunchKernelGGL(ds_level_kernel, dim3(blocks(nn)), dim3(256), 0, st, (const float*)(I.boxes + 6 * (size_t)T.off[l - 1]), nc, nn,
                           I.boxes + 6 * (size_t)T.off[l]);
    }
    HIPCHK(hipGetLastError());
    *index_out_host = I;
    return 0;
}

extern "C" int sta_tri_query(const sta_tri_index* index_host, const float* qry, int64_t Q, double radius, double* d2_out, int32_t* tri_out,
                             float* point_out, void* stream) {
    const char* who = "tri_query";
    if (ds_check_q(who, Q)) return -1;
    REQUIRE(radius >= 0.0, "%s: radius must be >= 0, +inf allowed (got %g)", who, radius);          // false for NaN
    REQUIRE(index_host && qry, "%s: null argument", who);
    if (ds_check_nt(who, index_host->nt)) return -1;
    DsTree T;
    ds_tree(index_host->nt, &T);
    bool same = index_host->levels == T.levels && index_host->tri && index_host->src && index_host->boxes && index_host->counters;
    for (int k = 0; k <= STA_DIST_MAX_LEVELS; ++k) same = same && index_host->level_offset[k] == T.off[k];
    REQUIRE(same, "%s: the index is not one of sta_tri_build (nt = %lld, levels = %d, %d expected)", who, (long long)index_host->nt, index_host->levels,
            T.levels);
    DsQuery P;
    P.tri = index_host->tri; P.src = (const int*)index_host->src; P.boxes = index_host->boxes; P.counters = (int*)index_host->counters;
    P.qry = qry; P.Q = (int)Q; P.r2 = radius * radius;
    P.d2_out = d2_out; P.tri_out = (int*)tri_out; P.point_out = point_out;
    P.tree = T;
    hipLaunchKernelGGL(ds_query_kernel, dim3(blocks(Q)), dim3(256), 0, (hipStream_t)stream, P);
    HIPCHK(hipGetLastError());
    return 0;
}
