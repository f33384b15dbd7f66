// libsta_dist.so: the C ABI of include/sta_dist.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other seven libraries includes or links any of this.  Static helpers carry the prefix ds_.
#include "../../include/sta_dist.h"
#include "sta_common.h"
#include "elementwise.h"      // cloud_scan_kernel (voxel.h)
#include "select.h"           // sel_block_scan (voxel.h)
#include "voxel.h"            // the stable LSD radix sort
#include "dist.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>

static_assert(DS_F == STA_DIST_FANOUT && DS_MAX_LEVELS == STA_DIST_MAX_LEVELS, "dist.h repeats the header's constants");
static_assert(DS_VALID == STA_DIST_N_VALID && DS_BAD_INDEX == STA_DIST_N_BAD_INDEX && DS_NON_FINITE == STA_DIST_N_NON_FINITE &&
              DS_NO_AREA == STA_DIST_N_NO_AREA && DS_STATUS == STA_DIST_STATUS && DS_STATUS_BOUND == STA_DIST_STATUS_BOUND && STA_DIST_COUNTERS == 8,
              "dist.h uses the counter layout by number");

static thread_local char ds_err[1024] = "";
static int ds_set_err(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(ds_err, sizeof(ds_err), fmt, ap); va_end(ap);
    return -1;
}
#define DS_HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return ds_set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define DS_REQUIRE(c, ...) do { if (!(c)) return ds_set_err(__VA_ARGS__); } while (0)

extern "C" const char* sta_tri_last_error(void) { return ds_err; }

// One bump layout per buffer serves the plan and the call: what the plan reports is what the call takes.
struct DsBump {
    char* base; int64_t used;
    void* take(int64_t bytes) { void* p = base ? base + used : nullptr; used += (bytes + 255) & ~(int64_t)255; return p; }
};
struct DsSort { unsigned long long* key[2]; int* idx[2]; int* hist; int* dtot; };
struct DsWork { DsSort sort; double* part; double* lu; };

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
    DsBump b{(char*)buf, 0};
    I->tri = (float*)b.take(nt * 36);
    I->src = (int32_t*)b.take(nt * 4);
    I->boxes = (float*)b.take((int64_t)T.off[T.levels] * 24);
    I->counters = (int32_t*)b.take(STA_DIST_COUNTERS * 4);
    I->nt = nt; I->levels = T.levels; I->reserved = 0;
    for (int k = 0; k <= STA_DIST_MAX_LEVELS; ++k) I->level_offset[k] = T.off[k];
    return b.used;
}
static int64_t ds_work_layout(void* buf, int64_t nt, DsWork* W) {
    DsBump b{(char*)buf, 0};
    const int64_t nbs = (nt + VOX_TILE - 1) / VOX_TILE;
    W->sort.key[0] = (unsigned long long*)b.take(nt * 8);
    W->sort.key[1] = (unsigned long long*)b.take(nt * 8);
    W->sort.idx[0] = (int*)b.take(nt * 4);
    W->sort.idx[1] = (int*)b.take(nt * 4);
    W->sort.hist = (int*)b.take(256 * nbs * 4);
    W->sort.dtot = (int*)b.take(256 * 4);
    W->part = (double*)b.take(DS_PARTS * 8 * 8);
    W->lu = (double*)b.take(8 * 8);
    return b.used;
}
static int ds_check_nt(const char* who, int64_t nt) {
    DS_REQUIRE(nt >= 1 && nt < (int64_t)1 << 27, "%s: nt must be in [1, 2^27) (got %lld)", who, (long long)nt);
    return 0;
}
static int ds_check_q(const char* who, int64_t Q) {
    DS_REQUIRE(Q >= 1 && Q < (int64_t)1 << 30, "%s: Q must be in [1, 2^30) (got %lld)", who, (long long)Q);
    return 0;
}
static unsigned ds_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// The stable LSD sort of voxel.h over all 64 bits of key[0] / idx[0]; returns the buffer (0 or 1) that holds the result.
static int ds_sort(hipStream_t st, const DsSort& L, int64_t m64) {
    const int m = (int)m64, nbs = (int)((m64 + VOX_TILE - 1) / VOX_TILE);
    int cur = 0;
    for (int p = 0; p < 8; ++p) {
        const int a = cur, b = cur ^ 1;
        hipLaunchKernelGGL(vox_hist_kernel, dim3(nbs), dim3(256), 0, st, (const unsigned long long*)L.key[a], m, 8 * p, nbs, L.hist);
        hipLaunchKernelGGL(vox_hist_scan_kernel, dim3(256), dim3(256), 0, st, L.hist, nbs, L.dtot);
        hipLaunchKernelGGL(vox_scatter_kernel, dim3(nbs), dim3(256), 0, st, (const unsigned long long*)L.key[a], (const int*)L.idx[a], m, 8 * p, nbs,
                           (const int*)L.hist, (const int*)L.dtot, L.key[b], L.idx[b]);
        cur = b;
    }
    return cur;
}

extern "C" int sta_tri_plan(int64_t nt, int64_t Q, int64_t* sizes_out) {
    const char* who = "tri_plan";
    DS_REQUIRE(sizes_out, "%s: null argument", who);
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
    DS_REQUIRE(nv >= 1 && nv < (int64_t)1 << 31, "%s: nv must be in [1, 2^31) (got %lld)", who, (long long)nv);
    DS_REQUIRE(verts && tris && index_buf && work && index_out_host && counters_out, "%s: null argument", who);
    DsTree T; sta_tri_index I; DsWork W;
    ds_tree(nt, &T);
    const int64_t need_i = ds_index_layout(index_buf, nt, T, &I), need_w = ds_work_layout(work, nt, &W);
    DS_REQUIRE(index_bytes >= need_i, "%s: index_buf of %lld bytes, %lld needed for %lld triangles", who, (long long)index_bytes, (long long)need_i, (long long)nt);
    DS_REQUIRE(work_bytes >= need_w, "%s: work of %lld bytes, %lld needed for %lld triangles", who, (long long)work_bytes, (long long)need_w, (long long)nt);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)nt;
    const unsigned parts = ds_blocks(nt) < DS_PARTS ? ds_blocks(nt) : DS_PARTS;
    hipLaunchKernelGGL(ds_bounds_kernel, dim3(parts), dim3(256), 0, st, verts, (long long)nv, (const int*)tris, n, W.part);
    hipLaunchKernelGGL(ds_bounds_final_kernel, dim3(1), dim3(256), 0, st, (const double*)W.part, (int)parts, W.lu, (int*)I.counters, (int*)counters_out);
    hipLaunchKernelGGL(ds_key_kernel, dim3(ds_blocks(nt)), dim3(256), 0, st, verts, (long long)nv, (const int*)tris, n, (const double*)W.lu, W.sort.key[0],
                       W.sort.idx[0]);
    const int r = ds_sort(st, W.sort, nt);
    hipLaunchKernelGGL(ds_gather_kernel, dim3(ds_blocks(nt)), dim3(256), 0, st, verts, (long long)nv, (const int*)tris, n,
                       (const unsigned long long*)W.sort.key[r], (const int*)W.sort.idx[r], I.tri, (int*)I.src);
    const int n0 = T.off[1] - T.off[0];
    hipLaunchKernelGGL(ds_leaf_kernel, dim3(ds_blocks(n0)), dim3(256), 0, st, (const float*)I.tri, n, (const int*)I.counters, n0, I.boxes);
    for (int l = 1; l < T.levels; ++l) {          // one launch per level
        const int nc = T.off[l] - T.off[l - 1], nn = T.off[l + 1] - T.off[l];
        hipLaunchKernelGGL(ds_level_kernel, dim3(ds_blocks(nn)), dim3(256), 0, st, (const float*)(I.boxes + 6 * (size_t)T.off[l - 1]), nc, nn,
                           I.boxes + 6 * (size_t)T.off[l]);
    }
    DS_HIPCHK(hipGetLastError());
    *index_out_host = I;
    return 0;
}

extern "C" int sta_tri_query(const sta_tri_index* index_host, const float* qry, int64_t Q, double radius, double* d2_out, int32_t* tri_out,
                             float* point_out, void* stream) {
    const char* who = "tri_query";
    if (ds_check_q(who, Q)) return -1;
    DS_REQUIRE(radius >= 0.0, "%s: radius must be >= 0, +inf allowed (got %g)", who, radius);          // false for NaN
    DS_REQUIRE(index_host && qry, "%s: null argument", who);
    if (ds_check_nt(who, index_host->nt)) return -1;
    DsTree T;
    ds_tree(index_host->nt, &T);
    bool same = index_host->levels == T.levels && index_host->tri && index_host->src && index_host->boxes && index_host->counters;
    for (int k = 0; k <= STA_DIST_MAX_LEVELS; ++k) same = same && index_host->level_offset[k] == T.off[k];
    DS_REQUIRE(same, "%s: the index is not one of sta_tri_build (nt = %lld, levels = %d, %d expected)", who, (long long)index_host->nt, index_host->levels,
               T.levels);
    DsQuery P;
    P.tri = index_host->tri; P.src = (const int*)index_host->src; P.boxes = index_host->boxes; P.counters = (int*)index_host->counters;
    P.qry = qry; P.Q = (int)Q; P.r2 = radius * radius;
    P.d2_out = d2_out; P.tri_out = (int*)tri_out; P.point_out = point_out;
    P.tree = T;
    hipLaunchKernelGGL(ds_query_kernel, dim3(ds_blocks(Q)), dim3(256), 0, (hipStream_t)stream, P);
    DS_HIPCHK(hipGetLastError());
    return 0;
}
