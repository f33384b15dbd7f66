// libsta_knn.so: the C ABI of include/sta_knn.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other ten libraries includes or links any of this, and it includes none of theirs (the index of
// libsta_cloud.so comes in as a host struct that the header restates).  Static helpers carry the prefix kn_.
// The error buffer, REQUIRE, HIPCHK and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_knn.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "knn.h"

#include <cmath>

static_assert(KN_MAX_K == STA_KNN_MAX_K && KN_RECORD == STA_KNN_RECORD && KN_USED <= KN_RECORD && KN_STATUS_BOUND == STA_KNN_STATUS_BOUND &&
              KN_STATUS_ORDER == STA_KNN_STATUS_ORDER, "knn.h repeats the header's constants");
// one wave's lists at the largest k: three of them fit the 160 KiB of a CU
static_assert((size_t)KN_MAX_K * 64 * (sizeof(double) + sizeof(int)) * 3 <= 160 * 1024, "three workgroups of kn_query_kernel per CU at k = 64");

extern "C" const char* sta_knn_last_error(void) { return g_err; }

static int kn_check_counts(const char* who, int64_t M, int64_t Q, int64_t k) {
    REQUIRE(M >= 1 && M < (int64_t)1 << 30, "%s: M must be in [1, 2^30) (got %lld)", who, (long long)M);
    REQUIRE(Q >= 1 && Q < (int64_t)1 << 30, "%s: Q must be in [1, 2^30) (got %lld)", who, (long long)Q);
    REQUIRE(k >= 1 && k <= STA_KNN_MAX_K, "%s: k must be in [1, %d] (got %lld)", who, STA_KNN_MAX_K, (long long)k);
    return 0;
}
static int kn_moments_blocks(int64_t Q) {
    const int64_t nb = (Q + 255) / 256;
    return (int)(nb < KN_MAX_QBLOCKS ? nb : KN_MAX_QBLOCKS);
}
// the workspace of a moments call: one partial row per workgroup
static int64_t kn_work_bytes(int64_t Q) {
    PlanBump b{nullptr, 0};
    b.take((int64_t)kn_moments_blocks(Q) * KN_RECORD * (int64_t)sizeof(double));
    return b.used;
}

extern "C" int sta_knn_plan(int64_t M, int64_t Q, int64_t k, int64_t* sizes_out) {
    const char* who = "knn_plan";
    REQUIRE(sizes_out, "%s: null argument", who);
    if (kn_check_counts(who, M, Q, k)) return -1;
    sizes_out[0] = Q * k * (int64_t)sizeof(double);
    sizes_out[1] = Q * k * (int64_t)sizeof(int32_t);
    sizes_out[2] = kn_work_bytes(Q);
    return 0;
}

extern "C" int sta_knn_query(const sta_knn_grid* grid_host, const float* qry, int64_t Q, const int32_t* order, int64_t self_base, int64_t k,
                             double radius, double* d2_out, int32_t* idx_out, int32_t* count_out, int32_t* status, void* stream) {
    const char* who = "knn_query";
    REQUIRE(grid_host, "%s: null argument", who);
    const sta_knn_grid& ix = *grid_host;
    REQUIRE(std::isfinite(ix.cell) && ix.cell > 0.0 && ix.C >= 0 && ix.C <= ix.n_finite && ix.n_finite <= ix.M && ix.M >= 1 && ix.M < (int64_t)1 << 30,
            "%s: not an index of sta_nn_build", who);
    for (int a = 0; a < 3; ++a)
        REQUIRE(ix.ext[a] >= 0 && ix.ext[a] <= (int64_t)1 << 21 && (ix.C == 0 || ix.ext[a] >= 1), "%s: not an index of sta_nn_build", who);
    if (kn_check_counts(who, ix.M, Q, k)) return -1;
    REQUIRE(std::isfinite(radius) && radius >= 0.0, "%s: radius must be finite and >= 0 (got %g)", who, radius);
    REQUIRE(radius <= (double)STA_KNN_MAX_RINGS * ix.cell, "%s: radius %.17g is more than %d cells of %.17g", who, radius, STA_KNN_MAX_RINGS, ix.cell);
    REQUIRE(ix.cell_key && ix.cell_start && ix.sorted_pts && ix.sorted_idx && qry && status, "%s: null argument", who);
    KnQuery P;
    P.cell_key = (const unsigned long long*)ix.cell_key; P.cell_start = (const int*)ix.cell_start; P.spts = ix.sorted_pts; P.sidx = (const int*)ix.sorted_idx;
    for (int a = 0; a < 3; ++a) { P.lo[a] = (double)ix.lo[a]; P.ext[a] = (int)ix.ext[a]; }
    P.C = (int)ix.C; P.n = (int)ix.n_finite; P.cell = ix.cell;
    P.qry = qry; P.order = (const int*)order; P.Q = (int)Q; P.self_base = self_base >= 0 ? (long long)self_base : -1; P.k = (int)k;
    {
#pragma clang fp contract(off)
        P.r2 = radius * radius;
        int r = 0;                                  // the first ring after which nothing further out can be inside the radius
        while (((double)r * ix.cell) * (1.0 - 9.313225746154785e-10) <= radius) ++r;
        P.kmax = r;                                 // <= STA_KNN_MAX_RINGS + 1
    }
    P.d2_out = d2_out; P.idx_out = (int*)idx_out; P.count_out = (int*)count_out; P.status = (int*)status;
    const size_t lds = (size_t)k * 64 * (sizeof(double) + sizeof(int));          // 768 B per lane at k = 64: 48 KiB, one wave per workgroup
    hipLaunchKernelGGL(kn_query_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), lds, (hipStream_t)stream, P);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_knn_moments(const float* ref, int64_t M, const float* qry, int64_t Q, const double* d2, const int32_t* idx, const int32_t* count,
                               int64_t k, const float* view, const double* view_host, int64_t min_count, float* normal_out, double* curv_out,
                               double* mean_dist_out, double* record_out, void* work, int64_t work_bytes, void* stream) {
    const char* who = "knn_moments";
    if (kn_check_counts(who, M, Q, k)) return -1;
    REQUIRE(min_count >= STA_KNN_MIN_COUNT, "%s: min_count must be at least %d (got %lld)", who, STA_KNN_MIN_COUNT, (long long)min_count);
    if (record_out) {
        const int64_t need = kn_work_bytes(Q);
        REQUIRE(work && work_bytes >= need, "%s: work of %lld bytes is required for Q = %lld (got %s%lld)", who, (long long)need, (long long)Q,
                work ? "" : "a null pointer and ", (long long)work_bytes);
    }
    REQUIRE(ref && idx && count, "%s: null argument", who);
    REQUIRE(d2 || !(mean_dist_out || record_out), "%s: mean_dist_out and record_out need d2", who);
    REQUIRE(qry || !(view || view_host), "%s: a viewpoint needs qry", who);
    KnMoments P;
    P.ref = ref; P.M = (long long)M; P.qry = qry; P.Q = (int)Q; P.d2 = d2; P.idx = (const int*)idx; P.count = (const int*)count; P.k = (int)k;
    P.view = view; P.has_vh = (!view && view_host) ? 1 : 0;
    for (int a = 0; a < 3; ++a) P.vh[a] = P.has_vh ? view_host[a] : 0.0;
    P.min_count = (int)(min_count < (int64_t)1 << 30 ? min_count : (int64_t)1 << 30);
    P.normal_out = normal_out; P.curv_out = curv_out; P.mean_dist_out = mean_dist_out; P.part = record_out ? (double*)work : nullptr;
    const int nb = kn_moments_blocks(Q);
    hipLaunchKernelGGL(kn_moments_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, P);
    HIPCHK(hipGetLastError());
    if (record_out) {
        hipLaunchKernelGGL(kn_record_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)work, nb, record_out);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
