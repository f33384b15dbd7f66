// libsta_reg.so: the C ABI of include/sta_reg.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other nine libraries includes or links any of this, and it includes none of theirs (the index of
// libsta_dist.so comes in as plain arguments).  Static helpers carry the prefix rg_.
// The error buffer, REQUIRE, HIPCHK and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_reg.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "reg.h"

static_assert(RG_F == STA_REG_FANOUT && RG_MAX_LEVELS == STA_REG_MAX_LEVELS && RG_VALID == STA_REG_N_VALID && RG_STATUS_BOUND == STA_REG_STATUS_BOUND &&
              RG_RECORD == STA_REG_RECORD && RG_USED <= RG_RECORD, "reg.h repeats the header's constants");

extern "C" const char* sta_reg_last_error(void) { return g_err; }

// levels, offsets: a function of nt alone
static void rg_tree(int64_t nt, RgTree* T) {
    T->nt = (int)nt;
    int64_t cnt = (nt + RG_F - 1) / RG_F, off = 0;
    int l = 0;
    for (int k = 0; k <= RG_MAX_LEVELS; ++k) T->off[k] = 0;
    for (;; ++l) {
        T->off[l] = (int)off;
        off += cnt;
        if (cnt == 1) break;
        cnt = (cnt + RG_F - 1) / RG_F;
    }
    T->levels = l + 1;
    for (int k = l + 1; k <= RG_MAX_LEVELS; ++k) T->off[k] = (int)off;        // off[levels] = the number of nodes, repeated behind it
}
static int rg_check_counts(const char* who, int64_t nt, int64_t Q) {
    REQUIRE(nt >= 1 && nt < (int64_t)1 << 27, "%s: nt must be in [1, 2^27) (got %lld)", who, (long long)nt);
    REQUIRE(Q >= 1 && Q < (int64_t)1 << 30, "%s: Q must be in [1, 2^30) (got %lld)", who, (long long)Q);
    return 0;
}
// the workspace of a pass: one partial row per workgroup of 256 queries
static int64_t rg_work_bytes(int64_t Q) {
    PlanBump b{nullptr, 0};
    b.take((int64_t)blocks(Q) * RG_RECORD * (int64_t)sizeof(double));
    return b.used;
}

extern "C" int sta_reg_plan(int64_t nt, int64_t Q, int64_t* sizes_out) {
    const char* who = "reg_plan";
    REQUIRE(sizes_out, "%s: null argument", who);
    if (rg_check_counts(who, nt, Q)) return -1;
    RgTree T;
    rg_tree(nt, &T);
    sizes_out[0] = T.off[T.levels];
    sizes_out[1] = rg_work_bytes(Q);
    return 0;
}

extern "C" int sta_reg_pass(const float* tri, const int32_t* src, const float* boxes, const int32_t* counters, int64_t nt, const float* qry,
                            const float* qnrm, int64_t Q, const double* T_host, const double* pivot_host, double radius, double min_cos,
                            double* d2_out, int32_t* tri_out, float* point_out, double* resid_out, double* record_out, void* work,
                            int64_t work_bytes, int32_t* status, void* stream) {
    const char* who = "reg_pass";
    if (rg_check_counts(who, nt, Q)) return -1;
    REQUIRE(radius >= 0.0, "%s: radius must be >= 0, +inf allowed (got %g)", who, radius);          // false for NaN
    REQUIRE(min_cos == min_cos, "%s: min_cos must not be NaN (got %g)", who, min_cos);
    if (record_out) {
        const int64_t need = rg_work_bytes(Q);
        REQUIRE(work && work_bytes >= need, "%s: work of %lld bytes is required for Q = %lld (got %s%lld)", who, (long long)need, (long long)Q,
                work ? "" : "a null pointer and ", (long long)work_bytes);
    }
    REQUIRE(tri && src && boxes && counters && qry && status, "%s: null argument", who);
    RgPass P;
    P.tri = tri; P.src = (const int*)src; P.boxes = boxes; P.counters = (const int*)counters;
    P.qry = qry; P.qnrm = qnrm; P.Q = (int)Q; P.r2 = radius * radius; P.min_cos = min_cos;
    static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int k = 0; k < 12; ++k) P.T[k] = T_host ? T_host[k] : eye[k];
    for (int k = 0; k < 3; ++k) P.pivot[k] = pivot_host ? pivot_host[k] : 0.0;
    P.d2_out = d2_out; P.tri_out = (int*)tri_out; P.point_out = point_out; P.resid_out = resid_out;
    P.part = record_out ? (double*)work : nullptr; P.status = (int*)status;
    rg_tree(nt, &P.tree);
    const unsigned nb = blocks(Q);
    hipLaunchKernelGGL(rg_pass_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, P);
    HIPCHK(hipGetLastError());
    if (record_out) {
        hipLaunchKernelGGL(rg_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)work, (int)nb, record_out);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
