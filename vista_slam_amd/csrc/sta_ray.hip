// libsta_ray.so: the C ABI of include/sta_ray.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation, no workspace: none of the other eight libraries includes or links any of this, and it includes none of theirs (the
// index of libsta_dist.so comes in as plain arguments).  Static helpers carry the prefix ry_.
// The error buffer, REQUIRE, HIPCHK and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_ray.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "ray.h"

static_assert(RY_F == STA_RAY_FANOUT && RY_MAX_LEVELS == STA_RAY_MAX_LEVELS && RY_VALID == STA_RAY_N_VALID && RY_STATUS_BOUND == STA_RAY_STATUS_BOUND,
              "ray.h repeats the header's constants");

extern "C" const char* sta_ray_last_error(void) { return g_err; }

// levels, offsets: a function of nt alone
static void ry_tree(int64_t nt, RyTree* T) {
    T->nt = (int)nt;
    int64_t cnt = (nt + RY_F - 1) / RY_F, off = 0;
    int l = 0;
    for (int k = 0; k <= RY_MAX_LEVELS; ++k) T->off[k] = 0;
    for (;; ++l) {
        T->off[l] = (int)off;
        off += cnt;
        if (cnt == 1) break;
        cnt = (cnt + RY_F - 1) / RY_F;
    }
    T->levels = l + 1;
    for (int k = l + 1; k <= RY_MAX_LEVELS; ++k) T->off[k] = (int)off;        // off[levels] = the number of nodes, repeated behind it
}
static int ry_check_counts(const char* who, int64_t nt, int64_t R) {
    REQUIRE(nt >= 1 && nt < (int64_t)1 << 27, "%s: nt must be in [1, 2^27) (got %lld)", who, (long long)nt);
    REQUIRE(R >= 1 && R < (int64_t)1 << 30, "%s: R must be in [1, 2^30) (got %lld)", who, (long long)R);
    return 0;
}

extern "C" int sta_ray_plan(int64_t nt, int64_t R, int64_t* sizes_out) {
    const char* who = "ray_plan";
    REQUIRE(sizes_out, "%s: null argument", who);
    if (ry_check_counts(who, nt, R)) return -1;
    RyTree T;
    ry_tree(nt, &T);
    sizes_out[0] = T.off[T.levels];
    return 0;
}

// the checks and the launch of both entry points; occ_out selects the kernel
static int ry_launch(const char* who, const float* tri, const int32_t* src, const float* boxes, const int32_t* counters, int64_t nt, const float* org,
                     const float* dir, int64_t R, double t_min, double t_max, double* t_out, int32_t* tri_out, float* bary_out, uint8_t* occ_out,
                     int32_t* status, void* stream) {
    if (ry_check_counts(who, nt, R)) return -1;
    REQUIRE(t_min >= 0.0 && t_min <= t_max, "%s: 0 <= t_min <= t_max is required, t_max = +inf allowed (got %g, %g)", who, t_min, t_max);      // false for NaN
    REQUIRE(tri && src && boxes && counters && org && dir && status, "%s: null argument", who);
    RyCast P;
    P.tri = tri; P.src = (const int*)src; P.boxes = boxes; P.counters = (const int*)counters;
    P.org = org; P.dir = dir; P.R = (int)R; P.t_min = t_min; P.t_max = t_max;
    P.t_out = t_out; P.tri_out = (int*)tri_out; P.bary_out = bary_out; P.occ_out = occ_out; P.status = (int*)status;
    ry_tree(nt, &P.tree);
    if (occ_out) hipLaunchKernelGGL(ry_cast_kernel<true>, dim3(blocks(R)), dim3(256), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(ry_cast_kernel<false>, dim3(blocks(R)), dim3(256), 0, (hipStream_t)stream, P);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_ray_cast(const float* tri, const int32_t* src, const float* boxes, const int32_t* counters, int64_t nt, const float* org,
                            const float* dir, int64_t R, double t_min, double t_max, double* t_out, int32_t* tri_out, float* bary_out,
                            int32_t* status, void* stream) {
    return ry_launch("ray_cast", tri, src, boxes, counters, nt, org, dir, R, t_min, t_max, t_out, tri_out, bary_out, nullptr, status, stream);
}

extern "C" int sta_ray_occluded(const float* tri, const int32_t* src, const float* boxes, const int32_t* counters, int64_t nt, const float* org,
                                const float* dir, int64_t R, double t_min, double t_max, uint8_t* occ_out, int32_t* status, void* stream) {
    const char* who = "ray_occluded";
    REQUIRE(occ_out, "%s: null argument", who);
    return ry_launch(who, tri, src, boxes, counters, nt, org, dir, R, t_min, t_max, nullptr, nullptr, nullptr, occ_out, status, stream);
}
