// libsta_surf.so: the C ABI of include/sta_surf.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other five libraries includes or links any of this.  Static helpers carry the prefix sf_.
// The error buffer, REQUIRE, HIPCHK, the bump and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_surf.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "surf.h"

static_assert(SF_CHUNK == STA_SURF_CHUNK && SF_STATUS_BOUND == STA_SURF_STATUS_BOUND, "surf.h repeats the header's constants");

extern "C" const char* sta_surf_last_error(void) { return g_err; }

static int64_t sf_chunks(int64_t nt) { return (nt + STA_SURF_CHUNK - 1) / STA_SURF_CHUNK; }
// One bump layout per workspace serves the plan and the call: what the plan reports is what the call takes.
static int64_t sf_components_layout(void* buf, int64_t nv, int** parent) {
    PlanBump b{(char*)buf, 0};
    *parent = (int*)b.take(4 * nv);
    return b.used;
}
static int64_t sf_weights_layout(void* buf, int64_t nt, double** S, double** O) {
    PlanBump b{(char*)buf, 0};
    *S = (double*)b.take(8 * sf_chunks(nt));
    *O = (double*)b.take(8 * sf_chunks(nt));
    return b.used;
}

static int sf_check_count(const char* who, const char* name, int64_t n) {
    REQUIRE(n >= 0 && n < (int64_t)1 << 31, "%s: %s must be in [0, 2^31) (got %lld)", who, name, (long long)n);
    return 0;
}

extern "C" int sta_surf_plan(int64_t nt, int64_t nv, int64_t ns, int64_t* sizes_out) {
    const char* who = "surf_plan";
    REQUIRE(sizes_out, "%s: null argument", who);
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv) || sf_check_count(who, "ns", ns)) return -1;
    int* parent; double* S; double* O;
    sizes_out[0] = sf_components_layout(nullptr, nv, &parent);
    sizes_out[1] = sf_weights_layout(nullptr, nt, &S, &O);
    sizes_out[2] = 0;
    return 0;
}

extern "C" int sta_surf_components(const int32_t* tris, int64_t nt, int64_t nv, int32_t* vlabel, int32_t* tlabel, int32_t* tcount, int32_t* status,
                                   void* work, int64_t work_bytes, void* stream) {
    const char* who = "surf_components";
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv)) return -1;
    int* parent;
    const int64_t need = sf_components_layout(work, nv, &parent);
    REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld vertices", who, (long long)work_bytes, (long long)need, (long long)nv);
    if (nt == 0 && nv == 0) return 0;
    REQUIRE(status && (nt == 0 || (tris && tlabel)) && (nv == 0 || (vlabel && tcount && work)), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sf_init_kernel, dim3(nv ? blocks(nv) : 1u), dim3(256), 0, st, parent, (int*)tcount, (int*)status, (long long)nv);
    if (nt > 0 && nv > 0) hipLaunchKernelGGL(sf_hook_kernel, dim3(blocks(nt)), dim3(256), 0, st, (const int*)tris, (long long)nt, (long long)nv, parent, (int*)status);
    if (nv > 0) hipLaunchKernelGGL(sf_flatten_kernel, dim3(blocks(nv)), dim3(256), 0, st, parent, (long long)nv, (int*)vlabel, (int*)status);
    if (nt > 0) hipLaunchKernelGGL(sf_count_kernel, dim3(blocks(nt)), dim3(256), 0, st, (const int*)tris, (long long)nt, (long long)nv, (const int*)vlabel, (int*)tlabel, (int*)tcount);
    if (nv > 0) hipLaunchKernelGGL(sf_unnamed_kernel, dim3(blocks(nv)), dim3(256), 0, st, (int*)vlabel, (const int*)tcount, (long long)nv);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_surf_weights(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, const uint8_t* tri_keep, double* P, double* total,
                                void* work, int64_t work_bytes, void* stream) {
    const char* who = "surf_weights";
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv)) return -1;
    double* S; double* O;
    const int64_t need = sf_weights_layout(work, nt, &S, &O), nchunks = sf_chunks(nt);
    REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld triangles", who, (long long)work_bytes, (long long)need, (long long)nt);
    REQUIRE(total && (nt == 0 || (tris && P && work)) && (nt == 0 || nv == 0 || verts), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    if (nt > 0) hipLaunchKernelGGL(sf_chunk_kernel, dim3((unsigned)nchunks), dim3(64), 0, st, verts, (long long)nv, (const int*)tris, (long long)nt,
                                   (const unsigned char*)tri_keep, P, S);
    hipLaunchKernelGGL(sf_offsets_kernel, dim3(1), dim3(64), 0, st, (const double*)S, (long long)nchunks, O, total);
    if (nt > 0) hipLaunchKernelGGL(sf_prefix_kernel, dim3(blocks(nt)), dim3(256), 0, st, P, (long long)nt, (const double*)O);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_surf_sample(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, const double* P, const double* total, const float* colors,
                               int64_t ns, uint64_t seed, float* points, int32_t* tri, float* colors_out, float* normals_out, void* stream) {
    const char* who = "surf_sample";
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv) || sf_check_count(who, "ns", ns)) return -1;
    REQUIRE(!colors_out || colors, "%s: colors_out without colors", who);
    if (ns == 0) return 0;
    REQUIRE(total && points && tri && (nt == 0 || (tris && P)) && (nt == 0 || nv == 0 || verts), "%s: null argument", who);
    SfSample a;
    a.verts = verts; a.tris = (const int*)tris; a.P = P; a.total = total; a.colors = colors;
    a.nv = nv; a.nt = nt; a.ns = ns; a.seed = seed;
    a.points = points; a.tri = (int*)tri; a.colors_out = colors_out; a.normals_out = normals_out;
    hipLaunchKernelGGL(sf_sample_kernel, dim3(blocks(ns)), dim3(256), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}
