// libsta_surf.so: the C ABI of include/sta_surf.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other five libraries includes or links any of this.  Static helpers carry the prefix sf_.
#include "../../include/sta_surf.h"
#include "sta_common.h"
#include "surf.h"

#include <cstdarg>
#include <cstdio>

static_assert(SF_CHUNK == STA_SURF_CHUNK && SF_STATUS_BOUND == STA_SURF_STATUS_BOUND, "surf.h repeats the header's constants");

static thread_local char sf_err[1024] = "";
static int sf_set_err(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(sf_err, sizeof(sf_err), fmt, ap); va_end(ap);
    return -1;
}
#define SF_HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return sf_set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define SF_REQUIRE(c, ...) do { if (!(c)) return sf_set_err(__VA_ARGS__); } while (0)

extern "C" const char* sta_surf_last_error(void) { return sf_err; }

static int64_t sf_r256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
static int64_t sf_chunks(int64_t nt) { return (nt + STA_SURF_CHUNK - 1) / STA_SURF_CHUNK; }
// One layout per workspace serves the plan and the call: what the plan reports is what the call takes.
static int64_t sf_components_bytes(int64_t nv) { return sf_r256(4 * nv); }
static int64_t sf_weights_bytes(int64_t nt) { return 2 * sf_r256(8 * sf_chunks(nt)); }      // S, then O

static int sf_check_count(const char* who, const char* name, int64_t n) {
    SF_REQUIRE(n >= 0 && n < (int64_t)1 << 31, "%s: %s must be in [0, 2^31) (got %lld)", who, name, (long long)n);
    return 0;
}
static unsigned sf_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int sta_surf_plan(int64_t nt, int64_t nv, int64_t ns, int64_t* sizes_out) {
    const char* who = "surf_plan";
    SF_REQUIRE(sizes_out, "%s: null argument", who);
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv) || sf_check_count(who, "ns", ns)) return -1;
    sizes_out[0] = sf_components_bytes(nv);
    sizes_out[1] = sf_weights_bytes(nt);
    sizes_out[2] = 0;
    return 0;
}

extern "C" int sta_surf_components(const int32_t* tris, int64_t nt, int64_t nv, int32_t* vlabel, int32_t* tlabel, int32_t* tcount, int32_t* status,
                                   void* work, int64_t work_bytes, void* stream) {
    const char* who = "surf_components";
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv)) return -1;
    const int64_t need = sf_components_bytes(nv);
    SF_REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld vertices", who, (long long)work_bytes, (long long)need, (long long)nv);
    if (nt == 0 && nv == 0) return 0;
    SF_REQUIRE(status && (nt == 0 || (tris && tlabel)) && (nv == 0 || (vlabel && tcount && work)), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    int* parent = (int*)work;
    hipLaunchKernelGGL(sf_init_kernel, dim3(nv ? sf_blocks(nv) : 1u), dim3(256), 0, st, parent, (int*)tcount, (int*)status, (long long)nv);
    if (nt > 0 && nv > 0) hipLaunchKernelGGL(sf_hook_kernel, dim3(sf_blocks(nt)), dim3(256), 0, st, (const int*)tris, (long long)nt, (long long)nv, parent, (int*)status);
    if (nv > 0) hipLaunchKernelGGL(sf_flatten_kernel, dim3(sf_blocks(nv)), dim3(256), 0, st, parent, (long long)nv, (int*)vlabel, (int*)status);
    if (nt > 0) hipLaunchKernelGGL(sf_count_kernel, dim3(sf_blocks(nt)), dim3(256), 0, st, (const int*)tris, (long long)nt, (long long)nv, (const int*)vlabel, (int*)tlabel, (int*)tcount);
    if (nv > 0) hipLaunchKernelGGL(sf_unnamed_kernel, dim3(sf_blocks(nv)), dim3(256), 0, st, (int*)vlabel, (const int*)tcount, (long long)nv);
    SF_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_surf_weights(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, const uint8_t* tri_keep, double* P, double* total,
                                void* work, int64_t work_bytes, void* stream) {
    const char* who = "surf_weights";
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv)) return -1;
    const int64_t need = sf_weights_bytes(nt), nchunks = sf_chunks(nt);
    SF_REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld triangles", who, (long long)work_bytes, (long long)need, (long long)nt);
    SF_REQUIRE(total && (nt == 0 || (tris && P && work)) && (nt == 0 || nv == 0 || verts), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    double* S = (double*)work;
    double* O = (double*)((char*)work + sf_r256(8 * nchunks));
    if (nt > 0) hipLaunchKernelGGL(sf_chunk_kernel, dim3((unsigned)nchunks), dim3(64), 0, st, verts, (long long)nv, (const int*)tris, (long long)nt,
                                   (const unsigned char*)tri_keep, P, S);
    hipLaunchKernelGGL(sf_offsets_kernel, dim3(1), dim3(64), 0, st, (const double*)S, (long long)nchunks, O, total);
    if (nt > 0) hipLaunchKernelGGL(sf_prefix_kernel, dim3(sf_blocks(nt)), dim3(256), 0, st, P, (long long)nt, (const double*)O);
    SF_HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_surf_sample(const float* verts, int64_t nv, const int32_t* tris, int64_t nt, const double* P, const double* total, const float* colors,
                               int64_t ns, uint64_t seed, float* points, int32_t* tri, float* colors_out, float* normals_out, void* stream) {
    const char* who = "surf_sample";
    if (sf_check_count(who, "nt", nt) || sf_check_count(who, "nv", nv) || sf_check_count(who, "ns", ns)) return -1;
    SF_REQUIRE(!colors_out || colors, "%s: colors_out without colors", who);
    if (ns == 0) return 0;
    SF_REQUIRE(total && points && tri && (nt == 0 || (tris && P)) && (nt == 0 || nv == 0 || verts), "%s: null argument", who);
    SfSample a;
    a.verts = verts; a.tris = (const int*)tris; a.P = P; a.total = total; a.colors = colors;
    a.nv = nv; a.nt = nt; a.ns = ns; a.seed = seed;
    a.points = points; a.tri = (int*)tri; a.colors_out = colors_out; a.normals_out = normals_out;
    hipLaunchKernelGGL(sf_sample_kernel, dim3(sf_blocks(ns)), dim3(256), 0, (hipStream_t)stream, a);
    SF_HIPCHK(hipGetLastError());
    return 0;
}
