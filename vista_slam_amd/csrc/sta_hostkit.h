// Host side of the handle-free libraries (sta_cloud.hip, sta_raster.hip, sta_tsdf.hip, sta_mesh.hip, sta_surf.hip, sta_simp.hip,
// sta_dist.hip): the error buffer behind each sta_*_last_error(), the argument and HIP checks, the bump that lays out a caller's
// workspace.  Everything here has internal linkage, so every library has an error buffer of its own and exports nothing of this.
// Needs <hip/hip_runtime.h> alone (sta_common.h): the product library (sta_api.hip) has its own REQUIRE / HIPCHK / Bump and does not
// include this.  The sort and scan layouts and their launch code are next to their kernels, at the end of voxel.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>

static thread_local char g_err[1024] = "";
static int set_err(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return -1;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define REQUIRE(c, ...) do { if (!(c)) return set_err(__VA_ARGS__); } while (0)

// One bump layout per buffer serves the plan and the call: what the plan reports is what the call takes.  A null base plans
// (every take returns null); every take is rounded up to 256 bytes.
struct PlanBump {
    char* base; int64_t used;
    void* take(int64_t bytes) { void* p = base ? base + used : nullptr; used += (bytes + 255) & ~(int64_t)255; return p; }
};

static inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }      // workgroups of 256 threads over n items
