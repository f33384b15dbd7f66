// libsta_simp.so: the C ABI of include/sta_simp.h.  A translation unit of its own - no handle, no allocation, no copy to the host, no
// synchronisation: none of the other six libraries includes or links any of this.  Static helpers carry the prefix sp_.
// The error buffer, REQUIRE, HIPCHK, the bump and blocks() are sta_hostkit.h's: one copy per library, none exported.
#include "../../include/sta_simp.h"
#include "sta_common.h"
#include "sta_hostkit.h"
#include "elementwise.h"      // cloud_scan_kernel (voxel.h)
#include "select.h"           // sel_block_scan (voxel.h)
#include "voxel.h"            // the stable LSD radix sort, vox_block_count / vox_block_rank
#include "simp.h"

#include <cmath>

static_assert(SP_SWEEPS == STA_SIMP_SWEEPS && SP_BIAS == (1ll << (STA_SIMP_INDEX_BITS - 1)), "simp.h repeats the header's constants");
static_assert(STA_SIMP_N_CELLS == 0 && STA_SIMP_N_VERTS == 1 && STA_SIMP_N_TRIS == 2 && STA_SIMP_N_DROPPED == 3 && STA_SIMP_N_INVALID == 4 &&
              STA_SIMP_N_COLLAPSED == 5 && STA_SIMP_N_DUPLICATE == 6 && STA_SIMP_N_FALLBACK == 7 && STA_SIMP_COUNTERS == 8, "simp.h uses the counter layout by number");

extern "C" const char* sta_simp_last_error(void) { return g_err; }

// One bump layout per workspace serves the plan and the call: what the plan reports is what the call takes.
static int64_t sp_nblk(int64_t n) { return (n + 255) / 256; }
struct SpCellsLayout { VoxSort sort; VoxScan scan; };
struct SpTrisLayout { VoxSort sort; VoxScan tscan, cscan; int* flag; int* used; };
struct SpPlaceLayout { VoxSort vsort, psort; };
static int64_t sp_cells_layout(void* buf, int64_t nv, SpCellsLayout* L) {
    PlanBump b{(char*)buf, 0};
    vox_take_sort(b, nv, &L->sort); vox_take_scan(b, sp_nblk(nv), &L->scan);
    return b.used;
}
static int64_t sp_tris_layout(void* buf, int64_t nt, int64_t nv, SpTrisLayout* L) {
    PlanBump b{(char*)buf, 0};
    vox_take_sort(b, nt, &L->sort); vox_take_scan(b, sp_nblk(nt), &L->tscan); vox_take_scan(b, sp_nblk(nv), &L->cscan);
    L->flag = (int*)b.take(nt * 4);
    L->used = (int*)b.take(nv * 4);
    return b.used;
}
static int64_t sp_place_layout(void* buf, int64_t nt, int64_t nv, SpPlaceLayout* L) {
    PlanBump b{(char*)buf, 0};
    vox_take_sort(b, nv, &L->vsort); vox_take_sort(b, 3 * nt, &L->psort);
    return b.used;
}

static int sp_check_counts(const char* who, int64_t nt, int64_t nv) {
    REQUIRE(nv >= 0 && nv < (int64_t)1 << 31, "%s: nv must be in [0, 2^31) (got %lld)", who, (long long)nv);
    REQUIRE(nt >= 0 && nt < ((int64_t)1 << 31) && 3 * nt < (int64_t)1 << 31, "%s: nt must be >= 0 and 3 * nt below 2^31 (got nt = %lld)", who, (long long)nt);
    return 0;
}
static int sp_check_grid(const char* who, double cell, double ox, double oy, double oz) {
    REQUIRE(std::isfinite(cell) && cell > 0.0, "%s: cell must be finite and > 0 (got %g)", who, cell);
    REQUIRE(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz), "%s: the origin must be finite (got %g, %g, %g)", who, ox, oy, oz);
    return 0;
}
static int sp_bits(int64_t n) { int b = 1; while (b < 63 && (n >> b) != 0) ++b; return b; }      // the bits that hold the value n

// The stable LSD sort of voxel.h over the low `bits` bits of key[cur] / idx[cur]; returns the buffer (0 or 1) that holds the result.
static int sp_sort(hipStream_t st, const VoxSort& L, int64_t m, int bits, int cur = 0) { return vox_sort(st, L, (int)m, (bits + 7) / 8, cur); }
static void sp_scan(hipStream_t st, const VoxScan& S, int64_t n) { vox_scan(st, S.counts, S.offs, (int)sp_nblk(n)); }

extern "C" int sta_simp_plan(int64_t nt, int64_t nv, int64_t* sizes_out) {
    const char* who = "simp_plan";
    REQUIRE(sizes_out, "%s: null argument", who);
    if (sp_check_counts(who, nt, nv)) return -1;
    SpCellsLayout cl; SpTrisLayout tl; SpPlaceLayout pl;
    sizes_out[0] = sp_cells_layout(nullptr, nv, &cl);
    sizes_out[1] = sp_tris_layout(nullptr, nt, nv, &tl);
    sizes_out[2] = sp_place_layout(nullptr, nt, nv, &pl);
    return 0;
}

extern "C" int sta_simp_cells(const float* verts, int64_t nv, double cell, double ox, double oy, double oz, int32_t* vcell, int64_t* counters,
                              void* work, int64_t work_bytes, void* stream) {
    const char* who = "simp_cells";
    if (sp_check_counts(who, 0, nv) || sp_check_grid(who, cell, ox, oy, oz)) return -1;
    SpCellsLayout L;
    const int64_t need = sp_cells_layout(work, nv, &L);
    REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld vertices", who, (long long)work_bytes, (long long)need, (long long)nv);
    REQUIRE(counters && (nv == 0 || (verts && vcell && work)), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sp_zero_kernel, dim3(1), dim3(64), 0, st, (long long*)counters, (1u << STA_SIMP_N_CELLS) | (1u << STA_SIMP_N_DROPPED));
    if (nv > 0) {
        SpGrid g; g.o[0] = ox; g.o[1] = oy; g.o[2] = oz; g.cell = cell;
        const int n = (int)nv;
        hipLaunchKernelGGL(sp_key_kernel, dim3(blocks(nv)), dim3(256), 0, st, verts, n, g, L.sort.key[0], L.sort.idx[0]);
        const int r = sp_sort(st, L.sort, nv, 64);         // all 64 bits: the dropped key, all ones, sorts behind the largest cell key, 2^63 - 1
        hipLaunchKernelGGL(sp_head_count_kernel, dim3(blocks(nv)), dim3(256), 0, st, (const unsigned long long*)L.sort.key[r], n, L.scan.counts);
        sp_scan(st, L.scan, nv);
        hipLaunchKernelGGL(sp_rank_kernel, dim3(blocks(nv)), dim3(256), 0, st, (const unsigned long long*)L.sort.key[r], (const int*)L.sort.idx[r], n,
                           (const int64_t*)L.scan.offs, (int)sp_nblk(nv), (int*)vcell, (long long*)counters);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_simp_triangles(const int32_t* tris, int64_t nt, int64_t nv, const int32_t* vcell, int32_t* tris_out, int32_t* tri_src,
                                  int32_t* cell_out, int32_t* vmap, int64_t* counters, void* work, int64_t work_bytes, void* stream) {
    const char* who = "simp_triangles";
    if (sp_check_counts(who, nt, nv)) return -1;
    SpTrisLayout L;
    const int64_t need = sp_tris_layout(work, nt, nv, &L);
    REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld triangles and %lld vertices", who, (long long)work_bytes, (long long)need,
            (long long)nt, (long long)nv);
    REQUIRE(counters && (nt == 0 || (tris && tris_out && tri_src)) && (nv == 0 || (vcell && cell_out && vmap)) && (nt + nv == 0 || work), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)nt, v = (int)nv;
    hipLaunchKernelGGL(sp_zero_kernel, dim3(1), dim3(64), 0, st, (long long*)counters,
                       (1u << STA_SIMP_N_VERTS) | (1u << STA_SIMP_N_TRIS) | (1u << STA_SIMP_N_INVALID) | (1u << STA_SIMP_N_COLLAPSED) | (1u << STA_SIMP_N_DUPLICATE));
    if (nv > 0) HIPCHK(hipMemsetAsync(L.used, 0, (size_t)nv * 4, st));
    if (nt > 0) {
        const int bits = sp_bits(nv);
        hipLaunchKernelGGL(sp_tri_key_kernel, dim3(blocks(nt)), dim3(256), 0, st, (const int*)tris, (const int*)vcell, n, (long long)nv, L.sort.key[0], L.sort.idx[0]);
        int r = sp_sort(st, L.sort, nt, bits);
        hipLaunchKernelGGL(sp_tri_rekey_kernel, dim3(blocks(nt)), dim3(256), 0, st, (const int*)tris, (const int*)vcell, n, (long long)nv, bits, L.sort.key[r],
                           (const int*)L.sort.idx[r]);
        r = sp_sort(st, L.sort, nt, 2 * bits, r);
        hipLaunchKernelGGL(sp_mark_kernel, dim3(blocks(nt)), dim3(256), 0, st, (const int*)tris, (const int*)vcell, n, (long long)nv, (const int*)L.sort.idx[r],
                           L.flag, (long long*)counters);
        hipLaunchKernelGGL(sp_flag_count_kernel, dim3(blocks(nt)), dim3(256), 0, st, (const int*)L.flag, n, L.tscan.counts);
        sp_scan(st, L.tscan, nt);
        hipLaunchKernelGGL(sp_tri_emit_kernel, dim3(blocks(nt)), dim3(256), 0, st, (const int*)tris, (const int*)vcell, n, (long long)nv, (const int*)L.flag,
                           (const int64_t*)L.tscan.offs, (int*)tris_out, (int*)tri_src, L.used);
    }
    if (nv > 0) {
        hipLaunchKernelGGL(sp_flag_count_kernel, dim3(blocks(nv)), dim3(256), 0, st, (const int*)L.used, v, L.cscan.counts);
        sp_scan(st, L.cscan, nv);
        hipLaunchKernelGGL(sp_cell_emit_kernel, dim3(blocks(nv)), dim3(256), 0, st, (const int*)L.used, v, (const int64_t*)L.cscan.offs, (int*)cell_out);
    }
    const int64_t rows = nt > nv ? nt : nv;
    hipLaunchKernelGGL(sp_remap_kernel, dim3(rows ? blocks(rows) : 1u), dim3(256), 0, st, n, v, (const int*)vcell, (const int*)cell_out,
                       nt > 0 ? (const int64_t*)(L.tscan.offs + sp_nblk(nt)) : (const int64_t*)nullptr,
                       nv > 0 ? (const int64_t*)(L.cscan.offs + sp_nblk(nv)) : (const int64_t*)nullptr, (int*)tris_out, (int*)tri_src, (int*)vmap,
                       (long long*)counters);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_simp_place(const float* verts, const float* colors, int64_t nv, const int32_t* tris, int64_t nt, const int32_t* vcell,
                              const int32_t* cell_out, double cell, double ox, double oy, double oz, int placement, double sv_ratio,
                              float* verts_out, float* colors_out, int64_t* counters, void* work, int64_t work_bytes, void* stream) {
    const char* who = "simp_place";
    if (sp_check_counts(who, nt, nv) || sp_check_grid(who, cell, ox, oy, oz)) return -1;
    REQUIRE(placement == STA_SIMP_PLACE_MEAN || placement == STA_SIMP_PLACE_QUADRIC, "%s: placement must be 0 or 1 (got %d)", who, placement);
    REQUIRE(sv_ratio >= 0.0 && sv_ratio < 1.0, "%s: sv_ratio must be in [0, 1) (got %g)", who, sv_ratio);
    REQUIRE((colors != nullptr) == (colors_out != nullptr), "%s: colors (%s) and colors_out (%s) go together", who, colors ? "given" : "NULL",
            colors_out ? "given" : "NULL");
    SpPlaceLayout L;
    const int64_t need = sp_place_layout(work, nt, nv, &L);
    REQUIRE(work_bytes >= need, "%s: work of %lld bytes, %lld needed for %lld triangles and %lld vertices", who, (long long)work_bytes, (long long)need,
            (long long)nt, (long long)nv);
    const bool quadric = placement == STA_SIMP_PLACE_QUADRIC && nt > 0;
    REQUIRE(counters && (nv == 0 || (verts && vcell && cell_out && verts_out && work)) && (!quadric || nv == 0 || tris), "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sp_zero_kernel, dim3(1), dim3(64), 0, st, (long long*)counters, 1u << STA_SIMP_N_FALLBACK);
    if (nv > 0) {
        const int bits = sp_bits(nv), n = (int)nv, m = quadric ? (int)(3 * nt) : 0;
        hipLaunchKernelGGL(sp_vkey_kernel, dim3(blocks(nv)), dim3(256), 0, st, (const int*)vcell, n, L.vsort.key[0], L.vsort.idx[0]);
        const int rv = sp_sort(st, L.vsort, nv, bits);
        int rp = 0;
        if (m > 0) {
            hipLaunchKernelGGL(sp_pkey_kernel, dim3(blocks(m)), dim3(256), 0, st, (const int*)tris, (const int*)vcell, m, (long long)nv, L.psort.key[0], L.psort.idx[0]);
            rp = sp_sort(st, L.psort, m, bits);
        }
        SpPlace P;
        P.verts = verts; P.colors = colors; P.tris = (const int*)tris; P.vcell = (const int*)vcell; P.cell_out = (const int*)cell_out;
        P.vkey = L.vsort.key[rv]; P.vidx = L.vsort.idx[rv]; P.pkey = L.psort.key[rp]; P.pidx = L.psort.idx[rp];
        P.nv = nv; P.m = m;
        P.g.o[0] = ox; P.g.o[1] = oy; P.g.o[2] = oz; P.g.cell = cell;
        P.placement = placement; P.sv_ratio = sv_ratio;
        P.verts_out = verts_out; P.colors_out = colors_out; P.counters = (long long*)counters;
        hipLaunchKernelGGL(sp_place_kernel, dim3(blocks(nv)), dim3(256), 0, st, P);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
