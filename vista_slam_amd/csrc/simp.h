// Mesh simplification by vertex clustering (libsta_simp.so; the contract is in include/sta_simp.h), included by sta_simp.hip after
// elementwise.h (cloud_scan_kernel), select.h (sel_block_scan) and voxel.h (the radix sort, vox_index, vox_finite3, vox_block_count /
// vox_block_rank).  Sort based: no table to size, no floating-point atomics, every output defined by the input alone.
//   sp_zero_kernel                                   the counters a stage owns
//   sp_key_kernel / sp_head_count_kernel / sp_rank_kernel   cell keys with the dropped-vertex rule; heads of the sorted runs; vcell
//   sp_tri_key_kernel / sp_tri_rekey_kernel          the sorted cluster triple: key s2 first, then (s0, s1) behind the first sort
//   sp_mark_kernel                                   survivors behind the second sort (a duplicate equals its sorted predecessor)
//   sp_flag_count_kernel / sp_tri_emit_kernel        ordered compaction of the survivors, rotated; used cells marked by integer stores
//   sp_cell_emit_kernel / sp_remap_kernel            ordered compaction of the used cells; output indices, vmap, the counts
//   sp_vkey_kernel / sp_pkey_kernel / sp_place_kernel   (cell, vertex) and (cell, corner) pairs; one lane per cell: mean, quadric, Jacobi
#pragma once

#pragma clang fp contract(off)

#define SP_SWEEPS 8
#define SP_BIAS (1ll << 20)
#define SP_DROPPED (~0ull)

// ---------------------------------------------------------------------------------------------------------
__global__ void sp_zero_kernel(long long* __restrict__ counters, unsigned mask) {
    const int i = threadIdx.x;
    if (i < 8 && ((mask >> i) & 1u)) counters[i] = 0;
}
// adds the number of lanes with `flag` to *c: one integer atomic per wavefront (every lane of the wavefront calls this)
__device__ __forceinline__ void sp_count(long long* c, bool flag) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)c, (unsigned long long)__popcll(b));
}

// ---------------------------------------------------------------------------------------------------------
// Stage 1
struct SpGrid { double o[3]; double cell; };

__device__ __forceinline__ bool sp_cell_index(const float* __restrict__ verts, long long v, const SpGrid& g, long long* i3) {
    const float x = verts[3 * (size_t)v], y = verts[3 * (size_t)v + 1], z = verts[3 * (size_t)v + 2];
    if (!vox_finite3(x, y, z)) return false;
    const double fx = floor(((double)x - g.o[0]) / g.cell), fy = floor(((double)y - g.o[1]) / g.cell), fz = floor(((double)z - g.o[2]) / g.cell);
    const double lo = -(double)SP_BIAS, hi = (double)SP_BIAS;
    if (!(fx >= lo && fx < hi && fy >= lo && fy < hi && fz >= lo && fz < hi)) return false;       // (false for NaN)
    i3[0] = (long long)fx; i3[1] = (long long)fy; i3[2] = (long long)fz;
    return true;
}
__global__ __launch_bounds__(256) void sp_key_kernel(const float* __restrict__ verts, int nv, const SpGrid g, unsigned long long* __restrict__ key,
                                                     int* __restrict__ idx) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    long long i3[3];
    unsigned long long k = SP_DROPPED;
    if (sp_cell_index(verts, v, g, i3))
        k = ((unsigned long long)(i3[2] + SP_BIAS) << 42) | ((unsigned long long)(i3[1] + SP_BIAS) << 21) | (unsigned long long)(i3[0] + SP_BIAS);
    key[v] = k; idx[v] = v;
}
__device__ __forceinline__ bool sp_is_head(const unsigned long long* __restrict__ key, int i, int n) {
    return i < n && key[i] != SP_DROPPED && (i == 0 || key[i] != key[i - 1]);
}
__global__ __launch_bounds__(256) void sp_head_count_kernel(const unsigned long long* __restrict__ key, int n, int* __restrict__ counts) {
    vox_block_count(sp_is_head(key, blockIdx.x * 256 + threadIdx.x, n), counts);
}
// sorted position i: the rank of its cell is the number of heads at or before i, minus one
__global__ __launch_bounds__(256) void sp_rank_kernel(const unsigned long long* __restrict__ key, const int* __restrict__ idx, int n,
                                                      const int64_t* __restrict__ offs, int nblk, int* __restrict__ vcell, long long* __restrict__ counters) {
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool head = sp_is_head(key, i, n);
    const unsigned long long b = __ballot(head);
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads();
    int incl = __popcll(b & (((1ull << lane) - 1ull) | (1ull << lane)));
    for (int w = 0; w < wave; ++w) incl += wc[w];
    const bool dropped = i < n && key[i] == SP_DROPPED;
    if (i < n) {
        const int v = idx[i];
        if (v >= 0 && v < n) vcell[v] = dropped ? -1 : (int)(offs[blockIdx.x] + incl - 1);        // (idx is a permutation of [0, n): the store's own guard)
    }
    sp_count(counters + 3, dropped);
    if (i == 0) counters[0] = offs[nblk];
}

// ---------------------------------------------------------------------------------------------------------
// Stage 2
#define SP_OK 0
#define SP_INVALID 1
#define SP_COLLAPSED 2
// the cluster triple of triangle t -> c[3]; a vcell outside [0, nv) counts as a dropped vertex
__device__ __forceinline__ int sp_triple(const int* __restrict__ tris, const int* __restrict__ vcell, long long t, long long nv, int* c) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int v = tris[3 * (size_t)t + j];
        if (v < 0 || v >= nv) return SP_INVALID;
        c[j] = vcell[v];
        if (c[j] < 0 || c[j] >= nv) return SP_INVALID;
    }
    return (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) ? SP_COLLAPSED : SP_OK;
}
__device__ __forceinline__ void sp_sort3(const int* c, int* s) {
    const int lo = min(c[0], min(c[1], c[2])), hi = max(c[0], max(c[1], c[2]));
    s[0] = lo; s[2] = hi; s[1] = (int)((long long)c[0] + c[1] + c[2] - lo - hi);
}
// the keys of a triangle that does not survive for sure sort behind every cluster: nv, and (nv, nv)
__global__ __launch_bounds__(256) void sp_tri_key_kernel(const int* __restrict__ tris, const int* __restrict__ vcell, int nt, long long nv,
                                                         unsigned long long* __restrict__ key, int* __restrict__ idx) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int c[3], s[3];
    unsigned long long k = (unsigned long long)nv;
    if (sp_triple(tris, vcell, t, nv, c) == SP_OK) { sp_sort3(c, s); k = (unsigned long long)s[2]; }
    key[t] = k; idx[t] = t;
}
__global__ __launch_bounds__(256) void sp_tri_rekey_kernel(const int* __restrict__ tris, const int* __restrict__ vcell, int nt, long long nv, int bits,
                                                           unsigned long long* __restrict__ key, const int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const int t = idx[i];
    int c[3], s[3];
    unsigned long long k = ((unsigned long long)nv << bits) | (unsigned long long)nv;
    if (t >= 0 && t < nt && sp_triple(tris, vcell, t, nv, c) == SP_OK) { sp_sort3(c, s); k = ((unsigned long long)s[0] << bits) | (unsigned long long)s[1]; }
    key[i] = k;
}
__global__ __launch_bounds__(256) void sp_mark_kernel(const int* __restrict__ tris, const int* __restrict__ vcell, int nt, long long nv,
                                                      const int* __restrict__ idx, int* __restrict__ flag, long long* __restrict__ counters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int why = -1;
    if (i < nt) {
        const int t = idx[i];
        if (t >= 0 && t < nt) {                                            // (idx is a permutation of [0, nt): the reads' own guard)
            int c[3], s[3];
            why = sp_triple(tris, vcell, t, nv, c);
            bool dup = false;
            if (why == SP_OK && i > 0) {
                const int tp = idx[i - 1];
                int cp[3], sq[3];
                if (tp >= 0 && tp < nt && sp_triple(tris, vcell, tp, nv, cp) == SP_OK) {
                    sp_sort3(c, s); sp_sort3(cp, sq);
                    dup = s[0] == sq[0] && s[1] == sq[1] && s[2] == sq[2];
                }
            }
            if (dup) why = 3;
            flag[t] = why == SP_OK ? 1 : 0;
        }
    }
    sp_count(counters + 4, why == SP_INVALID);
    sp_count(counters + 5, why == SP_COLLAPSED);
    sp_count(counters + 6, why == 3);
}
__global__ __launch_bounds__(256) void sp_flag_count_kernel(const int* __restrict__ flag, int n, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    vox_block_count(i < n && flag[i] != 0, counts);
}
// survivor t -> row j in ascending t: its source, its rotated cluster triple (cells for now), its three cells marked as used
__global__ __launch_bounds__(256) void sp_tri_emit_kernel(const int* __restrict__ tris, const int* __restrict__ vcell, int nt, long long nv,
                                                          const int* __restrict__ flag, const int64_t* __restrict__ offs, int* __restrict__ tris_out,
                                                          int* __restrict__ tri_src, int* __restrict__ used) {
    __shared__ int wc[4];
    const int t = blockIdx.x * 256 + threadIdx.x;
    int c[3];
    const bool keep = t < nt && flag[t] != 0 && sp_triple(tris, vcell, t, nv, c) == SP_OK;
    const int rank = vox_block_rank(keep, wc);
    if (!keep) return;
    const long long j = offs[blockIdx.x] + rank;
    if (j < 0 || j >= nt) return;                                          // (j <= t: the stores' own guard)
    int r0 = c[0], r1 = c[1], r2 = c[2];
    if (c[1] < c[0] && c[1] < c[2]) { r0 = c[1]; r1 = c[2]; r2 = c[0]; }
    else if (c[2] < c[0] && c[2] < c[1]) { r0 = c[2]; r1 = c[0]; r2 = c[1]; }
    tri_src[j] = t;
    tris_out[3 * (size_t)j] = r0; tris_out[3 * (size_t)j + 1] = r1; tris_out[3 * (size_t)j + 2] = r2;
    used[r0] = 1; used[r1] = 1; used[r2] = 1;                              // integer stores of the same value: no order to depend on
}
__global__ __launch_bounds__(256) void sp_cell_emit_kernel(const int* __restrict__ used, int nv, const int64_t* __restrict__ offs, int* __restrict__ cell_out) {
    __shared__ int wc[4];
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool keep = c < nv && used[c] != 0;
    const int rank = vox_block_rank(keep, wc);
    if (c < nv) cell_out[c] = keep ? (int)(offs[blockIdx.x] + rank) : -1;
}
// one lane per row of max(nt, nv): output indices for the cells of the output triangles, -1 rows behind them, vmap, the two counts
__global__ __launch_bounds__(256) void sp_remap_kernel(int nt, int nv, const int* __restrict__ vcell, const int* __restrict__ cell_out,
                                                       const int64_t* __restrict__ n_tris, const int64_t* __restrict__ n_verts,
                                                       int* __restrict__ tris_out, int* __restrict__ tri_src, int* __restrict__ vmap,
                                                       long long* __restrict__ counters) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nt) {
        const bool live = n_tris != nullptr && i < *n_tris;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int c = live ? tris_out[3 * (size_t)i + j] : -1;
            tris_out[3 * (size_t)i + j] = (c >= 0 && c < nv) ? cell_out[c] : -1;
        }
        if (!live) tri_src[i] = -1;
    }
    if (i < nv) {
        const int c = vcell[i];
        vmap[i] = (c >= 0 && c < nv) ? cell_out[c] : -1;
    }
    if (i == 0) { counters[1] = n_verts ? *n_verts : 0; counters[2] = n_tris ? *n_tris : 0; }
}

// ---------------------------------------------------------------------------------------------------------
// Stage 3
__global__ __launch_bounds__(256) void sp_vkey_kernel(const int* __restrict__ vcell, int nv, unsigned long long* __restrict__ key, int* __restrict__ idx) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int c = vcell[v];
    key[v] = (c >= 0 && c < nv) ? (unsigned long long)c : (unsigned long long)nv;
    idx[v] = v;
}
__global__ __launch_bounds__(256) void sp_pkey_kernel(const int* __restrict__ tris, const int* __restrict__ vcell, int m, long long nv,
                                                      unsigned long long* __restrict__ key, int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int t = i / 3;
    int c[3];
    key[i] = sp_triple(tris, vcell, t, nv, c) != SP_INVALID ? (unsigned long long)c[i - 3 * t] : (unsigned long long)nv;
    idx[i] = i;
}
__device__ __forceinline__ int sp_lower_bound(const unsigned long long* __restrict__ key, int n, unsigned long long c) {
    int lo = 0, hi = n;
    while (lo < hi) {                                                      // at most 32 steps
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ bool sp_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }     // false for NaN

// one Jacobi rotation on (p, q) with r the third index; every name is a register
#define SP_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                     \
    if (apq != 0.0) {                                                                                       \
        const double theta = (aqq - app) / (2.0 * apq);                                                     \
        const double h = sqrt(theta * theta + 1.0);                                                         \
        double t = 1.0 / (fabs(theta) + h);                                                                 \
        if (theta < 0.0) t = -t;                                                                            \
        const double c = 1.0 / sqrt(t * t + 1.0);                                                           \
        const double s = t * c;                                                                             \
        const double z = t * apq;                                                                           \
        app = app - z; aqq = aqq + z; apq = 0.0;                                                            \
        { const double x_ = c * arp - s * arq, y_ = s * arp + c * arq; arp = x_; arq = y_; }                \
        { const double x_ = c * v0p - s * v0q, y_ = s * v0p + c * v0q; v0p = x_; v0q = y_; }                \
        { const double x_ = c * v1p - s * v1q, y_ = s * v1p + c * v1q; v1p = x_; v1q = y_; }                \
        { const double x_ = c * v2p - s * v2q, y_ = s * v2p + c * v2q; v2p = x_; v2q = y_; }                \
    }

struct SpPlace {
    const float* verts; const float* colors; const int* tris; const int* vcell; const int* cell_out;
    const unsigned long long* vkey; const int* vidx;          // (vcell[v], v) sorted
    const unsigned long long* pkey; const int* pidx;          // (cell of the corner, 3 t + j) sorted; unused with placement 0
    long long nv; int m;                                      // m = 3 nt
    SpGrid g; int placement; double sv_ratio;
    float* verts_out; float* colors_out; long long* counters;
};
__global__ __launch_bounds__(256) void sp_place_kernel(const SpPlace P) {
    const long long cl = (long long)blockIdx.x * 256 + threadIdx.x;
    bool fallback = false;
    int o = -1;
    if (cl < P.nv) o = P.cell_out[cl];
    if (o >= 0 && o < P.nv) {
        const int nv = (int)P.nv;
        const unsigned long long ck = (unsigned long long)cl;
        const int first = sp_lower_bound(P.vkey, nv, ck);
        double sx = 0.0, sy = 0.0, sz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
        int count = 0, v0 = -1;
        for (int r = first; r < nv && P.vkey[r] == ck; ++r) {
            const int v = P.vidx[r];
            if (v < 0 || v >= nv) break;                                   // (vidx is a permutation of [0, nv): the reads' own guard)
            if (v0 < 0) v0 = v;
            sx = sx + (double)P.verts[3 * (size_t)v]; sy = sy + (double)P.verts[3 * (size_t)v + 1]; sz = sz + (double)P.verts[3 * (size_t)v + 2];
            if (P.colors) { cr = cr + (double)P.colors[3 * (size_t)v]; cg = cg + (double)P.colors[3 * (size_t)v + 1]; cb = cb + (double)P.colors[3 * (size_t)v + 2]; }
            ++count;
        }
        if (count > 0) {                                                   // (a used cell holds a vertex)
            const double n = (double)count;
            const double mx = sx / n, my = sy / n, mz = sz / n;
            double x0 = mx, x1 = my, x2 = mz;
            if (P.placement == 1) {
                double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
                const int pfirst = sp_lower_bound(P.pkey, P.m, ck);
                for (int r = pfirst; r < P.m && P.pkey[r] == ck; ++r) {
                    const int t = P.pidx[r] / 3;
                    if (t < 0 || 3 * (long long)t + 2 >= P.m) break;       // (pidx is a permutation of [0, m): the reads' own guard)
                    const int ia = P.tris[3 * (size_t)t], ib = P.tris[3 * (size_t)t + 1], ic = P.tris[3 * (size_t)t + 2];
                    if (ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) continue;      // (a key below nv says so already)
                    const float* A = P.verts + 3 * (size_t)ia; const float* B = P.verts + 3 * (size_t)ib; const float* C = P.verts + 3 * (size_t)ic;
                    const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
                    const double ux = (double)B[0] - ax, uy = (double)B[1] - ay, uz = (double)B[2] - az;
                    const double wx = (double)C[0] - ax, wy = (double)C[1] - ay, wz = (double)C[2] - az;
                    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                    if (!(sp_finite(nx) && sp_finite(ny) && sp_finite(nz))) continue;
                    a00 = a00 + nx * nx; a01 = a01 + nx * ny; a02 = a02 + nx * nz;
                    a11 = a11 + ny * ny; a12 = a12 + ny * nz; a22 = a22 + nz * nz;
                    const double d = (nx * (mx - ax) + ny * (my - ay)) + nz * (mz - az);
                    g0 = g0 + nx * d; g1 = g1 + ny * d; g2 = g2 + nz * d;
                }
                double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
                for (int sweep = 0; sweep < SP_SWEEPS; ++sweep) {
                    SP_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
                    SP_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
                    SP_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
                }
                double lmax = a00;
                if (a11 > lmax) lmax = a11;
                if (a22 > lmax) lmax = a22;
                const double thr = P.sv_ratio * lmax;
                double y0 = 0.0, y1 = 0.0, y2 = 0.0;
                if (a00 > thr) { const double w = ((v00 * g0 + v10 * g1) + v20 * g2) / a00; y0 = y0 + v00 * w; y1 = y1 + v10 * w; y2 = y2 + v20 * w; }
                if (a11 > thr) { const double w = ((v01 * g0 + v11 * g1) + v21 * g2) / a11; y0 = y0 + v01 * w; y1 = y1 + v11 * w; y2 = y2 + v21 * w; }
                if (a22 > thr) { const double w = ((v02 * g0 + v12 * g1) + v22 * g2) / a22; y0 = y0 + v02 * w; y1 = y1 + v12 * w; y2 = y2 + v22 * w; }
                const double q0 = mx - y0, q1 = my - y1, q2 = mz - y2;
                long long i3[3] = {0, 0, 0};
                bool ok = lmax > 0.0 && sp_finite(q0) && sp_finite(q1) && sp_finite(q2) && sp_cell_index(P.verts, v0, P.g, i3);
                if (ok) {
                    const double l0 = P.g.o[0] + (double)i3[0] * P.g.cell, h0 = P.g.o[0] + (double)(i3[0] + 1) * P.g.cell;
                    const double l1 = P.g.o[1] + (double)i3[1] * P.g.cell, h1 = P.g.o[1] + (double)(i3[1] + 1) * P.g.cell;
                    const double l2 = P.g.o[2] + (double)i3[2] * P.g.cell, h2 = P.g.o[2] + (double)(i3[2] + 1) * P.g.cell;
                    ok = l0 <= q0 && q0 <= h0 && l1 <= q1 && q1 <= h1 && l2 <= q2 && q2 <= h2;
                }
                if (ok) { x0 = q0; x1 = q1; x2 = q2; } else fallback = true;
            }
            P.verts_out[3 * (size_t)o] = (float)x0; P.verts_out[3 * (size_t)o + 1] = (float)x1; P.verts_out[3 * (size_t)o + 2] = (float)x2;
            if (P.colors_out) { P.colors_out[3 * (size_t)o] = (float)(cr / n); P.colors_out[3 * (size_t)o + 1] = (float)(cg / n); P.colors_out[3 * (size_t)o + 2] = (float)(cb / n); }
        }
    }
    sp_count(P.counters + 7, fallback);
}
