// Point-to-triangle distances (libsta_dist.so; the contract is in include/sta_dist.h), included by sta_dist.hip after voxel.h (the stable
// radix sort).  Sort based, no floating-point atomics, every output defined by the input alone.
//   ds_bounds_kernel / ds_bounds_final_kernel   class of every triangle, min / max of the box centres of the valid ones, the four counts
//   ds_key_kernel                               the Morton key of a valid triangle, 2^63 for the others; payload = the input index
//   ds_gather_kernel                            coordinates and input index in sorted order
//   ds_leaf_kernel / ds_level_kernel            the boxes of level 0 and of one level above: a lane per node, F reads, no atomics
//   ds_query_kernel                             one lane per query: a greedy descent for a first best, then a stackless walk in index order
// Nothing here indexes a private array with a run-time value: the walk's state is (level, node), the level table lives in LDS.
#pragma once

#pragma clang fp contract(off)

#define DS_F 8
#define DS_MAX_LEVELS 9
#define DS_PARTS 1024          // workgroups of ds_bounds_kernel at the most: what one workgroup of ds_bounds_final_kernel folds
#define DS_VALID 0
#define DS_BAD_INDEX 1
#define DS_NON_FINITE 2
#define DS_NO_AREA 3
#define DS_STATUS 4
#define DS_STATUS_BOUND 1

// the shape of the tree (host values in the kernel arguments): off[l] = first node of level l, off[levels] = the number of nodes
struct DsTree { int nt; int levels; int off[DS_MAX_LEVELS + 1]; };

__device__ __forceinline__ bool ds_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }      // false for NaN

// The class of triangle t and, for all but a bad-index one, its nine coordinates.
__device__ __forceinline__ int ds_load(const float* __restrict__ verts, long long nv, const int* __restrict__ tris, int t, float* p) {
    const int i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return DS_BAD_INDEX;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = verts[3 * (size_t)i0 + k]; p[3 + k] = verts[3 * (size_t)i1 + k]; p[6 + k] = verts[3 * (size_t)i2 + k];
        fin = fin && ds_finite(p[k]) && ds_finite(p[3 + k]) && ds_finite(p[6 + k]);
    }
    if (!fin) return DS_NON_FINITE;
    const double ux = (double)p[3] - (double)p[0], uy = (double)p[4] - (double)p[1], uz = (double)p[5] - (double)p[2];
    const double vx = (double)p[6] - (double)p[0], vy = (double)p[7] - (double)p[1], vz = (double)p[8] - (double)p[2];
    const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
    const double w = sqrt((nx * nx + ny * ny) + nz * nz);
    return (w > 0.0 && w <= 1.7976931348623157e308) ? DS_VALID : DS_NO_AREA;
}
// m_k = (double(min_k) + double(max_k)) * 0.5
__device__ __forceinline__ double ds_centre(const float* p, int k) {
    const float lo = fminf(fminf(p[k], p[3 + k]), p[6 + k]), hi = fmaxf(fmaxf(p[k], p[3 + k]), p[6 + k]);
    return ((double)lo + (double)hi) * 0.5;
}

// ---------------------------------------------------------------------------------------------------------
// Bounds and counts.  part [gridDim.x][8] doubles = {L xyz, U xyz, (count valid, bad index), (non finite, no area)} - the counts as
// two int pairs in the bits of a double.  min / max are exact and order-free, the counts integers: nothing depends on the grid.
__device__ __forceinline__ double ds_pack(int a, int b) { return __longlong_as_double(((long long)(unsigned)b << 32) | (unsigned)a); }
__device__ __forceinline__ int ds_lo(double d) { return (int)(unsigned)(__double_as_longlong(d) & 0xffffffffll); }
__device__ __forceinline__ int ds_hi(double d) { return (int)(unsigned)((unsigned long long)__double_as_longlong(d) >> 32); }

__device__ __forceinline__ void ds_fold(double* mn, double* mx, int* cnt, double* out) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fmin(mn[a], __shfl_xor(mn[a], o)); mx[a] = fmax(mx[a], __shfl_xor(mx[a], o)); }
#pragma unroll
        for (int a = 0; a < 4; ++a) cnt[a] += __shfl_xor(cnt[a], o);
    }
    __shared__ double red[4][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int a = 0; a < 3; ++a) { red[wave][a] = mn[a]; red[wave][3 + a] = mx[a]; }
        red[wave][6] = ds_pack(cnt[0], cnt[1]); red[wave][7] = ds_pack(cnt[2], cnt[3]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            for (int a = 0; a < 3; ++a) { mn[a] = fmin(mn[a], red[w][a]); mx[a] = fmax(mx[a], red[w][3 + a]); }
            cnt[0] += ds_lo(red[w][6]); cnt[1] += ds_hi(red[w][6]); cnt[2] += ds_lo(red[w][7]); cnt[3] += ds_hi(red[w][7]);
        }
        for (int a = 0; a < 3; ++a) { out[a] = mn[a]; out[3 + a] = mx[a]; }
        out[6] = ds_pack(cnt[0], cnt[1]); out[7] = ds_pack(cnt[2], cnt[3]);
    }
}
__global__ __launch_bounds__(256) void ds_bounds_kernel(const float* __restrict__ verts, long long nv, const int* __restrict__ tris, int nt,
                                                        double* __restrict__ part) {
    const double inf = __builtin_huge_val();
    double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    int cnt[4] = {0, 0, 0, 0};
    for (int t = blockIdx.x * 256 + threadIdx.x; t < nt; t += gridDim.x * 256) {
        float p[9];
        const int cls = ds_load(verts, nv, tris, t, p);
        cnt[0] += cls == DS_VALID; cnt[1] += cls == DS_BAD_INDEX; cnt[2] += cls == DS_NON_FINITE; cnt[3] += cls == DS_NO_AREA;
        if (cls == DS_VALID) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { const double m = ds_centre(p, a); mn[a] = fmin(mn[a], m); mx[a] = fmax(mx[a], m); }
        }
    }
    ds_fold(mn, mx, cnt, part + 8 * (size_t)blockIdx.x);
}
// one workgroup folds the n <= DS_PARTS partial rows to lu[8] and writes the counters twice: the index's copy and the caller's
__global__ __launch_bounds__(256) void ds_bounds_final_kernel(const double* __restrict__ part, int n, double* __restrict__ lu, int* __restrict__ counters,
                                                              int* __restrict__ counters_out) {
    const double inf = __builtin_huge_val();
    double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    int cnt[4] = {0, 0, 0, 0};
    for (int b = threadIdx.x; b < n; b += 256) {
        const double* p = part + 8 * (size_t)b;
        for (int a = 0; a < 3; ++a) { mn[a] = fmin(mn[a], p[a]); mx[a] = fmax(mx[a], p[3 + a]); }
        cnt[0] += ds_lo(p[6]); cnt[1] += ds_hi(p[6]); cnt[2] += ds_lo(p[7]); cnt[3] += ds_hi(p[7]);
    }
    ds_fold(mn, mx, cnt, lu);
    if (threadIdx.x == 0) {          // the thread that wrote lu holds the totals
        for (int a = 0; a < 8; ++a) { const int v = a < 4 ? cnt[a] : 0; counters[a] = v; counters_out[a] = v; }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Keys.  bit b of g -> bit 3 b
__device__ __forceinline__ unsigned long long ds_spread(unsigned long long g) {
    g &= 0x1fffffull;
    g = (g | (g << 32)) & 0x1f00000000ffffull;
    g = (g | (g << 16)) & 0x1f0000ff0000ffull;
    g = (g | (g << 8)) & 0x100f00f00f00f00full;
    g = (g | (g << 4)) & 0x10c30c30c30c30c3ull;
    g = (g | (g << 2)) & 0x1249249249249249ull;
    return g;
}
__device__ __forceinline__ unsigned long long ds_quant(double m, double L, double U) {
    if (U == L) return 0ull;
    const double a = m - L;
    const double b = U - L;
    const double c = a / b;
    const double g = floor(c * 2097152.0);
    if (!(g >= 0.0)) return 0ull;                 // (m >= L, so this is never taken; a guard for the conversion)
    return g > 2097151.0 ? 2097151ull : (unsigned long long)g;
}
__global__ __launch_bounds__(256) void ds_key_kernel(const float* __restrict__ verts, long long nv, const int* __restrict__ tris, int nt,
                                                     const double* __restrict__ lu, unsigned long long* __restrict__ key, int* __restrict__ idx) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    float p[9];
    unsigned long long k = 1ull << 63;
    if (ds_load(verts, nv, tris, t, p) == DS_VALID) {
        k = 0ull;
#pragma unroll
        for (int a = 0; a < 3; ++a) k |= ds_spread(ds_quant(ds_centre(p, a), lu[a], lu[3 + a])) << a;
    }
    key[t] = k; idx[t] = t;
}
__global__ __launch_bounds__(256) void ds_gather_kernel(const float* __restrict__ verts, long long nv, const int* __restrict__ tris, int nt,
                                                        const unsigned long long* __restrict__ key, const int* __restrict__ idx,
                                                        float* __restrict__ tri, int* __restrict__ src) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const int t = idx[i];
    float p[9];
    const bool ok = (key[i] >> 63) == 0ull && t >= 0 && t < nt && ds_load(verts, nv, tris, t, p) == DS_VALID;
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < 9; ++k) tri[9 * (size_t)i + k] = ok ? p[k] : nan;
    src[i] = t;
}

// ---------------------------------------------------------------------------------------------------------
// Boxes.  fminf / fmaxf of float32 are exact; a NaN row (a position that is not valid) is skipped by the count.
__global__ __launch_bounds__(256) void ds_leaf_kernel(const float* __restrict__ tri, int nt, const int* __restrict__ counters, int n_nodes,
                                                      float* __restrict__ boxes) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_nodes) return;
    int n_valid = counters[DS_VALID];
    n_valid = n_valid < nt ? n_valid : nt;
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll
    for (int c = 0; c < DS_F; ++c) {
        const int i = DS_F * j + c;
        if (i < n_valid) {
            const float* p = tri + 9 * (size_t)i;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(lo[k], fminf(fminf(p[k], p[3 + k]), p[6 + k]));
                hi[k] = fmaxf(hi[k], fmaxf(fmaxf(p[k], p[3 + k]), p[6 + k]));
            }
        }
    }
    float* o = boxes + 6 * (size_t)j;
    for (int k = 0; k < 3; ++k) { o[k] = lo[k]; o[3 + k] = hi[k]; }
}
// nodes [0, n_nodes) of a level from the n_child nodes of the level below; an empty child (+inf, -inf) leaves min / max alone
__global__ __launch_bounds__(256) void ds_level_kernel(const float* __restrict__ child, int n_child, int n_nodes, float* __restrict__ boxes) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_nodes) return;
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll
    for (int c = 0; c < DS_F; ++c) {
        const int i = DS_F * j + c;
        if (i < n_child) {
            const float* p = child + 6 * (size_t)i;
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], p[k]); hi[k] = fmaxf(hi[k], p[3 + k]); }
        }
    }
    float* o = boxes + 6 * (size_t)j;
    for (int k = 0; k < 3; ++k) { o[k] = lo[k]; o[3 + k] = hi[k]; }
}

// ---------------------------------------------------------------------------------------------------------
// Query.
struct DsBest { double d2; int tri; double c[3]; };

// bound of the box at p (6 floats) for q; +inf and empty = true for a node without a valid triangle
__device__ __forceinline__ double ds_bound(const float* __restrict__ p, double qx, double qy, double qz, bool* empty) {
    const float lx = p[0], ly = p[1], lz = p[2], hx = p[3], hy = p[4], hz = p[5];
    *empty = lx > hx;
    const double ex = fmax(fmax((double)lx - qx, qx - (double)hx), 0.0);
    const double ey = fmax(fmax((double)ly - qy, qy - (double)hy), 0.0);
    const double ez = fmax(fmax((double)lz - qz, qz - (double)hz), 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}
__device__ __forceinline__ double ds_dot(double x0, double x1, double x2, double y0, double y1, double y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }
__device__ __forceinline__ double ds_clamp(double p, float a, float b, float c) {
    const double lo = (double)fminf(fminf(a, b), c), hi = (double)fmaxf(fmaxf(a, b), c);
    double r = p >= lo ? p : lo;
    r = r <= hi ? r : hi;
    return r;
}
// the closest point of the triangle at p (9 floats), clamped, and its d2: the rules of include/sta_dist.h in their order
__device__ __forceinline__ void ds_closest(const float* __restrict__ p, double qx, double qy, double qz, int t, DsBest& best) {
    const float fa0 = p[0], fa1 = p[1], fa2 = p[2], fb0 = p[3], fb1 = p[4], fb2 = p[5], fc0 = p[6], fc1 = p[7], fc2 = p[8];
    const double a0 = fa0, a1 = fa1, a2 = fa2, b0 = fb0, b1 = fb1, b2 = fb2, c0 = fc0, c1 = fc1, c2 = fc2;
    const double ab0 = b0 - a0, ab1 = b1 - a1, ab2 = b2 - a2, ac0 = c0 - a0, ac1 = c1 - a1, ac2 = c2 - a2;
    const double d1 = ds_dot(ab0, ab1, ab2, qx - a0, qy - a1, qz - a2), d2 = ds_dot(ac0, ac1, ac2, qx - a0, qy - a1, qz - a2);
    const double d3 = ds_dot(ab0, ab1, ab2, qx - b0, qy - b1, qz - b2), d4 = ds_dot(ac0, ac1, ac2, qx - b0, qy - b1, qz - b2);
    const double d5 = ds_dot(ab0, ab1, ab2, qx - c0, qy - c1, qz - c2), d6 = ds_dot(ac0, ac1, ac2, qx - c0, qy - c1, qz - c2);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e1 = d4 - d3, e2 = d5 - d6;
    double x, y, z;
    if (d1 <= 0.0 && d2 <= 0.0) { x = a0; y = a1; z = a2; }
    else if (d3 >= 0.0 && d4 <= d3) { x = b0; y = b1; z = b2; }
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { const double v = d1 / (d1 - d3); x = a0 + ab0 * v; y = a1 + ab1 * v; z = a2 + ab2 * v; }
    else if (d6 >= 0.0 && d5 <= d6) { x = c0; y = c1; z = c2; }
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { const double w = d2 / (d2 - d6); x = a0 + ac0 * w; y = a1 + ac1 * w; z = a2 + ac2 * w; }
    else if (va <= 0.0 && e1 >= 0.0 && e2 >= 0.0) { const double w = e1 / (e1 + e2); x = b0 + (c0 - b0) * w; y = b1 + (c1 - b1) * w; z = b2 + (c2 - b2) * w; }
    else {
        const double denom = 1.0 / ((va + vb) + vc), v = vb * denom, w = vc * denom;
        x = (a0 + ab0 * v) + ac0 * w; y = (a1 + ab1 * v) + ac1 * w; z = (a2 + ab2 * v) + ac2 * w;
    }
    x = ds_clamp(x, fa0, fb0, fc0); y = ds_clamp(y, fa1, fb1, fc1); z = ds_clamp(z, fa2, fb2, fc2);
    const double dx = qx - x, dy = qy - y, dz = qz - z;
    const double dd = (dx * dx + dy * dy) + dz * dz;
    if (dd < best.d2 || (dd == best.d2 && t < best.tri)) { best.d2 = dd; best.tri = t; best.c[0] = x; best.c[1] = y; best.c[2] = z; }
}
__device__ __forceinline__ void ds_leaf(const float* __restrict__ tri, const int* __restrict__ src, int node, int n_valid, double qx, double qy,
                                        double qz, DsBest& best) {
#pragma unroll 1
    for (int c = 0; c < DS_F; ++c) {
        const int i = DS_F * node + c;
        if (i < n_valid) ds_closest(tri + 9 * (size_t)i, qx, qy, qz, src[i], best);
    }
}

struct DsQuery {
    const float* tri; const int* src; const float* boxes; int* counters;
    const float* qry; int Q; double r2;
    double* d2_out; int* tri_out; float* point_out;
    DsTree tree;
};
__global__ __launch_bounds__(256) void ds_query_kernel(const DsQuery P) {
    __shared__ int s_off[DS_MAX_LEVELS + 1];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l <= DS_MAX_LEVELS; ++l) s_off[l] = P.tree.off[l];          // static indices: the arguments stay in registers
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.Q) return;
    const float fx = P.qry[3 * (size_t)i], fy = P.qry[3 * (size_t)i + 1], fz = P.qry[3 * (size_t)i + 2];
    const double qx = fx, qy = fy, qz = fz;
    const int levels = P.tree.levels, top = levels - 1, nodes = s_off[levels];
    int n_valid = P.counters[DS_VALID];
    n_valid = n_valid < P.tree.nt ? n_valid : P.tree.nt;
    DsBest best;
    best.d2 = P.r2; best.tri = 0x7fffffff; best.c[0] = 0.0; best.c[1] = 0.0; best.c[2] = 0.0;
    bool bound_hit = false;
    if (ds_finite(fx) && ds_finite(fy) && ds_finite(fz) && n_valid > 0) {
        // 1. a first best: down from the root into the non-empty child of the smallest bound
        {
            int node = 0;
            bool found = true;
            for (int lev = top; lev > 0 && found; --lev) {
                const int first = DS_F * node, cnt = s_off[lev] - s_off[lev - 1];
                double bb = 0.0, bm = 0.0; int pick = -1;
#pragma unroll 1
                for (int c = 0; c < DS_F; ++c) {
                    if (first + c < cnt) {
                        bool empty;
                        const float* bx = P.boxes + 6 * (size_t)(s_off[lev - 1] + first + c);
                        const double b = ds_bound(bx, qx, qy, qz, &empty);
                        // boxes overlap, so many bounds are 0: among equal bounds the box whose centre is nearest (a heuristic only:
                        // whatever leaf is scored first, phase 2 finds the minimum)
                        const double mx = ((double)bx[0] + (double)bx[3]) * 0.5 - qx, my = ((double)bx[1] + (double)bx[4]) * 0.5 - qy,
                                     mz = ((double)bx[2] + (double)bx[5]) * 0.5 - qz;
                        const double m = (mx * mx + my * my) + mz * mz;
                        if (!empty && (pick < 0 || b < bb || (b == bb && m < bm))) { bb = b; bm = m; pick = first + c; }
                    }
                }
                found = pick >= 0;
                node = pick;
            }
            if (found) ds_leaf(P.tri, P.src, node, n_valid, qx, qy, qz, best);
        }
        // 2. every node in depth-first index order, without a stack
        int lev = top, node = 0;
        bool done = false;
        for (int it = 0; it <= nodes && !done; ++it) {
            bool empty;
            const double b = ds_bound(P.boxes + 6 * (size_t)(s_off[lev] + node), qx, qy, qz, &empty);
            const bool enter = !empty && !(b > best.d2);
            if (enter && lev > 0) { --lev; node *= DS_F; continue; }
            if (enter) ds_leaf(P.tri, P.src, node, n_valid, qx, qy, qz, best);
            // the node after (lev, node): its next sibling, or the node after its parent
            for (int k = 0; k < DS_MAX_LEVELS; ++k) {
                if (lev == top) { done = true; break; }
                if ((node & (DS_F - 1)) != DS_F - 1 && node + 1 < s_off[lev + 1] - s_off[lev]) { ++node; break; }
                node /= DS_F; ++lev;
            }
        }
        bound_hit = !done;
    }
    if (bound_hit) atomicOr(P.counters + DS_STATUS, DS_STATUS_BOUND);          // an integer flag: order-free
    const bool hit = best.tri != 0x7fffffff && !bound_hit;
    if (P.d2_out) P.d2_out[i] = hit ? best.d2 : __builtin_huge_val();
    if (P.tri_out) P.tri_out[i] = hit ? best.tri : -1;
    if (P.point_out) {
        const float nan = __builtin_nanf("");
        P.point_out[3 * (size_t)i] = hit ? (float)best.c[0] : nan;
        P.point_out[3 * (size_t)i + 1] = hit ? (float)best.c[1] : nan;
        P.point_out[3 * (size_t)i + 2] = hit ? (float)best.c[2] : nan;
    }
}
