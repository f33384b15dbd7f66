// Registration against the triangle index (libsta_reg.so; the contract is in include/sta_reg.h), included by sta_reg.hip; it includes
// sta_common.h alone.  Two kernels:
//   rg_pass_kernel    one lane per query: q' = T q in float64, the exact nearest triangle (a greedy descent for a first best, then the
//                     stackless walk in index order that the distance query of libsta_dist.so uses - restated here on three doubles,
//                     that library's files are not included), the plane of the winner, the residual, the Jacobian row, and the
//                     lane's 50 terms folded to one partial row per workgroup
//   rg_final_kernel   one workgroup folds the partial rows in a fixed order
// No floating-point atomics, every output defined by the input alone.  Nothing here indexes a private array with a run-time value: the
// walk's state is (level, node), the level table lives in LDS, the terms of the record are folded one at a time (a term is made,
// reduced over the wave and stored before the next one is made: the epilogue holds the query, the closest point, the normal and the
// Jacobian row, not fifty accumulators).
#pragma once
#include "sta_common.h"

#pragma clang fp contract(off)

#define RG_F 8
#define RG_MAX_LEVELS 9
#define RG_VALID 0
#define RG_STATUS_BOUND 1
#define RG_RECORD 64          // doubles in a record and in a partial row
#define RG_USED 50            // ... of which the first 50 are sums, the rest 0

// the shape of the tree (host values in the kernel arguments): off[l] = first node of level l, off[levels] = the number of nodes
struct RgTree { int nt; int levels; int off[RG_MAX_LEVELS + 1]; };

__device__ __forceinline__ bool rg_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for NaN

struct RgBest { double d2; int tri; int pos; double c[3]; };

// bound of the box at p (6 floats) for q'; empty = true for a node without a valid triangle
__device__ __forceinline__ double rg_bound(const float* __restrict__ p, double qx, double qy, double qz, bool* empty) {
    const float lx = p[0], ly = p[1], lz = p[2], hx = p[3], hy = p[4], hz = p[5];
    *empty = lx > hx;
    const double ex = fmax(fmax((double)lx - qx, qx - (double)hx), 0.0);
    const double ey = fmax(fmax((double)ly - qy, qy - (double)hy), 0.0);
    const double ez = fmax(fmax((double)lz - qz, qz - (double)hz), 0.0);
    return (ex * ex + ey * ey) + ez * ez;
}
__device__ __forceinline__ double rg_dot(double x0, double x1, double x2, double y0, double y1, double y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }
__device__ __forceinline__ double rg_clamp(double p, float a, float b, float c) {
    const double lo = (double)fminf(fminf(a, b), c), hi = (double)fmaxf(fmaxf(a, b), c);
    double r = p >= lo ? p : lo;
    r = r <= hi ? r : hi;
    return r;
}
// the closest point of the triangle at sorted position i (9 floats at p), clamped, and its d2: rule 2 of include/sta_reg.h in its order
__device__ __forceinline__ void rg_closest(const float* __restrict__ p, double qx, double qy, double qz, int t, int i, RgBest& best) {
    const float fa0 = p[0], fa1 = p[1], fa2 = p[2], fb0 = p[3], fb1 = p[4], fb2 = p[5], fc0 = p[6], fc1 = p[7], fc2 = p[8];
    const double a0 = fa0, a1 = fa1, a2 = fa2, b0 = fb0, b1 = fb1, b2 = fb2, c0 = fc0, c1 = fc1, c2 = fc2;
    const double ab0 = b0 - a0, ab1 = b1 - a1, ab2 = b2 - a2, ac0 = c0 - a0, ac1 = c1 - a1, ac2 = c2 - a2;
    const double d1 = rg_dot(ab0, ab1, ab2, qx - a0, qy - a1, qz - a2), d2 = rg_dot(ac0, ac1, ac2, qx - a0, qy - a1, qz - a2);
    const double d3 = rg_dot(ab0, ab1, ab2, qx - b0, qy - b1, qz - b2), d4 = rg_dot(ac0, ac1, ac2, qx - b0, qy - b1, qz - b2);
    const double d5 = rg_dot(ab0, ab1, ab2, qx - c0, qy - c1, qz - c2), d6 = rg_dot(ac0, ac1, ac2, qx - c0, qy - c1, qz - c2);
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
    x = rg_clamp(x, fa0, fb0, fc0); y = rg_clamp(y, fa1, fb1, fc1); z = rg_clamp(z, fa2, fb2, fc2);
    const double dx = qx - x, dy = qy - y, dz = qz - z;
    const double dd = (dx * dx + dy * dy) + dz * dz;
    if (dd < best.d2 || (dd == best.d2 && t < best.tri)) { best.d2 = dd; best.tri = t; best.pos = i; best.c[0] = x; best.c[1] = y; best.c[2] = z; }
}
__device__ __forceinline__ void rg_leaf(const float* __restrict__ tri, const int* __restrict__ src, int node, int n_valid, double qx, double qy,
                                        double qz, RgBest& best) {
#pragma unroll 1
    for (int c = 0; c < RG_F; ++c) {
        const int i = RG_F * node + c;
        if (i < n_valid) rg_closest(tri + 9 * (size_t)i, qx, qy, qz, src[i], i, best);
    }
}

// One term of the record: the xor butterfly over the wave (a + b on both sides: every lane ends with the same bits), lane 0 stores.
__device__ __forceinline__ void rg_emit(double* __restrict__ row, int lane, double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) *row = v;
}
// ((w0 + w1) + w2) + w3 of the four waves' rows, entries behind RG_USED are 0
__device__ __forceinline__ void rg_store_row(const double (*red)[RG_RECORD], double* __restrict__ out) {
    if (threadIdx.x < RG_RECORD) {
        const int r = threadIdx.x;
        out[r] = r < RG_USED ? ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r] : 0.0;
    }
}

struct RgPass {
    const float* tri; const int* src; const float* boxes; const int* counters;
    const float* qry; const float* qnrm; int Q; double r2, min_cos;
    double T[12]; double pivot[3];
    double* d2_out; int* tri_out; float* point_out; double* resid_out; double* part; int* status;
    RgTree tree;
};
__global__ __launch_bounds__(256) void rg_pass_kernel(const RgPass P) {
    __shared__ int s_off[RG_MAX_LEVELS + 1];
    __shared__ double red[4][RG_RECORD];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l <= RG_MAX_LEVELS; ++l) s_off[l] = P.tree.off[l];          // static indices: the arguments stay in registers
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool active = i < P.Q;          // (an inactive lane of the last workgroup stays for the fold: all its terms are 0)
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (active) {
        const double x = (double)P.qry[3 * (size_t)i], y = (double)P.qry[3 * (size_t)i + 1], z = (double)P.qry[3 * (size_t)i + 2];
        qx = ((P.T[0] * x + P.T[1] * y) + P.T[2] * z) + P.T[3];
        qy = ((P.T[4] * x + P.T[5] * y) + P.T[6] * z) + P.T[7];
        qz = ((P.T[8] * x + P.T[9] * y) + P.T[10] * z) + P.T[11];
    }
    const bool finite = active && rg_finite(qx) && rg_finite(qy) && rg_finite(qz);
    const int levels = P.tree.levels, top = levels - 1, nodes = s_off[levels];
    int n_valid = P.counters[RG_VALID];
    n_valid = n_valid < P.tree.nt ? n_valid : P.tree.nt;
    RgBest best;
    best.d2 = P.r2; best.tri = 0x7fffffff; best.pos = 0; best.c[0] = 0.0; best.c[1] = 0.0; best.c[2] = 0.0;
    bool bound_hit = false;
    if (finite && n_valid > 0) {
        // 1. a first best: down from the root into the non-empty child of the smallest bound
        {
            int node = 0;
            bool found = true;
            for (int lev = top; lev > 0 && found; --lev) {
                const int first = RG_F * node, cnt = s_off[lev] - s_off[lev - 1];
                double bb = 0.0, bm = 0.0; int pick = -1;
#pragma unroll 1
                for (int c = 0; c < RG_F; ++c) {
                    if (first + c < cnt) {
                        bool empty;
                        const float* bx = P.boxes + 6 * (size_t)(s_off[lev - 1] + first + c);
                        const double b = rg_bound(bx, qx, qy, qz, &empty);
                        // among equal bounds the box whose centre is nearest (a heuristic only: whatever leaf is scored first, phase 2
                        // finds the minimum)
                        const double mx = ((double)bx[0] + (double)bx[3]) * 0.5 - qx, my = ((double)bx[1] + (double)bx[4]) * 0.5 - qy,
                                     mz = ((double)bx[2] + (double)bx[5]) * 0.5 - qz;
                        const double m = (mx * mx + my * my) + mz * mz;
                        if (!empty && (pick < 0 || b < bb || (b == bb && m < bm))) { bb = b; bm = m; pick = first + c; }
                    }
                }
                found = pick >= 0;
                node = pick;
            }
            if (found) rg_leaf(P.tri, P.src, node, n_valid, qx, qy, qz, best);
        }
        // 2. every node in depth-first index order, without a stack
        int lev = top, node = 0;
        bool done = false;
        for (int it = 0; it <= nodes && !done; ++it) {
            bool empty;
            const double b = rg_bound(P.boxes + 6 * (size_t)(s_off[lev] + node), qx, qy, qz, &empty);
            const bool enter = !empty && !(b > best.d2);
            if (enter && lev > 0) { --lev; node *= RG_F; continue; }
            if (enter) rg_leaf(P.tri, P.src, node, n_valid, qx, qy, qz, best);
            // the node after (lev, node): its next sibling, or the node after its parent
            for (int k = 0; k < RG_MAX_LEVELS; ++k) {
                if (lev == top) { done = true; break; }
                if ((node & (RG_F - 1)) != RG_F - 1 && node + 1 < s_off[lev + 1] - s_off[lev]) { ++node; break; }
                node /= RG_F; ++lev;
            }
        }
        bound_hit = !done;
    }
    if (bound_hit) atomicOr(P.status, RG_STATUS_BOUND);          // an integer flag: order-free
    const bool found = best.tri != 0x7fffffff && !bound_hit;

    // 3. the plane of the winner (best.pos < n_valid <= nt whenever found; position 0 is read otherwise and its values are dropped)
    const float* tp = P.tri + 9 * (size_t)(found ? best.pos : 0);
    const double A0 = tp[0], A1 = tp[1], A2 = tp[2];
    const double u0 = (double)tp[3] - A0, u1 = (double)tp[4] - A1, u2 = (double)tp[5] - A2;
    const double v0 = (double)tp[6] - A0, v1 = (double)tp[7] - A1, v2 = (double)tp[8] - A2;
    const double n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
    const double w = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    const double h0 = n0 / w, h1 = n1 / w, h2 = n2 / w;
    const double cx = best.c[0], cy = best.c[1], cz = best.c[2];
    const double r = rg_dot(qx - cx, qy - cy, qz - cz, h0, h1, h2);
    // 4. normal agreement
    bool rejected = false;
    if (P.qnrm && found) {
        const double a = (double)P.qnrm[3 * (size_t)i], b = (double)P.qnrm[3 * (size_t)i + 1], c = (double)P.qnrm[3 * (size_t)i + 2];
        const double m0 = (P.T[0] * a + P.T[1] * b) + P.T[2] * c, m1 = (P.T[4] * a + P.T[5] * b) + P.T[6] * c,
                     m2 = (P.T[8] * a + P.T[9] * b) + P.T[10] * c;
        rejected = rg_dot(m0, m1, m2, h0, h1, h2) < P.min_cos * sqrt(rg_dot(m0, m1, m2, m0, m1, m2));
    }
    const bool matched = found && !rejected;
    // 5. per-query outputs
    if (active) {
        const double nan = __builtin_nan("");
        if (P.d2_out) P.d2_out[i] = found ? best.d2 : __builtin_huge_val();
        if (P.tri_out) P.tri_out[i] = found ? best.tri : -1;
        if (P.point_out) {
            const float nanf_ = __builtin_nanf("");
            P.point_out[3 * (size_t)i] = found ? (float)cx : nanf_;
            P.point_out[3 * (size_t)i + 1] = found ? (float)cy : nanf_;
            P.point_out[3 * (size_t)i + 2] = found ? (float)cz : nanf_;
        }
        if (P.resid_out) P.resid_out[i] = found ? r : nan;
    }
    if (!P.part) return;          // (uniform over the launch)
    // 6. the lane's terms, one at a time; an unmatched lane contributes 0 beyond entry 3, never a NaN
    const int lane = threadIdx.x & 63;
    double* row = red[threadIdx.x >> 6];
#define RG_TERM(slot, cond, value) rg_emit(row + (slot), lane, (cond) ? (value) : 0.0)
    RG_TERM(0, finite, 1.0);
    RG_TERM(1, matched, 1.0);
    RG_TERM(2, matched, best.d2);
    RG_TERM(3, finite, matched ? best.d2 : P.r2);
    RG_TERM(4, matched, qx); RG_TERM(5, matched, qy); RG_TERM(6, matched, qz);
    RG_TERM(7, matched, cx); RG_TERM(8, matched, cy); RG_TERM(9, matched, cz);
    RG_TERM(10, matched, qx * cx); RG_TERM(11, matched, qx * cy); RG_TERM(12, matched, qx * cz);
    RG_TERM(13, matched, qy * cx); RG_TERM(14, matched, qy * cy); RG_TERM(15, matched, qy * cz);
    RG_TERM(16, matched, qz * cx); RG_TERM(17, matched, qz * cy); RG_TERM(18, matched, qz * cz);
    RG_TERM(19, active && !finite, 1.0);
    RG_TERM(20, rejected, 1.0);
    RG_TERM(21, matched, r * r);
    RG_TERM(22, matched, fabs(r));
    const double x0 = qx - P.pivot[0], x1 = qy - P.pivot[1], x2 = qz - P.pivot[2];
    const double j0 = x1 * h2 - x2 * h1, j1 = x2 * h0 - x0 * h2, j2 = x0 * h1 - x1 * h0;
    RG_TERM(23, matched, j0 * r); RG_TERM(24, matched, j1 * r); RG_TERM(25, matched, j2 * r);
    RG_TERM(26, matched, h0 * r); RG_TERM(27, matched, h1 * r); RG_TERM(28, matched, h2 * r);
    RG_TERM(29, matched, j0 * j0); RG_TERM(30, matched, j0 * j1); RG_TERM(31, matched, j0 * j2);
    RG_TERM(32, matched, j0 * h0); RG_TERM(33, matched, j0 * h1); RG_TERM(34, matched, j0 * h2);
    RG_TERM(35, matched, j1 * j1); RG_TERM(36, matched, j1 * j2);
    RG_TERM(37, matched, j1 * h0); RG_TERM(38, matched, j1 * h1); RG_TERM(39, matched, j1 * h2);
    RG_TERM(40, matched, j2 * j2);
    RG_TERM(41, matched, j2 * h0); RG_TERM(42, matched, j2 * h1); RG_TERM(43, matched, j2 * h2);
    RG_TERM(44, matched, h0 * h0); RG_TERM(45, matched, h0 * h1); RG_TERM(46, matched, h0 * h2);
    RG_TERM(47, matched, h1 * h1); RG_TERM(48, matched, h1 * h2);
    RG_TERM(49, matched, h2 * h2);
#undef RG_TERM
    __syncthreads();
    rg_store_row(red, P.part + (size_t)blockIdx.x * RG_RECORD);
}

// one workgroup of 256 threads: thread t adds the partial rows t, t + 256, ... in ascending order, then the butterfly and the waves
__global__ __launch_bounds__(256) void rg_final_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    __shared__ double red[4][RG_RECORD];
    double acc[RG_USED];
#pragma unroll
    for (int r = 0; r < RG_USED; ++r) acc[r] = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) {
#pragma unroll
        for (int r = 0; r < RG_USED; ++r) acc[r] += part[(size_t)b * RG_RECORD + r];
    }
    const int lane = threadIdx.x & 63;
    double* row = red[threadIdx.x >> 6];
#pragma unroll
    for (int r = 0; r < RG_USED; ++r) rg_emit(row + r, lane, acc[r]);
    __syncthreads();
    rg_store_row(red, out);
}
