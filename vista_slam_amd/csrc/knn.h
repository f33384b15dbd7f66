// The k nearest neighbours on the grid of sta_nn_build and the moments of the neighbourhoods (libsta_knn.so; the contract is in
// include/sta_knn.h), included by sta_knn.hip.  It includes sta_common.h alone: nothing of libsta_cloud.so, whose ring walk
// (cl_query_kernel, cl_scan_row) is restated here for a list of k instead of one best.
//   kn_query_kernel         one lane per query, one wave per workgroup; the lane's sorted k-list lives in dynamic LDS, interleaved by
//                           lane (slot j of lane l at [j][l]: the 64 lanes of a slot fall in 64 different banks)
//   kn_moments_kernel       one lane per query: mean neighbour distance, covariance about the mean, 8 Jacobi sweeps, the oriented
//                           normal, the surface variation, the record partial of its workgroup
//   kn_record_final_kernel  the per-workgroup record partials folded in a fixed order
// Nothing here indexes a private array at run time (that would go to scratch): the list is LDS, the 3x3 algebra is named registers.
// Every fp64 operation is written out and nothing is contracted (the pragma below holds to the end of the translation unit).
#pragma once
#pragma clang fp contract(off)
#include "sta_common.h"

#define KN_MAX_K 64
#define KN_RECORD 8
#define KN_USED 4                 // record entries that are summed; the others are 0
#define KN_SWEEPS 8
#define KN_MAX_QBLOCKS 2048       // workgroups of a moments launch; a thread walks its queries with this stride
#define KN_STATUS_BOUND 1
#define KN_STATUS_ORDER 2

struct KnQuery {
    const unsigned long long* cell_key; const int* cell_start; const float* spts; const int* sidx;
    double lo[3]; int ext[3]; int C; int n; double cell;       // n = n_finite: the rows of spts / sidx that the grid names
    const float* qry; const int* order; int Q; long long self_base; int k; double r2; int kmax;
    double* d2_out; int* idx_out; int* count_out; int* status;
};

// a lane's list: d2 [k][64] doubles, then idx [k][64] ints
struct KnList { double* d2; int* idx; int k; int cnt; double kd; int ki; };      // kd, ki: the register copy of the k-th entry (+inf, INT_MAX while not full)

// (d2, oi) enters when it is before the k-th entry in (d2, index) order; a sorted shift from the end places it
__device__ __forceinline__ void kn_offer(KnList& L, double d2, int oi) {
    if (!(d2 < L.kd || (d2 == L.kd && oi < L.ki))) return;
    int j = L.cnt < L.k ? L.cnt : L.k - 1;
    while (j > 0) {                                             // at most k - 1 steps
        const double pd = L.d2[(j - 1) * 64];
        const int pi = L.idx[(j - 1) * 64];
        if (!(d2 < pd || (d2 == pd && oi < pi))) break;
        L.d2[j * 64] = pd; L.idx[j * 64] = pi;
        --j;
    }
    L.d2[j * 64] = d2; L.idx[j * 64] = oi;
    if (L.cnt < L.k) ++L.cnt;
    if (L.cnt == L.k) { L.kd = L.d2[(L.k - 1) * 64]; L.ki = L.idx[(L.k - 1) * 64]; }
}

// the cells x0 .. x1 of row (iz, iy): a contiguous key range, found by one binary search (cl_scan_row, restated)
__device__ __forceinline__ void kn_scan_row(const KnQuery& P, int iz, int iy, int x0, int x1, double qx, double qy, double qz, long long self, KnList& L) {
    x0 = max(x0, 0); x1 = min(x1, P.ext[0] - 1);
    if (x0 > x1) return;
    const unsigned long long row = ((unsigned long long)iz << 42) | ((unsigned long long)iy << 21);
    const unsigned long long klo = row | (unsigned long long)x0, khi = row | (unsigned long long)x1;
    int a = 0, n = P.C;
    while (n > 0) {                                     // first cell with key >= klo: at most 31 steps
        const int h = n >> 1;
        if (P.cell_key[a + h] < klo) { a += h + 1; n -= h + 1; } else n = h;
    }
    if (a >= P.C || P.cell_key[a] > khi) return;
    int b = a + 1;
    while (b < P.C && P.cell_key[b] <= khi) ++b;        // at most x1 - x0 further cells, and never beyond C
    int s = P.cell_start[a], e = P.cell_start[b];
    if (s < 0 || e > P.n || s > e) {                    // not an index of sta_nn_build: cut the walk to the rows that exist
        atomicOr(P.status, KN_STATUS_BOUND);
        s = min(max(s, 0), P.n); e = min(max(e, s), P.n);
    }
    for (int i = s; i < e; ++i) {
        const float px = P.spts[3 * (size_t)i], py = P.spts[3 * (size_t)i + 1], pz = P.spts[3 * (size_t)i + 2];
        const double dx = qx - (double)px, dy = qy - (double)py, dz = qz - (double)pz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= P.r2 && d2 <= L.kd) {
            const int oi = P.sidx[i];
            if ((long long)oi != self) kn_offer(L, d2, oi);
        }
    }
}

__global__ __launch_bounds__(64) void kn_query_kernel(const KnQuery P) {
    extern __shared__ __attribute__((aligned(16))) char kn_smem[];
    const double inf = __builtin_huge_val();
    const int lane = threadIdx.x;
    const long long slot = (long long)blockIdx.x * 64 + lane;
    if (slot >= P.Q) return;                            // (no barrier in this kernel: a lane may leave)
    long long i = slot;
    if (P.order) {
        i = (long long)P.order[slot];
        if (i < 0 || i >= P.Q) { atomicOr(P.status, KN_STATUS_ORDER); return; }
    }
    KnList L;
    L.d2 = (double*)kn_smem + lane;
    L.idx = (int*)(kn_smem + (size_t)P.k * 64 * sizeof(double)) + lane;
    L.k = P.k; L.cnt = 0; L.kd = inf; L.ki = 0x7fffffff;
    const double qx = (double)P.qry[3 * (size_t)i], qy = (double)P.qry[3 * (size_t)i + 1], qz = (double)P.qry[3 * (size_t)i + 2];
    const bool finite = fabs(qx) <= 1.7976931348623157e308 && fabs(qy) <= 1.7976931348623157e308 && fabs(qz) <= 1.7976931348623157e308;
    if (finite && P.C > 0) {
        const long long self = P.self_base >= 0 ? P.self_base + i : -1;
        // clamped in fp64 to the grid and the search margin BEFORE it becomes an integer, as in sta_nn_query
        const int c0 = (int)fmin(fmax(floor(qx / P.cell) - P.lo[0], (double)(-(P.kmax + 1))), (double)(P.ext[0] + P.kmax));
        const int c1 = (int)fmin(fmax(floor(qy / P.cell) - P.lo[1], (double)(-(P.kmax + 1))), (double)(P.ext[1] + P.kmax));
        const int c2 = (int)fmin(fmax(floor(qz / P.cell) - P.lo[2], (double)(-(P.kmax + 1))), (double)(P.ext[2] + P.kmax));
        for (int r = 0; r <= P.kmax; ++r) {
            for (int dz = -r; dz <= r; ++dz) {
                const int iz = c2 + dz;
                if (iz < 0 || iz >= P.ext[2]) continue;
                for (int dy = -r; dy <= r; ++dy) {
                    const int iy = c1 + dy;
                    if (iy < 0 || iy >= P.ext[1]) continue;
                    if (dz == -r || dz == r || dy == -r || dy == r) kn_scan_row(P, iz, iy, c0 - r, c0 + r, qx, qy, qz, self, L);
                    else { kn_scan_row(P, iz, iy, c0 - r, c0 - r, qx, qy, qz, self, L); kn_scan_row(P, iz, iy, c0 + r, c0 + r, qx, qy, qz, self, L); }
                }
            }
            // every cell not yet visited is r + 1 or more cells away on some axis (include/sta_knn.h: the argument for the k-th)
            const double bound = ((double)r * P.cell) * (1.0 - 9.313225746154785e-10);
            if (L.cnt == L.k && L.kd < bound * bound) break;
        }
    }
    const size_t base = (size_t)i * (size_t)P.k;
    for (int j = 0; j < P.k; ++j) {
        const bool used = j < L.cnt;
        if (P.d2_out) P.d2_out[base + j] = used ? L.d2[j * 64] : inf;
        if (P.idx_out) P.idx_out[base + j] = used ? L.idx[j * 64] : -1;
    }
    if (P.count_out) P.count_out[i] = L.cnt;
}

// ---------------------------------------------------------------------------------------------------------
// one Jacobi rotation on (p, q) with r the third index; every name is a register (the statement of include/sta_knn.h)
#define KN_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                                     \
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

struct KnMoments {
    const float* ref; long long M; const float* qry; int Q; const double* d2; const int* idx; const int* count; int k;
    const float* view; double vh[3]; int has_vh; int min_count;
    float* normal_out; double* curv_out; double* mean_dist_out; double* part;       // any may be NULL; part [gridDim.x][KN_RECORD]
};

__global__ __launch_bounds__(256) void kn_moments_kernel(const KnMoments P) {
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P.Q; i += (long long)gridDim.x * 256) {
        const size_t base = (size_t)i * (size_t)P.k;
        int c = min(max(P.count[i], 0), P.k);
        double sd = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        for (int j = 0; j < c; ++j) {
            const long long v = (long long)P.idx[base + j];
            if (v < 0 || v >= P.M) { c = j; break; }                        // the list ends here: nothing is read through this index
            if (P.d2) sd = sd + sqrt(P.d2[base + j]);
            sx = sx + (double)P.ref[3 * (size_t)v]; sy = sy + (double)P.ref[3 * (size_t)v + 1]; sz = sz + (double)P.ref[3 * (size_t)v + 2];
        }
        const double n = (double)c;
        const double md = c >= 1 ? sd / n : inf;
        if (P.mean_dist_out) P.mean_dist_out[i] = md;
        if (c >= 1) { acc0 = acc0 + 1.0; acc1 = acc1 + md; acc2 = acc2 + md * md; }
        double nx = nan, ny = nan, nz = nan, curv = nan;
        if (c >= P.min_count) {
            acc3 = acc3 + 1.0;
            const double mx = sx / n, my = sy / n, mz = sz / n;
            double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
            for (int j = 0; j < c; ++j) {
                const size_t v = (size_t)P.idx[base + j];                   // inside [0, M): the first walk ended the list before any other
                const double dx = (double)P.ref[3 * v] - mx, dy = (double)P.ref[3 * v + 1] - my, dz = (double)P.ref[3 * v + 2] - mz;
                a00 = a00 + dx * dx; a01 = a01 + dx * dy; a02 = a02 + dx * dz;
                a11 = a11 + dy * dy; a12 = a12 + dy * dz; a22 = a22 + dz * dz;
            }
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
            for (int sweep = 0; sweep < KN_SWEEPS; ++sweep) {
                KN_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
                KN_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
                KN_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
            }
            // rank of every eigenvalue in the stable ascending order (the lowest column first among equals)
            const int r0 = (a11 < a00 ? 1 : 0) + (a22 < a00 ? 1 : 0);
            const int r1 = (a00 <= a11 ? 1 : 0) + (a22 < a11 ? 1 : 0);
            const int r2 = (a00 <= a22 ? 1 : 0) + (a11 <= a22 ? 1 : 0);
            const double l0 = r0 == 0 ? a00 : r1 == 0 ? a11 : a22;
            const double l1 = r0 == 1 ? a00 : r1 == 1 ? a11 : a22;
            const double l2 = r0 == 2 ? a00 : r1 == 2 ? a11 : a22;
            const double ex = r0 == 0 ? v00 : r1 == 0 ? v01 : v02;
            const double ey = r0 == 0 ? v10 : r1 == 0 ? v11 : v12;
            const double ez = r0 == 0 ? v20 : r1 == 0 ? v21 : v22;
            const double len = sqrt((ex * ex + ey * ey) + ez * ez);
            nx = ex / len; ny = ey / len; nz = ez / len;
            bool flip;
            if (P.view || P.has_vh) {
                const double qx = (double)P.qry[3 * (size_t)i], qy = (double)P.qry[3 * (size_t)i + 1], qz = (double)P.qry[3 * (size_t)i + 2];
                const double wx = P.view ? (double)P.view[3 * (size_t)i] : P.vh[0], wy = P.view ? (double)P.view[3 * (size_t)i + 1] : P.vh[1],
                             wz = P.view ? (double)P.view[3 * (size_t)i + 2] : P.vh[2];
                flip = ((wx - qx) * nx + (wy - qy) * ny) + (wz - qz) * nz < 0.0;
            } else {
                double big = nx;
                if (fabs(ny) > fabs(big)) big = ny;
                if (fabs(nz) > fabs(big)) big = nz;
                flip = big < 0.0;
            }
            if (flip) { nx = -nx; ny = -ny; nz = -nz; }
            const double tr = (l0 + l1) + l2;
            curv = tr == 0.0 ? 0.0 : l0 / tr;
        }
        if (P.normal_out) { P.normal_out[3 * (size_t)i] = (float)nx; P.normal_out[3 * (size_t)i + 1] = (float)ny; P.normal_out[3 * (size_t)i + 2] = (float)nz; }
        if (P.curv_out) P.curv_out[i] = curv;
    }
    if (!P.part) return;                                                    // (uniform over the grid: no lane has left before the barrier)
    // a thread's sum runs over its queries in ascending order, then a xor butterfly over the 64 lanes (a + b on both sides: every
    // lane holds the same bits), then the four waves in ascending order: cl_query_kernel's reduction, restated
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc0 += __shfl_xor(acc0, o); acc1 += __shfl_xor(acc1, o); acc2 += __shfl_xor(acc2, o); acc3 += __shfl_xor(acc3, o);
    }
    __shared__ double red[4][KN_USED];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = acc0; red[wave][1] = acc1; red[wave][2] = acc2; red[wave][3] = acc3; }
    __syncthreads();
    if (threadIdx.x < KN_RECORD) {
        const int r = threadIdx.x;
        P.part[(size_t)blockIdx.x * KN_RECORD + r] = r < KN_USED ? ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r] : 0.0;
    }
}

// one workgroup of 256 threads: thread t adds the partial rows t, t + 256, ... in ascending order, then as above
__global__ __launch_bounds__(256) void kn_record_final_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) {
        acc0 += part[(size_t)b * KN_RECORD]; acc1 += part[(size_t)b * KN_RECORD + 1];
        acc2 += part[(size_t)b * KN_RECORD + 2]; acc3 += part[(size_t)b * KN_RECORD + 3];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc0 += __shfl_xor(acc0, o); acc1 += __shfl_xor(acc1, o); acc2 += __shfl_xor(acc2, o); acc3 += __shfl_xor(acc3, o);
    }
    __shared__ double red[4][KN_USED];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave][0] = acc0; red[wave][1] = acc1; red[wave][2] = acc2; red[wave][3] = acc3; }
    __syncthreads();
    if (threadIdx.x < KN_RECORD) {
        const int r = threadIdx.x;
        out[r] = r < KN_USED ? ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r] : 0.0;
    }
}
