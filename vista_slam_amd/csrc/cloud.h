// Exact nearest neighbours on a uniform grid (libsta_cloud.so; the contract is in include/sta_cloud.h), included by sta_cloud.hip
// after voxel.h, whose bounds, radix-sort and head kernels build the index.  Launch code in sta_cloud.hip.
//   cl_grid_kernel        bounds -> smallest cell index and extent per axis (device side: the build does not wait for them)
//   cl_key_kernel         key = ((iz - lo_z) << 42) | ((iy - lo_y) << 21) | (ix - lo_x), all-ones for a non-finite point
//   cl_finish_kernel      cell_key[c] = key at the cell's first sorted position; coordinates copied in sorted order
//   cl_query_kernel       one lane per query: rings of cells of growing Chebyshev distance, one binary search per (iz, iy) row
//   cl_record_final_kernel  the per-workgroup record partials folded in a fixed order
//   cl_transform_kernel   out = float(T p)
// Every fp64 operation is written out and nothing is contracted (the pragma below holds to the end of the translation unit).
#pragma once
#pragma clang fp contract(off)

#define CL_RECORD 24
#define CL_MAX_QBLOCKS 2048        // workgroups of a query launch; a thread walks its queries with this stride

// min / max of the finite points (vox_bounds_final_kernel's out[8]) -> the grid of the build.  ext <= 0 when nothing is finite.
struct ClGrid { long long lo[3]; long long ext[3]; long long dropped; long long pad; };

__device__ __forceinline__ double cl_cell_of(double x, double cell) { return floor(x / cell); }

__global__ void cl_grid_kernel(const float* __restrict__ bounds, double cell, ClGrid* __restrict__ g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double big = 2305843009213693952.0;     // 2^61: whatever is beyond is refused by the host, the clamp only keeps the conversion defined
    for (int a = 0; a < 3; ++a) {
        double lo = cl_cell_of((double)bounds[a], cell), hi = cl_cell_of((double)bounds[3 + a], cell);
        lo = fmin(fmax(lo, -big), big); hi = fmin(fmax(hi, -big), big);
        if (!(lo == lo)) lo = big;
        if (!(hi == hi)) hi = -big;
        g->lo[a] = (long long)lo;
        g->ext[a] = (long long)hi - (long long)lo + 1;
    }
    g->dropped = (long long)__float_as_int(bounds[6]);
    g->pad = 0;
}

__global__ __launch_bounds__(256) void cl_key_kernel(const float* __restrict__ pts, int M, double cell, const ClGrid* __restrict__ g,
                                                     unsigned long long* __restrict__ key, int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    unsigned long long k = ~0ull;
    if (vox_finite3(p[0], p[1], p[2])) {
        unsigned long long r[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // inside [0, 2^21) for every grid the host accepts; the clamp keeps the key's fields apart for one it refuses
            const double rel = cl_cell_of((double)p[a], cell) - (double)g->lo[a];
            r[a] = (unsigned long long)fmin(fmax(rel, 0.0), 2097151.0);
        }
        k = (r[2] << 42) | (r[1] << 21) | r[0];
    }
    key[i] = k; idx[i] = i;
}

// n_cells = *total (occupied cells, plus one for the non-finite points if there are any: their key is all-ones and sorts last)
__global__ __launch_bounds__(256) void cl_finish_kernel(const float* __restrict__ pts, int M, const unsigned long long* __restrict__ skey,
                                                        const int* __restrict__ sidx, const int* __restrict__ cell_start,
                                                        const int64_t* __restrict__ total, unsigned long long* __restrict__ cell_key,
                                                        float* __restrict__ spts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const size_t j = (size_t)sidx[i];                     // a permutation of [0, M)
    spts[3 * (size_t)i] = pts[3 * j]; spts[3 * (size_t)i + 1] = pts[3 * j + 1]; spts[3 * (size_t)i + 2] = pts[3 * j + 2];
    if (i < (int)*total) cell_key[i] = skey[cell_start[i]];          // cell_start[i] < M for i < total
}

// ---------------------------------------------------------------------------------------------------------
struct ClQuery {
    const unsigned long long* cell_key; const int* cell_start; const float* spts; const int* sidx;
    double lo[3]; int ext[3]; int C; double cell;
    const float* qry; int Q; double T[12]; double r2; int kmax;
    double* d2_out; int* idx_out; double* part;        // any may be NULL; part [gridDim.x][CL_RECORD]
};

struct ClBest { double d2; int idx; float p[3]; };

// the cells x0 .. x1 of row (iz, iy): a contiguous key range, found by one binary search
__device__ __forceinline__ void cl_scan_row(const ClQuery& P, int iz, int iy, int x0, int x1, const double* q, ClBest& best) {
    x0 = max(x0, 0); x1 = min(x1, P.ext[0] - 1);
    if (x0 > x1) return;
    const unsigned long long row = ((unsigned long long)iz << 42) | ((unsigned long long)iy << 21);
    const unsigned long long klo = row | (unsigned long long)x0, khi = row | (unsigned long long)x1;
    int a = 0, n = P.C;
    while (n > 0) {                                     // first cell with key >= klo
        const int h = n >> 1;
        if (P.cell_key[a + h] < klo) { a += h + 1; n -= h + 1; } else n = h;
    }
    if (a >= P.C || P.cell_key[a] > khi) return;
    int b = a + 1;
    while (b < P.C && P.cell_key[b] <= khi) ++b;        // at most x1 - x0 further cells
    const int s = P.cell_start[a], e = P.cell_start[b];
    for (int i = s; i < e; ++i) {
        const float px = P.spts[3 * (size_t)i], py = P.spts[3 * (size_t)i + 1], pz = P.spts[3 * (size_t)i + 2];
        const double dx = q[0] - (double)px, dy = q[1] - (double)py, dz = q[2] - (double)pz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= P.r2 && d2 <= best.d2) {
            const int oi = P.sidx[i];
            if (d2 < best.d2 || oi < best.idx) { best.d2 = d2; best.idx = oi; best.p[0] = px; best.p[1] = py; best.p[2] = pz; }
        }
    }
}

__global__ __launch_bounds__(256) void cl_query_kernel(const ClQuery P) {
    const double inf = __builtin_huge_val();
    double acc[CL_RECORD];
#pragma unroll
    for (int r = 0; r < CL_RECORD; ++r) acc[r] = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P.Q; i += (long long)gridDim.x * 256) {
        const double x = (double)P.qry[3 * (size_t)i], y = (double)P.qry[3 * (size_t)i + 1], z = (double)P.qry[3 * (size_t)i + 2];
        double q[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = ((P.T[4 * a] * x + P.T[4 * a + 1] * y) + P.T[4 * a + 2] * z) + P.T[4 * a + 3];
        const bool finite = fabs(q[0]) <= 1.7976931348623157e308 && fabs(q[1]) <= 1.7976931348623157e308 && fabs(q[2]) <= 1.7976931348623157e308;
        ClBest best; best.d2 = inf; best.idx = -1; best.p[0] = best.p[1] = best.p[2] = 0.f;
        if (finite && P.C > 0) {
            int c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                // clamped in fp64 to the grid and the search margin BEFORE it becomes an integer: a query far outside lands in a
                // cell between its own and the grid, so every reference cell is in a ring no further out than its true one
                const double rel = cl_cell_of(q[a], P.cell) - P.lo[a];
                c[a] = (int)fmin(fmax(rel, (double)(-(P.kmax + 1))), (double)(P.ext[a] + P.kmax));
            }
            for (int k = 0; k <= P.kmax; ++k) {
                for (int dz = -k; dz <= k; ++dz) {
                    const int iz = c[2] + dz;
                    if (iz < 0 || iz >= P.ext[2]) continue;
                    for (int dy = -k; dy <= k; ++dy) {
                        const int iy = c[1] + dy;
                        if (iy < 0 || iy >= P.ext[1]) continue;
                        if (dz == -k || dz == k || dy == -k || dy == k) cl_scan_row(P, iz, iy, c[0] - k, c[0] + k, q, best);
                        else { cl_scan_row(P, iz, iy, c[0] - k, c[0] - k, q, best); cl_scan_row(P, iz, iy, c[0] + k, c[0] + k, q, best); }
                    }
                }
                // every cell not yet visited is k + 1 or more cells away on some axis: its points are further than k cells, less the
                // rounding of the two divisions that named the cells (at most 2 * 2^21 * 2^-53 = 2^-31 of a cell for |cell index| <= 2^21: half the 2^-30 margin at k = 1)
                const double bound = ((double)k * P.cell) * (1.0 - 9.313225746154785e-10);
                if (best.d2 < bound * bound) break;
            }
        }
        if (P.d2_out) P.d2_out[i] = best.d2;
        if (P.idx_out) P.idx_out[i] = best.idx;
        if (finite) {
            acc[0] += 1.0;
            if (best.idx >= 0) {
                acc[1] += 1.0; acc[2] += best.d2; acc[3] += best.d2;          // d2 <= radius^2: min(d2, radius^2) = d2
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    acc[4 + a] += q[a]; acc[7 + a] += (double)best.p[a];
#pragma unroll
                    for (int b = 0; b < 3; ++b) acc[10 + 3 * a + b] += q[a] * (double)best.p[b];
                }
            } else acc[3] += P.r2;
        } else acc[19] += 1.0;
    }
    if (!P.part) return;
    // a thread's sum runs over its queries in ascending order, then a xor butterfly over the 64 lanes (a + b on both sides: every
    // lane holds the same bits), then the four waves in ascending order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int r = 0; r < 20; ++r) acc[r] += __shfl_xor(acc[r], o);
    }
    __shared__ double red[4][CL_RECORD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { for (int r = 0; r < CL_RECORD; ++r) red[wave][r] = acc[r]; }
    __syncthreads();
    if (threadIdx.x < CL_RECORD) {
        const int r = threadIdx.x;
        P.part[(size_t)blockIdx.x * CL_RECORD + r] = ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r];
    }
}

// one workgroup of 256 threads: thread t adds the partial rows t, t + 256, ... in ascending order, then as above
__global__ __launch_bounds__(256) void cl_record_final_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    double acc[CL_RECORD];
#pragma unroll
    for (int r = 0; r < CL_RECORD; ++r) acc[r] = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) {
#pragma unroll
        for (int r = 0; r < 20; ++r) acc[r] += part[(size_t)b * CL_RECORD + r];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int r = 0; r < 20; ++r) acc[r] += __shfl_xor(acc[r], o);
    }
    __shared__ double red[4][CL_RECORD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { for (int r = 0; r < CL_RECORD; ++r) red[wave][r] = acc[r]; }
    __syncthreads();
    if (threadIdx.x < CL_RECORD) {
        const int r = threadIdx.x;
        out[r] = ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r];
    }
}

struct ClMat { double T[12]; };
__global__ __launch_bounds__(256) void cl_transform_kernel(const float* pts, long long M, const ClMat m, float* out) {      // out may be pts
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const double x = (double)pts[3 * (size_t)i], y = (double)pts[3 * (size_t)i + 1], z = (double)pts[3 * (size_t)i + 2];
    float o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = (float)(((m.T[4 * a] * x + m.T[4 * a + 1] * y) + m.T[4 * a + 2] * z) + m.T[4 * a + 3]);
    out[3 * (size_t)i] = o[0]; out[3 * (size_t)i + 1] = o[1]; out[3 * (size_t)i + 2] = o[2];
}
