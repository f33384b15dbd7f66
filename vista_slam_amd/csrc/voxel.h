// Voxel-grid fusion of a point cloud (sta_voxel_downsample; the contract is in include/sta_mi355.h), included by sta_api.hip after
// elementwise.h (cloud_scan_kernel, cloud_write_record) and select.h (sel_block_scan); launch code in sta_rows.inc.  Sort based: no
// table to size, no floating-point atomics, every output defined by the input alone.
//   vox_bounds_kernel / vox_bounds_final_kernel   min / max of the finite points per axis + the number of dropped points -> 8 words
//   vox_key_kernel                                key = (iz << (nx+ny)) | (iy << nx) | ix relative to the grid's corner, payload = input index
//   vox_hist_kernel / vox_hist_scan_kernel / vox_scatter_kernel   one pass of a stable LSD radix sort (8-bit digits, tiles of 1024 keys)
//   vox_head_count_kernel / vox_head_emit_kernel  first sorted position of every occupied voxel (cloud_scan_kernel between the two)
//   vox_row_count_kernel / vox_row_emit_kernel    min_points: ordered compaction of the voxels to output rows (cloud_scan_kernel again)
//   vox_reduce_kernel / vox_reduce_long_kernel    per-row fp64 sums in a fixed order, means, counts, indices, inverse, PLY records
#pragma once
#include "sta_skew.h"       // STA_SKEW points: nothing unless -DSTA_WAVE_SKEW (libsta_mi355_skew.so)

#define VOX_TILE 1024          // keys per workgroup and sort pass: four chunks of 256
#define VOX_LONG 1024          // a voxel of more points than this is reduced by a whole workgroup of 1024 threads, not by one wave
#define VOX_MAX_EXTENT (1 << 21)

// The grid of one call (host values in the kernel arguments): o = corner, vs = voxel size, lo = smallest voxel index per axis,
// nx / ny = key bits of x and y.
struct VoxGrid { double o[3]; double vs; int lo[3]; int nx, ny; };

// floor((double(p) - o) / vs): an IEEE fp64 subtraction and division, nothing to contract; the host evaluates the same expression
// for the bounds (vox_index_host in sta_rows.inc) and numpy does for the tests
__device__ __forceinline__ long long vox_index(float p, double o, double vs) {
#pragma clang fp contract(off)
    const double d = (double)p - o;
    return (long long)floor(d / vs);
}
__device__ __forceinline__ bool vox_finite3(float x, float y, float z) {
    return fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f && fabsf(z) <= 3.4028234663852886e38f;   // false for NaN
}

// ---------------------------------------------------------------------------------------------------------
// Bounds.  min / max are exact and order-free, the dropped count is an integer: the result does not depend on the grid.
// part [gridDim.x][8] = {min xyz, max xyz, dropped (int bits), 0}
__global__ __launch_bounds__(256) void vox_bounds_kernel(const float* __restrict__ pts, int M, float* __restrict__ part) {
    STA_SKEW_ENTRY(714);
    const float inf = __builtin_huge_valf();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    int dropped = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < M; i += gridDim.x * 256) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (vox_finite3(x, y, z)) {
            mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
            mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
        } else ++dropped;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], o)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o)); }
        dropped += __shfl_xor(dropped, o);
    }
    __shared__ float red[4][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int a = 0; a < 3; ++a) { red[wave][a] = mn[a]; red[wave][3 + a] = mx[a]; }
        red[wave][6] = __int_as_float(dropped);
    }
    __syncthreads(); STA_SKEW(700);
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], red[w][a]); mx[a] = fmaxf(mx[a], red[w][3 + a]); }
            dropped += __float_as_int(red[w][6]);
        }
        float* o = part + 8 * (size_t)blockIdx.x;
        for (int a = 0; a < 3; ++a) { o[a] = mn[a]; o[3 + a] = mx[a]; }
        o[6] = __int_as_float(dropped); o[7] = 0.f;
    }
}
// one workgroup of 256 threads folds the n <= 1024 partial rows to out[8]
__global__ __launch_bounds__(256) void vox_bounds_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    STA_SKEW_ENTRY(715);
    const float inf = __builtin_huge_valf();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    int dropped = 0;
    for (int b = threadIdx.x; b < n; b += 256) {
        const float* p = part + 8 * (size_t)b;
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], p[a]); mx[a] = fmaxf(mx[a], p[3 + a]); }
        dropped += __float_as_int(p[6]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], o)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o)); }
        dropped += __shfl_xor(dropped, o);
    }
    __shared__ float red[4][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int a = 0; a < 3; ++a) { red[wave][a] = mn[a]; red[wave][3 + a] = mx[a]; }
        red[wave][6] = __int_as_float(dropped);
    }
    __syncthreads(); STA_SKEW(701);
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], red[w][a]); mx[a] = fmaxf(mx[a], red[w][3 + a]); }
            dropped += __float_as_int(red[w][6]);
        }
        for (int a = 0; a < 3; ++a) { out[a] = mn[a]; out[3 + a] = mx[a]; }
        out[6] = __int_as_float(dropped); out[7] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Keys.  A dropped point gets the all-ones key: the host runs enough passes that it sorts behind every voxel.
__global__ __launch_bounds__(256) void vox_key_kernel(const float* __restrict__ pts, int M, const VoxGrid g, unsigned long long* __restrict__ key,
                                                      int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    unsigned long long k = ~0ull;
    if (vox_finite3(x, y, z)) {
        const unsigned long long ix = (unsigned long long)(vox_index(x, g.o[0], g.vs) - g.lo[0]);
        const unsigned long long iy = (unsigned long long)(vox_index(y, g.o[1], g.vs) - g.lo[1]);
        const unsigned long long iz = (unsigned long long)(vox_index(z, g.o[2], g.vs) - g.lo[2]);
        k = (iz << (g.nx + g.ny)) | (iy << g.nx) | ix;
    }
    key[i] = k; idx[i] = i;
}

// ---------------------------------------------------------------------------------------------------------
// One pass of the sort on the digit (key >> shift) & 255.  Workgroup b owns keys [b * VOX_TILE, (b + 1) * VOX_TILE).
// hist [256][nblk]: digit-major, so that one exclusive scan along a row and one over the 256 row totals give every workgroup the
// first output position of each of its digits.
__global__ __launch_bounds__(256) void vox_hist_kernel(const unsigned long long* __restrict__ key, int M, int shift, int nblk, int* __restrict__ hist) {
    STA_SKEW_ENTRY(716);
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads(); STA_SKEW(702);
    const int base = blockIdx.x * VOX_TILE;
#pragma unroll
    for (int c = 0; c < VOX_TILE / 256; ++c) {
        const int i = base + c * 256 + threadIdx.x;
        if (i < M) atomicAdd(&h[(int)(key[i] >> shift) & 255], 1);         // integer LDS atomic: the counts do not depend on the order
    }
    __syncthreads(); STA_SKEW(703);
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}
// grid (256): workgroup d scans row d of hist in place (exclusive) in chunks of 256 with a carried base, total -> dtot[d]
__global__ __launch_bounds__(256) void vox_hist_scan_kernel(int* __restrict__ hist, int nblk, int* __restrict__ dtot) {
    STA_SKEW_ENTRY(717);
    __shared__ int wsum[4], tot;
    int* row = hist + (size_t)blockIdx.x * nblk;
    int run = 0;
    for (int c0 = 0; c0 < nblk; c0 += 256) {
        const int i = c0 + threadIdx.x;
        const int v = i < nblk ? row[i] : 0;
        const int incl = sel_block_scan(v, wsum);
        if (i < nblk) row[i] = run + incl - v;
        if (threadIdx.x == 255) tot = incl;
        __syncthreads(); STA_SKEW(704);
        run += tot;
        __syncthreads(); STA_SKEW(705);              // wsum and tot are rewritten by the next chunk
    }
    if (threadIdx.x == 0) dtot[blockIdx.x] = run;
}
// Stable scatter.  Per chunk of 256 keys: a lane's rank among the equal digits of its wave is the popcount of the peer ballot below
// it (eight ballots, one per digit bit, leave the lanes that hold the same digit), the waves' counts per digit go through LDS, the
// running first position of every digit is carried from chunk to chunk - the same ordered walk as patch_select_kernel's.
__global__ __launch_bounds__(256) void vox_scatter_kernel(const unsigned long long* __restrict__ kin, const int* __restrict__ iin, int M, int shift,
                                                          int nblk, const int* __restrict__ hist, const int* __restrict__ dtot,
                                                          unsigned long long* __restrict__ kout, int* __restrict__ iout) {
    STA_SKEW_ENTRY(718);
    __shared__ int base[256], wcnt[4][256], wsum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    {
        const int v = dtot[t];
        const int incl = sel_block_scan(v, wsum);
        base[t] = incl - v + hist[(size_t)t * nblk + blockIdx.x];
        wcnt[0][t] = 0; wcnt[1][t] = 0; wcnt[2][t] = 0; wcnt[3][t] = 0;
    }
    __syncthreads(); STA_SKEW(706);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int first = blockIdx.x * VOX_TILE;
    for (int c = 0; c < VOX_TILE / 256; ++c) {
        const int i = first + c * 256 + t;
        const bool valid = i < M;
        const unsigned long long k = valid ? kin[i] : 0ull;
        const int d = (int)(k >> shift) & 255;
        unsigned long long peer = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long m = __ballot(bit);
            peer &= bit ? m : ~m;
        }
        const int rank = __popcll(peer & below);
        if (valid && rank == 0) wcnt[wave][d] = __popcll(peer);
        __syncthreads(); STA_SKEW(707);
        if (valid) {
            int pos = base[d] + rank;
            for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
            kout[pos] = k; iout[pos] = iin[i];          // pos < M: the positions of a pass are a permutation of [0, M)
        }
        __syncthreads(); STA_SKEW(708);
        base[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
        wcnt[0][t] = 0; wcnt[1][t] = 0; wcnt[2][t] = 0; wcnt[3][t] = 0;
        __syncthreads(); STA_SKEW(709);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Heads and rows: two ordered compactions with the count / scan / emit structure of the cloud_* kernels (cloud_scan_kernel itself
// is the scan: int counts per workgroup of 256 -> int64 offsets, total in offs[nblk]).
// rank of a kept thread among the kept threads of its workgroup (wc: 4 ints of LDS)
__device__ __forceinline__ int vox_block_rank(bool keep, int* wc) {
    const unsigned long long b = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads(); STA_SKEW(710);
    int rank = __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += wc[w];
    return rank;
}
__device__ __forceinline__ void vox_block_count(bool keep, int* __restrict__ counts) {
    const unsigned long long b = __ballot(keep);
    __shared__ int wc[4];
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
    __syncthreads(); STA_SKEW(711);
    if (threadIdx.x == 0) counts[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}
// sorted position i < n (the kept points) starts a voxel iff its key differs from the one before
__global__ __launch_bounds__(256) void vox_head_count_kernel(const unsigned long long* __restrict__ key, int n, int* __restrict__ counts) {
    STA_SKEW_ENTRY(720);
    const int i = blockIdx.x * 256 + threadIdx.x;
    vox_block_count(i < n && (i == 0 || key[i] != key[i - 1]), counts);
}
// seg[u] = first sorted position of voxel u, seg[U] = n
__global__ __launch_bounds__(256) void vox_head_emit_kernel(const unsigned long long* __restrict__ key, int n, const int64_t* __restrict__ offs, int nblk,
                                                            int* __restrict__ seg) {
    STA_SKEW_ENTRY(721);
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool head = i < n && (i == 0 || key[i] != key[i - 1]);
    const int rank = vox_block_rank(head, wc);
    if (head) seg[offs[blockIdx.x] + rank] = i;
    if (i == 0) seg[offs[nblk]] = n;
}
// voxel u < U (U = *n_vox, device memory) becomes an output row iff it holds at least min_points points
__global__ __launch_bounds__(256) void vox_row_count_kernel(const int* __restrict__ seg, const int64_t* __restrict__ n_vox, int min_points,
                                                            int* __restrict__ counts) {
    STA_SKEW_ENTRY(722);
    const int u = blockIdx.x * 256 + threadIdx.x;
    vox_block_count(u < (int)*n_vox && seg[u + 1] - seg[u] >= min_points, counts);
}
// rows[r] = {first, end} sorted positions of output row r; rows of more than VOX_LONG points are also listed in long_rows (an
// integer counter hands out the slots: the list's order is free, every entry is reduced on its own)
__global__ __launch_bounds__(256) void vox_row_emit_kernel(const int* __restrict__ seg, const int64_t* __restrict__ n_vox, int min_points,
                                                           const int64_t* __restrict__ offs, int2* __restrict__ rows, int* __restrict__ n_long,
                                                           int* __restrict__ long_rows) {
    STA_SKEW_ENTRY(723);
    __shared__ int wc[4];
    const int u = blockIdx.x * 256 + threadIdx.x;
    int s = 0, e = 0;
    const bool in = u < (int)*n_vox;
    if (in) { s = seg[u]; e = seg[u + 1]; }
    const bool keep = in && e - s >= min_points;
    const int rank = vox_block_rank(keep, wc);
    if (!keep) return;
    const int r = (int)offs[blockIdx.x] + rank;
    rows[r] = make_int2(s, e);
    if (e - s > VOX_LONG) long_rows[atomicAdd(n_long, 1)] = r;          // at most n / VOX_LONG such rows: inside the list
}

// ---------------------------------------------------------------------------------------------------------
// Reduce.  The order of the fp64 additions of a row depends on its length alone: lane (thread) l adds the points l, l + L, l + 2 L, ...
// of the row in ascending order (L = 64 lanes for a row of at most VOX_LONG points, 1024 threads above), then a xor butterfly over
// the 64 lanes, then - long rows - the 16 wave sums in ascending order.  Inside a row the sorted payload is the ascending input index.
struct VoxOut {
    const float* pts; const float* col;                 // inputs [M,3]; col may be NULL (colour sums stay 0)
    const unsigned long long* key; const int* idx;      // sorted
    const int2* rows; int V;
    VoxGrid g;
    float* pts_out; float* col_out; int* counts_out; int* index_out; int* inverse_out; uint8_t* rec;    // any may be NULL
};
__device__ __forceinline__ void vox_gather(const VoxOut& p, int first, int end, int stride, int row, double* acc) {
    for (int i = first; i < end; i += stride) {
        const int j = p.idx[i];
        acc[0] += (double)p.pts[3 * (size_t)j]; acc[1] += (double)p.pts[3 * (size_t)j + 1]; acc[2] += (double)p.pts[3 * (size_t)j + 2];
        if (p.col) { acc[3] += (double)p.col[3 * (size_t)j]; acc[4] += (double)p.col[3 * (size_t)j + 1]; acc[5] += (double)p.col[3 * (size_t)j + 2]; }
        if (p.inverse_out) p.inverse_out[j] = row;
    }
}
__device__ __forceinline__ void vox_wave_sum(double* acc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] += __shfl_xor(acc[q], o);       // a + b on both sides: every lane holds the same bits
    }
}
// mean = fp64 sum / fp64 count, rounded once to fp32; the voxel index comes back out of the row's key
__device__ __forceinline__ void vox_write_row(const VoxOut& p, int row, int s, int e, const double* acc) {
    const double n = (double)(e - s);
    const float x = (float)(acc[0] / n), y = (float)(acc[1] / n), z = (float)(acc[2] / n);
    const float cr = (float)(acc[3] / n), cg = (float)(acc[4] / n), cb = (float)(acc[5] / n);
    const size_t r = (size_t)row;
    if (p.pts_out) { p.pts_out[3 * r] = x; p.pts_out[3 * r + 1] = y; p.pts_out[3 * r + 2] = z; }
    if (p.col_out) { p.col_out[3 * r] = cr; p.col_out[3 * r + 1] = cg; p.col_out[3 * r + 2] = cb; }
    if (p.counts_out) p.counts_out[r] = e - s;
    if (p.index_out) {
        const unsigned long long k = p.key[s];
        p.index_out[3 * r] = (int)(k & ((1ull << p.g.nx) - 1ull)) + p.g.lo[0];
        p.index_out[3 * r + 1] = (int)((k >> p.g.nx) & ((1ull << p.g.ny) - 1ull)) + p.g.lo[1];
        p.index_out[3 * r + 2] = (int)(k >> (p.g.nx + p.g.ny)) + p.g.lo[2];
    }
    if (p.rec) cloud_write_record(p.rec + r * 27, x, y, z, cr, cg, cb);
}
// one wave per row, four rows per workgroup; long rows are left to vox_reduce_long_kernel
__global__ __launch_bounds__(256) void vox_reduce_kernel(const VoxOut p) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= p.V) return;
    const int2 se = p.rows[row];
    if (se.y - se.x > VOX_LONG) return;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    vox_gather(p, se.x + lane, se.y, 64, row, acc);
    vox_wave_sum(acc);
    if (lane == 0) vox_write_row(p, row, se.x, se.y, acc);
}
// one workgroup of 1024 threads per long row, walking the list
__global__ __launch_bounds__(1024) void vox_reduce_long_kernel(const VoxOut p, const int* __restrict__ n_long, const int* __restrict__ long_rows) {
    STA_SKEW_ENTRY(719);
    __shared__ double part[16][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = *n_long;
    for (int slot = blockIdx.x; slot < n; slot += gridDim.x) {
        const int row = long_rows[slot];
        const int2 se = p.rows[row];
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        vox_gather(p, se.x + (int)threadIdx.x, se.y, 1024, row, acc);
        vox_wave_sum(acc);
        if (lane == 0) { for (int q = 0; q < 6; ++q) part[wave][q] = acc[q]; }
        __syncthreads(); STA_SKEW(712);
        if (threadIdx.x == 0) {
#pragma unroll 1
            for (int w = 1; w < 16; ++w) { for (int q = 0; q < 6; ++q) acc[q] += part[w][q]; }
            vox_write_row(p, row, se.x, se.y, acc);
        }
        __syncthreads(); STA_SKEW(713);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Host side, shared by every translation unit that sorts or scans (sta_rows.inc and the handle-free libraries): the two layouts, their
// takers and the launch code.  B is any bump with `void* take(int64_t bytes)`; the take order is part of every workspace's layout.
struct VoxSort { unsigned long long* key[2]; int* idx[2]; int* hist; int* dtot; };      // m keys and payloads, twice; the pass's histogram
struct VoxScan { int* counts; int64_t* offs; };                                         // counts[nblk], offs[nblk + 1]: offs[nblk] = the total

// own_idx0 = false: idx[0] lives elsewhere (libsta_cloud.so sorts its payload into the index buffer) and is the caller's to set
template <class B> static void vox_take_sort(B& b, int64_t m, VoxSort* L, bool own_idx0 = true) {
    const int64_t nbs = (m + VOX_TILE - 1) / VOX_TILE;
    L->key[0] = (unsigned long long*)b.take(m * 8);
    L->key[1] = (unsigned long long*)b.take(m * 8);
    L->idx[0] = own_idx0 ? (int*)b.take(m * 4) : nullptr;
    L->idx[1] = (int*)b.take(m * 4);
    L->hist = (int*)b.take(256 * nbs * 4);
    L->dtot = (int*)b.take(256 * 4);
}
template <class B> static void vox_take_scan(B& b, int64_t nblk, VoxScan* S) {
    S->counts = (int*)b.take(nblk * 4);
    S->offs = (int64_t*)b.take((nblk + 1) * 8);
}

// The stable LSD sort of m keys and payloads on the digits 0 .. passes - 1, from key[cur] / idx[cur]; returns the buffer (0 or 1) that
// holds the result: cur after an even number of passes.  The caller counts the passes its keys need.
static inline int vox_sort(hipStream_t st, const VoxSort& L, int m, int passes, int cur = 0) {
    const int nbs = (m + VOX_TILE - 1) / VOX_TILE;
    for (int p = 0; p < passes; ++p, cur ^= 1) {
        const int a = cur, b = cur ^ 1;
        hipLaunchKernelGGL(vox_hist_kernel, dim3(nbs), dim3(256), 0, st, (const unsigned long long*)L.key[a], m, 8 * p, nbs, L.hist);
        hipLaunchKernelGGL(vox_hist_scan_kernel, dim3(256), dim3(256), 0, st, L.hist, nbs, L.dtot);
        hipLaunchKernelGGL(vox_scatter_kernel, dim3(nbs), dim3(256), 0, st, (const unsigned long long*)L.key[a], (const int*)L.idx[a], m, 8 * p, nbs,
                           (const int*)L.hist, (const int*)L.dtot, L.key[b], L.idx[b]);
    }
    return cur;
}
// The exclusive scan of counts[nblk] into offs[nblk + 1] by cloud_scan_kernel (elementwise.h), which reads these three fields alone.
static inline void vox_scan(hipStream_t st, int* counts, int64_t* offs, int nblk) {
    CloudParams sc{};
    sc.counts = counts; sc.offs = offs; sc.nblk = nblk;
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), dim3(1024), 0, st, sc);
}
