// Sparse TSDF fusion and marching tetrahedra (libsta_tsdf.so; the contract is in include/sta_tsdf.h), included by sta_tsdf.hip after
// elementwise.h (cloud_scan_kernel), select.h (sel_block_scan) and voxel.h (the radix sort, vox_block_count / vox_block_rank).
// No table to size, no floating-point atomics: every output is defined by the inputs alone.
//   ts_key_kernel                                 eight block keys per pixel (the sentinel for what does not count), the two counters
//   ts_head_count_kernel / ts_head_emit_kernel    ordered compaction of the sorted keys to the distinct ones (cloud_scan_kernel between)
//   ts_clear_kernel
//   ts_integrate_kernel                           one workgroup per block, one thread per lattice point, the view loop inside
//   ts_mesh_mask_kernel                           per block: which of the 7 edges of every lattice point carry a vertex, their prefix,
//                                                 the block's vertex and triangle counts (cloud_scan_kernel over both afterwards)
//   ts_mesh_emit_kernel                           per block: vertices and triangles at their final positions
#pragma once
#pragma clang fp contract(off)

#define TS_BIAS 1048576ll
#define TS_FIELD 0x1FFFFFull
#define TS_SENTINEL 0xFFFFFFFFFFFFFFFFull

// ---------------------------------------------------------------------------------------------------------
// The case table, generated at compile time by the rule of the header (tests/tsdf_cases.py generates it again in numpy).
// e[t][m] = {triangles, six codes 4 * inside corner + outside corner or -1}; cv[t][k] = corner k of tetrahedron t in the unit cube.
struct TsTable { signed char e[6][16][7]; signed char cv[6][4][3]; };
constexpr TsTable ts_make_table() {
    TsTable T{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int t = 0; t < 6; ++t) {
        int cv[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}};
        cv[1][perm[t][0]] = 1;
        cv[2][perm[t][0]] = 1; cv[2][perm[t][1]] = 1;
        for (int k = 0; k < 4; ++k) { for (int a = 0; a < 3; ++a) T.cv[t][k][a] = (signed char)cv[k][a]; }
        for (int m = 0; m < 16; ++m) {
            for (int q = 0; q < 7; ++q) T.e[t][m][q] = (signed char)(q == 0 ? 0 : -1);
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, nin = 0, nout = 0;
            for (int k = 0; k < 4; ++k) { if ((m >> k) & 1) in[nin++] = k; else out[nout++] = k; }
            if (nin == 0 || nout == 0) continue;
            int tri[2][3][2] = {}, ntri = 1;
            if (nin == 1) { for (int q = 0; q < 3; ++q) { tri[0][q][0] = in[0]; tri[0][q][1] = out[q]; } }
            else if (nin == 3) { for (int q = 0; q < 3; ++q) { tri[0][q][0] = in[q]; tri[0][q][1] = out[0]; } }
            else {
                ntri = 2;
                tri[0][0][0] = in[0]; tri[0][0][1] = out[0]; tri[0][1][0] = in[0]; tri[0][1][1] = out[1]; tri[0][2][0] = in[1]; tri[0][2][1] = out[1];
                tri[1][0][0] = in[0]; tri[1][0][1] = out[0]; tri[1][1][0] = in[1]; tri[1][1][1] = out[1]; tri[1][2][0] = in[1]; tri[1][2][1] = out[0];
            }
            int dir[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                for (int k = 0; k < nout; ++k) dir[a] += nin * cv[out[k]][a];
                for (int k = 0; k < nin; ++k) dir[a] -= nout * cv[in[k]][a];
            }
            for (int r = 0; r < ntri; ++r) {
                int P[3][3] = {};
                for (int q = 0; q < 3; ++q) { for (int a = 0; a < 3; ++a) P[q][a] = cv[tri[r][q][0]][a] + cv[tri[r][q][1]][a]; }
                const int ux = P[1][0] - P[0][0], uy = P[1][1] - P[0][1], uz = P[1][2] - P[0][2];
                const int wx = P[2][0] - P[0][0], wy = P[2][1] - P[0][1], wz = P[2][2] - P[0][2];
                const int s = (uy * wz - uz * wy) * dir[0] + (uz * wx - ux * wz) * dir[1] + (ux * wy - uy * wx) * dir[2];
                const int order[3] = {0, s < 0 ? 2 : 1, s < 0 ? 1 : 2};
                for (int q = 0; q < 3; ++q) T.e[t][m][1 + 3 * r + q] = (signed char)(4 * tri[r][order[q]][0] + tri[r][order[q]][1]);
            }
            T.e[t][m][0] = (signed char)ntri;
        }
    }
    return T;
}
static constexpr TsTable ts_table_host = ts_make_table();
__constant__ const TsTable ts_table = ts_make_table();

// ---------------------------------------------------------------------------------------------------------
struct TsGrid { double o[3]; double vs, trunc, depth_max; };

// the header's OBSERVED; D = double(depth) * double(scale)
__device__ __forceinline__ bool ts_observed(float ob, float dep, float sc, double depth_max, double* D) {
    const double d = (double)dep * (double)sc;
    *D = d;
    return ob > 0.f && d > 0.0 && d <= depth_max && d < __builtin_huge_val();
}
__device__ __forceinline__ void ts_wave_count(bool flag, unsigned long long* counter) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (unsigned long long)__popcll(b));     // integer: order-free
}

// key [8 n]: slot s = 4 sz + 2 sy + sx of pixel i is the corner with + trunc on the axes whose bit is set
__global__ __launch_bounds__(256) void ts_key_kernel(const float* __restrict__ depths, const float* __restrict__ scales, const double* __restrict__ K,
                                                     const double* __restrict__ c2w, const float* __restrict__ obs, int n, int HW, int W, const TsGrid g,
                                                     unsigned long long* __restrict__ key, unsigned long long* __restrict__ counters) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    bool seen = false, dropped = false;
    long long blo[3] = {0, 0, 0}, bhi[3] = {0, 0, 0};
    if (i < n) {
        const int v = i / HW, pix = i - v * HW, iy = pix / W, ix = pix - iy * W;
        double D;
        seen = ts_observed(obs[i], depths[i], scales[v], g.depth_max, &D);
        if (seen) {
            const double* Kv = K + 4 * (size_t)v;
            const double* T = c2w + 12 * (size_t)v;
            const double lx = ((double)ix - Kv[2]) / Kv[0] * D, ly = ((double)iy - Kv[3]) / Kv[1] * D, lz = D;
            const double P[3] = {((T[0] * lx + T[1] * ly) + T[2] * lz) + T[3], ((T[4] * lx + T[5] * ly) + T[6] * lz) + T[7],
                                 ((T[8] * lx + T[9] * ly) + T[10] * lz) + T[11]};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double flo = floor(((P[a] - g.trunc) - g.o[a]) / g.vs), fhi = floor(((P[a] + g.trunc) - g.o[a]) / g.vs);
                if (!(flo >= -8388608.0 && flo < 8388608.0 && fhi >= -8388608.0 && fhi < 8388608.0)) dropped = true;        // a NaN fails
                else { blo[a] = (long long)flo >> 3; bhi[a] = (long long)fhi >> 3; }
            }
        }
    }
    ts_wave_count(seen, counters);
    ts_wave_count(dropped, counters + 1);
    if (i >= n) return;
    unsigned long long* out = key + 8 * (size_t)i;
    const bool live = seen && !dropped;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        unsigned long long k = TS_SENTINEL;
        // a corner repeats an earlier one of this pixel iff on an axis with its bit set both ends fall into one block
        const bool dup = ((s & 1) && bhi[0] == blo[0]) || ((s & 2) && bhi[1] == blo[1]) || ((s & 4) && bhi[2] == blo[2]);
        if (live && !dup) {
            const unsigned long long bx = (unsigned long long)(((s & 1) ? bhi[0] : blo[0]) + TS_BIAS);
            const unsigned long long by = (unsigned long long)(((s & 2) ? bhi[1] : blo[1]) + TS_BIAS);
            const unsigned long long bz = (unsigned long long)(((s & 4) ? bhi[2] : blo[2]) + TS_BIAS);
            k = (bz << 42) | (by << 21) | bx;
        }
        out[s] = k;
    }
}

// sorted position i starts a block iff its key is no sentinel and differs from the one before
__global__ __launch_bounds__(256) void ts_head_count_kernel(const unsigned long long* __restrict__ key, int n, int* __restrict__ counts) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    vox_block_count(i < n && key[i] != TS_SENTINEL && (i == 0 || key[i] != key[i - 1]), counts);
}
__global__ __launch_bounds__(256) void ts_head_emit_kernel(const unsigned long long* __restrict__ key, int n, const int64_t* __restrict__ offs,
                                                           long long max_blocks, unsigned long long* __restrict__ keys_out) {
    __shared__ int wc[4];
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    const bool head = i < n && key[i] != TS_SENTINEL && (i == 0 || key[i] != key[i - 1]);
    const int rank = vox_block_rank(head, wc);
    if (!head) return;
    const long long r = (long long)offs[blockIdx.x] + rank;
    if (r < max_blocks) keys_out[r] = key[i];
}

__global__ __launch_bounds__(256) void ts_clear_kernel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ rgb, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    tsdf[i] = 1.f; weight[i] = 0.f;
    if (rgb) { rgb[3 * i] = 0.f; rgb[3 * i + 1] = 0.f; rgb[3 * i + 2] = 0.f; }
}

// ---------------------------------------------------------------------------------------------------------
// Integration.
struct TsInt {
    const unsigned long long* keys; float* tsdf; float* weight; float* rgb;
    const float* depths; const float* scales; const double* K; const double* w2c; const float* obs; const float* imgs;
    int H, W, v0, v1;
    double o[3]; double vs, trunc, depth_max, max_weight;
};

// Can a lattice point of the block with centre h (radius rad around it, already padded) pass the header's pc_z and pixel-range tests in
// this view?  Conservative: false only when every point provably fails one of them, true for anything that cannot be bounded (a NaN, a
// sphere that reaches the camera plane, a focal length that is not positive).  The bound on the camera coordinates is the sphere of
// radius |T|_F * rad around the centre's, widened by 1e-9 of the magnitudes that enter the sums - seven orders above their rounding.
__device__ __forceinline__ bool ts_view_may_touch(const double* __restrict__ Kv, const double* __restrict__ T, int H, int W, double hx, double hy, double hz,
                                                  double rad) {
    const double cx = ((T[0] * hx + T[1] * hy) + T[2] * hz) + T[3], cy = ((T[4] * hx + T[5] * hy) + T[6] * hz) + T[7];
    const double cz = ((T[8] * hx + T[9] * hy) + T[10] * hz) + T[11];
    double nf = 0.0, mag = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        nf += T[4 * r] * T[4 * r] + T[4 * r + 1] * T[4 * r + 1] + T[4 * r + 2] * T[4 * r + 2];
        mag += fabs(T[4 * r] * hx) + fabs(T[4 * r + 1] * hy) + fabs(T[4 * r + 2] * hz) + fabs(T[4 * r + 3]);
    }
    const double R = sqrt(nf) * rad * 1.000001 + 1e-9 * mag;
    if (!(R < 1e300)) return true;
    const double zmax = cz + R, zmin = cz - R;
    if (zmax <= 0.0) return false;                       // every pc_z <= 0
    if (!(zmin > 0.0) || !(Kv[0] > 0.0) || !(Kv[1] > 0.0)) return true;
    const double c[2] = {cx, cy};
    const int lim[2] = {W, H};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double lo = c[a] - R, hi = c[a] + R;
        const double rmax = hi >= 0.0 ? hi / zmin : hi / zmax, rmin = lo >= 0.0 ? lo / zmax : lo / zmin;
        const double umax = Kv[a] * rmax + Kv[2 + a], umin = Kv[a] * rmin + Kv[2 + a];
        const double slop = 2.0 + 1e-9 * (fabs(Kv[a] * rmax) + fabs(Kv[a] * rmin) + fabs(Kv[2 + a]));
        if (umax < -slop) return false;                  // every floor(u + 0.5) < 0
        if (umin > (double)(lim[a] - 1) + slop) return false;
    }
    return true;
}

__global__ __launch_bounds__(512) void ts_integrate_kernel(const TsInt p) {
    __shared__ unsigned long long live[8];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long key = p.keys[blockIdx.x];
    const long long bx = (long long)(key & TS_FIELD) - TS_BIAS, by = (long long)((key >> 21) & TS_FIELD) - TS_BIAS,
                    bz = (long long)((key >> 42) & TS_FIELD) - TS_BIAS;
    const double x = p.o[0] + (double)(8 * bx + (t & 7)) * p.vs, y = p.o[1] + (double)(8 * by + ((t >> 3) & 7)) * p.vs,
                 z = p.o[2] + (double)(8 * bz + (t >> 6)) * p.vs;
    const double hx = p.o[0] + ((double)(8 * bx) + 3.5) * p.vs, hy = p.o[1] + ((double)(8 * by) + 3.5) * p.vs, hz = p.o[2] + ((double)(8 * bz) + 3.5) * p.vs;
    const double rad = 6.07 * p.vs;                      // > 3.5 * sqrt(3) voxels
    const size_t cell = (size_t)blockIdx.x * 512 + t;
    const bool colour = p.rgb != nullptr && p.imgs != nullptr;
    const size_t HW = (size_t)p.H * p.W;
    float ts = p.tsdf[cell], wt = p.weight[cell], col[3] = {0.f, 0.f, 0.f};
    if (colour) { col[0] = p.rgb[3 * cell]; col[1] = p.rgb[3 * cell + 1]; col[2] = p.rgb[3 * cell + 2]; }
    const double wmax = (double)(p.W - 1), hmax = (double)(p.H - 1);
    for (int base = p.v0; base < p.v1; base += 512) {
        // the block's frustum test of 512 views at once, one view per thread -> eight 64-bit masks
        const int vt = base + t;
        const bool keep = vt < p.v1 && ts_view_may_touch(p.K + 4 * (size_t)vt, p.w2c + 12 * (size_t)vt, p.H, p.W, hx, hy, hz, rad);
        const unsigned long long b = __ballot(keep);
        if (lane == 0) live[wave] = b;
        __syncthreads();
#pragma unroll 1
        for (int gq = 0; gq < 8; ++gq) {
            const unsigned long long mv = live[gq];
            // the mask is the same in every lane: hand it to the scalar unit, so that the loop, v and the view's 16 doubles are scalar
            unsigned long long m = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(mv >> 32)) << 32) |
                                   (unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)mv);
            while (m) {
                const int v = base + 64 * gq + __builtin_ctzll(m);
                m &= m - 1;
                const double* __restrict__ T = p.w2c + 12 * (size_t)v;
                const double* __restrict__ Kv = p.K + 4 * (size_t)v;
                const double pcz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
                if (!(pcz > 0.0)) continue;
                const double pcx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3], pcy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
                const double u = Kv[0] * (pcx / pcz) + Kv[2], w_ = Kv[1] * (pcy / pcz) + Kv[3];
                const double px = floor(u + 0.5), py = floor(w_ + 0.5);
                if (!(px >= 0.0 && px <= wmax && py >= 0.0 && py <= hmax)) continue;
                const size_t pix = (size_t)(int)py * p.W + (size_t)(int)px;
                const float ob = p.obs[(size_t)v * HW + pix];
                double D;
                if (!ts_observed(ob, p.depths[(size_t)v * HW + pix], p.scales[v], p.depth_max, &D)) continue;
                const double sdf = D - pcz;
                if (sdf < -p.trunc) continue;
                const double d = fmin(sdf / p.trunc, 1.0), w = (double)ob, Wo = (double)wt, den = Wo + w;
                ts = (float)((Wo * (double)ts + w * d) / den);
                if (colour) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const double c = ((double)p.imgs[((size_t)v * 3 + ch) * HW + pix] + 1.0) * 0.5;
                        col[ch] = (float)((Wo * (double)col[ch] + w * c) / den);
                    }
                }
                wt = (float)fmin(den, p.max_weight);
            }
        }
        __syncthreads();                                 // live is rewritten by the next chunk
    }
    p.tsdf[cell] = ts; p.weight[cell] = wt;
    if (colour) { p.rgb[3 * cell] = col[0]; p.rgb[3 * cell + 1] = col[1]; p.rgb[3 * cell + 2] = col[2]; }
}

// ---------------------------------------------------------------------------------------------------------
// Mesh.
struct TsMesh {
    const unsigned long long* keys; int nb;
    const float* tsdf; const float* weight; const float* rgb;
    double o[3]; double vs, min_weight;
};

// rank of the block (dx, dy, dz) away from the one with this key, -1 if it is not in keys or outside the key's fields
__device__ __forceinline__ int ts_neighbour(const unsigned long long* __restrict__ keys, int nb, unsigned long long key, int dx, int dy, int dz) {
    const long long fx = (long long)(key & TS_FIELD) + dx, fy = (long long)((key >> 21) & TS_FIELD) + dy, fz = (long long)((key >> 42) & TS_FIELD) + dz;
    if (fx < 0 || fy < 0 || fz < 0 || fx > (long long)TS_FIELD || fy > (long long)TS_FIELD || fz > (long long)TS_FIELD) return -1;
    const unsigned long long k = ((unsigned long long)fz << 42) | ((unsigned long long)fy << 21) | (unsigned long long)fx;
    int lo = 0, hi = nb;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < nb && keys[lo] == k ? lo : -1;
}
// 0 unknown, 1 known and outside, 2 inside
__device__ __forceinline__ int ts_state(const TsMesh& p, size_t cell) {
    if (!((double)p.weight[cell] >= p.min_weight)) return 0;
    return p.tsdf[cell] < 0.f ? 2 : 1;
}
// case of tetrahedron t of the cube with base (cx, cy, cz) in a halo of side S, -1 unless its four corners are known
template <int S>
__device__ __forceinline__ int ts_case(const unsigned char* st, int cx, int cy, int cz, int t) {
    int m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = st[((cz + ts_table.cv[t][k][2]) * S + (cy + ts_table.cv[t][k][1])) * S + (cx + ts_table.cv[t][k][0])];
        if (s == 0) return -1;
        m |= (s == 2) << k;
    }
    return m;
}
// the vertex of code 4 i + j in tetrahedron t: the corner that owns it (offset in the cube) and its type
__device__ __forceinline__ void ts_edge(int t, int code, int* ox, int* oy, int* oz, int* type) {
    const int i = code >> 2, j = code & 3, lo = i < j ? i : j, hi = i < j ? j : i;
    *ox = ts_table.cv[t][lo][0]; *oy = ts_table.cv[t][lo][1]; *oz = ts_table.cv[t][lo][2];
    *type = (ts_table.cv[t][hi][0] - *ox) + 2 * (ts_table.cv[t][hi][1] - *oy) + 4 * (ts_table.cv[t][hi][2] - *oz) - 1;
}

// Halo of 10^3 states (lattice points -1 .. 8 of the block), all 9^3 cubes with a corner among the block's own points: every emitted
// tetrahedron ORs the types of its vertices into the mask of their owners (integer LDS atomics; only the block's own points are kept).
__global__ __launch_bounds__(256) void ts_mesh_mask_kernel(const TsMesh p, unsigned char* __restrict__ mask_out, unsigned short* __restrict__ pre_out,
                                                           int* __restrict__ vcnt, int* __restrict__ tcnt) {
    __shared__ int nr[27], mask[512], wsum[4], tri_total;
    __shared__ unsigned char st[1000];
    const int t = threadIdx.x, rank = blockIdx.x;
    if (t < 27) nr[t] = t == 13 ? rank : ts_neighbour(p.keys, p.nb, p.keys[rank], t % 3 - 1, (t / 3) % 3 - 1, t / 9 - 1);
    mask[t] = 0; mask[t + 256] = 0;
    if (t == 0) tri_total = 0;
    __syncthreads();
    for (int h = t; h < 1000; h += 256) {
        const int gx = h % 10 - 1, gy = (h / 10) % 10 - 1, gz = h / 100 - 1;
        const int r = nr[((gx + 8) >> 3) + 3 * ((gy + 8) >> 3) + 9 * ((gz + 8) >> 3)];
        st[h] = (unsigned char)(r >= 0 ? ts_state(p, (size_t)r * 512 + (((gz & 7) * 8 + (gy & 7)) * 8 + (gx & 7))) : 0);
    }
    __syncthreads();
    int ntri = 0;
    for (int q = t; q < 729; q += 256) {
        const int cx = q % 9, cy = (q / 9) % 9, cz = q / 81;           // halo coordinates of the base: lattice point cx - 1, ...
        const bool own = cx >= 1 && cy >= 1 && cz >= 1;
#pragma unroll 1
        for (int tet = 0; tet < 6; ++tet) {
            const int m = ts_case<10>(st, cx, cy, cz, tet);
            if (m <= 0 || m == 15) continue;
            const int n = ts_table.e[tet][m][0];
            if (own) ntri += n;
            for (int k = 0; k < 3 * n; ++k) {
                int ox, oy, oz, type;
                ts_edge(tet, ts_table.e[tet][m][1 + k], &ox, &oy, &oz, &type);
                const int ax = cx + ox - 1, ay = cy + oy - 1, az = cz + oz - 1;
                if (ax >= 0 && ax < 8 && ay >= 0 && ay < 8 && az >= 0 && az < 8) atomicOr(&mask[(az * 8 + ay) * 8 + ax], 1 << type);
            }
        }
    }
    if (ntri) atomicAdd(&tri_total, ntri);
    __syncthreads();
    const int m0 = mask[2 * t], m1 = mask[2 * t + 1], c0 = __popc(m0), c1 = __popc(m1);
    const int incl = sel_block_scan(c0 + c1, wsum);
    const size_t g = (size_t)rank * 512 + 2 * t;
    mask_out[g] = (unsigned char)m0; mask_out[g + 1] = (unsigned char)m1;
    pre_out[g] = (unsigned short)(incl - c0 - c1); pre_out[g + 1] = (unsigned short)(incl - c1);
    if (t == 255) vcnt[rank] = incl;
    if (t == 0) tcnt[rank] = tri_total;
}

// Halo of 9^3 states and values (lattice points 0 .. 8).  Vertices: a thread writes those of two lattice points.  Triangles: a thread
// owns two cubes, the counts are scanned over the workgroup, the vertex ids come from the owners' masks and prefixes.
__global__ __launch_bounds__(256) void ts_mesh_emit_kernel(const TsMesh p, const unsigned char* __restrict__ mask, const unsigned short* __restrict__ pre,
                                                           const int64_t* __restrict__ voffs, const int64_t* __restrict__ toffs, float* __restrict__ verts,
                                                           float* __restrict__ cols, int* __restrict__ tris) {
    __shared__ int nr[8], wsum[4];
    __shared__ unsigned char st[729];
    __shared__ float val[729];
    const int t = threadIdx.x, rank = blockIdx.x;
    const unsigned long long key = p.keys[rank];
    if (t < 8) nr[t] = t == 0 ? rank : ts_neighbour(p.keys, p.nb, key, t & 1, (t >> 1) & 1, t >> 2);
    __syncthreads();
    for (int h = t; h < 729; h += 256) {
        const int gx = h % 9, gy = (h / 9) % 9, gz = h / 81;
        const int r = nr[(gx >> 3) + 2 * (gy >> 3) + 4 * (gz >> 3)];
        int s = 0; float v = 0.f;
        if (r >= 0) {
            const size_t cell = (size_t)r * 512 + (((gz & 7) * 8 + (gy & 7)) * 8 + (gx & 7));
            s = ts_state(p, cell); v = p.tsdf[cell];
        }
        st[h] = (unsigned char)s; val[h] = v;
    }
    __syncthreads();
    const long long bx = (long long)(key & TS_FIELD) - TS_BIAS, by = (long long)((key >> 21) & TS_FIELD) - TS_BIAS,
                    bz = (long long)((key >> 42) & TS_FIELD) - TS_BIAS;
    if (verts) {
        for (int e = 0; e < 2; ++e) {
            const int l = 2 * t + e, lx = l & 7, ly = (l >> 3) & 7, lz = l >> 6;
            const size_t g = (size_t)rank * 512 + l;
            const int m = mask[g];
            if (!m) continue;
            long long vid = (long long)voffs[rank] + pre[g];
            const double da = (double)val[(lz * 9 + ly) * 9 + lx];
            const double ax = (double)(8 * bx + lx), ay = (double)(8 * by + ly), az = (double)(8 * bz + lz);
            for (int type = 0; type < 7; ++type) {
                if (!((m >> type) & 1)) continue;
                const int dx = (type + 1) & 1, dy = ((type + 1) >> 1) & 1, dz = (type + 1) >> 2;
                const int ex = lx + dx, ey = ly + dy, ez = lz + dz;
                const double db = (double)val[(ez * 9 + ey) * 9 + ex];
                const double tt = da / (da - db);
                verts[3 * vid] = (float)(p.o[0] + (ax + (dx ? tt : 0.0)) * p.vs);
                verts[3 * vid + 1] = (float)(p.o[1] + (ay + (dy ? tt : 0.0)) * p.vs);
                verts[3 * vid + 2] = (float)(p.o[2] + (az + (dz ? tt : 0.0)) * p.vs);
                if (cols) {
                    const int rb = nr[(ex >> 3) + 2 * (ey >> 3) + 4 * (ez >> 3)];         // the other end is known: its block exists
                    const size_t gb = (size_t)(rb < 0 ? rank : rb) * 512 + (((ez & 7) * 8 + (ey & 7)) * 8 + (ex & 7));
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const double ca = (double)p.rgb[3 * g + ch], cb = (double)p.rgb[3 * gb + ch];
                        cols[3 * vid + ch] = (float)(ca + tt * (cb - ca));
                    }
                }
                ++vid;
            }
        }
    }
    if (!tris) return;
    int cnt = 0;
    for (int e = 0; e < 2; ++e) {
        const int l = 2 * t + e, cx = l & 7, cy = (l >> 3) & 7, cz = l >> 6;
#pragma unroll 1
        for (int tet = 0; tet < 6; ++tet) {
            const int m = ts_case<9>(st, cx, cy, cz, tet);
            if (m > 0 && m < 15) cnt += ts_table.e[tet][m][0];
        }
    }
    const int incl = sel_block_scan(cnt, wsum);
    if (!cnt) return;
    long long tid = (long long)toffs[rank] + (incl - cnt);
    for (int e = 0; e < 2; ++e) {
        const int l = 2 * t + e, cx = l & 7, cy = (l >> 3) & 7, cz = l >> 6;
#pragma unroll 1
        for (int tet = 0; tet < 6; ++tet) {
            const int m = ts_case<9>(st, cx, cy, cz, tet);
            if (m <= 0 || m == 15) continue;
            const int n = ts_table.e[tet][m][0];
            for (int k = 0; k < 3 * n; ++k) {
                int ox, oy, oz, type;
                ts_edge(tet, ts_table.e[tet][m][1 + k], &ox, &oy, &oz, &type);
                const int ax = cx + ox, ay = cy + oy, az = cz + oz;
                const int r = nr[(ax >> 3) + 2 * (ay >> 3) + 4 * (az >> 3)];                // the owner is known: its block exists
                const size_t g = (size_t)(r < 0 ? rank : r) * 512 + (((az & 7) * 8 + (ay & 7)) * 8 + (ax & 7));
                tris[3 * tid + k] = (int)((long long)voffs[r < 0 ? rank : r] + pre[g] + __popc(mask[g] & ((1 << type) - 1)));
            }
            tid += n;
        }
    }
}
