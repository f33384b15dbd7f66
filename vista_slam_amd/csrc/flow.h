// The keyframe gate: Shi-Tomasi corners and pyramidal Lucas-Kanade flow (sta_flow_pyramid / sta_flow_corners / sta_flow_track; the
// contract is in include/sta_mi355.h), included by sta_api.hip after select.h and voxel.h (the stable radix sort of voxel.h orders the
// corner candidates); launch code in sta_rows.inc.  Integer arithmetic wherever the contract is integer, float64 with contraction
// off for the per-point solve: every output is defined by the input alone.
//   flow_pyrdown_kernel     one level from the level below (5x5 binomial, reflect-101), tiles of 35x35 source pixels in LDS; the first
//                           launch of a pyramid also converts the frame (uint8 copy or fp32 -> uint8) and writes level 0
//   flow_response_kernel    Sobel products and their box sums from one LDS tile -> the integer minimal-eigenvalue response, integer max
//   flow_key_kernel         candidates (R > 0, quality, 3x3 maximum) -> sort keys ((Rmax - R) << index bits) | pixel, all ones otherwise
//   flow_rank_kernel        sorted order -> the rank map [H, W]
//   flow_suppress_kernel    the sequential greedy suppression in rounds, one workgroup, the first max_corners accepted in rank order
//   flow_track_kernel       one wave per (point, frame): template in registers, source patch in LDS, float64 scalars in every lane
//   flow_stats_kernel       per frame: n, the number of tracked points, the sum of their float64 displacements in a fixed order
#pragma once
#include "sta_skew.h"       // STA_SKEW points: nothing unless -DSTA_WAVE_SKEW (libsta_mi355_skew.so)

#define FLOW_MAX_LEVELS 4
#define FLOW_MAX_WIN 21
#define FLOW_MAX_FRAMES 32
#define FLOW_MAX_PIXELS (1 << 21)
#define FLOW_R_BITS 27            // R <= 2 * 49 * (4 * 255)^2 < 2^27
#define FLOW_MAX_MIN_DISTANCE 32
#define FLOW_W_BITS 14

struct FlowLevels { int levels; int h[FLOW_MAX_LEVELS], w[FLOW_MAX_LEVELS]; long long off[FLOW_MAX_LEVELS]; long long bytes; };

// periodic reflect-101 into [0, n)
__device__ __forceinline__ int flow_reflect(int i, int n) {
    if (n == 1) return 0;
    const int m = 2 * (n - 1);
    i %= m;
    if (i < 0) i += m;
    return i >= n ? m - i : i;
}
// uint8(trunc(fp32 * 255.0f)) as the reference converts its grey frame; values outside [0, 1] (and NaN) are clamped into the byte
__device__ __forceinline__ int flow_to_u8(float v) {
    const float s = v * 255.0f;
    return s >= 255.0f ? 255 : (s > 0.0f ? (int)s : 0);
}

// ---------------------------------------------------------------------------------------------------------
// Pyramid.  grid (ceil(Ws / 32), ceil(Hs / 32), B): a workgroup stages the 35x35 extended source pixels behind its 16x16 outputs.
// src_out != NULL: the 32x32 interior of the tile is written there as well (level 0 of the pyramid); dst == NULL: nothing above it.
template <bool F32>
__global__ __launch_bounds__(256) void flow_pyrdown_kernel(const void* __restrict__ src, long long src_stride, int Hs, int Ws,
                                                           uint8_t* __restrict__ src_out, uint8_t* __restrict__ dst, int Hd, int Wd,
                                                           long long pyr_stride) {
    STA_SKEW_ENTRY(908);
    __shared__ uint8_t tile[35][36];
    const int ox0 = blockIdx.x * 16, oy0 = blockIdx.y * 16, sx0 = 2 * ox0 - 2, sy0 = 2 * oy0 - 2;
    const size_t frame = blockIdx.z;
    for (int i = threadIdx.x; i < 35 * 35; i += 256) {
        const int ly = i / 35, lx = i - ly * 35, y = sy0 + ly, x = sx0 + lx;
        const size_t at = frame * (size_t)src_stride + (size_t)flow_reflect(y, Hs) * Ws + flow_reflect(x, Ws);
        const int v = F32 ? flow_to_u8(((const float*)src)[at]) : (int)((const uint8_t*)src)[at];
        tile[ly][lx] = (uint8_t)v;
        if (src_out && ly >= 2 && ly < 34 && lx >= 2 && lx < 34 && y < Hs && x < Ws)
            src_out[frame * (size_t)pyr_stride + (size_t)y * Ws + x] = (uint8_t)v;
    }
    __syncthreads(); STA_SKEW(900);
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15, oy = oy0 + ty, ox = ox0 + tx;
    if (!dst || oy >= Hd || ox >= Wd) return;
    const int k[5] = {1, 4, 6, 4, 1};
    int s = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
#pragma unroll
        for (int b = 0; b < 5; ++b) s += k[a] * k[b] * (int)tile[2 * ty + a][2 * tx + b];
    }
    dst[frame * (size_t)pyr_stride + (size_t)oy * Wd + ox] = (uint8_t)((s + 128) >> 8);
}

// ---------------------------------------------------------------------------------------------------------
// Corners.
// floor(sqrt(v)), v < 2^63: a float64 square root, then +-1 by integer compares - no rounding mode can change the result
__device__ __forceinline__ long long flow_isqrt(long long v) {
    long long s = (long long)__dsqrt_rn((double)v);
    if (s * s > v) --s;
    if ((s + 1) * (s + 1) <= v) ++s;
    return s;
}
// grid (ceil(W / 16), ceil(H / 16)), r = block_size / 2 <= 3.  The Sobel products are defined on the image and extended by
// reflection (NOT the products of an extended gradient: gx gy changes sign under a flip); a reflected position of a tile's halo lies
// inside the tile's own staged region, so the box sums read LDS alone.
__global__ __launch_bounds__(256) void flow_response_kernel(const uint8_t* __restrict__ img, int H, int W, int r, int* __restrict__ R,
                                                            int* __restrict__ rmax) {
    STA_SKEW_ENTRY(909);
    __shared__ int im[24][25];
    __shared__ int pxx[22][23], pxy[22][23], pyy[22][23];
    __shared__ int wmax[4];
    const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16, ispan = 16 + 2 * r + 2, pspan = 16 + 2 * r;
    for (int i = threadIdx.x; i < ispan * ispan; i += 256) {
        const int ly = i / ispan, lx = i - ly * ispan;
        im[ly][lx] = img[(size_t)flow_reflect(y0 - r - 1 + ly, H) * W + flow_reflect(x0 - r - 1 + lx, W)];
    }
    __syncthreads(); STA_SKEW(901);
    for (int i = threadIdx.x; i < pspan * pspan; i += 256) {
        const int ly = i / pspan, lx = i - ly * pspan, y = y0 - r + ly, x = x0 - r + lx;
        if (y < 0 || y >= H || x < 0 || x >= W) continue;
        const int gx = (im[ly][lx + 2] - im[ly][lx]) + 2 * (im[ly + 1][lx + 2] - im[ly + 1][lx]) + (im[ly + 2][lx + 2] - im[ly + 2][lx]);
        const int gy = (im[ly + 2][lx] - im[ly][lx]) + 2 * (im[ly + 2][lx + 1] - im[ly][lx + 1]) + (im[ly + 2][lx + 2] - im[ly][lx + 2]);
        pxx[ly][lx] = gx * gx; pxy[ly][lx] = gx * gy; pyy[ly][lx] = gy * gy;
    }
    __syncthreads(); STA_SKEW(902);
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15, y = y0 + ty, x = x0 + tx;
    int resp = 0;
    if (y < H && x < W) {
        int a = 0, b = 0, c = 0;
        for (int dy = -r; dy <= r; ++dy) {
            const int ly = flow_reflect(y + dy, H) - (y0 - r);
            for (int dx = -r; dx <= r; ++dx) {
                const int lx = flow_reflect(x + dx, W) - (x0 - r);
                a += pxx[ly][lx]; b += pxy[ly][lx]; c += pyy[ly][lx];
            }
        }
        const long long d = (long long)a - c;
        resp = (int)((long long)a + c - flow_isqrt(d * d + 4ll * b * b));
        R[(size_t)y * W + x] = resp;
    }
    int mx = resp;                                   // the maximum matters only when it is positive: 0 stands for "none"
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads(); STA_SKEW(903);
    if (threadIdx.x == 0) {
        mx = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
        if (mx > 0) atomicMax(rmax, mx);             // integer atomic: the result does not depend on the order
    }
}
// every pixel gets a key; the candidates' keys order them by R descending, the lower pixel index first
__global__ __launch_bounds__(256) void flow_key_kernel(const int* __restrict__ R, int H, int W, const int* __restrict__ rmax, double quality,
                                                       int idx_bits, unsigned long long* __restrict__ key, int* __restrict__ idx,
                                                       int* __restrict__ n_cand) {
    const int i = blockIdx.x * 256 + threadIdx.x, N = H * W;
    bool cand = false;
    if (i < N) {
        const int v = R[i], m = *rmax, y = i / W, x = i - y * W;
        {
#pragma clang fp contract(off)
            cand = v > 0 && (double)v >= quality * (double)m;
        }
        for (int yy = max(0, y - 1); cand && yy <= min(H - 1, y + 1); ++yy)
            for (int xx = max(0, x - 1); xx <= min(W - 1, x + 1); ++xx) cand = cand && R[(size_t)yy * W + xx] <= v;
        key[i] = cand ? ((unsigned long long)(m - v) << idx_bits) | (unsigned long long)i : ~0ull;
        idx[i] = i;
    }
    const unsigned long long b = __ballot(cand);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_cand, __popcll(b));
}
// cell[pixel] = its rank among the candidates (state 0 = undecided in bits 24..25), -1 for every other pixel; the sorted payload is a
// permutation of the pixels, so every cell is written
__global__ __launch_bounds__(256) void flow_rank_kernel(const int* __restrict__ sidx, int N, const int* __restrict__ n_cand, int* __restrict__ cell) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) cell[sidx[i]] = i < *n_cand ? i : -1;
}
// One workgroup of 1024 threads, thread t on rank lo + t.  A round decides an undecided candidate when that is already certain:
// rejected iff a stronger candidate inside the radius is accepted, accepted iff every stronger one inside the radius is rejected.
// Both are final, so reading a neighbour's state early or late changes only the round in which a decision falls, never the decision:
// the fixed point is the sequential greedy result for any tie structure.  Rank lo itself always decides (everything stronger is
// decided), the decided prefix is emitted in rank order and lo moves behind it; the loop ends with the candidates or at max_corners.
__global__ __launch_bounds__(1024) void flow_suppress_kernel(int* cell, const int* __restrict__ sidx, const int* __restrict__ n_cand, int H, int W,
                                                             int min_distance, int max_corners, float* __restrict__ corners,
                                                             int* __restrict__ n_out) {
    STA_SKEW_ENTRY(910);
    __shared__ int wfirst[16], wsum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int M = *n_cand, md2 = min_distance * min_distance, reach = min_distance - 1;
    int lo = 0, n_acc = 0;
    while (lo < M && n_acc < max_corners) {
        const int r = lo + t;
        int st = 0, x = 0, y = 0;
        if (r < M) {
            const int p = sidx[r];
            y = p / W; x = p - y * W;
            st = cell[p] >> 24;
            if (st == 0) {
                bool any_acc = false, any_und = false;
                for (int dy = -reach; dy <= reach; ++dy) {
                    const int yy = y + dy;
                    if (yy < 0 || yy >= H) continue;
                    for (int dx = -reach; dx <= reach; ++dx) {
                        const int xx = x + dx;
                        if (xx < 0 || xx >= W || dx * dx + dy * dy >= md2) continue;
                        const int c = cell[(size_t)yy * W + xx];
                        if (c < 0 || (c & 0xFFFFFF) >= r) continue;
                        any_acc = any_acc || (c >> 24) == 1;
                        any_und = any_und || (c >> 24) == 0;
                    }
                }
                st = any_acc ? 2 : (any_und ? 0 : 1);
                if (st) cell[p] = (st << 24) | r;
            }
        }
        // u = the first thread whose rank is undecided or past the candidates
        const unsigned long long open = __ballot(r >= M || st == 0);
        if (lane == 0) wfirst[wave] = open ? wave * 64 + __ffsll((long long)open) - 1 : 1024;
        __syncthreads(); STA_SKEW(904);                                 // also orders this round's cell writes before the next round's reads
        int u = 1024;
#pragma unroll
        for (int w = 0; w < 16; ++w) u = min(u, wfirst[w]);
        if (u == 0) break;                               // cannot happen (rank lo decides); never spin on it
        // ordered emission of the accepted ranks of [lo, lo + u)
        int v = (t < u && st == 1) ? 1 : 0;
        const int mine = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(v, o);
            if (lane >= o) v += up;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads(); STA_SKEW(905);
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { if (w < wave) before += wsum[w]; total += wsum[w]; }
        const int pos = n_acc + before + v - mine;
        if (mine && pos < max_corners) { corners[2 * (size_t)pos] = (float)x; corners[2 * (size_t)pos + 1] = (float)y; }
        n_acc += total; lo += u;
        __syncthreads(); STA_SKEW(906);                                 // wfirst / wsum are rewritten by the next round
    }
    if (t == 0) *n_out = min(n_acc, max_corners);
}

// ---------------------------------------------------------------------------------------------------------
// Tracking.
struct FlowTrack {
    const uint8_t* prev; const uint8_t* next;       // pyramids: prev one, next B of them `lv.bytes` apart
    FlowLevels lv;
    const float* pts; const int* n_dev; int n_cap;  // n = min(*n_dev, n_cap), or n_cap when n_dev is NULL
    int win, max_iter;
    double eps, min_eig;
    float* out; uint8_t* status;                    // [B, n_cap, 2], [B, n_cap]
};
__device__ __forceinline__ long long flow_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);      // integers: every lane ends with the same exact sum
    return v;
}
// rint((1 - a)(1 - b) 2^14) ... : float64 products in the order written, rounded half to even
__device__ __forceinline__ void flow_weights(double a, double b, int* w) {
#pragma clang fp contract(off)
    const double na = 1.0 - a, nb = 1.0 - b;
    w[0] = (int)rint(na * nb * 16384.0);
    w[1] = (int)rint(a * nb * 16384.0);
    w[2] = (int)rint(na * b * 16384.0);
    w[3] = (1 << FLOW_W_BITS) - w[0] - w[1] - w[2];
}
__device__ __forceinline__ int flow_descale(int s, int k) { return (s + (1 << (k - 1))) >> k; }
// the window's origin must lie in [-win, W) x [-win, H) (compared as doubles: the estimate of a lost point may be anything)
__device__ __forceinline__ bool flow_outside(double fx, double fy, int win, int W, int H) {
    return !(fx >= (double)-win && fx < (double)W && fy >= (double)-win && fy < (double)H);
}
// grid (n_cap, B), one wave per workgroup: point blockIdx.x of the previous frame into next frame blockIdx.y.  Lane l owns the window
// pixels l, l + 64, ... (7 at win = 21); the scalar float64 step is computed by every lane from the same reduced integers, so the
// branches are uniform and nothing is broadcast.  __syncthreads() is the barrier of that single wave.
__global__ __launch_bounds__(64) void flow_track_kernel(const FlowTrack a) {
#pragma clang fp contract(off)
    __shared__ short img[24 * 24];                   // extended level image behind the template: window + 1 for the bilinear taps + 1 for Scharr
    __shared__ short gxs[22 * 22], gys[22 * 22];     // Scharr gradients at the window + 1 positions, 0 outside the level
    __shared__ short nxt[22 * 22];                   // next level image at the window + 1 positions of the current estimate
    const int lane = threadIdx.x, pt = blockIdx.x, frame = blockIdx.y;
    const int n = a.n_dev ? min(*a.n_dev, a.n_cap) : a.n_cap;
    if (pt >= n) return;
    const int win = a.win, nw = win * win, span = win + 1, ispan = win + 3;
    const double half = (double)((win - 1) / 2);
    const double x = (double)a.pts[2 * (size_t)pt], y = (double)a.pts[2 * (size_t)pt + 1];
    const double eps2 = a.eps * a.eps, area2 = (double)(2 * win * win);
    const uint8_t* nbase = a.next + (size_t)frame * (size_t)a.lv.bytes;
    int wy[7], wx[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) { const int k = lane + 64 * j; wy[j] = k / win; wx[j] = k - wy[j] * win; }
    int status = 1;
    double qx = 0.0, qy = 0.0;
    const int L = a.lv.levels - 1;
    for (int l = L; l >= 0; --l) {
        const int H = a.lv.h[l], W = a.lv.w[l];
        const uint8_t* pim = a.prev + a.lv.off[l];
        const uint8_t* nim = nbase + a.lv.off[l];
        const double sc = 1.0 / (double)(1 << l);
        const double px = x * sc - half, py = y * sc - half;
        if (l == L) { qx = x * sc; qy = y * sc; } else { qx = 2.0 * qx; qy = 2.0 * qy; }
        const double fx = floor(px), fy = floor(py);
        if (flow_outside(fx, fy, win, W, H)) { if (l == 0) status = 0; continue; }
        const int ipx = (int)fx, ipy = (int)fy;
        __syncthreads();                             // the level above has finished with the LDS patches
        for (int i = lane; i < ispan * ispan; i += 64) {
            const int ly = i / ispan, lx = i - ly * ispan;
            img[ly * 24 + lx] = pim[(size_t)flow_reflect(ipy - 1 + ly, H) * W + flow_reflect(ipx - 1 + lx, W)];
        }
        __syncthreads();
        for (int i = lane; i < span * span; i += 64) {
            const int ly = i / span, lx = i - ly * span, yy = ipy + ly, xx = ipx + lx;
            int gx = 0, gy = 0;
            if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                const short* p = img + ly * 24 + lx;       // p[0] = (yy - 1, xx - 1)
                gx = 3 * (p[2] - p[0]) + 10 * (p[26] - p[24]) + 3 * (p[50] - p[48]);
                gy = 3 * (p[48] - p[0]) + 10 * (p[49] - p[1]) + 3 * (p[50] - p[2]);
            }
            gxs[ly * 22 + lx] = (short)gx; gys[ly * 22 + lx] = (short)gy;
        }
        __syncthreads();
        int w[4];
        flow_weights(px - fx, py - fy, w);
        int I[7], Ix[7], Iy[7];
        long long s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            I[j] = 0; Ix[j] = 0; Iy[j] = 0;
            if (lane + 64 * j < nw) {
                const short* p = img + (wy[j] + 1) * 24 + wx[j] + 1;
                const short* g = gxs + wy[j] * 22 + wx[j];
                const short* h = gys + wy[j] * 22 + wx[j];
                I[j] = flow_descale(w[0] * p[0] + w[1] * p[1] + w[2] * p[24] + w[3] * p[25], FLOW_W_BITS - 5);
                Ix[j] = flow_descale(w[0] * g[0] + w[1] * g[1] + w[2] * g[22] + w[3] * g[23], FLOW_W_BITS);
                Iy[j] = flow_descale(w[0] * h[0] + w[1] * h[1] + w[2] * h[22] + w[3] * h[23], FLOW_W_BITS);
                s11 += (long long)Ix[j] * Ix[j]; s12 += (long long)Ix[j] * Iy[j]; s22 += (long long)Iy[j] * Iy[j];
            }
        }
        const double FS = 1.0 / (double)(1 << 20);
        const double A11 = FS * (double)flow_wave_sum(s11), A12 = FS * (double)flow_wave_sum(s12), A22 = FS * (double)flow_wave_sum(s22);
        const double D = A11 * A22 - A12 * A12;
        const double dA = A11 - A22;
        const double e = (A11 + A22 - __dsqrt_rn(dA * dA + 4.0 * A12 * A12)) / area2;
        if (e < a.min_eig || D < 1.1920928955078125e-07) { if (l == 0) status = 0; continue; }
        qx = qx - half; qy = qy - half;
        double pdx = 0.0, pdy = 0.0;
        int sx = 0, sy = 0;
        bool staged = false;
        for (int j = 0; j < a.max_iter; ++j) {
            const double gx = floor(qx), gy = floor(qy);
            if (flow_outside(gx, gy, win, W, H)) { if (l == 0) status = 0; break; }
            const int iqx = (int)gx, iqy = (int)gy;
            if (!staged || iqx != sx || iqy != sy) {       // the patch moves only when the estimate crosses a pixel
                __syncthreads();
                for (int i = lane; i < span * span; i += 64) {
                    const int ly = i / span, lx = i - ly * span;
                    nxt[ly * 22 + lx] = nim[(size_t)flow_reflect(iqy + ly, H) * W + flow_reflect(iqx + lx, W)];
                }
                __syncthreads();
                staged = true; sx = iqx; sy = iqy;
            }
            int v[4];
            flow_weights(qx - gx, qy - gy, v);
            long long t1 = 0, t2 = 0;
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                if (lane + 64 * k < nw) {
                    const short* p = nxt + wy[k] * 22 + wx[k];
                    const int d = flow_descale(v[0] * p[0] + v[1] * p[1] + v[2] * p[22] + v[3] * p[23], FLOW_W_BITS - 5) - I[k];
                    t1 += (long long)d * Ix[k]; t2 += (long long)d * Iy[k];
                }
            }
            const double b1 = FS * (double)flow_wave_sum(t1), b2 = FS * (double)flow_wave_sum(t2);
            const double dx = (A12 * b2 - A22 * b1) / D, dy = (A12 * b1 - A11 * b2) / D;
            qx = qx + dx; qy = qy + dy;
            if (dx * dx + dy * dy <= eps2) break;
            if (j > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) { qx = qx - dx * 0.5; qy = qy - dy * 0.5; break; }
            pdx = dx; pdy = dy;
        }
        qx = qx + half; qy = qy + half;
    }
    if (lane == 0) {
        const size_t o = (size_t)frame * a.n_cap + pt;
        a.out[2 * o] = (float)qx; a.out[2 * o + 1] = (float)qy;
        a.status[o] = (uint8_t)status;
    }
}
// grid (B), 256 threads: stats[frame] = {n, n_good, sum of sqrt(dx^2 + dy^2)} as doubles.  Thread t adds the points t, t + 256, ... in
// ascending order, then a xor butterfly over the lanes, then the four wave sums in ascending order: the order depends on n alone.
__global__ __launch_bounds__(256) void flow_stats_kernel(const float* __restrict__ pts, const int* __restrict__ n_dev, int n_cap,
                                                         const float* __restrict__ out, const uint8_t* __restrict__ status,
                                                         double* __restrict__ stats) {
#pragma clang fp contract(off)
    STA_SKEW_ENTRY(911);
    __shared__ double wsum[4];
    __shared__ int wgood[4];
    const int n = n_dev ? min(*n_dev, n_cap) : n_cap, frame = blockIdx.x;
    double s = 0.0;
    int good = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const size_t o = (size_t)frame * n_cap + i;
        if (status[o] != 1) continue;
        const double dx = (double)out[2 * o] - (double)pts[2 * (size_t)i], dy = (double)out[2 * o + 1] - (double)pts[2 * (size_t)i + 1];
        s += __dsqrt_rn(dx * dx + dy * dy);
        ++good;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); good += __shfl_xor(good, o); }
    if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6] = s; wgood[threadIdx.x >> 6] = good; }
    __syncthreads(); STA_SKEW(907);
    if (threadIdx.x == 0) {
        stats[3 * (size_t)frame] = (double)n;
        stats[3 * (size_t)frame + 1] = (double)(wgood[0] + wgood[1] + wgood[2] + wgood[3]);
        stats[3 * (size_t)frame + 2] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}
