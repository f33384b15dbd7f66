// Token selections from per-pixel maps (sta_select_patches; the contract is in include/sta_mi355.h), included by sta_api.hip next
// to geo.h; launch code in sta_rows.inc.  B <= SEQ_MAX maps, each of its own frame size, become the packed per-entry selections the
// varlen routes take: patch scores, ascending index lists, (y, x) lists, counts and bounding windows.  Two launches, no workspace:
//   patch_score_kernel<KIND>   grid (blocks, B): pools every 16x16 patch of entry blockIdx.y to an int32 score
//   patch_select_kernel        grid (B): one workgroup per entry thresholds (+ dilates) or radix-selects the top k, then compacts in order
// Everything is integer arithmetic on the scores, so the result is defined bit for bit (tests/select_cases.py restates it in numpy).
#pragma once
#include "sta_skew.h"       // STA_SKEW points: nothing unless -DSTA_WAVE_SKEW (libsta_mi355_skew.so)

#define SEL_MAX_PATCHES 8192      // one entry's scores (32 KiB) + two flag grids (16 KiB) stay in static LDS below 64 KiB
#define SEL_MAX_MARGIN 8

// The geometry of one call, in the kernel arguments (host values, nothing is copied for them): entry b is the map at map[b] of
// H[b] x W[b] pixels, its hp x wp patch grid sits at off[b] of every packed output; k[b] = its top_k (rule 1 only).
struct SelGeo { const void* map[SEQ_MAX]; int H[SEQ_MAX], W[SEQ_MAX], off[SEQ_MAX + 1], k[SEQ_MAX]; };

enum { SEL_U8 = 0, SEL_F32_THRES = 1, SEL_F32_SUM = 2 };

// non-zero bytes of a dword: fold every byte onto its bit 0 (the shifts only ever bring bits of the SAME byte to bit 0)
__device__ __forceinline__ int sel_nonzero_bytes(unsigned w) {
    w |= w >> 4; w |= w >> 2; w |= w >> 1;
    return __popc(w & 0x01010101u);
}
// one pixel's contribution.  Count forms: the predicate (strict >, false for NaN on either side), negated by invert.  Sum form:
// rint(clamp(v, 0, 32767) * 256), half to even; the two selects ARE the clamp: NaN, -inf and negatives fail v > 0, +inf fails v < 32767
template <int KIND>
__device__ __forceinline__ int sel_pixel(float v, float thres, bool invert) {
    if (KIND == SEL_F32_SUM) {
        v = v > 0.f ? v : 0.f;
        v = v < 32767.f ? v : 32767.f;
        return (int)rintf(v * 256.f);
    }
    return (int)((v > thres) != invert);
}

// Sixteen lanes own one patch, one lane per pixel row (four patches per wave, sixteen per workgroup); the sixteen partial scores are
// reduced by xor-shuffles that stay inside the 16-lane row.  A 16-byte aligned map is read with 16-byte loads (one per lane for
// bytes, four for floats); any other base address takes the element-wise path of the same kernel.
template <int KIND>
__global__ __launch_bounds__(256) void patch_score_kernel(const SelGeo g, float thres, int invert, int32_t* __restrict__ score) {
    const int b = blockIdx.y;
    const int W = g.W[b], wp = W >> 4, N = (g.H[b] >> 4) * wp;
    const unsigned char* base = (const unsigned char*)g.map[b];
    const bool vec = (((uintptr_t)base) & 15) == 0;
    const int r = threadIdx.x & 15, sub = threadIdx.x >> 4;
    const bool inv = invert != 0;
    for (int p0 = blockIdx.x * 16; p0 < N; p0 += gridDim.x * 16) {
        const int p = p0 + sub;
        int s = 0;
        if (p < N) {
            const int py = p / wp, px = p - py * wp;
            const size_t pix = (size_t)(py * 16 + r) * W + px * 16;          // first of this lane's 16 pixels
            if (KIND == SEL_U8) {
                const unsigned char* q = base + pix;
                if (vec) {
                    const uint4 u = ldg16(q);
                    s = sel_nonzero_bytes(u.x) + sel_nonzero_bytes(u.y) + sel_nonzero_bytes(u.z) + sel_nonzero_bytes(u.w);
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) s += q[i] != 0;
                }
                if (inv) s = 16 - s;
            } else {
                const float* q = (const float*)base + pix;
                if (vec) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint4 u = ldg16(q + 4 * i);
                        s += sel_pixel<KIND>(__uint_as_float(u.x), thres, inv) + sel_pixel<KIND>(__uint_as_float(u.y), thres, inv) +
                             sel_pixel<KIND>(__uint_as_float(u.z), thres, inv) + sel_pixel<KIND>(__uint_as_float(u.w), thres, inv);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) s += sel_pixel<KIND>(q[i], thres, inv);
                }
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
        if (r == 0 && p < N) score[g.off[b] + p] = s;
    }
}

// inclusive scan of one int per thread over the 256 threads of a workgroup (wsum: 4 ints of LDS, free again after the next barrier)
__device__ __forceinline__ int sel_block_scan(int v, int* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads(); STA_SKEW(600);
    for (int w = 0; w < wave; ++w) v += wsum[w];
    return v;
}

// One workgroup of 256 threads per entry.  rule 0: flag = score >= min_score, dilated by `margin` patches (Chebyshev, separable:
// a row pass then a column pass on the flag grid in LDS, inside the entry's own grid).  rule 1: an MSB-first radix select (8-bit
// digits over the 31 key bits of the non-negative scores, a 256-bin LDS histogram per pass) finds the k-th largest score T and the
// quota q = k - #(score > T); a patch is selected iff score > T, or score == T and fewer than q equal-scored patches precede it.
// Then ONE ordered walk in chunks of 256 patches: a lane's rank inside its wave is the popcount of the 64-bit ballot below it, wave
// totals go through LDS, the running bases (selected so far, equal-scored so far) are carried from chunk to chunk.  Index and
// (y, x) lists come out ascending; the bounding rectangle is a min / max reduction; the tail of the slot is filled with -1.
__global__ __launch_bounds__(256) void patch_select_kernel(const SelGeo g, int rule, int min_score, int margin, const int32_t* __restrict__ score,
                                                           int64_t* __restrict__ index, int64_t* __restrict__ pos, int32_t* __restrict__ n_sel,
                                                           int32_t* __restrict__ window) {
    STA_SKEW_ENTRY(609);
    __shared__ int sc[SEL_MAX_PATCHES];
    __shared__ unsigned char flag[SEL_MAX_PATCHES], tmp[SEL_MAX_PATCHES];
    __shared__ int hist[256];
    __shared__ int wsum[4], wtot[2][4], pick[2], box[4][4];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int hp = g.H[b] >> 4, wp = g.W[b] >> 4, N = hp * wp, off = g.off[b];
    const int32_t* s_in = score + off;
    int T = 0, q = 0;
    if (rule == 1) {
        for (int i = t; i < N; i += 256) sc[i] = s_in[i];
        unsigned prefix = 0u, mask = 0u; int krem = g.k[b];
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[t] = 0;
            __syncthreads(); STA_SKEW(601);
            for (int i = t; i < N; i += 256) {
                const int s = sc[i];
                if (((unsigned)s & mask) == prefix) atomicAdd(&hist[(s >> shift) & 255], 1);
            }
            __syncthreads(); STA_SKEW(602);
            const int d = 255 - t, v = hist[d];               // thread t owns digit 255 - t: the scan runs from the largest digit down
            const int incl = sel_block_scan(v, wsum);
            if (incl - v < krem && krem <= incl) { pick[0] = d; pick[1] = krem - (incl - v); }
            __syncthreads(); STA_SKEW(603);
            prefix |= (unsigned)pick[0] << shift; mask |= 255u << shift; krem = pick[1];
        }
        T = (int)prefix; q = krem;
    } else {
        for (int i = t; i < N; i += 256) flag[i] = s_in[i] >= min_score;
        if (margin > 0) {
            __syncthreads(); STA_SKEW(604);
            for (int i = t; i < N; i += 256) {
                const int y = i / wp, x = i - y * wp;
                const int x0 = x - margin > 0 ? x - margin : 0, x1 = x + margin < wp - 1 ? x + margin : wp - 1;
                unsigned char f = 0;
                for (int xx = x0; xx <= x1; ++xx) f |= flag[y * wp + xx];
                tmp[i] = f;
            }
            __syncthreads(); STA_SKEW(605);
            for (int i = t; i < N; i += 256) {
                const int y = i / wp, x = i - y * wp;
                const int y0 = y - margin > 0 ? y - margin : 0, y1 = y + margin < hp - 1 ? y + margin : hp - 1;
                unsigned char f = 0;
                for (int yy = y0; yy <= y1; ++yy) f |= tmp[yy * wp + x];
                flag[i] = f;
            }
        }
        __syncthreads(); STA_SKEW(606);
    }
    int64_t* idx = index + off;
    int64_t* ps = pos + 2 * (size_t)off;
    const unsigned long long below = (1ull << lane) - 1ull;
    int base_gt = 0, base_eq = 0;
    int ymin = hp, ymax = -1, xmin = wp, xmax = -1;
    for (int c0 = 0, par = 0; c0 < N; c0 += 256, par ^= 1) {
        const int i = c0 + t;
        bool gt = false, eq = false;
        if (i < N) {
            if (rule == 1) { const int s = sc[i]; gt = s > T; eq = s == T; }
            else gt = flag[i] != 0;
        }
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        if (lane == 0) wtot[par][wave] = __popcll(bg) | (__popcll(be) << 16);
        __syncthreads(); STA_SKEW(607);
        int pre = 0, tot = 0;
        for (int w = 0; w < 4; ++w) { const int v = wtot[par][w]; tot += v; if (w < wave) pre += v; }
        const int eq_before = base_eq + (pre >> 16) + __popcll(be & below);
        const int taken = eq_before < q ? eq_before : q;          // equal-scored patches before this one that were selected
        if (gt || (eq && eq_before < q)) {
            const int rank = base_gt + (pre & 0xffff) + __popcll(bg & below) + taken;       // <= i: inside the slot
            const int y = i / wp, x = i - y * wp;
            idx[rank] = i;
            ps[2 * rank] = y; ps[2 * rank + 1] = x;
            ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
            xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax;
        }
        base_gt += tot & 0xffff; base_eq += tot >> 16;
    }
    const int n = base_gt + (base_eq < q ? base_eq : q);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(ymin, o), c = __shfl_xor(ymax, o), d = __shfl_xor(xmin, o), e = __shfl_xor(xmax, o);
        ymin = a < ymin ? a : ymin; ymax = c > ymax ? c : ymax; xmin = d < xmin ? d : xmin; xmax = e > xmax ? e : xmax;
    }
    if (lane == 0) { box[wave][0] = ymin; box[wave][1] = ymax; box[wave][2] = xmin; box[wave][3] = xmax; }
    __syncthreads(); STA_SKEW(608);
    if (t == 0) {
        for (int w = 1; w < 4; ++w) {
            ymin = box[w][0] < ymin ? box[w][0] : ymin; ymax = box[w][1] > ymax ? box[w][1] : ymax;
            xmin = box[w][2] < xmin ? box[w][2] : xmin; xmax = box[w][3] > xmax ? box[w][3] : xmax;
        }
        n_sel[b] = n;
        window[4 * b + 0] = n ? ymin : 0; window[4 * b + 1] = n ? xmin : 0;
        window[4 * b + 2] = n ? ymax - ymin + 1 : 0; window[4 * b + 3] = n ? xmax - xmin + 1 : 0;
    }
    for (int i = n + t; i < N; i += 256) { idx[i] = -1; ps[2 * i] = -1; ps[2 * i + 1] = -1; }
}
