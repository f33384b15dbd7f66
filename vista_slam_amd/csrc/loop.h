// Loop candidates: ORB keypoints and descriptors, bag-of-words vectors from a vocabulary tree and their L1 scores (sta_orb_extract /
// sta_bow_transform / sta_bow_score; the contract is in include/sta_mi355.h), included by sta_api.hip after voxel.h and flow.h
// (flow_reflect, flow_to_u8 and flow_wave_sum are flow.h's); launch code in sta_rows.inc.  Integer arithmetic wherever the contract is
// integer, float64 with contraction off elsewhere: every output is defined by the input alone.  Integer atomics only (a histogram and
// list slots whose order no result depends on).
//   orb_level0_kernel     the frame -> level 0 (uint8 copy or fp32 -> uint8)
//   orb_resize_kernel     level l from level l - 1, 11-bit bilinear
//   orb_fast_kernel       FAST-9 score of every pixel of every level from a 22x22 LDS tile (one launch, blockIdx.z = level)
//   orb_nms_kernel        strict 3x3 maximum inside the edge -> survivor map + the 256-bin score histogram per level
//   orb_cut_kernel        the first cut: the score of the 2 n_l-th largest survivor per level
//   orb_harris_kernel     integer Harris response of the survivors at or above the cut -> the level's candidate list
//   orb_rank_kernel       rank by counting (R descending, then pixel ascending): the first n_l of a level -> their slots
//   orb_blur_kernel       7x7 integer blur of every level
//   orb_describe_kernel   one wave per kept keypoint: moments, angle bin, 256 rotated comparisons, the output row
//   bow_walk_kernel       one wave per descriptor down the tree, lane = child
//   bow_reduce_kernel     one workgroup: word ids -> sorted distinct words, counts, weighted and L1-normalised values
//   bow_score_kernel      one wave per database row: the L1 score against the query, binary search over the row's words
#pragma once
#include "sta_skew.h"       // STA_SKEW points: nothing unless -DSTA_WAVE_SKEW (libsta_mi355_skew.so)

#define ORB_MAX_LEVELS 8
#define ORB_MAX_FEATURES 4096
#define ORB_MIN_EDGE 22
#define ORB_MAX_EDGE 64
#define ORB_MAX_PIXELS (1 << 21)
#define ORB_MAX_ROWS (ORB_MAX_FEATURES + ORB_MAX_LEVELS)   // the rounded per-level counts can sum to a little more than nfeatures
#define BOW_MAX_K 64
#define BOW_MAX_DEPTH 10
#define BOW_NO_WORD 0x7fffffff

// The levels of one call.  h / w / nfeat are given for all `levels`, only the first `built` of them exist in memory: off[l] = byte
// offset of level l in each level-shaped plane of `bytes` bytes, cand_off / cand_cap = its candidate list, sel_off = its first slot
// (the sum of nfeat below it).
struct OrbLevels {
    int levels, built;
    int h[ORB_MAX_LEVELS], w[ORB_MAX_LEVELS], nfeat[ORB_MAX_LEVELS];
    long long off[ORB_MAX_LEVELS];
    long long bytes;
    int cand_off[ORB_MAX_LEVELS], cand_cap[ORB_MAX_LEVELS], sel_off[ORB_MAX_LEVELS];
    int cand_total, slots, rows;         // rows = the capacity of the outputs = max(nfeatures, sum of nfeat)
    int edge, thr;
};

template <bool F32>
__global__ __launch_bounds__(256) void orb_level0_kernel(const void* __restrict__ src, int N, uint8_t* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) dst[i] = F32 ? (uint8_t)flow_to_u8(((const float*)src)[i]) : ((const uint8_t*)src)[i];
}

// source index and weight of output coordinate x: f = (x + 0.5) r - 0.5, s = floor(f), a = f - s; s < 0 -> (0, 0); s >= n - 1 -> (n - 1, 0)
__device__ __forceinline__ void orb_tap(int x, double r, int n, int* i0, int* i1, int* c1) {
#pragma clang fp contract(off)
    const double f = ((double)x + 0.5) * r - 0.5;
    const double fl = floor(f);
    double a = f - fl;
    int s = (int)fl;
    if (s < 0) { s = 0; a = 0.0; }
    else if (s >= n - 1) { s = n - 1; a = 0.0; }
    *i0 = s; *i1 = min(s + 1, n - 1);
    *c1 = (int)rint(a * 2048.0);
}
// grid (ceil(Wd / 16), ceil(Hd / 16)); ry = Hs / Hd and rx = Ws / Wd are the host's float64 quotients
__global__ __launch_bounds__(256) void orb_resize_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, uint8_t* __restrict__ dst, int Hd, int Wd,
                                                         double ry, double rx) {
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= Wd || y >= Hd) return;
    int x0, x1, cx1, y0, y1, cy1;
    orb_tap(x, rx, Ws, &x0, &x1, &cx1);
    orb_tap(y, ry, Hs, &y0, &y1, &cy1);
    const int cx0 = 2048 - cx1, cy0 = 2048 - cy1;
    const int p00 = src[(size_t)y0 * Ws + x0], p01 = src[(size_t)y0 * Ws + x1], p10 = src[(size_t)y1 * Ws + x0], p11 = src[(size_t)y1 * Ws + x1];
    const int s = cy0 * (cx0 * p00 + cx1 * p01) + cy1 * (cx0 * p10 + cx1 * p11);       // <= 2^22 * 255
    dst[(size_t)y * Wd + x] = (uint8_t)((s + (1 << 21)) >> 22);
}

// grid (ceil(W_0 / 16), ceil(H_0 / 16), built): the workgroups past a smaller level's extent leave at once.  score = 0 for a pixel
// nearer than 3 to the border and for a non-corner.
__global__ __launch_bounds__(256) void orb_fast_kernel(const uint8_t* __restrict__ img, const OrbLevels lv, uint8_t* __restrict__ score) {
    STA_SKEW_ENTRY(1010);
    __shared__ uint8_t t[22][23];
    const int l = blockIdx.z, H = lv.h[l], W = lv.w[l], x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    if (x0 >= W || y0 >= H) return;
    const uint8_t* im = img + lv.off[l];
    for (int i = threadIdx.x; i < 22 * 22; i += 256) {
        const int ly = i / 22, lx = i - ly * 22, y = y0 - 3 + ly, x = x0 - 3 + lx;
        t[ly][lx] = (y >= 0 && y < H && x >= 0 && x < W) ? im[(size_t)y * W + x] : (uint8_t)0;
    }
    __syncthreads(); STA_SKEW(1000);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    int s = 0;
    if (x >= 3 && x < W - 3 && y >= 3 && y < H - 3) {
        const int ox[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        const int oy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
        const int p = t[ty + 3][tx + 3];
        int d[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = p - (int)t[ty + 3 + oy[i]][tx + 3 + ox[i]];
        int A = -256, Bm = -256;
#pragma unroll
        for (int s0 = 0; s0 < 16; ++s0) {
            int mn = 256, mx = -256;
#pragma unroll
            for (int j = 0; j < 9; ++j) { const int v = d[(s0 + j) & 15]; mn = min(mn, v); mx = max(mx, v); }
            A = max(A, mn); Bm = max(Bm, -mx);                     // min over the arc of (ring - p) = -max of (p - ring)
        }
        const int sc = max(A, Bm) - 1;
        s = sc >= lv.thr ? sc : 0;
    }
    score[lv.off[l] + (size_t)y * W + x] = (uint8_t)s;
}

// same grid.  surv = the score of a corner that is strictly above its 8 neighbours and lies inside the edge, else 0; hist [built][256]
__global__ __launch_bounds__(256) void orb_nms_kernel(const uint8_t* __restrict__ score, const OrbLevels lv, uint8_t* __restrict__ surv,
                                                      int* __restrict__ hist) {
    const int l = blockIdx.z, H = lv.h[l], W = lv.w[l], e = lv.edge;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= W || y >= H) return;
    const uint8_t* sc = score + lv.off[l];
    int s = 0;
    if (x >= e && x < W - e && y >= e && y < H - e) {              // e >= 22: the 8 neighbours are inside the level
        s = sc[(size_t)y * W + x];
        if (s > 0) {
            bool top = true;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
                    if (dx != 0 || dy != 0) top = top && (int)sc[(size_t)(y + dy) * W + x + dx] < s;
            if (!top) s = 0;
        }
        if (s > 0) atomicAdd(hist + 256 * l + s, 1);
    }
    surv[lv.off[l] + (size_t)y * W + x] = (uint8_t)s;
}

// one workgroup, thread l < built: cut[l] = the smallest score that is kept.  More than 2 n_l survivors: the score of the 2 n_l-th
// largest (its ties stay); otherwise every survivor.
__global__ __launch_bounds__(64) void orb_cut_kernel(const int* __restrict__ hist, const OrbLevels lv, int* __restrict__ cut) {
    const int l = threadIdx.x;
    if (l >= lv.built) return;
    const int want = 2 * lv.nfeat[l];
    int total = 0;
    for (int s = 1; s < 256; ++s) total += hist[256 * l + s];
    int c = 1;
    if (total > want) {
        int acc = 0;
        c = 255;
        for (int s = 255; s >= 1; --s) { acc += hist[256 * l + s]; if (acc >= want) { c = s; break; } }
    }
    cut[l] = c;
}

// same grid as orb_fast_kernel.  R = 25 (a b - c^2) - (a + b)^2 over the 7x7 block of the unblurred level; the candidate takes a slot of
// its level's list (the slots' order is free: orb_rank_kernel orders by value)
__global__ __launch_bounds__(256) void orb_harris_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ surv, const OrbLevels lv,
                                                         const int* __restrict__ cut, int* __restrict__ ncand, long long* __restrict__ candR,
                                                         int* __restrict__ candP) {
    const int l = blockIdx.z, H = lv.h[l], W = lv.w[l];
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= W || y >= H) return;
    const int s = surv[lv.off[l] + (size_t)y * W + x];
    if (s == 0 || s < cut[l]) return;
    const uint8_t* im = img + lv.off[l];
    int a = 0, b = 0, c = 0;
    for (int dy = -3; dy <= 3; ++dy) {
        const uint8_t* r0 = im + (size_t)(y + dy - 1) * W + x;
        const uint8_t* r1 = r0 + W;
        const uint8_t* r2 = r1 + W;
        for (int dx = -3; dx <= 3; ++dx) {
            const int ix = 2 * ((int)r1[dx + 1] - (int)r1[dx - 1]) + ((int)r0[dx + 1] - (int)r0[dx - 1]) + ((int)r2[dx + 1] - (int)r2[dx - 1]);
            const int iy = 2 * ((int)r2[dx] - (int)r0[dx]) + ((int)r2[dx - 1] - (int)r0[dx - 1]) + ((int)r2[dx + 1] - (int)r0[dx + 1]);
            a += ix * ix; b += iy * iy; c += ix * iy;
        }
    }
    const long long R = 25ll * ((long long)a * b - (long long)c * c) - (long long)(a + b) * (long long)(a + b);
    const int slot = atomicAdd(ncand + l, 1);
    if (slot < lv.cand_cap[l]) { candR[lv.cand_off[l] + slot] = R; candP[lv.cand_off[l] + slot] = y * W + x; }
}

// grid (ceil(max cand_cap / 256), built).  rank = the number of candidates of the level that come first (larger R, or the same R at a
// lower pixel index); the candidates of rank < n_l go to slot sel_off[l] + rank
__global__ __launch_bounds__(256) void orb_rank_kernel(const OrbLevels lv, const int* __restrict__ ncand, const long long* __restrict__ candR,
                                                       const int* __restrict__ candP, long long* __restrict__ selR, int* __restrict__ selP) {
    STA_SKEW_ENTRY(1011);
    __shared__ long long sR[256];
    __shared__ int sP[256];
    const int l = blockIdx.y, M = min(ncand[l], lv.cand_cap[l]), i = blockIdx.x * 256 + threadIdx.x;
    if ((int)blockIdx.x * 256 >= M) return;
    const long long* cR = candR + lv.cand_off[l];
    const int* cP = candP + lv.cand_off[l];
    const long long myR = i < M ? cR[i] : 0;
    const int myP = i < M ? cP[i] : 0;
    int rank = 0;
    for (int base = 0; base < M; base += 256) {
        __syncthreads(); STA_SKEW(1001);
        const int j = base + threadIdx.x;
        if (j < M) { sR[threadIdx.x] = cR[j]; sP[threadIdx.x] = cP[j]; }
        __syncthreads(); STA_SKEW(1002);
        const int cnt = min(256, M - base);
        for (int k = 0; k < cnt; ++k) rank += (sR[k] > myR || (sR[k] == myR && sP[k] < myP)) ? 1 : 0;
    }
    if (i < M && rank < lv.nfeat[l]) { selR[lv.sel_off[l] + rank] = myR; selP[lv.sel_off[l] + rank] = myP; }
}

// same grid as orb_fast_kernel: B = (sum_ab k[a] k[b] ext(y + a - 3, x + b - 3) + 2^15) >> 16, reflect-101
__global__ __launch_bounds__(256) void orb_blur_kernel(const uint8_t* __restrict__ img, const OrbLevels lv, uint8_t* __restrict__ blur) {
    STA_SKEW_ENTRY(1012);
    __shared__ uint8_t t[22][23];
    __shared__ int hs[22][17];
    const int l = blockIdx.z, H = lv.h[l], W = lv.w[l], x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
    if (x0 >= W || y0 >= H) return;
    const uint8_t* im = img + lv.off[l];
    for (int i = threadIdx.x; i < 22 * 22; i += 256) {
        const int ly = i / 22, lx = i - ly * 22;
        t[ly][lx] = im[(size_t)flow_reflect(y0 - 3 + ly, H) * W + flow_reflect(x0 - 3 + lx, W)];
    }
    __syncthreads(); STA_SKEW(1003);
    const int k[7] = {18, 33, 49, 56, 49, 33, 18};
    for (int i = threadIdx.x; i < 22 * 16; i += 256) {             // rows first: exact integers, so the order of the two passes is free
        const int ly = i >> 4, lx = i & 15;
        int s = 0;
#pragma unroll
        for (int b = 0; b < 7; ++b) s += k[b] * (int)t[ly][lx + b];
        hs[ly][lx] = s;
    }
    __syncthreads(); STA_SKEW(1004);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    int s = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a) s += k[a] * hs[ty + a][tx];
    blur[lv.off[l] + (size_t)y * W + x] = (uint8_t)((s + (1 << 15)) >> 16);
}

__device__ __forceinline__ long long orb_cross(const int* __restrict__ trig, int j, long long mx, long long my) {
    return (long long)trig[2 * j] * my - (long long)trig[2 * j + 1] * mx;
}
// grid (max(slots, 1)), one wave per slot.  Level l keeps cnt_l = min(candidates, n_l) keypoints; slot sel_off[l] + rank with
// rank < cnt_l becomes output row (sum of cnt below l) + rank.  Slot 0's wave also writes the total.
__global__ __launch_bounds__(64) void orb_describe_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ blur, const OrbLevels lv,
                                                          const int* __restrict__ ncand, const long long* __restrict__ selR,
                                                          const int* __restrict__ selP, const int* __restrict__ trig,
                                                          const signed char* __restrict__ pattern, int* __restrict__ kp,
                                                          long long* __restrict__ resp, uint8_t* __restrict__ desc, int* __restrict__ n_out) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    int l = -1, base = 0, total = 0;
    for (int k = 0; k < lv.built; ++k) {
        const int cnt = min(min(ncand[k], lv.cand_cap[k]), lv.nfeat[k]);
        if (slot >= lv.sel_off[k] && slot < lv.sel_off[k] + lv.nfeat[k]) { l = k; base = total; }
        total += cnt;
    }
    if (slot == 0 && lane == 0) *n_out = total;
    if (l < 0) return;
    const int rank = slot - lv.sel_off[l];
    if (rank >= min(min(ncand[l], lv.cand_cap[l]), lv.nfeat[l])) return;
    const int row = base + rank;
    if (row >= lv.rows) return;                                    // cannot happen: rows >= the sum of nfeat
    const int H = lv.h[l], W = lv.w[l], P = selP[slot], y = P / W, x = P - y * W;
    const uint8_t* im = img + lv.off[l];
    const uint8_t* bl = blur + lv.off[l];
    const int umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    long long m10 = 0, m01 = 0;
    for (int i = lane; i < 31 * 31; i += 64) {
        const int v = i / 31 - 15, u = i - (v + 15) * 31 - 15;
        if (abs(u) <= umax[abs(v)]) {
            const int I = im[(size_t)(y + v) * W + x + u];
            m10 += u * I; m01 += v * I;
        }
    }
    m10 = flow_wave_sum(m10); m01 = flow_wave_sum(m01);
    int bin = 360;
    if (m10 != 0 || m01 != 0) {
        for (int k = lane; k < 360; k += 64)                       // ascending per lane: the first hit is the lane's smallest
            if (bin == 360 && orb_cross(trig, (2 * k + 719) % 720, m10, m01) >= 0 && orb_cross(trig, 2 * k + 1, m10, m01) < 0) bin = k;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bin = min(bin, __shfl_xor(bin, o));
    if (bin == 360) bin = 0;
    const long long Cs = trig[4 * bin], Sn = trig[4 * bin + 1];   // trig[2 bin] = (cos, sin) of bin degrees
    int nib = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const signed char* p = pattern + 4 * (4 * lane + b);
        const long long x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
        const int ax = (int)((x1 * Cs - y1 * Sn + (1ll << 29)) >> 30), ay = (int)((x1 * Sn + y1 * Cs + (1ll << 29)) >> 30);
        const int bx = (int)((x2 * Cs - y2 * Sn + (1ll << 29)) >> 30), by = (int)((x2 * Sn + y2 * Cs + (1ll << 29)) >> 30);
        // |pattern| <= 13 and edge >= 22 keep every read inside the level; the clamps make a table that breaks the rule harmless
        const int va = bl[(size_t)min(max(y + ay, 0), H - 1) * W + min(max(x + ax, 0), W - 1)];
        const int vb = bl[(size_t)min(max(y + by, 0), H - 1) * W + min(max(x + bx, 0), W - 1)];
        nib |= (va < vb ? 1 : 0) << b;
    }
    const int other = __shfl_xor(nib, 1);
    if ((lane & 1) == 0) desc[(size_t)row * 32 + (lane >> 1)] = (uint8_t)(nib | (other << 4));
    if (lane == 0) {
        kp[4 * (size_t)row] = x; kp[4 * (size_t)row + 1] = y; kp[4 * (size_t)row + 2] = l; kp[4 * (size_t)row + 3] = bin;
        resp[row] = selR[slot];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Bag of words.
struct BowVocab {
    const uint8_t* node_desc; const int* child_first; const int* child_count; const int* word_of; const double* word_weight;
    int n_nodes, n_words;
};
// grid (ceil(n_cap / 4)), one wave per descriptor, lane = child.  wid[i] = the word of descriptor i, BOW_NO_WORD for a row at or past
// n, a word of weight <= 0 and a walk that leaves the arrays (Python validates a vocabulary; the bounds here keep a bad one harmless)
__global__ __launch_bounds__(256) void bow_walk_kernel(const uint8_t* __restrict__ desc, const int* __restrict__ n_dev, int n_cap, const BowVocab v,
                                                       int* __restrict__ wid) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_cap) return;
    const int n = n_dev ? min(max(*n_dev, 0), n_cap) : n_cap;
    int word = -1;
    if (i < n) {
        const unsigned* q = (const unsigned*)(desc + (size_t)i * 32);
        unsigned qd[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) qd[j] = q[j];
        int node = 0;
        for (int step = 0; step <= BOW_MAX_DEPTH; ++step) {
            const int cc = v.child_count[node], cf = v.child_first[node];
            if (cc <= 0) { word = v.word_of[node]; break; }
            int key = BOW_NO_WORD;
            if (lane < cc && cf > node && cf + lane < v.n_nodes) {
                const unsigned* c = (const unsigned*)(v.node_desc + (size_t)(cf + lane) * 32);
                int dist = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) dist += __popc(qd[j] ^ c[j]);
                key = dist * 64 + lane;                            // the smallest distance, the first among equals
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o));
            if (key == BOW_NO_WORD) break;
            node = cf + (key & 63);
        }
    }
    if (lane == 0) {
        bool keep = false;
        if (word >= 0 && word < v.n_words) keep = v.word_weight[word] > 0.0;
        wid[i] = keep ? word : BOW_NO_WORD;
    }
}

// One workgroup of 1024 threads, n_cap <= ORB_MAX_ROWS.  Rank sort of the word ids in LDS (by value, then by index), heads and tails of
// the runs through one block scan -> words, counts; vals = count x weight; the L1 norm: thread t adds the words t, t + 1024, ... in
// ascending order, a xor butterfly over the lanes, the 16 wave sums in ascending order - the order depends on the number of words alone.
__global__ __launch_bounds__(1024) void bow_reduce_kernel(const int* __restrict__ wid, int n_cap, const double* __restrict__ weight,
                                                          int* __restrict__ words, int* __restrict__ counts, double* __restrict__ vals,
                                                          int* __restrict__ n_words) {
#pragma clang fp contract(off)
    STA_SKEW_ENTRY(1013);
    __shared__ int key[ORB_MAX_ROWS], sorted[ORB_MAX_ROWS], endv[ORB_MAX_ROWS];
    __shared__ int wcount[16];
    __shared__ double wsum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < n_cap; i += 1024) key[i] = wid[i];
    __syncthreads(); STA_SKEW(1005);
    for (int i = t; i < n_cap; i += 1024) {
        const int my = key[i];
        int r = 0;
        for (int j = 0; j < n_cap; ++j) { const int kj = key[j]; r += (kj < my || (kj == my && j < i)) ? 1 : 0; }
        sorted[r] = my;
    }
    __syncthreads(); STA_SKEW(1006);
    // thread t owns the consecutive elements [lo, hi)
    const int chunk = (n_cap + 1023) / 1024, lo = min(t * chunk, n_cap), hi = min(lo + chunk, n_cap);
    int heads = 0;
    for (int i = lo; i < hi; ++i) heads += (sorted[i] != BOW_NO_WORD && (i == 0 || sorted[i - 1] != sorted[i])) ? 1 : 0;
    int incl = heads;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
    if (lane == 63) wcount[wave] = incl;
    __syncthreads(); STA_SKEW(1007);
    int before = 0, nw = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { if (w < wave) before += wcount[w]; nw += wcount[w]; }
    int seen = before + incl - heads;                              // heads before element lo
    for (int i = lo; i < hi; ++i) {
        const int s = sorted[i];
        if (s == BOW_NO_WORD) break;
        if (i == 0 || sorted[i - 1] != s) { key[seen] = i; ++seen; }                      // key is free since the sort: start of run `seen`
        if (i == n_cap - 1 || sorted[i + 1] != s) endv[seen - 1] = i + 1;                 // a tail's run is the last head's at or before it
    }
    __syncthreads(); STA_SKEW(1008);
    double part = 0.0;
    for (int s = t; s < nw; s += 1024) {
        const int c = endv[s] - key[s], w = sorted[key[s]];
        words[s] = w; counts[s] = c;
        part += (double)c * weight[w];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) wsum[wave] = part;
    __syncthreads(); STA_SKEW(1009);
    double norm = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) norm += wsum[w];
    for (int s = t; s < nw; s += 1024) {
        const double val = (double)(endv[s] - key[s]) * weight[sorted[key[s]]];
        vals[s] = val / norm;                                      // every kept weight is > 0: norm > 0 whenever nw > 0
    }
    if (t == 0) *n_words = nw;
}

// grid (m), one wave per database row rows[blockIdx.x].  Lane l takes the query's words l, l + 64, ... in ascending order and looks each
// up in the row (sorted, distinct) by bisection; a xor butterfly adds the lanes.  sim = -0.5 sum(|a - b| - |a| - |b|) over the common
// words; a row index outside [0, max_views) scores 0.  The query holds at most q_cap entries, a row at most cap: the two are independent.
__global__ __launch_bounds__(64) void bow_score_kernel(const int* __restrict__ qw, const double* __restrict__ qv, const int* __restrict__ qn, int q_cap,
                                                       const int* __restrict__ dw, const double* __restrict__ dv, const int* __restrict__ dn,
                                                       int max_views, int cap, const int* __restrict__ rows, double* __restrict__ sim) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, r = rows[blockIdx.x];
    double sum = 0.0;
    if (r >= 0 && r < max_views) {
        const int nq = min(max(*qn, 0), q_cap), nd = min(max(dn[r], 0), cap);
        const int* w = dw + (size_t)r * cap;
        const double* v = dv + (size_t)r * cap;
        for (int i = lane; i < nq; i += 64) {
            const int want = qw[i];
            int lo = 0, hi = nd;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (w[mid] < want) lo = mid + 1; else hi = mid; }
            if (lo < nd && w[lo] == want) { const double a = qv[i], b = v[lo]; sum += (fabs(a - b) - fabs(a)) - fabs(b); }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) sim[blockIdx.x] = -0.5 * sum;
}
