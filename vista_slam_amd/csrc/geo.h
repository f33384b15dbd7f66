// f5: geometric consistency of depth maps (vista_slam/utils/slam_utils.py:269-419), included by sta_api.hip next to
// elementwise.h; launch code in sta_rows.inc.
//   view_consistency_check(depth, intrinsics, poses, threshold)       -> per-pixel vote over the +-window neighbouring views
//   compute_symmetric_geo_valid_mask(depths, intri, relative_pose)    -> per-edge forward / backward masks, err < 2 * median(err)
// Both warp a pixel of a source view into a target view: cam_t = M [K_s^-1 [x,y,1] d, 1], uvw = K_t cam_t.  A set-up kernel
// (one thread per warp) inverts and composes the matrices once, in double, so the per-pixel kernels only multiply:
//   cam_t = A [x,y,1] * d + t     with A = M[:3,:3] K_s^-1, t = M[:3,3], M = X^-1 Y (top three rows; see geo_compose).
// f6 (slam_utils.py:82-266), at the end of this file, reuses the set-up and generalises the selection:
//   compute_geo_valid_mask_batched(depth1, depth2, K1, K2, T1, T2, q) -> masks, err < torch.quantile(err of the whole batch, q)
//   compute_local_pointclouds / depth_from_pointcloud_dot_batched     -> element-wise behind one K^-1 per view
#pragma once
#include "sta_skew.h"       // STA_SKEW points: nothing unless -DSTA_WAVE_SKEW (libsta_mi355_skew.so)

struct GeoPair { float A[9]; float t[3]; float K[9]; float pad[3]; };      // 96 bytes per warp
static_assert(sizeof(GeoPair) == 96, "GeoPair layout");

// general inverses by cofactors, double (singular input -> inf / NaN entries, like torch.inverse's garbage: never an index)
__device__ inline void geo_inv3(const double* m, double* o) {
    const double A = m[4] * m[8] - m[5] * m[7], B = -(m[3] * m[8] - m[5] * m[6]), C = m[3] * m[7] - m[4] * m[6];
    const double id = 1.0 / (m[0] * A + m[1] * B + m[2] * C);
    o[0] = A * id; o[1] = -(m[1] * m[8] - m[2] * m[7]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = B * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id;  o[5] = -(m[0] * m[5] - m[2] * m[3]) * id;
    o[6] = C * id; o[7] = -(m[0] * m[7] - m[1] * m[6]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}
__device__ inline void geo_inv4(const double* m, double* inv) {
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double id = 1.0 / (m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12]);
    for (int q = 0; q < 16; ++q) inv[q] *= id;
}

// One warp: source intrinsics Ks, target intrinsics Kt, the source-to-common transform Y and the target-to-common transform X
// (either may be null = identity).  The reference drops the fourth coordinate after every 4x4 product and appends a fresh 1
// (`world[:3]`, `pts[:3]`), so only the top three rows of Y and of X^-1 take part:
//   cam_t = Xi[:3,:3] (Y[:3,:3] c + Y[:3,3]) + Xi[:3,3],   Xi = X^-1 (general 4x4 inverse, like torch.inverse).
__device__ inline void geo_compose(const float* Ks, const float* Kt, const float* Y, const float* X, GeoPair* out) {
    double ks[9], ki[9], y[16], xi[16];
    for (int q = 0; q < 9; ++q) ks[q] = (double)Ks[q];
    geo_inv3(ks, ki);
    for (int q = 0; q < 16; ++q) { y[q] = Y ? (double)Y[q] : (q % 5 == 0 ? 1.0 : 0.0); xi[q] = q % 5 == 0 ? 1.0 : 0.0; }
    if (X) {
        double x[16];
        for (int q = 0; q < 16; ++q) x[q] = (double)X[q];
        geo_inv4(x, xi);
    }
    double R[9], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = xi[r * 4] * y[c] + xi[r * 4 + 1] * y[4 + c] + xi[r * 4 + 2] * y[8 + c];
        t[r] = xi[r * 4] * y[3] + xi[r * 4 + 1] * y[7] + xi[r * 4 + 2] * y[11] + xi[r * 4 + 3];
    }
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out->A[r * 3 + c] = (float)(R[r * 3] * ki[c] + R[r * 3 + 1] * ki[3 + c] + R[r * 3 + 2] * ki[6 + c]);
        out->t[r] = (float)t[r];
    }
    for (int q = 0; q < 9; ++q) out->K[q] = Kt[q];
    out->pad[0] = out->pad[1] = out->pad[2] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------
// view_consistency_check (slam_utils.py:346-419).  pairs [n, S = 2w+1]: slot s of view i is neighbour j = i - w + s.
__global__ void vote_pairs_kernel(const float* K, const float* poses, int n, int w, GeoPair* pairs) {
    const int S = 2 * w + 1, id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n * S) return;
    const int i = id / S, j = i - w + (id - i * S);
    if (j < 0 || j >= n || j == i) return;
    geo_compose(K + i * 9, K + j * 9, poses + i * 16, poses + j * 16, pairs + id);
}

// one neighbour's bilinear tap (grid_sample, align_corners=True, zero padding): four loads from clamped addresses.  geo_tap only
// ISSUES them - the raw values travel with the in-frame bits of their corners, and nothing reads them before geo_agree, so the
// loop below keeps them in flight across the previous neighbour's compare.
struct GeoTap { float l00, l01, l10, l11, wx, wy, z; bool b00, b01, b10, b11; };
__device__ inline GeoTap geo_tap(const GeoPair& g, const float* dj, float fx, float fy, float d, int H, int W) {
    const float rx = fmaf(g.A[0], fx, fmaf(g.A[1], fy, g.A[2])), ry = fmaf(g.A[3], fx, fmaf(g.A[4], fy, g.A[5])),
                rz = fmaf(g.A[6], fx, fmaf(g.A[7], fy, g.A[8]));
    const float cx = fmaf(rx, d, g.t[0]), cy = fmaf(ry, d, g.t[1]), cz = fmaf(rz, d, g.t[2]);
    const float uw = g.K[6] * cx + g.K[7] * cy + g.K[8] * cz;               // the UNCLAMPED third coordinate divides
    const float u = (g.K[0] * cx + g.K[1] * cy + g.K[2] * cz) / uw, v = (g.K[3] * cx + g.K[4] * cy + g.K[5] * cz) / uw;
    const float x0 = floorf(u), y0 = floorf(v);
    // float comparisons: NaN / inf / huge coordinates fail them and never become an index
    const bool bx0 = x0 >= 0.f && x0 <= (float)(W - 1), bx1 = x0 >= -1.f && x0 <= (float)(W - 2);
    const bool by0 = y0 >= 0.f && y0 <= (float)(H - 1), by1 = y0 >= -1.f && y0 <= (float)(H - 2);
    const int ix0 = bx0 ? (int)x0 : 0, ix1 = bx1 ? (int)x0 + 1 : 0, iy0 = by0 ? (int)y0 : 0, iy1 = by1 ? (int)y0 + 1 : 0;
    GeoTap t;
    t.l00 = dj[iy0 * W + ix0]; t.l01 = dj[iy0 * W + ix1]; t.l10 = dj[iy1 * W + ix0]; t.l11 = dj[iy1 * W + ix1];
    t.b00 = bx0 && by0; t.b01 = bx1 && by0; t.b10 = bx0 && by1; t.b11 = bx1 && by1;
    t.wx = u - x0; t.wy = v - y0;
    t.z = cz < 1e-6f ? 1e-6f : cz;                                           // clamp(min=1e-6); NaN stays NaN
    return t;
}
__device__ inline int geo_agree(const GeoTap& t, float thr) {
    // a corner outside the frame is skipped, not multiplied (its weight may be inf / NaN)
    const float wx0 = 1.f - t.wx, wy0 = 1.f - t.wy;
    float s = 0.f;
    s += t.b00 ? t.l00 * (wx0 * wy0) : 0.f;
    s += t.b01 ? t.l01 * (t.wx * wy0) : 0.f;
    s += t.b10 ? t.l10 * (wx0 * t.wy) : 0.f;
    s += t.b11 ? t.l11 * (t.wx * t.wy) : 0.f;
    return fabsf(s - t.z) < thr ? 1 : 0;
}
// grid (ceil(HW / 256), n): view i is uniform per workgroup, so the pair matrices are scalar loads.  The loop issues
// neighbour k+1's four gathers before it compares neighbour k; it is unrolled by two over the taps a and b so that no tap is
// ever copied (a register move would wait for the loads it moves).
__global__ __launch_bounds__(256) void view_consistency_kernel(const float* depth, const GeoPair* pairs, int n, int H, int W, int w,
                                                               float thr, int32_t* count_out) {
    const int i = blockIdx.y, hw = H * W, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int y = pix / W, x = pix - y * W;
    const float fx = (float)x, fy = (float)y;
    const float d = depth[(int64_t)i * hw + pix];
    const int lo = max(0, i - w), hi = min(n, i + w + 1);
    const GeoPair* row = pairs + (int64_t)i * (2 * w + 1) + (w - i);         // row[j] = the warp i -> j
    int count = 0;
    int j = lo == i ? lo + 1 : lo;
    GeoTap a, b;
    if (j < hi) a = geo_tap(row[j], depth + (int64_t)j * hw, fx, fy, d, H, W);
    while (j < hi) {
        const int j1 = j + 1 == i ? j + 2 : j + 1;
        if (j1 < hi) b = geo_tap(row[j1], depth + (int64_t)j1 * hw, fx, fy, d, H, W);
        count += geo_agree(a, thr);
        if (j1 >= hi) break;
        j = j1 + 1 == i ? j1 + 2 : j1 + 1;
        if (j < hi) a = geo_tap(row[j], depth + (int64_t)j * hw, fx, fy, d, H, W);
        count += geo_agree(b, thr);
    }
    count_out[(int64_t)i * hw + pix] = count;
}

// ---------------------------------------------------------------------------------------------------------
// compute_symmetric_geo_valid_mask (slam_utils.py:269-343) for P edges: slot = p * 2 + direction.  Direction 0 warps view 0 by
// rel_pose and reads view 1, direction 1 warps view 1 by rel_pose^-1 and reads view 0.
// Workspace: err [P*2, HW] uint32 = the fp32 bits of |sampled - z| (sign bit clear, a NaN error included) or GEO_INVALID for a
// pixel that warps outside the frame; state [P*2, 8] int32; hist [4, P*2, 256] uint32.
constexpr unsigned GEO_INVALID = 0xffffffffu;
enum { GEO_COUNT = 0, GEO_NAN = 1, GEO_PREFIX = 2, GEO_K = 3, GEO_THRES = 4, GEO_STATE = 8 };

__global__ void sym_pairs_kernel(const float* K, const float* rel, int P, GeoPair* pairs) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= 2 * P) return;
    const int p = id >> 1;
    if ((id & 1) == 0) geo_compose(K + p * 9, K + p * 9, rel + p * 16, nullptr, pairs + id);
    else geo_compose(K + p * 9, K + p * 9, nullptr, rel + p * 16, pairs + id);
}

// one 8-bit digit of the block's keys into the slot's global histogram: LDS atomics, then one global add per non-empty bin
__device__ inline void geo_hist_block(unsigned* lds, bool active, unsigned digit, unsigned* ghist) {
    lds[threadIdx.x] = 0;                                  // (256 threads = 256 bins)
    __syncthreads(); STA_SKEW(800);
    if (active) atomicAdd(&lds[digit], 1u);
    __syncthreads(); STA_SKEW(801);
    const unsigned c = lds[threadIdx.x];
    if (c) atomicAdd(&ghist[threadIdx.x], c);
}

// grid (ceil(HW / 256), 2, P): the warp, the rounded target pixel (round half to even), validity, err; counts valid pixels and
// valid NaN errors per slot and takes the first radix pass (top byte) on the way
__global__ __launch_bounds__(256) void geo_warp_kernel(const float* depths, const GeoPair* pairs, int H, int W, unsigned* err,
                                                       int* state, unsigned* hist0) {
    STA_SKEW_ENTRY(807);
    __shared__ unsigned lds[256];
    __shared__ int wc[8];
    const int dir = blockIdx.y, slot = blockIdx.z * 2 + dir, hw = H * W, pix = blockIdx.x * 256 + threadIdx.x;
    const float* src = depths + (int64_t)slot * hw;
    const float* tgt = depths + (int64_t)(slot ^ 1) * hw;
    bool valid = false;
    unsigned bits = GEO_INVALID;
    if (pix < hw) {
        const GeoPair& g = pairs[slot];
        const int y = pix / W, x = pix - y * W;
        const float fx = (float)x, fy = (float)y, d = src[pix];
        const float rx = fmaf(g.A[0], fx, fmaf(g.A[1], fy, g.A[2])), ry = fmaf(g.A[3], fx, fmaf(g.A[4], fy, g.A[5])),
                    rz = fmaf(g.A[6], fx, fmaf(g.A[7], fy, g.A[8]));
        const float cx = fmaf(rx, d, g.t[0]), cy = fmaf(ry, d, g.t[1]), cz = fmaf(rz, d, g.t[2]);
        const float uw = (g.K[6] * cx + g.K[7] * cy + g.K[8] * cz) + 1e-8f;
        const float ur = rintf((g.K[0] * cx + g.K[1] * cy + g.K[2] * cz) / uw), vr = rintf((g.K[3] * cx + g.K[4] * cy + g.K[5] * cz) / uw);
        valid = ur >= 0.f && ur < (float)W && vr >= 0.f && vr < (float)H;      // NaN / inf fail and never become an index
        const int idx = valid ? (int)vr * W + (int)ur : 0;
        const float e = tgt[idx] - cz;
        if (valid) bits = __float_as_uint(e) & 0x7fffffffu;
        err[(int64_t)slot * hw + pix] = bits;
    }
    const bool isnan_ = valid && bits > 0x7f800000u;
    const unsigned long long bv = __ballot(valid), bn = __ballot(isnan_);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { wc[wave] = __popcll(bv); wc[4 + wave] = __popcll(bn); }
    geo_hist_block(lds, valid, bits >> 24, hist0 + slot * 256);              // (its barriers also publish wc)
    if (threadIdx.x == 0) {
        const int cv = wc[0] + wc[1] + wc[2] + wc[3], cn = wc[4] + wc[5] + wc[6] + wc[7];
        if (cv) atomicAdd(&state[slot * GEO_STATE + GEO_COUNT], cv);
        if (cn) atomicAdd(&state[slot * GEO_STATE + GEO_NAN], cn);
    }
}

// radix pass `pass` (1..3): keys whose top 8 * pass bits equal the prefix chosen so far
__global__ __launch_bounds__(256) void geo_hist_kernel(const unsigned* err, int hw, const int* state, int pass, unsigned* hist) {
    STA_SKEW_ENTRY(808);
    __shared__ unsigned lds[256];
    const int slot = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    const unsigned prefix = (unsigned)state[slot * GEO_STATE + GEO_PREFIX];
    const int hb = 32 - 8 * pass;
    const unsigned bits = pix < hw ? err[(int64_t)slot * hw + pix] : GEO_INVALID;
    const bool active = bits != GEO_INVALID && ((bits ^ prefix) >> hb) == 0;
    geo_hist_block(lds, active, (bits >> (hb - 8)) & 255u, hist + slot * 256);
}

// one wave per slot: the bin that holds the k-th smallest key of this pass; k = (count - 1) / 2 is torch.median's LOWER middle
// element.  After the last pass the prefix IS the median's bit pattern: thres = 2 * median, 1e10 for an empty direction, NaN
// when a valid error is NaN (torch.median propagates it).
__global__ __launch_bounds__(64) void geo_pick_kernel(const unsigned* hist, int pass, int* state, float* thres_out) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    int* st = state + slot * GEO_STATE;
    const int count = st[GEO_COUNT];
    if (count == 0) {
        if (pass == 3 && lane == 0) { st[GEO_THRES] = __float_as_int(1e10f); if (thres_out) thres_out[slot] = 1e10f; }
        return;
    }
    const int k = pass == 0 ? (count - 1) / 2 : st[GEO_K];
    const unsigned prefix = pass == 0 ? 0u : (unsigned)st[GEO_PREFIX];
    const unsigned* h = hist + slot * 256 + lane * 4;
    const int b0 = (int)h[0], b1 = (int)h[1], b2 = (int)h[2], b3 = (int)h[3];
    const int sum = b0 + b1 + b2 + b3;
    int incl = sum;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    const int excl = incl - sum;
    if (k >= excl && k < incl) {                           // exactly one lane: the pass's keys number more than k
        int r = k - excl, b = 0;
        if (r >= b0) { r -= b0; b = 1; if (r >= b1) { r -= b1; b = 2; if (r >= b2) { r -= b2; b = 3; } } }
        const unsigned np = prefix | ((unsigned)(lane * 4 + b) << (24 - 8 * pass));
        st[GEO_PREFIX] = (int)np; st[GEO_K] = r;
        if (pass == 3) {
            const float th = st[GEO_NAN] > 0 ? __uint_as_float(0x7fc00000u) : 2.0f * __uint_as_float(np);
            st[GEO_THRES] = __float_as_int(th);
            if (thres_out) thres_out[slot] = th;
        }
    }
}

// grid (ceil(HW / 256), P*2): mask = valid && err < thres, one byte per pixel
__global__ __launch_bounds__(256) void geo_mask_kernel(const unsigned* err, int hw, const int* state, uint8_t* mask) {
    const int slot = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const float thres = __int_as_float(state[slot * GEO_STATE + GEO_THRES]);
    const unsigned bits = err[(int64_t)slot * hw + pix];
    mask[(int64_t)slot * hw + pix] = bits != GEO_INVALID && __uint_as_float(bits) < thres ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------
// f6: compute_geo_valid_mask_batched (slam_utils.py:193-266), compute_local_pointclouds (:82-121) and
// depth_from_pointcloud_dot_batched (:124-165).
//   mask[b] = valid && |z2 - depth2[b, int(v2), int(u2)]| < quantile(valid errors of the WHOLE batch, q)
// The warp is geo_compose's with Y = T1[b], X = T2[b] and the two intrinsics rebuilt from the four entries the reference reads
// (fx, fy, cx, cy; :217-223, :243-249).  The error plane [B, HW] has f5's format and is selected from as ONE array: the state
// and the histograms below exist once per call, whatever B is.
//   state [GQ_STATE] int32; hist0 [256] (top byte, shared by both ranks); hist [3 passes, 2 ranks, 256].
enum { GQ_COUNT = 0, GQ_NAN = 1, GQ_PREFIX = 2 /* +rank */, GQ_K = 4 /* +rank */, GQ_THRES = 6, GQ_STATE = 8 };
constexpr int GQ_PER = 8;                                  // keys per thread of geo_q_hist_kernel

__device__ inline void geo_four_entries(const float* K, float* o) {
    o[0] = K[0]; o[1] = 0.f; o[2] = K[2]; o[3] = 0.f; o[4] = K[4]; o[5] = K[5]; o[6] = 0.f; o[7] = 0.f; o[8] = 1.f;
}
__global__ void geo_q_pairs_kernel(const float* K1, const float* K2, const float* T1, const float* T2, int B, GeoPair* pairs) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float ks[9], kt[9];
    geo_four_entries(K1 + b * 9, ks); geo_four_entries(K2 + b * 9, kt);
    geo_compose(ks, kt, T1 + b * 16, T2 + b * 16, pairs + b);
}

// grid (B * gx), gx = ceil(HW / 256): image b = blockIdx.x / gx is uniform per workgroup.  u2 = fx2 x2 / z2 + cx2 divides by the
// unclamped z2 (no epsilon; a point behind camera 2 projects like any other), the target pixel is the coordinate TRUNCATED toward
// zero, so (-1, 0) lands on column 0.  The float comparisons fail for NaN / inf / beyond-int32 values: never an index.
__global__ __launch_bounds__(256) void geo_q_warp_kernel(const float* depth1, const float* depth2, const GeoPair* pairs, int H, int W,
                                                         int gx, unsigned* err, int* state, unsigned* hist0) {
    STA_SKEW_ENTRY(809);
    __shared__ unsigned lds[256];
    __shared__ int wc[8];
    const int b = blockIdx.x / gx, hw = H * W, pix = (blockIdx.x - b * gx) * 256 + threadIdx.x;
    bool valid = false;
    unsigned bits = GEO_INVALID;
    if (pix < hw) {
        const GeoPair& g = pairs[b];
        const int y = pix / W, x = pix - y * W;
        const float fx = (float)x, fy = (float)y, d = depth1[(int64_t)b * hw + pix];
        const float rx = fmaf(g.A[0], fx, fmaf(g.A[1], fy, g.A[2])), ry = fmaf(g.A[3], fx, fmaf(g.A[4], fy, g.A[5])),
                    rz = fmaf(g.A[6], fx, fmaf(g.A[7], fy, g.A[8]));
        const float cx = fmaf(rx, d, g.t[0]), cy = fmaf(ry, d, g.t[1]), cz = fmaf(rz, d, g.t[2]);
        const float u = g.K[0] * cx / cz + g.K[2], v = g.K[4] * cy / cz + g.K[5];
        valid = u > -1.f && u < (float)W && v > -1.f && v < (float)H;
        const int idx = valid ? (int)v * W + (int)u : 0;
        const float e = cz - depth2[(int64_t)b * hw + idx];
        if (valid) bits = __float_as_uint(e) & 0x7fffffffu;
        err[(int64_t)b * hw + pix] = bits;
    }
    const bool isnan_ = valid && bits > 0x7f800000u;
    const unsigned long long bv = __ballot(valid), bn = __ballot(isnan_);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { wc[wave] = __popcll(bv); wc[4 + wave] = __popcll(bn); }
    geo_hist_block(lds, valid, bits >> 24, hist0);                           // (its barriers also publish wc)
    if (threadIdx.x == 0) {
        const int cv = wc[0] + wc[1] + wc[2] + wc[3], cn = wc[4] + wc[5] + wc[6] + wc[7];
        if (cv) atomicAdd(&state[GQ_COUNT], cv);
        if (cn) atomicAdd(&state[GQ_NAN], cn);
    }
}

// radix pass `pass` (1..3) for both ranks at once: hist [2, 256], rank r counts the keys under its own prefix.  A workgroup takes
// 256 * GQ_PER consecutive keys, so the number of global adds per pass stays small next to the number of keys.
__global__ __launch_bounds__(256) void geo_q_hist_kernel(const unsigned* err, int total, const int* state, int pass, unsigned* hist) {
    STA_SKEW_ENTRY(805);
    __shared__ unsigned lds[512];
    const unsigned p0 = (unsigned)state[GQ_PREFIX], p1 = (unsigned)state[GQ_PREFIX + 1];
    const int hb = 32 - 8 * pass;
    lds[threadIdx.x] = 0; lds[256 + threadIdx.x] = 0;
    __syncthreads(); STA_SKEW(802);
    const int base = blockIdx.x * (256 * GQ_PER) + threadIdx.x;
#pragma unroll
    for (int q = 0; q < GQ_PER; ++q) {
        const int i = base + q * 256;
        const unsigned bits = i < total ? err[i] : GEO_INVALID;
        if (bits == GEO_INVALID) continue;
        const unsigned digit = (bits >> (hb - 8)) & 255u;
        if (((bits ^ p0) >> hb) == 0) atomicAdd(&lds[digit], 1u);
        if (((bits ^ p1) >> hb) == 0) atomicAdd(&lds[256 + digit], 1u);
    }
    __syncthreads(); STA_SKEW(803);
    const unsigned c0 = lds[threadIdx.x], c1 = lds[256 + threadIdx.x];
    if (c0) atomicAdd(&hist[threadIdx.x], c0);
    if (c1) atomicAdd(&hist[256 + threadIdx.x], c1);
}

// One workgroup of two waves, wave r = rank r.  Pass 0 fixes the ranks the way torch.quantile (linear interpolation) does, in
// fp32: rank = q * (n - 1), lo = floor, hi = ceil; both waves read hist0.  After pass 3 the two prefixes ARE the bit patterns of
// the lo-th and the hi-th smallest error a and b, and thres = lerp(a, b, w = rank - lo) as ATen evaluates it: one fused
// multiply-add per branch, w < 0.5 ? fma(w, b - a, a) : fma(-(b - a), 1 - w, b).  NaN when a valid error is NaN (quantile
// propagates it) or when no pixel is valid (torch raises; the caller reads count_out).
__global__ __launch_bounds__(128) void geo_q_pick_kernel(const unsigned* hist, int pass, float q, int* st, float* thres_out, int* count_out) {
    STA_SKEW_ENTRY(806);
    __shared__ unsigned ab[2];
    const int r = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int count = st[GQ_COUNT];
    if (count == 0) {                                      // (uniform: the whole workgroup leaves)
        if (pass == 3 && threadIdx.x == 0) {
            st[GQ_THRES] = (int)0x7fc00000u;
            if (thres_out) *thres_out = __uint_as_float(0x7fc00000u);
            if (count_out) *count_out = 0;
        }
        return;
    }
    const float rank = __fmul_rn(q, (float)(count - 1));
    int k;
    unsigned prefix = 0u;
    if (pass == 0) {
        k = (int)(r == 0 ? floorf(rank) : ceilf(rank));
        k = k < 0 ? 0 : (k > count - 1 ? count - 1 : k);
    } else { k = st[GQ_K + r]; prefix = (unsigned)st[GQ_PREFIX + r]; }
    const unsigned* h = hist + (pass == 0 ? 0 : r * 256) + lane * 4;
    const int b0 = (int)h[0], b1 = (int)h[1], b2 = (int)h[2], b3 = (int)h[3];
    const int sum = b0 + b1 + b2 + b3;
    int incl = sum;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    const int excl = incl - sum;
    if (k >= excl && k < incl) {                           // exactly one lane per wave: the pass's keys number more than k
        int rr = k - excl, bn = 0;
        if (rr >= b0) { rr -= b0; bn = 1; if (rr >= b1) { rr -= b1; bn = 2; if (rr >= b2) { rr -= b2; bn = 3; } } }
        const unsigned np = prefix | ((unsigned)(lane * 4 + bn) << (24 - 8 * pass));
        st[GQ_PREFIX + r] = (int)np; st[GQ_K + r] = rr;    // (wave r reads and writes only its own two words)
        ab[r] = np;
    }
    if (pass != 3) return;
    __syncthreads(); STA_SKEW(804);
    if (threadIdx.x == 0) {
        const float a = __uint_as_float(ab[0]), b = __uint_as_float(ab[1]);
        const float w = rank - floorf(rank), diff = b - a;
        float th = w < 0.5f ? fmaf(w, diff, a) : fmaf(-diff, 1.0f - w, b);
        if (st[GQ_NAN] > 0) th = __uint_as_float(0x7fc00000u);
        st[GQ_THRES] = __float_as_int(th);
        if (thres_out) *thres_out = th;
        if (count_out) *count_out = count;
    }
}

// mask = valid && err < thres over the whole error plane, one byte per pixel (a NaN threshold leaves it all 0)
__global__ __launch_bounds__(256) void geo_q_mask_kernel(const unsigned* err, int total, const int* state, uint8_t* mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float thres = __int_as_float(state[GQ_THRES]);
    const unsigned bits = err[i];
    mask[i] = bits != GEO_INVALID && __uint_as_float(bits) < thres ? 1 : 0;
}

// K^-1 of every view (n = 1 for shared intrinsics), once, in double
__global__ void geo_kinv_kernel(const float* K, int n, float* kinv) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double k[9], ki[9];
    for (int q = 0; q < 9; ++q) k[q] = (double)K[v * 9 + q];
    geo_inv3(k, ki);
    for (int q = 0; q < 9; ++q) kinv[v * 9 + q] = (float)ki[q];
}

// compute_local_pointclouds: out[n, y, x, :] = K^-1 [x, y, 1] * depth.  grid (N * gx), gx = ceil(3 HW / 256): one thread per
// OUTPUT float, so the stores are contiguous (the three threads of a pixel share its depth load).
__global__ __launch_bounds__(256) void geo_local_points_kernel(const float* depths, const float* kinv, int k_batched, int H, int W,
                                                               int gx, float* out) {
    const int n = blockIdx.x / gx, hw = H * W, e = (blockIdx.x - n * gx) * 256 + threadIdx.x;
    if (e >= 3 * hw) return;
    const int pix = e / 3, c = e - pix * 3, y = pix / W, x = pix - y * W;
    const float* ki = kinv + (k_batched ? n * 9 : 0) + c * 3;
    const float ray = fmaf(ki[0], (float)x, fmaf(ki[1], (float)y, ki[2]));
    out[(int64_t)n * 3 * hw + e] = ray * depths[(int64_t)n * hw + pix];
}

// depth_from_pointcloud_dot_batched: the dot product of each point with its unit ray K^-1 [x, y, 1] / |.|
__global__ __launch_bounds__(256) void geo_ray_depth_kernel(const float* pts, const float* kinv, int k_batched, int H, int W, int gx,
                                                            float* out) {
    const int n = blockIdx.x / gx, hw = H * W, pix = (blockIdx.x - n * gx) * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int y = pix / W, x = pix - y * W;
    const float* ki = kinv + (k_batched ? n * 9 : 0);
    const float fx = (float)x, fy = (float)y;
    const float rx = fmaf(ki[0], fx, fmaf(ki[1], fy, ki[2])), ry = fmaf(ki[3], fx, fmaf(ki[4], fy, ki[5])),
                rz = fmaf(ki[6], fx, fmaf(ki[7], fy, ki[8]));
    const float nrm = sqrtf(rx * rx + ry * ry + rz * rz);
    const float* p = pts + ((int64_t)n * hw + pix) * 3;
    out[(int64_t)n * hw + pix] = p[0] * (rx / nrm) + p[1] * (ry / nrm) + p[2] * (rz / nrm);
}
