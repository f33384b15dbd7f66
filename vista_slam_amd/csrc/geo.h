// f5: geometric consistency of depth maps (vista_slam/utils/slam_utils.py:269-419), included by sta_api.hip next to
// elementwise.h; launch code in sta_rows.inc.
//   view_consistency_check(depth, intrinsics, poses, threshold)       -> per-pixel vote over the +-window neighbouring views
//   compute_symmetric_geo_valid_mask(depths, intri, relative_pose)    -> per-edge forward / backward masks, err < 2 * median(err)
// Both warp a pixel of a source view into a target view: cam_t = M [K_s^-1 [x,y,1] d, 1], uvw = K_t cam_t.  A set-up kernel
// (one thread per warp) inverts and composes the matrices once, in double, so the per-pixel kernels only multiply:
//   cam_t = A [x,y,1] * d + t     with A = M[:3,:3] K_s^-1, t = M[:3,3], M = X^-1 Y (top three rows; see geo_compose).
#pragma once

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
    __syncthreads();
    if (active) atomicAdd(&lds[digit], 1u);
    __syncthreads();
    const unsigned c = lds[threadIdx.x];
    if (c) atomicAdd(&ghist[threadIdx.x], c);
}

// grid (ceil(HW / 256), 2, P): the warp, the rounded target pixel (round half to even), validity, err; counts valid pixels and
// valid NaN errors per slot and takes the first radix pass (top byte) on the way
__global__ __launch_bounds__(256) void geo_warp_kernel(const float* depths, const GeoPair* pairs, int H, int W, unsigned* err,
                                                       int* state, unsigned* hist0) {
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
