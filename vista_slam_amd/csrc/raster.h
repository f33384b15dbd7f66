// The headless rasteriser (libsta_raster.so; the contract is in include/sta_raster.h).  Launch code in sta_raster.hip.
//   rs_clear_kernel     every key = all-ones
//   rs_points_kernel    one lane per point: project, pack, a 64-bit atomicMin per footprint pixel behind an early-out load
//   rs_lines_kernel     one wavefront per segment: every lane clips the segment (the same arithmetic, so the same result), lanes over
//                       the DDA steps
//   rs_resolve_kernel   one lane per output pixel: keys -> rgba / depth / id, box filter over the ssaa block
// Every fp64 operation is written out and nothing is contracted (the pragma below holds to the end of the translation unit).
#pragma once
#pragma clang fp contract(off)

#define RS_EMPTY 0xFFFFFFFFFFFFFFFFull

struct RsCam {
    double T[12];
    double fx, fy, cx, cy;
    double near, far;
    double s, off;          // ssaa and (ssaa - 1) * 0.5
    int Hs, Ws;
};

__global__ __launch_bounds__(256) void rs_clear_kernel(unsigned long long* __restrict__ keys, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = RS_EMPTY;
}

__device__ __forceinline__ void rs_camera(const RsCam& c, const float* __restrict__ p, double* pc) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) pc[a] = ((c.T[4 * a] * x + c.T[4 * a + 1] * y) + c.T[4 * a + 2] * z) + c.T[4 * a + 3];
}

__device__ __forceinline__ bool rs_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and +-inf

// The footprint of size p around (ix, iy), clipped to the canvas; the bounds check of every write of the library.
// Measurement builds of tools/render_bench.py (never the product): RS_NO_EARLY_OUT issues every atomic; RS_NO_WRITE none (the pass
// without its key traffic); RS_COUNT_ATOMICS counts, in two further slots behind the four counters, the footprint pixels on the canvas
// [4] and the atomics the early-out load let through [5].
__device__ __forceinline__ void rs_splat(unsigned long long* __restrict__ keys, int Hs, int Ws, int ix, int iy, int p, unsigned long long key,
                                         unsigned long long* counters = nullptr) {
    const int lo = (p - 1) / 2, hi = p / 2;
    const int x0 = max(ix - lo, 0), x1 = min(ix + hi, Ws - 1), y0 = max(iy - lo, 0), y1 = min(iy + hi, Hs - 1);
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            unsigned long long* k = keys + (size_t)y * Ws + x;
#if defined(RS_NO_WRITE)
            if (key == 0ull) *k = key;                                          // (no key is 0: the depth is positive)
#elif defined(RS_NO_EARLY_OUT)
            atomicMin(k, key);
#elif defined(RS_COUNT_ATOMICS)
            if (counters) atomicAdd(counters + 4, 1ull);
            if (*k > key) { atomicMin(k, key); if (counters) atomicAdd(counters + 5, 1ull); }
#else
            if (*k > key) atomicMin(k, key);                                    // the early-out load: a stale value only costs the atomic
#endif
        }
}

__device__ __forceinline__ unsigned rs_channel(double c) {
    if (!(c == c)) return 0u;
    c = fmin(fmax(c, 0.0), 1.0);
    return (unsigned)rint(c * 255.0);
}

__device__ __forceinline__ void rs_count(unsigned long long* counters, int slot, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(counters + slot, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void rs_points_kernel(unsigned long long* __restrict__ keys, const RsCam c, const float* __restrict__ pts,
                                                        const void* __restrict__ colors, int color_kind, unsigned id_base, long long M,
                                                        int psize, unsigned long long* counters) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < M;
    bool bad = false, clipped = false, outside = false;
    int ix = 0, iy = 0;
    unsigned zbits = 0;
    if (live) {
        double pc[3];
        rs_camera(c, pts + 3 * (size_t)i, pc);
        bad = !(rs_finite(pc[0]) && rs_finite(pc[1]) && rs_finite(pc[2]));
        if (!bad) clipped = !(c.near <= pc[2] && pc[2] <= c.far);
        if (!bad && !clipped) {
            const double u = c.fx * (pc[0] / pc[2]) + c.cx, v = c.fy * (pc[1] / pc[2]) + c.cy;
            const double us = u * c.s + c.off, vs = v * c.s + c.off;
            const double fx = floor(us + 0.5), fy = floor(vs + 0.5);
            const double lo = (double)((psize - 1) / 2), hi = (double)(psize / 2);
            outside = !(fx + hi >= 0.0 && fx - lo <= (double)(c.Ws - 1) && fy + hi >= 0.0 && fy - lo <= (double)(c.Hs - 1));
            if (!outside) { ix = (int)fx; iy = (int)fy; zbits = __float_as_uint((float)pc[2]); }
        }
    }
    if (counters) {
        rs_count(counters, 0, live);
        rs_count(counters, 1, bad);
        rs_count(counters, 2, clipped);
        rs_count(counters, 3, outside);
    }
    if (!live || bad || clipped || outside) return;
    unsigned payload;
    if (color_kind == 1) {
        const unsigned char* q = (const unsigned char*)colors + 3 * (size_t)i;
        payload = ((unsigned)q[0] << 24) | ((unsigned)q[1] << 16) | ((unsigned)q[2] << 8) | 255u;
    } else if (color_kind == 2) {
        const float* q = (const float*)colors + 3 * (size_t)i;
        payload = (rs_channel((double)q[0]) << 24) | (rs_channel((double)q[1]) << 16) | (rs_channel((double)q[2]) << 8) | 255u;
    } else {
        payload = id_base + (unsigned)i;
    }
    rs_splat(keys, c.Hs, c.Ws, ix, iy, psize, ((unsigned long long)zbits << 32) | payload, counters);
}

// One end of the depth clip: t is the literal 0 / 1 (the end itself) or a parameter whose z is exactly `plane`.
__device__ __forceinline__ void rs_clip_end(const double* a, const double* b, double t, bool moved, double plane, const double* self, double* out) {
    if (!moved) { out[0] = self[0]; out[1] = self[1]; out[2] = self[2]; return; }
    out[0] = a[0] + t * (b[0] - a[0]);
    out[1] = a[1] + t * (b[1] - a[1]);
    out[2] = plane;
}

__global__ __launch_bounds__(256) void rs_lines_kernel(unsigned long long* __restrict__ keys, const RsCam c, const float* __restrict__ segs,
                                                       const unsigned char* __restrict__ colors, long long S, int width) {
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= S) return;
    double a[3], b[3];
    rs_camera(c, segs + 6 * (size_t)j, a);
    rs_camera(c, segs + 6 * (size_t)j + 3, b);
    if (!(rs_finite(a[0]) && rs_finite(a[1]) && rs_finite(a[2]) && rs_finite(b[0]) && rs_finite(b[1]) && rs_finite(b[2]))) return;
    const double za = a[2], zb = b[2], dz = zb - za;
    if ((za < c.near && zb < c.near) || (za > c.far && zb > c.far)) return;
    const bool m0 = za < c.near || za > c.far, m1 = zb < c.near || zb > c.far;
    const double pl0 = za < c.near ? c.near : c.far, pl1 = zb < c.near ? c.near : c.far;
    const double t0 = m0 ? (pl0 - za) / dz : 0.0, t1 = m1 ? (pl1 - za) / dz : 1.0;
    double e0p[3], e1p[3];
    rs_clip_end(a, b, t0, m0, pl0, a, e0p);
    rs_clip_end(a, b, t1, m1, pl1, b, e1p);
    const double us0 = (c.fx * (e0p[0] / e0p[2]) + c.cx) * c.s + c.off, vs0 = (c.fy * (e0p[1] / e0p[2]) + c.cy) * c.s + c.off;
    const double us1 = (c.fx * (e1p[0] / e1p[2]) + c.cx) * c.s + c.off, vs1 = (c.fy * (e1p[1] / e1p[2]) + c.cy) * c.s + c.off;
    const double w0 = 1.0 / e0p[2], w1 = 1.0 / e1p[2];
    const double lim = 1099511627776.0;
    if (!(fabs(us0) <= lim && fabs(vs0) <= lim && fabs(us1) <= lim && fabs(vs1) <= lim)) return;
    // Liang-Barsky
    const double xmin = -0.5 - 8.0, xmax = ((double)c.Ws - 0.5) + 8.0, ymin = -0.5 - 8.0, ymax = ((double)c.Hs - 0.5) + 8.0;
    const double dx = us1 - us0, dy = vs1 - vs0;
    double e0 = 0.0, e1 = 1.0;
    bool c0 = false, c1 = false;
    const double P[4] = {-dx, dx, -dy, dy}, Q[4] = {us0 - xmin, xmax - us0, vs0 - ymin, ymax - vs0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double p = P[e], q = Q[e];
        if (p == 0.0) { if (q < 0.0) return; }
        else if (p < 0.0) { const double r = q / p; if (r > e1) return; if (r > e0) { e0 = r; c0 = true; } }
        else { const double r = q / p; if (r < e0) return; if (r < e1) { e1 = r; c1 = true; } }
    }
    const double dw = w1 - w0;
    const double U0 = c0 ? us0 + e0 * dx : us0, V0 = c0 ? vs0 + e0 * dy : vs0, W0 = c0 ? w0 + e0 * dw : w0;
    const double U1 = c1 ? us0 + e1 * dx : us1, V1 = c1 ? vs0 + e1 * dy : vs1, W1 = c1 ? w0 + e1 * dw : w1;
    const double fax = floor(U0 + 0.5), fay = floor(V0 + 0.5), fbx = floor(U1 + 0.5), fby = floor(V1 + 0.5);
    const double lo = -16.0, hi = 8192.0 + 16.0;
    if (!(fax >= lo && fax < hi && fay >= lo && fay < hi && fbx >= lo && fbx < hi && fby >= lo && fby < hi)) return;
    const int ax = (int)fax, ay = (int)fay, bx = (int)fbx, by = (int)fby;
    const int n = max(abs(bx - ax), abs(by - ay));
    const unsigned char* q = colors + 3 * (size_t)j;
    const unsigned payload = ((unsigned)q[0] << 24) | ((unsigned)q[1] << 16) | ((unsigned)q[2] << 8) | 255u;
    const double dU = U1 - U0, dV = V1 - V0, dW = W1 - W0;
    for (int k = lane; k <= n; k += 64) {
        const double t = n > 0 ? (double)k / (double)n : 0.0;
        const double fx = floor((U0 + t * dU) + 0.5), fy = floor((V0 + t * dV) + 0.5);
        const double w = W0 + t * dW;
        if (!(fx >= lo && fx < hi && fy >= lo && fy < hi)) continue;      // (t is in [0, 1]: between the end pixels; kept as the write's own guard)
        const unsigned zbits = __float_as_uint((float)(1.0 / w));
        rs_splat(keys, c.Hs, c.Ws, (int)fx, (int)fy, width, ((unsigned long long)zbits << 32) | payload);
    }
}

struct RsBackground { unsigned char v[4]; };

__global__ __launch_bounds__(256) void rs_resolve_kernel(const unsigned long long* __restrict__ keys, int H, int W, int s, const RsBackground bg,
                                                         unsigned char* __restrict__ rgba, float* __restrict__ depth, unsigned* __restrict__ ids) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i % W);
    const size_t Ws = (size_t)W * s;
    unsigned long long best = RS_EMPTY;
    unsigned sum[4] = {0u, 0u, 0u, 0u};
    for (int sy = 0; sy < s; ++sy)
        for (int sx = 0; sx < s; ++sx) {
            const unsigned long long k = keys[((size_t)y * s + sy) * Ws + (size_t)x * s + sx];
            best = k < best ? k : best;
            if (k == RS_EMPTY) {
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) sum[ch] += bg.v[ch];
            } else {
                const unsigned p = (unsigned)k;
                sum[0] += p >> 24; sum[1] += (p >> 16) & 255u; sum[2] += (p >> 8) & 255u; sum[3] += s == 1 ? (p & 255u) : 255u;
            }
        }
    if (rgba) {
        const unsigned n = (unsigned)(s * s), h = n / 2;
        uchar4 o;
        o.x = (unsigned char)((sum[0] + h) / n); o.y = (unsigned char)((sum[1] + h) / n);
        o.z = (unsigned char)((sum[2] + h) / n); o.w = (unsigned char)((sum[3] + h) / n);
        ((uchar4*)rgba)[i] = o;
    }
    if (depth) depth[i] = best == RS_EMPTY ? __uint_as_float(0x7F800000u) : __uint_as_float((unsigned)(best >> 32));
    if (ids) ids[i] = (unsigned)best;
}
