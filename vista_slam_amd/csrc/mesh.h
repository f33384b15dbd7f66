// Triangles for the headless rasteriser and vertex normals (libsta_mesh.so; the contract is in include/sta_mesh.h).  Launch code in
// sta_mesh.hip.  raster.h (the camera, the channel rule, the per-wave counters) and voxel.h (the stable radix sort) are included unchanged.
//   ms_setup_kernel     one lane per triangle: camera, near clip, and per piece snap, area, cull, box; a piece whose clamped box has at
//                       most MS_SMALL_MAX pixels is drawn by the lane, a larger one is appended to the list in the caller's workspace
//   ms_drain_kernel     a fixed grid of wavefronts over that list: every lane of a wave repeats the triangle's setup with the same
//                       arithmetic (nothing floating-point crosses lanes), the lanes go over the box's pixels
//   ms_pair_kernel      the 3 nt (vertex, corner) pairs of the vertex normals: key = the vertex (nv for a triangle with a bad index)
//   ms_normal_kernel    one lane per vertex: binary search of its run in the sorted pairs, the face normals summed in order
// Every fp64 operation is written out and nothing is contracted (raster.h's pragma holds to the end of the translation unit).
#pragma once
#pragma clang fp contract(off)

// The largest clamped box (in key-buffer pixels) a setup lane draws itself.  A tuning value, not part of the contract: measured with
// tools/mesh_bench.py --threshold (profiles/r28_mesh.txt).
#ifndef MS_SMALL_MAX
#define MS_SMALL_MAX 64
#endif
#define MS_DRAIN_BLOCKS 2048        // x 4 wavefronts

struct MsParams {
    RsCam cam;
    const float* verts; const int* tris; const float* colors;
    long long nv, nt;
    double ucol[3];                 // colors == NULL: the call's one colour
    double eye[3], ambient;
    int kind, lit, cull;
    unsigned id_base;
    unsigned long long* keys;
    unsigned long long* counters;
    unsigned* list; unsigned* list_n;
};

struct MsVert { double x, y, z, c[3]; };
struct MsPiece {
    long long X[3], Y[3], A2;
    double w[3], q[3][3];           // 1 / z and colour * (1 / z) per vertex
    int x0, x1, y0, y1;
};
struct MsTri { MsVert p[4]; double L; unsigned payload; int np; };      // np pieces: (p0, p1, p2) and (p0, p2, p3)

#define MS_BAD 1
#define MS_BEHIND 2
#define MS_CLIPPED 4
#define MS_TOO_LARGE 1
#define MS_DEGENERATE 2
#define MS_CULLED 3
#define MS_OFF 4

__device__ __forceinline__ unsigned ms_pack(double r, double g, double b) {
    return (rs_channel(r) << 24) | (rs_channel(g) << 16) | (rs_channel(b) << 8) | 255u;
}

// P(in, out) of the header
__device__ __forceinline__ void ms_cut(const MsVert& in, const MsVert& out, double near, bool colours, MsVert& r) {
    const double t = (near - in.z) / (out.z - in.z);
    r.x = in.x + t * (out.x - in.x);
    r.y = in.y + t * (out.y - in.y);
    r.z = near;
    if (colours) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) r.c[ch] = in.c[ch] + t * (out.c[ch] - in.c[ch]);
    }
}

// Triangle t -> its pieces, payload and light factor.  Returns MS_BAD, MS_BEHIND (T.np = 0), 0 or MS_CLIPPED.
__device__ __forceinline__ int ms_triangle(const MsParams& P, long long t, MsTri& T) {
    T.np = 0; T.L = 1.0; T.payload = 0u;
    const int i0 = P.tris[3 * (size_t)t], i1 = P.tris[3 * (size_t)t + 1], i2 = P.tris[3 * (size_t)t + 2];
    if (i0 < 0 || i0 >= P.nv || i1 < 0 || i1 >= P.nv || i2 < 0 || i2 >= P.nv) return MS_BAD;
    const float* A = P.verts + 3 * (size_t)i0; const float* B = P.verts + 3 * (size_t)i1; const float* Cc = P.verts + 3 * (size_t)i2;
    MsVert v0, v1, v2;
    double pc[3];
    rs_camera(P.cam, A, pc); v0.x = pc[0]; v0.y = pc[1]; v0.z = pc[2];
    rs_camera(P.cam, B, pc); v1.x = pc[0]; v1.y = pc[1]; v1.z = pc[2];
    rs_camera(P.cam, Cc, pc); v2.x = pc[0]; v2.y = pc[1]; v2.z = pc[2];
    if (!(rs_finite(v0.x) && rs_finite(v0.y) && rs_finite(v0.z) && rs_finite(v1.x) && rs_finite(v1.y) && rs_finite(v1.z) &&
          rs_finite(v2.x) && rs_finite(v2.y) && rs_finite(v2.z))) return MS_BAD;
    const double near = P.cam.near;
    const bool in0 = v0.z >= near, in1 = v1.z >= near, in2 = v2.z >= near;
    const int nin = (int)in0 + (int)in1 + (int)in2;
    if (nin == 0) return MS_BEHIND;
    const bool colours = P.kind == 1 && P.colors != nullptr;
    if (colours) {
        const float* ca = P.colors + 3 * (size_t)i0; const float* cb = P.colors + 3 * (size_t)i1; const float* cc = P.colors + 3 * (size_t)i2;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { v0.c[ch] = (double)ca[ch]; v1.c[ch] = (double)cb[ch]; v2.c[ch] = (double)cc[ch]; }
    }
    if (P.kind == 0) T.payload = P.id_base + (unsigned)t;
    if (P.kind == 2 || P.lit) {
        const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
        const double ux = (double)B[0] - ax, uy = (double)B[1] - ay, uz = (double)B[2] - az;
        const double vx = (double)Cc[0] - ax, vy = (double)Cc[1] - ay, vz = (double)Cc[2] - az;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
        if (P.kind == 2) {
            T.payload = nn > 0.0 ? ms_pack((nx / nn) * 0.5 + 0.5, (ny / nn) * 0.5 + 0.5, (nz / nn) * 0.5 + 0.5) : ms_pack(0.5, 0.5, 0.5);
        } else {
            const double dx = P.eye[0] - ax, dy = P.eye[1] - ay, dz = P.eye[2] - az;
            const double dd = sqrt((dx * dx + dy * dy) + dz * dz);
            const double dot = (nx * dx + ny * dy) + nz * dz;
            T.L = (nn > 0.0 && dd > 0.0) ? P.ambient + (1.0 - P.ambient) * (fabs(dot) / (nn * dd)) : P.ambient;
        }
    }
    if (P.kind == 1 && !colours) T.payload = ms_pack(P.ucol[0] * T.L, P.ucol[1] * T.L, P.ucol[2] * T.L);
    if (nin == 3) { T.p[0] = v0; T.p[1] = v1; T.p[2] = v2; T.np = 1; return 0; }
    // (i, j, k): the cyclic rotation that starts at the one vertex that is in (nin == 1) or out (nin == 2)
    const int i = nin == 1 ? (in0 ? 0 : in1 ? 1 : 2) : (!in0 ? 0 : !in1 ? 1 : 2);
    const MsVert vi = i == 0 ? v0 : i == 1 ? v1 : v2, vj = i == 0 ? v1 : i == 1 ? v2 : v0, vk = i == 0 ? v2 : i == 1 ? v0 : v1;
    if (nin == 1) {
        T.p[0] = vi; ms_cut(vi, vj, near, colours, T.p[1]); ms_cut(vi, vk, near, colours, T.p[2]);
        T.np = 1;
    } else {
        T.p[0] = vj; T.p[1] = vk; ms_cut(vk, vi, near, colours, T.p[2]); ms_cut(vj, vi, near, colours, T.p[3]);
        T.np = 2;
    }
    return MS_CLIPPED;
}

// A piece (a, b, c): snap, area, cull, box.  Returns 0 (to draw) or the reason it is dropped.
__device__ __forceinline__ int ms_piece(const MsParams& P, const MsVert& a, const MsVert& b, const MsVert& c, bool colours, MsPiece& S) {
    const RsCam& cam = P.cam;
    const MsVert* v[3] = {&a, &b, &c};
    const double lim = 268435456.0;
    bool big = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double us = (cam.fx * (v[k]->x / v[k]->z) + cam.cx) * cam.s + cam.off, vs = (cam.fy * (v[k]->y / v[k]->z) + cam.cy) * cam.s + cam.off;
        const double xd = floor(us * 256.0 + 0.5), yd = floor(vs * 256.0 + 0.5);
        if (!(fabs(xd) <= lim && fabs(yd) <= lim)) { big = true; S.X[k] = 0; S.Y[k] = 0; }
        else { S.X[k] = (long long)xd; S.Y[k] = (long long)yd; }
        S.w[k] = 1.0 / v[k]->z;
        if (colours) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) S.q[k][ch] = v[k]->c[ch] * S.w[k];
        }
    }
    if (big) return MS_TOO_LARGE;
    long long A2 = (S.X[1] - S.X[0]) * (S.Y[2] - S.Y[0]) - (S.Y[1] - S.Y[0]) * (S.X[2] - S.X[0]);
    if (A2 == 0) return MS_DEGENERATE;
    if ((P.cull == 1 && A2 > 0) || (P.cull == 2 && A2 < 0)) return MS_CULLED;
    if (A2 < 0) {
        A2 = -A2;
        long long tl = S.X[1]; S.X[1] = S.X[2]; S.X[2] = tl;
        tl = S.Y[1]; S.Y[1] = S.Y[2]; S.Y[2] = tl;
        double td = S.w[1]; S.w[1] = S.w[2]; S.w[2] = td;
        if (colours) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { td = S.q[1][ch]; S.q[1][ch] = S.q[2][ch]; S.q[2][ch] = td; }
        }
    }
    S.A2 = A2;
    const long long xmin = min(S.X[0], min(S.X[1], S.X[2])), xmax = max(S.X[0], max(S.X[1], S.X[2]));
    const long long ymin = min(S.Y[0], min(S.Y[1], S.Y[2])), ymax = max(S.Y[0], max(S.Y[1], S.Y[2]));
    // (>> floors: ceil(a / 256) = floor((a + 255) / 256)); the clamp makes the four fit an int and is the bounds check of every write
    const long long x0 = max((xmin + 255) >> 8, 0ll), x1 = min(xmax >> 8, (long long)cam.Ws - 1);
    const long long y0 = max((ymin + 255) >> 8, 0ll), y1 = min(ymax >> 8, (long long)cam.Hs - 1);
    if (x0 > x1 || y0 > y1) return MS_OFF;
    S.x0 = (int)x0; S.x1 = (int)x1; S.y0 = (int)y0; S.y1 = (int)y1;
    return 0;
}

__device__ __forceinline__ bool ms_edge_in(long long e, long long dx, long long dy) { return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0))); }

// One pixel (x, y) of the piece's clamped box: coverage, depth, payload, the merge.
// Measurement builds of tools/mesh_bench.py (never the product): MS_COUNT_ATOMICS counts, in three further slots behind the eight
// counters, the covered fragments that pass the far test [8], the atomics the early-out load let through [9] and (in ms_setup_kernel)
// the pieces that reach the draw [10].
__device__ __forceinline__ void ms_fragment(const MsParams& P, const MsPiece& S, bool colours, unsigned payload, double L, int x, int y) {
    const long long px = 256ll * x, py = 256ll * y;
    const long long dx0 = S.X[2] - S.X[1], dy0 = S.Y[2] - S.Y[1];       // b -> c
    const long long dx1 = S.X[0] - S.X[2], dy1 = S.Y[0] - S.Y[2];       // c -> a
    const long long dx2 = S.X[1] - S.X[0], dy2 = S.Y[1] - S.Y[0];       // a -> b
    const long long e0 = dx0 * (py - S.Y[1]) - dy0 * (px - S.X[1]);
    const long long e1 = dx1 * (py - S.Y[2]) - dy1 * (px - S.X[2]);
    const long long e2 = dx2 * (py - S.Y[0]) - dy2 * (px - S.X[0]);
    if (!(ms_edge_in(e0, dx0, dy0) && ms_edge_in(e1, dx1, dy1) && ms_edge_in(e2, dx2, dy2))) return;
    const double f0 = (double)e0, f1 = (double)e1, f2 = (double)e2, fa = (double)S.A2;
    const double w = ((f0 * S.w[0] + f1 * S.w[1]) + f2 * S.w[2]) / fa;
    const double depth = 1.0 / w;
    if (!(depth <= P.cam.far)) return;
    if (colours) {
        double c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double cw = ((f0 * S.q[0][ch] + f1 * S.q[1][ch]) + f2 * S.q[2][ch]) / fa;
            c[ch] = cw / w;
            if (P.lit) c[ch] = c[ch] * L;
        }
        payload = ms_pack(c[0], c[1], c[2]);
    }
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)depth) << 32) | payload;
    unsigned long long* k = P.keys + (size_t)y * P.cam.Ws + x;          // (x, y) is inside the clamped box: on the canvas
#if defined(MS_COUNT_ATOMICS)
    if (P.counters) atomicAdd(P.counters + 8, 1ull);
    if (*k > key) { atomicMin(k, key); if (P.counters) atomicAdd(P.counters + 9, 1ull); }
#else
    if (*k > key) atomicMin(k, key);                                    // the early-out load: a stale value only costs the atomic
#endif
}

__global__ __launch_bounds__(256) void ms_setup_kernel(const MsParams P) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < P.nt;
    const bool colours = P.kind == 1 && P.colors != nullptr;
    MsTri T; T.np = 0;
    int flags = 0;
    if (live) flags = ms_triangle(P, t, T);
    if (P.counters) {
        rs_count(P.counters, 0, live);
        rs_count(P.counters, 1, flags == MS_BAD);
        rs_count(P.counters, 2, flags == MS_BEHIND);
        rs_count(P.counters, 3, flags == MS_CLIPPED);
    }
    for (int p = 0; p < 2; ++p) {                                        // (uniform: the ballots of rs_count need every lane)
        MsPiece S;
        int why = -1;
        if (p < T.np) why = ms_piece(P, T.p[0], p == 0 ? T.p[1] : T.p[2], p == 0 ? T.p[2] : T.p[3], colours, S);
        if (P.counters) {
            rs_count(P.counters, 4, why == MS_TOO_LARGE);
            rs_count(P.counters, 5, why == MS_DEGENERATE);
            rs_count(P.counters, 6, why == MS_CULLED);
            rs_count(P.counters, 7, why == MS_OFF);
#if defined(MS_COUNT_ATOMICS)
            rs_count(P.counters, 10, why == 0);
#endif
        }
        if (why != 0) continue;
        const long long area = (long long)(S.x1 - S.x0 + 1) * (S.y1 - S.y0 + 1);
        if (area > MS_SMALL_MAX) {
            const unsigned at = atomicAdd(P.list_n, 1u);                  // at < 2 nt: at most two pieces per triangle
            P.list[at] = ((unsigned)t << 1) | (unsigned)p;
            continue;
        }
        for (int y = S.y0; y <= S.y1; ++y)
            for (int x = S.x0; x <= S.x1; ++x) ms_fragment(P, S, colours, T.payload, T.L, x, y);
    }
}

__global__ __launch_bounds__(256) void ms_drain_kernel(const MsParams P) {
    const long long n = min((long long)*P.list_n, 2 * P.nt);            // (the setup pass appends at most 2 nt: the reads' own guard)
    const int lane = threadIdx.x & 63;
    const bool colours = P.kind == 1 && P.colors != nullptr;
    // (a 64-bit index: n can be 2^32 - 2, and a 32-bit one would wrap before it reaches it)
    for (long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += (long long)gridDim.x * 4) {
        const unsigned ent = P.list[e];
        const long long t = (long long)(ent >> 1);
        const int p = (int)(ent & 1u);
        if (t >= P.nt) continue;                                          // (the setup pass wrote t < nt: kept as the read's own guard)
        MsTri T;
        ms_triangle(P, t, T);
        if (p >= T.np) continue;
        MsPiece S;
        if (ms_piece(P, T.p[0], p == 0 ? T.p[1] : T.p[2], p == 0 ? T.p[2] : T.p[3], colours, S) != 0) continue;
        const unsigned bw = (unsigned)(S.x1 - S.x0 + 1), area = bw * (unsigned)(S.y1 - S.y0 + 1);      // at most 8192 x 8192 = 2^26 pixels
        for (unsigned i = (unsigned)lane; i < area; i += 64u) ms_fragment(P, S, colours, T.payload, T.L, S.x0 + (int)(i % bw), S.y0 + (int)(i / bw));
    }
}

// ---------------------------------------------------------------------------------------------------------
// Vertex normals
__global__ __launch_bounds__(256) void ms_pair_kernel(const int* __restrict__ tris, int m, long long nv, unsigned long long* __restrict__ key,
                                                      int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int t = i / 3;
    const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    const bool ok = a >= 0 && a < nv && b >= 0 && b < nv && c >= 0 && c < nv;
    key[i] = ok ? (unsigned long long)tris[i] : (unsigned long long)nv;      // nv sorts behind every vertex
    idx[i] = i;
}

__global__ __launch_bounds__(256) void ms_normal_kernel(const float* __restrict__ verts, const int* __restrict__ tris, long long nv, int m,
                                                        const unsigned long long* __restrict__ key, const int* __restrict__ idx,
                                                        float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    int lo = 0, hi = m;                                                   // the first position whose key is >= v
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] < (unsigned long long)v) lo = mid + 1; else hi = mid;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int r = lo; r < m && key[r] == (unsigned long long)v; ++r) {
        const int t = idx[r] / 3;
        if (t < 0 || 3 * (long long)t + 2 >= m) break;                    // (idx is a permutation of [0, m): kept as the read's own guard)
        const int ia = tris[3 * (size_t)t], ib = tris[3 * (size_t)t + 1], ic = tris[3 * (size_t)t + 2];
        if (ia < 0 || ia >= nv || ib < 0 || ib >= nv || ic < 0 || ic >= nv) continue;      // (a key below nv says so already: the reads' own guard)
        const float* A = verts + 3 * (size_t)ia; const float* B = verts + 3 * (size_t)ib; const float* Cc = verts + 3 * (size_t)ic;
        const double ax = (double)A[0], ay = (double)A[1], az = (double)A[2];
        const double ux = (double)B[0] - ax, uy = (double)B[1] - ay, uz = (double)B[2] - az;
        const double wx = (double)Cc[0] - ax, wy = (double)Cc[1] - ay, wz = (double)Cc[2] - az;
        sx = sx + (uy * wz - uz * wy);
        sy = sy + (uz * wx - ux * wz);
        sz = sz + (ux * wy - uy * wx);
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = len > 0.0 && rs_finite(len);
    out[3 * (size_t)v] = ok ? (float)(sx / len) : 0.0f;
    out[3 * (size_t)v + 1] = ok ? (float)(sy / len) : 0.0f;
    out[3 * (size_t)v + 2] = ok ? (float)(sz / len) : 0.0f;
}
