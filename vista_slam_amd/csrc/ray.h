// Rays against the triangle index (libsta_ray.so; the contract is in include/sta_ray.h), included by sta_ray.hip after sta_common.h.
// One kernel, one lane per ray: a greedy descent for a first best, then the stackless walk in index order that the distance query of
// libsta_dist.so uses - restated here, that library's files are not included.  No floating-point atomics, every output defined by the
// input alone.
// Nothing here indexes a private array with a run-time value: the permuted components of the sheared form are selected with ternaries
// on kz, the walk's state is (level, node), the level table lives in LDS.
#pragma once

#pragma clang fp contract(off)

#define RY_F 8
#define RY_MAX_LEVELS 9
#define RY_VALID 0
#define RY_STATUS_BOUND 1
// The order in which the walk visits the children of a node.  0: index order, what the library is built with.  1: the order of the ray's
// signs - child (p ^ m) at step p, m = the octant of -d in the bit order of the Morton key (x lowest) - a measured variant
// (tools/ray_bench.py builds it next to the library; profiles/r32_ray.txt has the times).  The outputs cannot depend on it.
#ifndef RY_SIGN_ORDER
#define RY_SIGN_ORDER 0
#endif

// the shape of the tree (host values in the kernel arguments): off[l] = first node of level l, off[levels] = the number of nodes
struct RyTree { int nt; int levels; int off[RY_MAX_LEVELS + 1]; };

__device__ __forceinline__ bool ry_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }      // false for NaN

// nextafterf(x, -inf) and nextafterf(x, +inf) of a float32 that is not NaN, on the bit pattern (no arithmetic: nothing is flushed)
__device__ __forceinline__ float ry_down(float x) {
    const unsigned b = __float_as_uint(x);
    if (b == 0xff800000u) return x;                              // -inf stays
    if ((b & 0x7fffffffu) == 0u) return __uint_as_float(0x80000001u);      // +-0 -> the smallest negative subnormal
    return __uint_as_float((b >> 31) ? b + 1u : b - 1u);
}
__device__ __forceinline__ float ry_up(float x) {
    const unsigned b = __float_as_uint(x);
    if (b == 0x7f800000u) return x;                              // +inf stays
    if ((b & 0x7fffffffu) == 0u) return __uint_as_float(0x00000001u);
    return __uint_as_float((b >> 31) ? b - 1u : b + 1u);
}

// what a lane keeps of its ray
struct RyRay {
    double ox, oy, oz;          // the origin
    double ix, iy, iz;          // 1 / d_k (unused where d_k == 0)
    float dx, dy, dz;           // d as given: its signs and zeros choose the planes
    double Sx, Sy, Sz;          // the shear of rule 3
    int kz;
    double t_min, t_max;
};

// one axis of rule 2: folds tn / tf into enter / exit, or tests the zero axis
__device__ __forceinline__ void ry_axis(float lo, float hi, float d, double o, double inv, double& enter, double& exit, bool& ok) {
    const double l = (double)ry_down(lo), h = (double)ry_up(hi);
    if (d != 0.0f) {
        const double near = d > 0.0f ? l : h, far = d > 0.0f ? h : l;
        const double tn = (near - o) * inv, tf = (far - o) * inv;
        enter = tn > enter ? tn : enter;
        exit = tf < exit ? tf : exit;
    } else {
        ok = ok && l <= o && o <= h;
    }
}
// rule 2 for the box (lx .. hz): passes?  enter and exit are written either way
__device__ __forceinline__ bool ry_slab(const RyRay& r, float lx, float ly, float lz, float hx, float hy, float hz, double& enter, double& exit) {
    enter = r.t_min; exit = r.t_max;
    bool ok = true;
    ry_axis(lx, hx, r.dx, r.ox, r.ix, enter, exit, ok);
    ry_axis(ly, hy, r.dy, r.oy, r.iy, enter, exit, ok);
    ry_axis(lz, hz, r.dz, r.oz, r.iz, enter, exit, ok);
    return ok && enter <= exit;
}
// rule 2 for the node box at p (6 floats); false for a node without a valid triangle
__device__ __forceinline__ bool ry_node(const RyRay& r, const float* __restrict__ p, double& enter) {
    const float lx = p[0], ly = p[1], lz = p[2], hx = p[3], hy = p[4], hz = p[5];
    double exit;
    const bool pass = ry_slab(r, lx, ly, lz, hx, hy, hz, enter, exit);
    return pass && !(lx > hx);
}

struct RyBest { double t; int tri; float b0, b1, b2; };

// the sheared position of the vertex (x, y, z): rule 3, the permutation by ternaries
__device__ __forceinline__ void ry_shear(const RyRay& r, float x, float y, float z, double& px, double& py, double& pz) {
    const double qx = (double)x - r.ox, qy = (double)y - r.oy, qz = (double)z - r.oz;
    const double a = r.kz == 0 ? qy : (r.kz == 1 ? qz : qx);          // P'_kx
    const double b = r.kz == 0 ? qz : (r.kz == 1 ? qx : qy);          // P'_ky
    const double c = r.kz == 0 ? qx : (r.kz == 1 ? qy : qz);          // P'_kz
    px = a - r.Sx * c;
    py = b - r.Sy * c;
    pz = r.Sz * c;
}
// rules 3 to 5 for the triangle at p (9 floats) with input index t: true iff it qualifies (best is then updated under the tie rule)
__device__ __forceinline__ bool ry_triangle(const RyRay& r, const float* __restrict__ p, int t, RyBest& best) {
    const float a0 = p[0], a1 = p[1], a2 = p[2], b0 = p[3], b1 = p[4], b2 = p[5], c0 = p[6], c1 = p[7], c2 = p[8];
    double enter, exit;
    if (!ry_slab(r, fminf(fminf(a0, b0), c0), fminf(fminf(a1, b1), c1), fminf(fminf(a2, b2), c2), fmaxf(fmaxf(a0, b0), c0),
                 fmaxf(fmaxf(a1, b1), c1), fmaxf(fmaxf(a2, b2), c2), enter, exit))
        return false;
    double Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz;
    ry_shear(r, a0, a1, a2, Ax, Ay, Az);
    ry_shear(r, b0, b1, b2, Bx, By, Bz);
    ry_shear(r, c0, c1, c2, Cx, Cy, Cz);
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) return false;
    const double det = (U + V) + W;
    if (!(det != 0.0)) return false;
    const double tt = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(r.t_min <= tt && tt <= r.t_max)) return false;
    double tc = tt >= enter ? tt : enter;
    tc = tc <= exit ? tc : exit;
    if (tc < best.t || (tc == best.t && t < best.tri)) {
        best.t = tc; best.tri = t;
        best.b0 = (float)(U / det); best.b1 = (float)(V / det); best.b2 = (float)(W / det);
    }
    return true;
}
// the valid triangles of level-0 node `node`; true iff one qualified
__device__ __forceinline__ bool ry_leaf(const RyRay& r, const float* __restrict__ tri, const int* __restrict__ src, int node, int n_valid, RyBest& best,
                                        bool any_hit) {
    bool got = false;
#pragma unroll 1
    for (int c = 0; c < RY_F; ++c) {
        const int i = RY_F * node + c;
        if (i < n_valid && !(any_hit && got)) got = ry_triangle(r, tri + 9 * (size_t)i, src[i], best) || got;
    }
    return got;
}

// the sibling of `node` that is visited after it among the `cnt` nodes of its level, -1 when it was the last of its group (m = 0: node + 1)
__device__ __forceinline__ int ry_next_sibling(int node, int m, int cnt) {
    const int base = node & ~(RY_F - 1);
    for (int p = ((node & (RY_F - 1)) ^ m) + 1; p < RY_F; ++p) {
        const int c = base | (p ^ m);
        if (c < cnt) return c;
    }
    return -1;
}
// the child of `node` that is visited first among the `cnt` nodes of the level below (m = 0: RY_F * node; that one always exists)
__device__ __forceinline__ int ry_first_child(int node, int m, int cnt) {
    const int base = RY_F * node;
    for (int p = 0; p < RY_F; ++p) {
        const int c = base | (p ^ m);
        if (c < cnt) return c;
    }
    return base;
}

struct RyCast {
    const float* tri; const int* src; const float* boxes; const int* counters;
    const float* org; const float* dir; int R; double t_min, t_max;
    double* t_out; int* tri_out; float* bary_out; unsigned char* occ_out; int* status;
    RyTree tree;
};
// ANY: leave at the first qualifying triangle and write occ_out alone
template <bool ANY>
__global__ __launch_bounds__(256) void ry_cast_kernel(const RyCast P) {
    __shared__ int s_off[RY_MAX_LEVELS + 1];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l <= RY_MAX_LEVELS; ++l) s_off[l] = P.tree.off[l];          // static indices: the arguments stay in registers
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.R) return;
    const float fox = P.org[3 * (size_t)i], foy = P.org[3 * (size_t)i + 1], foz = P.org[3 * (size_t)i + 2];
    const float fdx = P.dir[3 * (size_t)i], fdy = P.dir[3 * (size_t)i + 1], fdz = P.dir[3 * (size_t)i + 2];
    const int levels = P.tree.levels, top = levels - 1, nodes = s_off[levels];
    int n_valid = P.counters[RY_VALID];
    n_valid = n_valid < P.tree.nt ? n_valid : P.tree.nt;
    RyBest best;
    best.t = __builtin_huge_val(); best.tri = 0x7fffffff; best.b0 = 0.0f; best.b1 = 0.0f; best.b2 = 0.0f;
    bool bound_hit = false, got = false;
    const bool usable = ry_finite(fox) && ry_finite(foy) && ry_finite(foz) && ry_finite(fdx) && ry_finite(fdy) && ry_finite(fdz) &&
                        (fdx != 0.0f || fdy != 0.0f || fdz != 0.0f);
    if (usable && n_valid > 0) {
        RyRay r;
        r.ox = fox; r.oy = foy; r.oz = foz; r.dx = fdx; r.dy = fdy; r.dz = fdz;
        const double dx = fdx, dy = fdy, dz = fdz;
        r.ix = 1.0 / dx; r.iy = 1.0 / dy; r.iz = 1.0 / dz;          // (inf where d_k == 0: never used)
        const float ax = fabsf(fdx), ay = fabsf(fdy), az = fabsf(fdz);
        r.kz = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);          // the first axis of the largest |d_k|
        const double dkz = r.kz == 0 ? dx : (r.kz == 1 ? dy : dz), dkx = r.kz == 0 ? dy : (r.kz == 1 ? dz : dx),
                     dky = r.kz == 0 ? dz : (r.kz == 1 ? dx : dy);
        r.Sx = dkx / dkz; r.Sy = dky / dkz; r.Sz = 1.0 / dkz;
        r.t_min = P.t_min; r.t_max = P.t_max;
        // 1. a first best: down from the root into the passing child of the smallest enter
        {
            int node = 0;
            double e;
            bool found = ry_node(r, P.boxes + 6 * (size_t)s_off[top], e);
            for (int lev = top; lev > 0 && found; --lev) {
                const int first = RY_F * node, cnt = s_off[lev] - s_off[lev - 1];
                double be = 0.0; int pick = -1;
#pragma unroll 1
                for (int c = 0; c < RY_F; ++c) {
                    if (first + c < cnt) {
                        const bool pass = ry_node(r, P.boxes + 6 * (size_t)(s_off[lev - 1] + first + c), e);
                        if (pass && (pick < 0 || e < be)) { be = e; pick = first + c; }
                    }
                }
                found = pick >= 0;
                node = pick;
            }
            if (found) got = ry_leaf(r, P.tri, P.src, node, n_valid, best, ANY);
        }
        // 2. every node in depth-first order, siblings in index order (or RY_SIGN_ORDER), without a stack
        const int m = RY_SIGN_ORDER ? ((fdx < 0.0f ? 1 : 0) | (fdy < 0.0f ? 2 : 0) | (fdz < 0.0f ? 4 : 0)) : 0;
        int lev = top, node = 0;
        bool done = ANY && got;
        int it = 0;
        for (; it <= nodes && !done; ++it) {
            double e;
            const bool pass = ry_node(r, P.boxes + 6 * (size_t)(s_off[lev] + node), e);
            const bool enter = pass && !(e > best.t);
            if (enter && lev > 0) { node = ry_first_child(node, m, s_off[lev] - s_off[lev - 1]); --lev; continue; }
            if (enter) got = ry_leaf(r, P.tri, P.src, node, n_valid, best, ANY) || got;
            if (ANY && got) { done = true; break; }
            // the node after (lev, node): its next sibling, or the node after its parent
            for (int k = 0; k < RY_MAX_LEVELS; ++k) {
                if (lev == top) { done = true; break; }
                const int next = ry_next_sibling(node, m, s_off[lev + 1] - s_off[lev]);
                if (next >= 0) { node = next; break; }
                node /= RY_F; ++lev;
            }
        }
        bound_hit = !done;
    }
    if (bound_hit) atomicOr(P.status, RY_STATUS_BOUND);          // an integer flag: order-free
    const bool hit = got && !bound_hit;
    if (ANY) {
        P.occ_out[i] = hit ? 1 : 0;
        return;
    }
    if (P.t_out) P.t_out[i] = hit ? best.t : __builtin_huge_val();
    if (P.tri_out) P.tri_out[i] = hit ? best.tri : -1;
    if (P.bary_out) {
        const float nan = __builtin_nanf("");
        P.bary_out[3 * (size_t)i] = hit ? best.b0 : nan;
        P.bary_out[3 * (size_t)i + 1] = hit ? best.b1 : nan;
        P.bary_out[3 * (size_t)i + 2] = hit ? best.b2 : nan;
    }
}
