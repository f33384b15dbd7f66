// Connected components and area-uniform surface samples of a triangle mesh (libsta_surf.so; the contract is in include/sta_surf.h).
// Launch code in sta_surf.hip.
//   sf_init_kernel      one lane per vertex: parent = itself, tcount = 0; lane 0 clears status
//   sf_hook_kernel      one lane per triangle: unites (i0, i1) and (i0, i2) - the larger root is linked under the smaller by compare-and-swap
//   sf_flatten_kernel   one lane per vertex: vlabel = its root
//   sf_count_kernel     one lane per triangle: tlabel, and one integer atomic add per distinct label of a wavefront
//   sf_unnamed_kernel   one lane per vertex: a root without a triangle is a vertex nobody names: vlabel = -1
//   sf_chunk_kernel     one wavefront per chunk of 1024 triangles: the weights into shared memory, lane 0 sums them in order
//   sf_offsets_kernel   one lane: the chunk offsets O and the total
//   sf_prefix_kernel    one lane per triangle: P = O + I
//   sf_sample_kernel    one lane per sample
// Every parent word is read and written with relaxed device-scope atomics while lanes of other workgroups may write it; a stale read costs a
// retry, never a wrong link, because the only link is the compare-and-swap of a root that still points to itself.
// Every fp64 operation is written out and nothing is contracted.
#pragma once
#pragma clang fp contract(off)

#define SF_CHUNK 1024               // STA_SURF_CHUNK
#define SF_STATUS_BOUND 1           // STA_SURF_STATUS_BOUND

__device__ __forceinline__ int sf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x, halving the path on the way: a parent only ever decreases, and only to an ancestor.  At most nv + 1 steps.
__device__ __forceinline__ int sf_find(int* parent, int x, long long nv, int* status) {
    int p = sf_load(parent + x);
    for (long long s = 0; p != x; ++s) {
        if (s > nv) { atomicOr(status, SF_STATUS_BOUND); break; }
        const int g = sf_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p; p = g;
    }
    return x;
}

// At most nv + 1 retries: a failed compare-and-swap returns a parent of `hi` that is smaller than hi, so every retry starts lower.
__device__ __forceinline__ void sf_unite(int* parent, int a, int b, long long nv, int* status) {
    for (long long s = 0; s <= nv; ++s) {
        a = sf_find(parent, a, nv, status);
        b = sf_find(parent, b, nv, status);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old; b = lo;
    }
    atomicOr(status, SF_STATUS_BOUND);
}

__device__ __forceinline__ bool sf_valid(const int* tris, long long t, long long nv, int& i0, int& i1, int& i2) {
    i0 = tris[3 * (size_t)t]; i1 = tris[3 * (size_t)t + 1]; i2 = tris[3 * (size_t)t + 2];
    return i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv;
}

__global__ void __launch_bounds__(256) sf_init_kernel(int* parent, int* tcount, int* status, long long nv) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v == 0) *status = 0;
    if (v >= nv) return;
    parent[v] = (int)v;
    tcount[v] = 0;
}

__global__ void __launch_bounds__(256) sf_hook_kernel(const int* tris, long long nt, long long nv, int* parent, int* status) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    int i0, i1, i2;
    if (!sf_valid(tris, t, nv, i0, i1, i2)) return;
    if (i1 != i0) sf_unite(parent, i0, i1, nv, status);
    if (i2 != i0 && i2 != i1) sf_unite(parent, i0, i2, nv, status);
}

__global__ void __launch_bounds__(256) sf_flatten_kernel(int* parent, long long nv, int* vlabel, int* status) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    vlabel[v] = sf_find(parent, (int)v, nv, status);
}

__global__ void __launch_bounds__(256) sf_count_kernel(const int* tris, long long nt, long long nv, const int* vlabel, int* tlabel, int* tcount) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (t < nt) {
        int i0, i1, i2;
        if (sf_valid(tris, t, nv, i0, i1, i2)) r = vlabel[i0];
        tlabel[t] = r;
    }
    // one add per distinct label of the wavefront; `todo` is the same in every lane, so the loop is uniform and ends after at most 64 rounds
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(r >= 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int rl = __shfl(r, lead, 64);
        const unsigned long long same = __ballot(r == rl) & todo;
        if (lane == lead && rl >= 0 && rl < nv) atomicAdd(tcount + rl, (int)__popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(256) sf_unnamed_kernel(int* vlabel, const int* tcount, long long nv) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    if (vlabel[v] == (int)v && tcount[v] == 0) vlabel[v] = -1;
}

struct SfFace { double A[3], B[3], Cc[3], n[3], len; };

// the doubles of the three vertices, (B - A) x (C - A) and its length, as include/sta_mesh.h writes them
__device__ __forceinline__ void sf_face(const float* verts, int i0, int i1, int i2, SfFace& f) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f.A[k] = (double)verts[3 * (size_t)i0 + k]; f.B[k] = (double)verts[3 * (size_t)i1 + k]; f.Cc[k] = (double)verts[3 * (size_t)i2 + k];
    }
    const double ux = f.B[0] - f.A[0], uy = f.B[1] - f.A[1], uz = f.B[2] - f.A[2];
    const double vx = f.Cc[0] - f.A[0], vy = f.Cc[1] - f.A[1], vz = f.Cc[2] - f.A[2];
    f.n[0] = uy * vz - uz * vy; f.n[1] = uz * vx - ux * vz; f.n[2] = ux * vy - uy * vx;
    f.len = sqrt((f.n[0] * f.n[0] + f.n[1] * f.n[1]) + f.n[2] * f.n[2]);
}

__device__ __forceinline__ bool sf_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for NaN and the infinities

__global__ void __launch_bounds__(64) sf_chunk_kernel(const float* verts, long long nv, const int* tris, long long nt, const unsigned char* keep,
                                                      double* P, double* S) {
    __shared__ double w[SF_CHUNK];
    const long long c = blockIdx.x, base = c * SF_CHUNK;
    const int lane = threadIdx.x;
    for (int j = lane; j < SF_CHUNK; j += 64) {
        const long long t = base + j;
        double wt = 0.0;
        int i0, i1, i2;
        if (t < nt && (!keep || keep[t]) && sf_valid(tris, t, nv, i0, i1, i2)) {
            SfFace f;
            sf_face(verts, i0, i1, i2, f);
            if (sf_finite(f.len)) wt = f.len;
        }
        w[j] = wt;
    }
    __syncthreads();
    if (lane == 0) {
        double acc = w[0];
        for (int j = 1; j < SF_CHUNK; ++j) { acc = acc + w[j]; w[j] = acc; }
        S[c] = acc;
    }
    __syncthreads();
    for (int j = lane; j < SF_CHUNK; j += 64)
        if (base + j < nt) P[base + j] = w[j];
}

__global__ void sf_offsets_kernel(const double* S, long long nchunks, double* O, double* total) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double acc = 0.0;
    for (long long c = 0; c < nchunks; ++c) { O[c] = acc; acc = acc + S[c]; }
    *total = acc;
}

__global__ void __launch_bounds__(256) sf_prefix_kernel(double* P, long long nt, const double* O) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    P[t] = O[t / SF_CHUNK] + P[t];
}

__device__ __forceinline__ unsigned long long sf_mix(unsigned long long seed, unsigned long long i) {
    unsigned long long z = seed + i * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double sf_unit(unsigned long long z) { return (double)(z >> 11) * 1.1102230246251565e-16; }      // 2^-53

struct SfSample {
    const float* verts; const int* tris; const double* P; const double* total; const float* colors;
    long long nv, nt, ns;
    unsigned long long seed;
    float* points; int* tri; float* colors_out; float* normals_out;
};

// the smallest t in [0, nt] with P[t] > x (STRICT) or P[t] >= x; nt when there is none.  At most 32 halvings of [0, nt), nt < 2^31.
template <bool STRICT>
__device__ __forceinline__ long long sf_search(const double* P, long long nt, double x) {
    long long lo = 0, hi = nt;
    for (int s = 0; s < 32 && lo < hi; ++s) {
        const long long mid = lo + (hi - lo) / 2;
        const double p = P[mid];
        if (STRICT ? p > x : p >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ void __launch_bounds__(256) sf_sample_kernel(SfSample a) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.ns) return;
    const double total = *a.total;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    long long t = -1;
    int i0 = 0, i1 = 0, i2 = 0;
    const double u0 = sf_unit(sf_mix(a.seed, 3ull * (unsigned long long)k + 1ull));
    const double u1 = sf_unit(sf_mix(a.seed, 3ull * (unsigned long long)k + 2ull));
    const double u2 = sf_unit(sf_mix(a.seed, 3ull * (unsigned long long)k + 3ull));
    if (total > 0.0 && sf_finite(total)) {
        const double x = (((double)k + u0) / (double)a.ns) * total;
        t = sf_search<true>(a.P, a.nt, x);
        if (t >= a.nt) t = sf_search<false>(a.P, a.nt, total);
        if (t >= a.nt || !sf_valid(a.tris, t, a.nv, i0, i1, i2)) t = -1;
    }
    float* pt = a.points + 3 * (size_t)k;
    a.tri[k] = (int)t;
    if (t < 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            pt[c] = (float)nan;
            if (a.colors_out) a.colors_out[3 * (size_t)k + c] = (float)nan;
            if (a.normals_out) a.normals_out[3 * (size_t)k + c] = (float)nan;
        }
        return;
    }
    SfFace f;
    sf_face(a.verts, i0, i1, i2, f);
    const double r = sqrt(u1);
    const double b0 = 1.0 - r, b1 = r * (1.0 - u2), b2 = r * u2;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pt[c] = (float)((b0 * f.A[c] + b1 * f.B[c]) + b2 * f.Cc[c]);
        if (a.colors_out) {
            const double ca = (double)a.colors[3 * (size_t)i0 + c], cb = (double)a.colors[3 * (size_t)i1 + c], cc = (double)a.colors[3 * (size_t)i2 + c];
            a.colors_out[3 * (size_t)k + c] = (float)((b0 * ca + b1 * cb) + b2 * cc);
        }
        if (a.normals_out) a.normals_out[3 * (size_t)k + c] = (float)(f.n[c] / f.len);
    }
}
