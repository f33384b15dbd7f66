#pragma once
// Sim(3) pose-graph optimisation (sta_sim3_op / sta_pgo_index / sta_pgo_linearize / sta_pgo_solve / sta_pgo_optimize; the contract is in
// include/sta_mi355.h, the yardstick is the numpy restatement tests/pgo_cases.py), included by sta_api.hip after loop.h.  float64
// throughout.  The Gauss-Newton matrix is a graph Laplacian with 7x7 weights: H x = per edge S_e (x_b - x_a), per node a signed sum over
// its incident half-edges in ascending edge order.  Nothing is assembled, and there is no floating-point atomic in this file.
#include "sta_common.h"
#include "sta_skew.h"       // STA_SKEW points: nothing unless -DSTA_WAVE_SKEW (libsta_mi355_skew.so)

// ---- the constants of the contract (the same names in tests/pgo_cases.py) ----
#define PGO_PHI_SERIES 0.25      // |phi| below: W's A and B from the moment series (above: the closed forms)
#define PGO_MOMENT_START 48      // the backward recurrence m_(k-1) = (e^sigma - sigma m_k) / k starts at m_48 = e^sigma / 49
#define PGO_MOMENT_TERMS 6       // terms of the theta^2 series of A and B (moments m_1 .. m_12)
#define PGO_QUAT_SERIES 1e-4     // |phi| (Exp) or |q.xyz| (Log) below: the two-term series
#define PGO_JL_TERMS 32          // Horner over 32 powers of ad
#define PGO_MAX_NODES 8192
#define PGO_MAX_EDGES 16384
#define PGO_THREADS 1024
enum { PGO_ST_INDEX = 1, PGO_ST_NONFINITE = 2, PGO_ST_MAXITER = 4, PGO_ST_BREAKDOWN = 8, PGO_ST_CHOL = 16, PGO_ST_UNCHANGED = 32 };
enum { SIM3_MUL = 0, SIM3_INV = 1, SIM3_BETWEEN = 2, SIM3_EXP = 3, SIM3_LOG = 4, SIM3_RETRACT = 5 };

__device__ __forceinline__ void pgo_rot(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
    R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
    R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
__device__ __forceinline__ void pgo_norm_q(double* q) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
__device__ __forceinline__ void pgo_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
// o = a b (o aliases neither)
__device__ inline void pgo_mul(const double* a, const double* b, double* o) {
    double R[9];
    pgo_rot(a + 3, R);
    for (int i = 0; i < 3; ++i) o[i] = a[7] * (R[3 * i] * b[0] + R[3 * i + 1] * b[1] + R[3 * i + 2] * b[2]) + a[i];
    const double x1 = a[3], y1 = a[4], z1 = a[5], w1 = a[6], x2 = b[3], y2 = b[4], z2 = b[5], w2 = b[6];
    o[3] = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2;
    o[4] = w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2;
    o[5] = w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2;
    o[6] = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
    pgo_norm_q(o + 3);
    o[7] = a[7] * b[7];
}
__device__ inline void pgo_inv(const double* a, double* o) {
    double R[9];
    pgo_rot(a + 3, R);
    for (int i = 0; i < 3; ++i) o[i] = -(R[i] * a[0] + R[3 + i] * a[1] + R[6 + i] * a[2]) / a[7];
    o[3] = -a[3]; o[4] = -a[4]; o[5] = -a[5]; o[6] = a[6];
    pgo_norm_q(o + 3);
    o[7] = 1.0 / a[7];
}
// W(phi, sigma) = C I + A phi^ + B phi^ phi^
__device__ inline void pgo_wcoef(double theta, double sigma, double& A, double& B, double& C) {
    const double es = exp(sigma);
    C = sigma != 0.0 ? expm1(sigma) / sigma : 1.0;
    if (theta < PGO_PHI_SERIES) {
        double m = es / (double)(PGO_MOMENT_START + 1);
        for (int k = PGO_MOMENT_START; k > 2 * PGO_MOMENT_TERMS; --k) m = (es - sigma * m) / (double)k;
        double mk[2 * PGO_MOMENT_TERMS + 1];
        mk[2 * PGO_MOMENT_TERMS] = m;
#pragma unroll
        for (int k = 2 * PGO_MOMENT_TERMS; k > 0; --k) mk[k - 1] = (es - sigma * mk[k]) / (double)k;
        const double t2 = theta * theta;
        double As = 0.0, Bs = 0.0, p = 1.0, fa = 1.0, fb = 2.0;
#pragma unroll
        for (int j = 0; j < PGO_MOMENT_TERMS; ++j) {
            As = As + p * mk[2 * j + 1] / fa;
            Bs = Bs + p * mk[2 * j + 2] / fb;
            p = -p * t2;
            fa = fa * (double)((2 * j + 2) * (2 * j + 3));
            fb = fb * (double)((2 * j + 3) * (2 * j + 4));
        }
        A = As; B = Bs;
    } else {
        const double den = sigma * sigma + theta * theta, sn = sin(theta), cs = cos(theta);
        const double Is = (es * (sigma * sn - theta * cs) + theta) / den;
        const double Ic = (es * (sigma * cs + theta * sn) - sigma) / den;
        A = Is / theta; B = (C - Ic) / (theta * theta);
    }
}
__device__ inline void pgo_exp(const double* xi, double* o) {
    const double* tau = xi; const double* phi = xi + 3; const double sigma = xi[6];
    const double theta = sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    const double k = theta < PGO_QUAT_SERIES ? 0.5 - theta * theta / 48.0 : sin(theta / 2) / theta;
    double A, B, C, px[3], ppx[3];
    pgo_wcoef(theta, sigma, A, B, C);
    pgo_cross(phi, tau, px);
    pgo_cross(phi, px, ppx);
    for (int i = 0; i < 3; ++i) { o[i] = C * tau[i] + A * px[i] + B * ppx[i]; o[3 + i] = k * phi[i]; }
    o[6] = cos(theta / 2);
    pgo_norm_q(o + 3);
    o[7] = exp(sigma);
}
__device__ inline void pgo_log(const double* T, double* xi) {
    double q[4] = {T[3], T[4], T[5], T[6]};
    pgo_norm_q(q);
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double w = q[3], n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const double f = n < PGO_QUAT_SERIES ? (2 / w) * (1 - n * n / (3 * w * w)) : 2 * atan2(n, w) / n;
    const double p0 = f * q[0], p1 = f * q[1], p2 = f * q[2], sigma = log(T[7]);
    const double theta = sqrt(p0 * p0 + p1 * p1 + p2 * p2);
    double A, B, C;
    pgo_wcoef(theta, sigma, A, B, C);
    // W = C I + A P + B P P, P = phi^
    const double P[9] = {0, -p2, p1, p2, 0, -p0, -p1, p0, 0};
    double W[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double pp = P[3 * i] * P[j] + P[3 * i + 1] * P[3 + j] + P[3 * i + 2] * P[6 + j];
            W[3 * i + j] = C * (i == j ? 1.0 : 0.0) + A * P[3 * i + j] + B * pp;
        }
    const double a = W[0], b = W[1], c = W[2], d = W[3], e = W[4], ff = W[5], g = W[6], h = W[7], i = W[8];
    const double c00 = e * i - ff * h, c01 = c * h - b * i, c02 = b * ff - c * e;
    const double c10 = ff * g - d * i, c11 = a * i - c * g, c12 = c * d - a * ff;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double det = a * c00 + b * c10 + c * c20;
    xi[0] = (c00 * T[0] + c01 * T[1] + c02 * T[2]) / det;
    xi[1] = (c10 * T[0] + c11 * T[1] + c12 * T[2]) / det;
    xi[2] = (c20 * T[0] + c21 * T[1] + c22 * T[2]) / det;
    xi[3] = p0; xi[4] = p1; xi[5] = p2; xi[6] = sigma;
}

// one thread per element.  MUL / BETWEEN: a, b [count,8]; INV: a [count,8]; EXP: a [count,7]; LOG: a [count,8] -> out [count,7];
// RETRACT: a = d [count,7], b = X [count,8], out = Exp(d) X where mask (null: everywhere) is set, a copy of X elsewhere
__global__ __launch_bounds__(256) void sim3_op_kernel(int op, const double* __restrict__ a, const double* __restrict__ b, const unsigned char* __restrict__ mask,
                                                      double* __restrict__ out, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double A[8], B[8], O[8], Tm[8];
    const int wa = (op == SIM3_EXP || op == SIM3_RETRACT) ? 7 : 8;
    for (int k = 0; k < wa; ++k) A[k] = a[i * wa + k];
    if (op == SIM3_MUL || op == SIM3_BETWEEN || op == SIM3_RETRACT) for (int k = 0; k < 8; ++k) B[k] = b[i * 8 + k];
    int wo = 8;
    switch (op) {
        case SIM3_MUL: pgo_mul(A, B, O); break;
        case SIM3_INV: pgo_inv(A, O); break;
        case SIM3_BETWEEN: pgo_inv(A, Tm); pgo_mul(Tm, B, O); break;
        case SIM3_EXP: pgo_exp(A, O); break;
        case SIM3_LOG: pgo_log(A, O); wo = 7; break;
        default:
            if (mask && !mask[i]) { for (int k = 0; k < 8; ++k) O[k] = B[k]; }
            else { pgo_exp(A, Tm); pgo_mul(Tm, B, O); }
    }
    for (int k = 0; k < wo; ++k) out[i * wo + k] = O[k];
}

// an edge is active iff both indices lie in [0, n), a != b and at least one endpoint is optimised
__device__ __forceinline__ bool pgo_edge(const int* __restrict__ edges, const unsigned char* __restrict__ opt, int n, int e, int& a, int& b, bool& in_range) {
    a = edges[2 * e]; b = edges[2 * e + 1];
    in_range = a >= 0 && a < n && b >= 0 && b < n;
    return in_range && a != b && (opt[a] | opt[b]);
}

// ONE workgroup.  off [n+1], inc [off[n]] = edge * 2 + side (side 0: the node is a), ascending within a node; tmp: 2 x 2E ints.
__global__ __launch_bounds__(PGO_THREADS) void pgo_index_kernel(const int* __restrict__ edges, const unsigned char* __restrict__ opt, int n, int E, int* tmp,
                                                                 int* off, int* inc, int* status) {
    STA_SKEW_ENTRY(1113);
    __shared__ int cur[PGO_MAX_NODES];
    __shared__ int part[PGO_THREADS];
    __shared__ int s_status;
    const int tid = threadIdx.x;
    int* tmp_half = tmp; int* tmp_node = tmp + 2 * (size_t)E;
    for (int k = tid; k < n; k += PGO_THREADS) cur[k] = 0;
    if (tid == 0) s_status = 0;
    __syncthreads(); STA_SKEW(1100);
    for (int e = tid; e < E; e += PGO_THREADS) {
        int a, b; bool inr;
        const bool act = pgo_edge(edges, opt, n, e, a, b, inr);
        if (!inr) atomicOr(&s_status, PGO_ST_INDEX);
        if (act) { if (opt[a]) atomicAdd(&cur[a], 1); if (opt[b]) atomicAdd(&cur[b], 1); }
    }
    __syncthreads(); STA_SKEW(1101);
    // exclusive scan: 8 consecutive nodes per thread, then the 1024 partial sums
    const int per = PGO_MAX_NODES / PGO_THREADS, k0 = tid * per;
    int sum = 0;
    for (int j = 0; j < per; ++j) if (k0 + j < n) sum += cur[k0 + j];
    part[tid] = sum;
    __syncthreads(); STA_SKEW(1102);
    for (int s = 1; s < PGO_THREADS; s <<= 1) {
        const int add = tid >= s ? part[tid - s] : 0;
        __syncthreads(); STA_SKEW(1103);
        part[tid] += add;
        __syncthreads(); STA_SKEW(1104);
    }
    int base = part[tid] - sum;
    const int total = part[PGO_THREADS - 1];
    for (int j = 0; j < per; ++j) if (k0 + j < n) { const int d = cur[k0 + j]; cur[k0 + j] = base; off[k0 + j] = base; base += d; }
    if (tid == 0) { off[n] = total; *status = s_status; }
    __syncthreads(); STA_SKEW(1105);
    for (int e = tid; e < E; e += PGO_THREADS) {
        int a, b; bool inr;
        if (!pgo_edge(edges, opt, n, e, a, b, inr)) continue;
        if (opt[a]) { const int p = atomicAdd(&cur[a], 1); tmp_half[p] = 2 * e; tmp_node[p] = a; }
        if (opt[b]) { const int p = atomicAdd(&cur[b], 1); tmp_half[p] = 2 * e + 1; tmp_node[p] = b; }
    }
    __syncthreads(); STA_SKEW(1106);          // workgroup-scope release / acquire: tmp and off were written by other threads of this workgroup
    // a list's entries are distinct (a != b): the rank of an entry is the number of smaller ones
    for (int i = tid; i < total; i += PGO_THREADS) {
        const int k = tmp_node[i], v = tmp_half[i], lo = off[k], hi = cur[k];
        int rank = 0;
        for (int j = lo; j < hi; ++j) rank += tmp_half[j] < v ? 1 : 0;
        inc[lo + rank] = v;
    }
}

// ad(xi) v for the order (tau, phi, sigma)
__device__ __forceinline__ void pgo_ad_apply(const double* xi, const double* v, double* o) {
    double c1[3], c2[3], c3[3];
    pgo_cross(xi + 3, v, c1);
    pgo_cross(xi, v + 3, c2);
    pgo_cross(xi + 3, v + 3, c3);
    for (int i = 0; i < 3; ++i) { o[i] = xi[6] * v[i] + c1[i] + c2[i] - xi[i] * v[6]; o[3 + i] = c3[i]; }
    o[6] = 0.0;
}

// grid over edges.  c [E] always; with full != 0 also r [E,7], S [E,49], v [E,7] (zeros on an inactive edge).  The cost term is computed
// by the same instructions in both forms.
__global__ __launch_bounds__(64) void pgo_linearize_kernel(const double* __restrict__ nodes, const int* __restrict__ edges, const double* __restrict__ poses,
                                                           const double* __restrict__ confs, const unsigned char* __restrict__ opt, int n, int E, int full,
                                                           double* __restrict__ r_out, double* __restrict__ S_out, double* __restrict__ v_out,
                                                           double* __restrict__ c_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    int a, b; bool inr;
    if (!pgo_edge(edges, opt, n, e, a, b, inr)) {
        c_out[e] = 0.0;
        if (full) {
            for (int k = 0; k < 7; ++k) { r_out[(size_t)e * 7 + k] = 0.0; v_out[(size_t)e * 7 + k] = 0.0; }
            for (int k = 0; k < 49; ++k) S_out[(size_t)e * 49 + k] = 0.0;
        }
        return;
    }
    double P[8], Xa[8], Xb[8], Xi[8], Ae[8], T[8], r[7], w[7];
    for (int k = 0; k < 8; ++k) { P[k] = poses[(size_t)e * 8 + k]; Xa[k] = nodes[(size_t)a * 8 + k]; Xb[k] = nodes[(size_t)b * 8 + k]; }
    for (int k = 0; k < 7; ++k) w[k] = confs[(size_t)e * 7 + k];
    pgo_inv(Xa, Xi);
    pgo_mul(P, Xi, Ae);
    pgo_mul(Ae, Xb, T);
    pgo_log(T, r);
    double c = 0.0;
    for (int k = 0; k < 7; ++k) c += w[k] * r[k] * r[k];
    c_out[e] = c;
    if (!full) return;
    // the augmented system (Jl | Ad(Ae)), rows of 14
    double M[7][14];
    for (int j = 0; j < 7; ++j) {                    // column j of Jl by Horner: y = e_j + ad(y) / (k + 1), k = 32 .. 1
        double y[7], t[7];
        for (int i = 0; i < 7; ++i) y[i] = i == j ? 1.0 : 0.0;
        for (int k = PGO_JL_TERMS; k > 0; --k) {
            pgo_ad_apply(r, y, t);
            for (int i = 0; i < 7; ++i) y[i] = (i == j ? 1.0 : 0.0) + t[i] / (double)(k + 1);
        }
        for (int i = 0; i < 7; ++i) M[i][j] = y[i];
    }
    {
        double R[9];
        pgo_rot(Ae + 3, R);
        const double* t = Ae;
        const double H[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
        for (int i = 0; i < 7; ++i) for (int j = 0; j < 7; ++j) M[i][7 + j] = 0.0;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                M[i][7 + j] = Ae[7] * R[3 * i + j];
                M[i][10 + j] = H[3 * i] * R[j] + H[3 * i + 1] * R[3 + j] + H[3 * i + 2] * R[6 + j];
                M[3 + i][10 + j] = R[3 * i + j];
            }
            M[i][13] = -t[i];
        }
        M[6][13] = 1.0;
    }
    for (int col = 0; col < 7; ++col) {              // elimination with partial pivoting: the first largest |entry|
        int p = col; double best = fabs(M[col][col]);
        for (int i = col + 1; i < 7; ++i) if (fabs(M[i][col]) > best) { best = fabs(M[i][col]); p = i; }
        if (p != col) for (int j = 0; j < 14; ++j) { const double s = M[col][j]; M[col][j] = M[p][j]; M[p][j] = s; }
        for (int i = col + 1; i < 7; ++i) {
            const double f = M[i][col] / M[col][col];
            for (int j = 0; j < 14; ++j) M[i][j] = M[i][j] - f * M[col][j];
        }
    }
    for (int i = 6; i >= 0; --i)                      // back substitution: columns 7 .. 13 become Jl^-1 Ad
        for (int j = 7; j < 14; ++j) {
            double acc = M[i][j];
            for (int k = i + 1; k < 7; ++k) acc = acc - M[i][k] * M[k][j];
            M[i][j] = acc / M[i][i];
        }
    for (int i = 0; i < 7; ++i) {
        double vi = 0.0;
        for (int k = 0; k < 7; ++k) vi += M[k][7 + i] * (w[k] * r[k]);
        v_out[(size_t)e * 7 + i] = vi;
        r_out[(size_t)e * 7 + i] = r[i];
        for (int j = 0; j < 7; ++j) {
            double s = 0.0;
            for (int k = 0; k < 7; ++k) s += M[k][7 + i] * (w[k] * M[k][7 + j]);
            S_out[(size_t)e * 49 + i * 7 + j] = s;
        }
    }
}

// a fixed-order sum over a workgroup of PGO_THREADS: within a wave a shuffle tree, then the 16 wave sums in ascending order
__device__ __forceinline__ double pgo_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads(); STA_SKEW(1107);
    double s = 0.0;
    for (int i = 0; i < PGO_THREADS / 64; ++i) s += red[i];
    __syncthreads(); STA_SKEW(1108);
    return s;
}

// ONE workgroup: f = the sum of c over the edges (thread t takes t, t + 1024, ... in ascending order, then the fixed tree);
// rec = {f, status}: PGO_ST_NONFINITE for a non-finite f, ored with *idx_status (may be null)
__global__ __launch_bounds__(PGO_THREADS) void pgo_cost_kernel(const double* __restrict__ c, int E, const int* __restrict__ idx_status, double* rec) {
    STA_SKEW_ENTRY(1115);
    __shared__ double red[PGO_THREADS / 64];
    double s = 0.0;
    for (int e = threadIdx.x; e < E; e += PGO_THREADS) s += c[e];
    const double f = pgo_block_sum(s, red);
    if (threadIdx.x == 0) {
        int st = idx_status ? *idx_status : 0;
        if (!isfinite(f)) st |= PGO_ST_NONFINITE;
        rec[0] = f; rec[1] = (double)st;
    }
}

// grid over nodes: g [n,7] and the diagonal blocks [n,49] in list order (zeros at a fixed node)
__global__ __launch_bounds__(64) void pgo_node_kernel(const int* __restrict__ off, const int* __restrict__ inc, const unsigned char* __restrict__ opt, int n,
                                                      const double* __restrict__ S, const double* __restrict__ v, double* __restrict__ g,
                                                      double* __restrict__ blocks) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double gk[7], bk[49];
    for (int i = 0; i < 7; ++i) gk[i] = 0.0;
    for (int i = 0; i < 49; ++i) bk[i] = 0.0;
    if (opt[k])
        for (int j = off[k]; j < off[k + 1]; ++j) {
            const int h = inc[j], e = h >> 1;
            const double sgn = (h & 1) ? 1.0 : -1.0;
            for (int i = 0; i < 7; ++i) gk[i] += sgn * v[(size_t)e * 7 + i];
            for (int i = 0; i < 49; ++i) bk[i] += S[(size_t)e * 49 + i];
        }
    for (int i = 0; i < 7; ++i) g[(size_t)k * 7 + i] = gk[i];
    for (int i = 0; i < 49; ++i) blocks[(size_t)k * 49 + i] = bk[i];
}

// workspace of pgo_solve_kernel, in doubles
__host__ __device__ inline size_t pgo_solve_ws_doubles(int n, int E) { return (size_t)n * (49 + 7 * 5) + (size_t)E * (7 + 28 + 1); }

// ONE workgroup of 1024 threads: preconditioned CG for (H + D / radius) d = -g.  Thread t owns nodes t, t + 1024, ...: the x, r, z, Ap
// rows of a node are touched by its owner alone (so is an edge's column of the packed S); p [n,7] and d_e [E,7] cross threads through global memory, with __syncthreads() - a
// workgroup-scope release / acquire, and all waves of a workgroup share one CU's L1 - between the writes and the reads.  Every loop is
// bounded by an argument; every scalar that decides a branch comes out of pgo_block_sum, so the control flow is uniform.
__global__ __launch_bounds__(PGO_THREADS) void pgo_solve_kernel(const int* __restrict__ edges, const unsigned char* __restrict__ opt, const int* __restrict__ off,
                                                                 const int* __restrict__ inc, const double* __restrict__ S, const double* __restrict__ g,
                                                                 const double* __restrict__ blocks, int n, int E, double radius, double dmin, double dmax,
                                                                 double rtol, int max_iter, double* ws, double* x, double* stats) {
    STA_SKEW_ENTRY(1114);
    __shared__ double red[PGO_THREADS / 64];
    const int tid = threadIdx.x;
    double* L = ws; double* Dk = L + (size_t)n * 49; double* r = Dk + (size_t)n * 7; double* z = r + (size_t)n * 7;
    double* p = z + (size_t)n * 7; double* Ap = p + (size_t)n * 7; double* de = Ap + (size_t)n * 7; double* Sp = de + (size_t)E * 7;
    int* ends = (int*)(Sp + (size_t)E * 28);          // [2][E]: an edge's a and b where that node is optimised, -1 elsewhere and on an inactive edge
    int status = 0, bad = 0;
    double s_rz = 0.0, s_rr = 0.0;

    auto chol_solve = [&](const double* Lk, const double* rhs, double* out) {
        double y[7];
        for (int i = 0; i < 7; ++i) { double acc = rhs[i]; for (int j = 0; j < i; ++j) acc -= Lk[i * 7 + j] * y[j]; y[i] = acc / Lk[i * 7 + i]; }
        for (int i = 6; i >= 0; --i) { double acc = y[i]; for (int j = i + 1; j < 7; ++j) acc -= Lk[j * 7 + i] * out[j]; out[i] = acc / Lk[i * 7 + i]; }
    };
    // H-or-A product of p into Ap (owner rows); damp != 0 adds D p.  Returns this thread's part of p . Ap
    auto product = [&](bool damp) -> double {
        for (int e = tid; e < E; e += PGO_THREADS) {
            const int a = ends[e], b = ends[E + e];
            double dp[7], o[7];
            if ((a & b) < 0) continue;
            for (int i = 0; i < 7; ++i) dp[i] = (b >= 0 ? p[(size_t)b * 7 + i] : 0.0) - (a >= 0 ? p[(size_t)a * 7 + i] : 0.0);
            for (int i = 0; i < 7; ++i) o[i] = 0.0;
            int q = 0;
#pragma unroll
            for (int i = 0; i < 7; ++i)
#pragma unroll
                for (int j = i; j < 7; ++j) {
                    const double sij = Sp[(size_t)q * E + e];
                    o[i] += sij * dp[j];
                    if (j != i) o[j] += sij * dp[i];
                    ++q;
                }
            for (int i = 0; i < 7; ++i) de[(size_t)e * 7 + i] = o[i];
        }
        __syncthreads(); STA_SKEW(1109);
        double part = 0.0;
        for (int k = tid; k < n; k += PGO_THREADS) {
            if (!opt[k]) continue;
            double acc[7];
            for (int i = 0; i < 7; ++i) acc[i] = 0.0;
            int j = off[k];
            const int j1 = off[k + 1];
            for (; j + 4 <= j1; j += 4) {           // four half-edges' loads in flight at once; the sums keep the list's order
                int h[4];
                double dv[4][7];
#pragma unroll
                for (int u = 0; u < 4; ++u) h[u] = inc[j + u];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int i = 0; i < 7; ++i) dv[u][i] = de[(size_t)(h[u] >> 1) * 7 + i];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int i = 0; i < 7; ++i) acc[i] += ((h[u] & 1) ? 1.0 : -1.0) * dv[u][i];
            }
            for (; j < j1; ++j) {
                const int h = inc[j], e = h >> 1;
                const double sgn = (h & 1) ? 1.0 : -1.0;
                for (int i = 0; i < 7; ++i) acc[i] += sgn * de[(size_t)e * 7 + i];
            }
            for (int i = 0; i < 7; ++i) {
                const double pk = p[(size_t)k * 7 + i];
                if (damp) acc[i] += Dk[(size_t)k * 7 + i] * pk;
                Ap[(size_t)k * 7 + i] = acc[i];
                part += pk * acc[i];
            }
        }
        return part;
    };

    // the upper triangle of every S_e, element-major [28][E]: the product's loads are contiguous across the lanes of a wave (the
    // edge-major [E,7,7] of the interface costs a wave 64 lines per load, and 16 waves' worth of them does not stay in the L1)
    for (int e = tid; e < E; e += PGO_THREADS) {
        int q = 0;
        int a, b; bool inr;
        const bool act = pgo_edge(edges, opt, n, e, a, b, inr);
        ends[e] = act && opt[a] ? a : -1;
        ends[E + e] = act && opt[b] ? b : -1;
        if (!act) continue;
        for (int i = 0; i < 7; ++i) for (int j = i; j < 7; ++j) Sp[(size_t)(q++) * E + e] = S[(size_t)e * 49 + i * 7 + j];
    }
    for (int k = tid; k < n; k += PGO_THREADS) {
        if (!opt[k]) { for (int i = 0; i < 7; ++i) { x[(size_t)k * 7 + i] = 0.0; p[(size_t)k * 7 + i] = 0.0; } continue; }
        double A[49], Lk[49], rk[7], zk[7];
        for (int i = 0; i < 49; ++i) { A[i] = blocks[(size_t)k * 49 + i]; Lk[i] = 0.0; }
        for (int i = 0; i < 7; ++i) {
            const double d = fmin(fmax(A[i * 7 + i], dmin), dmax) / radius;
            Dk[(size_t)k * 7 + i] = d;
            A[i * 7 + i] += d;
        }
        for (int j = 0; j < 7; ++j) {
            double d = A[j * 7 + j];
            for (int q = 0; q < j; ++q) d -= Lk[j * 7 + q] * Lk[j * 7 + q];
            if (!(d > 0.0)) bad = 1;
            Lk[j * 7 + j] = sqrt(d);
            for (int i = j + 1; i < 7; ++i) {
                double s = A[i * 7 + j];
                for (int q = 0; q < j; ++q) s -= Lk[i * 7 + q] * Lk[j * 7 + q];
                Lk[i * 7 + j] = s / Lk[j * 7 + j];
            }
        }
        for (int i = 0; i < 49; ++i) L[(size_t)k * 49 + i] = Lk[i];
        for (int i = 0; i < 7; ++i) rk[i] = -g[(size_t)k * 7 + i];
        chol_solve(Lk, rk, zk);
        for (int i = 0; i < 7; ++i) {
            x[(size_t)k * 7 + i] = 0.0; r[(size_t)k * 7 + i] = rk[i]; z[(size_t)k * 7 + i] = zk[i]; p[(size_t)k * 7 + i] = zk[i];
            s_rz += rk[i] * zk[i]; s_rr += rk[i] * rk[i];
        }
    }
    bad = __syncthreads_or(bad); STA_SKEW(1116);
    double rz = pgo_block_sum(s_rz, red);
    const double gn = sqrt(pgo_block_sum(s_rr, red));
    double rn = gn;
    int it = 0;
    bool conv = false, run = true;
    if (bad) { status |= PGO_ST_CHOL; run = false; }
    else if (!isfinite(gn)) { status |= PGO_ST_BREAKDOWN; run = false; }
    else if (!(gn > 0.0)) run = false;
    if (run) {
        for (int k_it = 1; k_it <= max_iter; ++k_it) {
            const double pAp = pgo_block_sum(product(true), red);
            if (!(pAp > 0.0) || !isfinite(pAp)) { status |= PGO_ST_BREAKDOWN; conv = true; break; }
            const double alpha = rz / pAp;
            s_rz = 0.0; s_rr = 0.0;
            for (int k = tid; k < n; k += PGO_THREADS) {
                if (!opt[k]) continue;
                double rk[7], zk[7];
                for (int i = 0; i < 7; ++i) {
                    x[(size_t)k * 7 + i] += alpha * p[(size_t)k * 7 + i];
                    rk[i] = r[(size_t)k * 7 + i] - alpha * Ap[(size_t)k * 7 + i];
                    r[(size_t)k * 7 + i] = rk[i];
                }
                chol_solve(L + (size_t)k * 49, rk, zk);
                for (int i = 0; i < 7; ++i) { z[(size_t)k * 7 + i] = zk[i]; s_rz += rk[i] * zk[i]; s_rr += rk[i] * rk[i]; }
            }
            const double rz_new = pgo_block_sum(s_rz, red);
            rn = sqrt(pgo_block_sum(s_rr, red));
            it = k_it;
            if (!isfinite(rz_new) || !isfinite(rn)) { status |= PGO_ST_BREAKDOWN; conv = true; break; }
            if (rn <= rtol * gn) { conv = true; break; }
            const double beta = rz_new / rz;
            for (int k = tid; k < n; k += PGO_THREADS) {
                if (!opt[k]) continue;
                for (int i = 0; i < 7; ++i) p[(size_t)k * 7 + i] = z[(size_t)k * 7 + i] + beta * p[(size_t)k * 7 + i];
            }
            rz = rz_new;
            __syncthreads(); STA_SKEW(1110);
        }
        if (!conv) status |= PGO_ST_MAXITER;
    }
    // the model decrease -2 d.g - d.H d: one more product, without the damping, on p = x
    __syncthreads(); STA_SKEW(1111);
    double s_xg = 0.0;
    for (int k = tid; k < n; k += PGO_THREADS) {
        if (!opt[k]) continue;
        for (int i = 0; i < 7; ++i) { const double xk = x[(size_t)k * 7 + i]; p[(size_t)k * 7 + i] = xk; s_xg += xk * g[(size_t)k * 7 + i]; }
    }
    __syncthreads(); STA_SKEW(1112);
    const double xHx = pgo_block_sum(product(false), red);
    const double xg = pgo_block_sum(s_xg, red);
    if (tid == 0) {
        stats[0] = (double)it; stats[1] = gn > 0.0 ? rn / gn : 0.0; stats[2] = -2.0 * xg - xHx; stats[3] = (double)status;
    }
}
