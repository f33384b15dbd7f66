#pragma once
// The device-resident pose graph (sta_graph_plan / sta_graph_reset / sta_graph_commit / sta_graph_export; the contract is in
// include/sta_mi355.h, the yardstick is the numpy restatement tests/graph_cases.py), included by sta_api.hip after pgo.h.  The state is
// float64, the maps are fp32; every sum is float64 in a fixed order and there is no floating-point atomic in this file.  The group
// product is pgo.h's pgo_mul, the one sta_sim3_op runs.
#include "sta_common.h"
#include "pgo.h"
#include "sta_skew.h"       // STA_SKEW points: nothing unless -DSTA_WAVE_SKEW (libsta_mi355_skew.so)

#define GRAPH_CHUNK 2048          // map elements per workgroup of graph_reduce_kernel / graph_export_kernel (whatever H * W is)
#define GRAPH_THREADS 256         // 4 waves; a lane takes 4 consecutive floats per pass, a chunk is at most 2 passes
#define GRAPH_MAX_CALL_EDGES 16   // candidate edges of one sta_graph_commit
#define GRAPH_MAX_CALL_NODES 32   // two nodes per accepted edge

// one new node: its two maps in the call's inputs, its pool slot, and - for a view that already has a first node - that node's maps
// (ref_*; null: no scale edge).  ref_* point into the pool, or into the call's inputs when the first node is made by this very call.
struct GraphNodeJob {
    const float* depth; const float* conf; const float* intri; const float* ref_depth; const float* ref_conf;
    int node, pad;
};
struct GraphReduceArgs {
    GraphNodeJob job[GRAPH_MAX_CALL_NODES];
    float *pool_depth, *pool_conf, *pool_intri;
    double* partials;             // [job][chunk][4] = sum c, sum w Dn Df, sum w Dn Dn, sum sqrt(cn cf)
    int hw, chunks;
};

// grid (chunks, jobs).  One pass over the node's depth and confidence map: copy to the pool slot, accumulate the four sums of the chunk.
// Every term is float64 from the fp32 inputs; a lane sums its elements in ascending order, a wave by a shuffle tree, the four waves in
// order through LDS; the chunk's partial is STORED (graph_link_kernel sums the chunks in ascending order).
__global__ __launch_bounds__(GRAPH_THREADS) void graph_reduce_kernel(const GraphReduceArgs a) {
    STA_SKEW_ENTRY(1201);
    const GraphNodeJob j = a.job[blockIdx.y];
    const int chunk = blockIdx.x, t = threadIdx.x;
    const int base = chunk * GRAPH_CHUNK;
    const int n = min(GRAPH_CHUNK, a.hw - base);                       // a multiple of 256: H * W is
    const size_t slot = (size_t)j.node * (size_t)a.hw + (size_t)base;
    const bool has_ref = j.ref_depth != nullptr;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int o = t * 4; o < n; o += GRAPH_THREADS * 4) {
        const float4 d = *reinterpret_cast<const float4*>(j.depth + base + o);
        const float4 c = *reinterpret_cast<const float4*>(j.conf + base + o);
        *reinterpret_cast<float4*>(a.pool_depth + slot + o) = d;
        *reinterpret_cast<float4*>(a.pool_conf + slot + o) = c;
        const float dv[4] = {d.x, d.y, d.z, d.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) s[0] += (double)cv[e];
        if (has_ref) {
            const float4 rd = *reinterpret_cast<const float4*>(j.ref_depth + base + o);
            const float4 rc = *reinterpret_cast<const float4*>(j.ref_conf + base + o);
            const float rdv[4] = {rd.x, rd.y, rd.z, rd.w}, rcv[4] = {rc.x, rc.y, rc.z, rc.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double cc = (double)cv[e] * (double)rcv[e], w = fmax(cc, 1e-6), wd = w * (double)dv[e];
                s[1] += wd * (double)rdv[e];
                s[2] += wd * (double)dv[e];
                s[3] += sqrt(cc);
            }
        }
    }
    __shared__ double part[GRAPH_THREADS / 64][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double v = s[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((t & 63) == 0) part[t >> 6][q] = v;
    }
    __syncthreads(); STA_SKEW(1200);
    if (t < 4) {
        double v = part[0][t];
        for (int w = 1; w < GRAPH_THREADS / 64; ++w) v += part[w][t];
        a.partials[((size_t)blockIdx.y * (size_t)a.chunks + (size_t)chunk) * 4 + t] = v;
    }
    if (chunk == 0 && t < 9) a.pool_intri[(size_t)j.node * 9 + t] = j.intri[t];
}

// one accepted edge (i, j): nodes n_i, n_j (partials of jobs 2 e and 2 e + 1), the views' first nodes (-1: this node is the first)
struct GraphEdgeJob {
    const float* pose;            // device 4x4, row-major
    double conf;                  // the relative pose confidence
    int n_i, n_j, first_i, first_j, view_i, view_j;
};
struct GraphLinkArgs {
    GraphEdgeJob job[GRAPH_MAX_CALL_EDGES];
    const double* partials;
    double *poses, *edge_poses, *edge_confs, *mean_conf, *best_conf;
    long long* edges;
    int *first_node, *best_node;
    int n_jobs, num_edges, hw, chunks;
};

// pp.mat2SE3's branch rule as mat_to_se3_kernel applies it, evaluated in float64, scale 1
__device__ inline void graph_mat_to_sim3(const float* P, double* o) {
    const double m00 = P[0], m01 = P[1], m02 = P[2], m10 = P[4], m11 = P[5], m12 = P[6], m20 = P[8], m21 = P[9], m22 = P[10];
    double qx, qy, qz, qw;
    const double tr = m00 + m11 + m22;
    if (tr > 0.0) { const double s = sqrt(tr + 1.0) * 2.0; qw = 0.25 * s; qx = (m21 - m12) / s; qy = (m02 - m20) / s; qz = (m10 - m01) / s; }
    else if (m00 > m11 && m00 > m22) { const double s = sqrt(1.0 + m00 - m11 - m22) * 2.0; qw = (m21 - m12) / s; qx = 0.25 * s; qy = (m01 + m10) / s; qz = (m02 + m20) / s; }
    else if (m11 > m22) { const double s = sqrt(1.0 + m11 - m00 - m22) * 2.0; qw = (m02 - m20) / s; qx = (m01 + m10) / s; qy = 0.25 * s; qz = (m12 + m21) / s; }
    else { const double s = sqrt(1.0 + m22 - m00 - m11) * 2.0; qw = (m10 - m01) / s; qx = (m02 + m20) / s; qy = (m12 + m21) / s; qz = 0.25 * s; }
    const double nrm = (qw < 0.0 ? -1.0 : 1.0) / sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    o[0] = P[3]; o[1] = P[7]; o[2] = P[11]; o[3] = qx * nrm; o[4] = qy * nrm; o[5] = qz * nrm; o[6] = qw * nrm; o[7] = 1.0;
}
__device__ inline void graph_append_edge(const GraphLinkArgs& a, int e, int n0, int n1, const double* T, const double* w) {
    a.edges[2 * (size_t)e] = n0; a.edges[2 * (size_t)e + 1] = n1;
    for (int q = 0; q < 8; ++q) a.edge_poses[8 * (size_t)e + q] = T[q];
    for (int q = 0; q < 7; ++q) a.edge_confs[7 * (size_t)e + q] = w[q];
}

// ONE wave.  Lane l sums the chunk partials of job l in ascending chunk order; lane 0 then walks the accepted edges in order and does
// connect_view_i_j's bookkeeping (slam.py:205-239, pose_graph.py:13-17,31-45), which is sequential by nature.
__global__ __launch_bounds__(64) void graph_link_kernel(const GraphLinkArgs a) {
    __shared__ double sums[GRAPH_MAX_CALL_NODES][4];
    const int lane = threadIdx.x;
    if (lane < 2 * a.n_jobs) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        const double* p = a.partials + (size_t)lane * (size_t)a.chunks * 4;
        for (int c = 0; c < a.chunks; ++c)
            for (int q = 0; q < 4; ++q) v[q] += p[(size_t)c * 4 + q];
        for (int q = 0; q < 4; ++q) sums[lane][q] = v[q];
    }
    __syncthreads();
    if (lane != 0) return;
    int E = a.num_edges;
    const double hw = (double)a.hw;
    for (int e = 0; e < a.n_jobs; ++e) {
        const GraphEdgeJob j = a.job[e];
        for (int side = 0; side < 2; ++side) {
            const int n = side ? j.n_j : j.n_i, view = side ? j.view_j : j.view_i, first = side ? j.first_j : j.first_i;
            const double* s = sums[2 * e + side];
            const double mean = s[0] / hw;
            a.mean_conf[n] = mean;
            if (a.first_node[view] < 0) a.first_node[view] = n;
            if (mean > a.best_conf[view]) { a.best_conf[view] = mean; a.best_node[view] = n; }
            if (first >= 0) {
                const double S[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, s[1] / s[2]};
                const double w[7] = {2.0, 2.0, 2.0, 2.0, 2.0, 2.0, s[3] / hw};
                graph_append_edge(a, E++, n, first, S, w);
                double base[8], T[8];
                for (int q = 0; q < 8; ++q) base[q] = a.poses[8 * (size_t)first + q];
                pgo_mul(base, S, T);
                for (int q = 0; q < 8; ++q) a.poses[8 * (size_t)n + q] = T[q];
            }
        }
        double M[8];
        graph_mat_to_sim3(j.pose, M);
        if (j.first_i < 0) {                                            // view i is new: poses[n_i] = poses[n_j] * sim3_ij
            double base[8], T[8];
            for (int q = 0; q < 8; ++q) base[q] = a.poses[8 * (size_t)j.n_j + q];
            pgo_mul(base, M, T);
            for (int q = 0; q < 8; ++q) a.poses[8 * (size_t)j.n_i + q] = T[q];
        }
        const double w[7] = {j.conf, j.conf, j.conf, j.conf, j.conf, j.conf, j.conf};
        graph_append_edge(a, E++, j.n_i, j.n_j, M, w);
    }
}

struct GraphResetArgs {
    double *poses, *edge_poses, *edge_confs, *mean_conf, *best_conf;
    long long* edges;
    int *first_node, *best_node;
    int max_nodes, max_edges, max_views;
};
// PoseGraphNodes.reset / PoseGraphEdges.reset (pose_graph.py:19-23,47-54): identity poses, edges -1, weights 1, tables -1 / -100
__global__ __launch_bounds__(256) void graph_reset_kernel(const GraphResetArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.max_nodes) {
        for (int q = 0; q < 8; ++q) a.poses[8 * (size_t)i + q] = (q == 6 || q == 7) ? 1.0 : 0.0;
        a.mean_conf[i] = 0.0;
    }
    if (i < a.max_edges) {
        for (int q = 0; q < 8; ++q) a.edge_poses[8 * (size_t)i + q] = (q == 6 || q == 7) ? 1.0 : 0.0;
        for (int q = 0; q < 7; ++q) a.edge_confs[7 * (size_t)i + q] = 1.0;
        a.edges[2 * (size_t)i] = -1; a.edges[2 * (size_t)i + 1] = -1;
    }
    if (i < a.max_views) { a.first_node[i] = -1; a.best_node[i] = -1; a.best_conf[i] = -100.0; }
}

struct GraphExportArgs {
    const double* node_poses;
    const float *pool_depth, *pool_conf, *pool_intri;
    const int* best_node;
    float *poses, *scales, *depths, *confs, *intrinsics;
    int hw, max_nodes, scaled, filter;
    float thres;
};
// grid (chunks, views): the best node of view blockIdx.y gathered into the arguments of save_data_all (slam.py:358-379); with `scaled`
// and `filter` get_view's depth * scale and depth[conf < thres] = 0 (slam.py:313-320), in fp32 like the reference.  A view without a
// node (refused on the host) is written as zeros.
__global__ __launch_bounds__(GRAPH_THREADS) void graph_export_kernel(const GraphExportArgs a) {
    const int v = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const int node = a.best_node[v];
    const bool ok = node >= 0 && node < a.max_nodes;
    const int base = chunk * GRAPH_CHUNK;
    const int n = min(GRAPH_CHUNK, a.hw - base);
    double T[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (ok)
        for (int q = 0; q < 8; ++q) T[q] = a.node_poses[8 * (size_t)node + q];
    const float sc = (float)T[7];
    const size_t src = (size_t)(ok ? node : 0) * (size_t)a.hw + (size_t)base, dst = (size_t)v * (size_t)a.hw + (size_t)base;
    for (int o = t * 4; o < n; o += GRAPH_THREADS * 4) {
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f), c = d;
        if (ok) {
            d = *reinterpret_cast<const float4*>(a.pool_depth + src + o);
            c = *reinterpret_cast<const float4*>(a.pool_conf + src + o);
        }
        if (a.scaled) { d.x *= sc; d.y *= sc; d.z *= sc; d.w *= sc; }
        if (a.filter) {
            if (c.x < a.thres) d.x = 0.f;
            if (c.y < a.thres) d.y = 0.f;
            if (c.z < a.thres) d.z = 0.f;
            if (c.w < a.thres) d.w = 0.f;
        }
        *reinterpret_cast<float4*>(a.depths + dst + o) = d;
        *reinterpret_cast<float4*>(a.confs + dst + o) = c;
    }
    if (chunk != 0) return;
    if (t < 9) a.intrinsics[(size_t)v * 9 + t] = ok ? a.pool_intri[(size_t)node * 9 + t] : 0.f;
    if (t == 0) {
        double R[9];
        pgo_rot(T + 3, R);
        float* P = a.poses + (size_t)v * 16;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) P[4 * r + c] = ok ? (float)R[3 * r + c] : 0.f;
            P[4 * r + 3] = (float)T[r];
        }
        P[12] = 0.f; P[13] = 0.f; P[14] = 0.f; P[15] = 1.f;
        a.scales[v] = sc;
    }
}
