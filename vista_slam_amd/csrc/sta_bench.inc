// FLOP model of the path (sta_flops_per_pair: product ABI) and - in -DSTA_TEST_HOOKS builds only - the GEMM / attention
// micro-benchmark and ablation entry points used by tools/gemm_*.py.
// Included by sta_api.hip (one translation unit).

// ------------------------------------------------------------------------------------------ FLOPs + GEMM bench
extern "C" double sta_flops_per_pair(const sta_handle* h, int H, int W) {
    if (!h) return 0;
    const sta_config& c = h->cfg;
    const double E = c.enc_embed_dim, D = c.dec_embed_dim, R = c.mlp_ratio;
    const double hp = H / 16, wp = W / 16, N = hp * wp, Np = N + 1;
    // per block: qkv 6NE^2 + proj 2NE^2 + mlp 4R NE^2  (R=4 -> 24 N E^2)
    double f_enc = 2 * N * 768 * E + c.enc_depth * ((8 + 4 * R) * N * E * E + 4 * N * N * E);
    double f_dec = 4 * N * E * D + 2.0 * c.dec_depth * ((16 + 4 * R) * Np * D * D + 8 * Np * Np * D);
    // DPT: reference op placement (out_conv after the upsample), per view
    auto conv = [](double hh, double ww, double ci, double co, double k) { return 2.0 * hh * ww * ci * co * k * k; };
    double h3 = floor((hp - 1) / 2) + 1, w3 = floor((wp - 1) / 2) + 1;
    double f = 0;
    f += conv(hp, wp, E, 96, 1) + 2.0 * hp * wp * 96 * 96 * 16;
    f += conv(hp, wp, D, 192, 1) + 2.0 * hp * wp * 192 * 192 * 4;
    f += conv(hp, wp, D, 384, 1);
    f += conv(hp, wp, D, 768, 1) + conv(h3, w3, 768, 768, 3);
    f += conv(4 * hp, 4 * wp, 96, 256, 3) + conv(2 * hp, 2 * wp, 192, 256, 3) + conv(hp, wp, 384, 256, 3) + conv(h3, w3, 768, 256, 3);
    f += 2 * conv(h3, w3, 256, 256, 3) + conv(hp, wp, 256, 256, 1);
    f += 4 * conv(hp, wp, 256, 256, 3) + conv(2 * hp, 2 * wp, 256, 256, 1);
    f += 4 * conv(2 * hp, 2 * wp, 256, 256, 3) + conv(4 * hp, 4 * wp, 256, 256, 1);
    f += 4 * conv(4 * hp, 4 * wp, 256, 256, 3) + conv(8 * hp, 8 * wp, 256, 256, 1);
    f += conv(8 * hp, 8 * wp, 256, 128, 3) + conv(16 * hp, 16 * wp, 128, 128, 3) + conv(16 * hp, 16 * wp, 128, 4, 1);
    double f_pose = 2.0 * (D * 512 + 2 * 512 * 512 + 512 * 13);
    return 2 * f_enc + f_dec + 2 * f + 2 * f_pose;
}

#ifdef STA_TEST_HOOKS      // everything below: libsta_mi355_test.so only (include/sta_mi355_debug.h)

__global__ void fill_rand_f16_kernel(f16* p, int64_t n, uint32_t seed, float scale) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += step) {
        uint32_t x = (uint32_t)i * 0x9E3779B1u + seed;
        x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
        p[i] = (f16)(((float)(x >> 8) * (2.0f / 16777216.0f) - 1.0f) * scale);
    }
}

template <bool SPLIT, int BM, int BN, int WMS, int WNS, int ABL>
static int bench_launch2s(const GemmParams& p, hipStream_t st) {
    constexpr int smem = gemm2_smem_bytes<SPLIT, BM, BN>();
    constexpr auto kern = gemm2_kernel<SPLIT, A_DENSE, EPI_F32, BM, BN, WMS, WNS, ABL>;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    CHK(set_smem_once<kern>(dev, smem));
    hipLaunchKernelGGL(kern, dim3((unsigned)(((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN))), dim3(WMS * WNS * 64), smem, st, p);
    return 0;
}
template <int BM, int BN, int WMS, int WNS, int ABL>
static int bench_launch2(bool split, const GemmParams& p, hipStream_t st) {
    if (split) return bench_launch2s<true, BM, BN, WMS, WNS, ABL>(p, st);
    STA_F16ONLY(return (bench_launch2s<false, BM, BN, WMS, WNS, ABL>(p, st)));
}

// tile: 0 = automatic product selection, 1 = 128x128, 2 = 256x256, 3 = 256x128; abl: gemm2 ablation (tile 2/3 only)
static float g_bench_ghz = 0.f;
extern "C" float sta_bench_gemm_last_ghz() { return g_bench_ghz; }

extern "C" int sta_bench_gemm(sta_handle* h, int M, int N, int K, int iters, int tile, int abl, float* ms_out, void* stream) {
    REQUIRE(h && ms_out && iters > 0, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    int64_t bytes = ((int64_t)M * K + (int64_t)N * K) * 4 + (int64_t)M * N * 4 + N * 4 + (1 << 16);
    CHK(ensure_ws(h, bytes, st));
    h->dry = false;
    Bump ws = cur_bump(h);
    Planes A = ws.act(M, K, true);
    Lin Wt; Wt.N = N; Wt.K = K; Wt.w = ws.act(N, K, true);
    Wt.bias = (float*)ws.take((int64_t)N * 4);
    float* C = (float*)ws.take((int64_t)M * N * 4);
    unsigned long long* clk = (unsigned long long*)ws.take(16);
    REQUIRE(!ws.overflow, "internal: bench workspace overflow");
    // random operands (both hi and lo halves of every row block get full-range random bits: the data
    // dependence of MFMA power is what matters for a throughput number)
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, A.hi, (int64_t)M * K * 2, 1u, 1.0f);
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, Wt.w.hi, (int64_t)N * K * 2, 3u, 0.03f);
    HIPCHK(hipMemsetAsync(Wt.bias, 0, (size_t)N * 4, st));
    if (!split) { A.lo = nullptr; }   // f16 mode reads the same buffer as [K/32][M][32]
    GemmParams p = gp_dense(A, K, Wt, M);
    p.range = h->range;
    p.C32 = C; p.ldc = N; p.ldr = N; p.zero_page = h->zero_page;
    const int keep = h->gemm_variant;
    auto once = [&]() -> int {
#ifdef STA_BENCH_EXPERIMENTS      // ablations and retired tile shapes (DESIGN.md section 5): build with -DSTA_BENCH_EXPERIMENTS
        if (tile >= 2 && abl > 0) {
            if (tile == 2) {
                switch (abl) {
                    case 1: return bench_launch2<256, 256, 2, 4, 1>(split, p, st);
                    case 2: return bench_launch2<256, 256, 2, 4, 2>(split, p, st);
                    case 3: return bench_launch2<256, 256, 2, 4, 3>(split, p, st);
                    case 4: return bench_launch2<256, 256, 2, 4, 4>(split, p, st);
                    case 5: return bench_launch2<256, 256, 2, 4, 5>(split, p, st);
                    case 6: return bench_launch2<256, 256, 2, 4, 6>(split, p, st);
                    default: return bench_launch2<256, 256, 2, 4, 7>(split, p, st);
                }
            }
            switch (abl) {
                case 1: return bench_launch2<192, 128, 2, 4, 1>(split, p, st);
                case 2: return bench_launch2<192, 128, 2, 4, 2>(split, p, st);
                case 3: return bench_launch2<192, 128, 2, 4, 3>(split, p, st);
                case 4: return bench_launch2<192, 128, 2, 4, 4>(split, p, st);
                case 5: return bench_launch2<192, 128, 2, 4, 5>(split, p, st);
                case 6: return bench_launch2<192, 128, 2, 4, 6>(split, p, st);
                default: return bench_launch2<192, 128, 2, 4, 7>(split, p, st);
            }
        }
#else
        if (abl > 0) return set_err("bench: main-loop ablations need a library built with -DSTA_BENCH_EXPERIMENTS");
#endif
        if (tile >= 100) {      // 100 + t: tile t with the in-place residual epilogue (attn.proj / mlp.fc2 form)
            GemmParams q = p; q.resid = q.C32; q.ldr = q.ldc;
            switch (tile - 100) {
                case 6: return bench_launch2<192, 128, 2, 4, 0>(split, q, st);
                case 21: return bench_launch2<256, 256, 4, 4, 0>(split, q, st);
                case 22: return bench_launch2<192, 256, 3, 4, 0>(split, q, st);
#ifdef STA_BENCH_EXPERIMENTS
                case 2: return bench_launch2<256, 256, 2, 4, 0>(split, q, st);
                case 20: return bench_launch2<192, 128, 3, 2, 0>(split, q, st);
                case 23: return bench_launch2<128, 256, 2, 4, 0>(split, q, st);
                case 25: return bench_launch2<192, 96, 2, 3, 0>(split, q, st);
                case 26: return bench_launch2<384, 128, 4, 2, 0>(split, q, st);
#endif
                default: return set_err("bench: unknown residual tile %d", tile);
            }
        }
        if (tile == 21) return bench_launch2<256, 256, 4, 4, 0>(split, p, st);   // 16 waves, wave tile 64x64
        if (tile == 22) return bench_launch2<192, 256, 3, 4, 0>(split, p, st);   // 12 waves, wave tile 64x64
        if (tile == 6) return bench_launch2<192, 128, 2, 4, 0>(split, p, st);
#ifdef STA_BENCH_EXPERIMENTS
        if (tile == 16) { GemmParams q = p; q.mx = 1; return launch_gemm2<true, A_DENSE, EPI_F32, 192, 128, 2, 4, 2, true>(q, st); }   // the shipped f16mx kernel (random bits as operands: timing only)
        if (tile == 17) { GemmParams q = p; q.mx = 1; q.resid = q.C32; q.ldr = q.ldc; return launch_gemm2<true, A_DENSE, EPI_F32, 192, 128, 2, 4, 2, true>(q, st); }
        if (tile == 20) return bench_launch2<192, 128, 3, 2, 0>(split, p, st);   // 6 waves, wave tile 64x64
        if (tile == 23) return bench_launch2<128, 256, 2, 4, 0>(split, p, st);   // 8 waves, wave tile 64x64
        if (tile == 25) return bench_launch2<192, 96, 2, 3, 0>(split, p, st);    // 6 waves, wave tile 96x32
        if (tile == 26) return bench_launch2<384, 128, 4, 2, 0>(split, p, st);   // 8 waves, wave tile 96x64
        if (tile == 2) return bench_launch2<256, 256, 2, 4, 0>(split, p, st);
        if (tile == 3) return bench_launch2<256, 128, 4, 2, 0>(split, p, st);
        if (tile == 10) return split ? launch_gemm2<true, A_DENSE, EPI_F32, 256, 128, 4, 2, 3>(p, st)
                                     : launch_gemm2<false, A_DENSE, EPI_F32, 256, 128, 4, 2, 3>(p, st);   // 3-stage ring experiment
        if (tile == 11) return bench_launch2<256, 256, 2, 4, 8>(split, p, st);   // staggered DMA issue
        if (tile == 12) return bench_launch2<192, 128, 2, 4, 8>(split, p, st);
        if (tile == 5) return bench_launch2<192, 256, 2, 4, 0>(split, p, st);
        if (tile == 13) { GemmParams q = p; q.resid = q.C32; q.ldr = q.ldc; return bench_launch2<192, 128, 2, 4, 0>(split, q, st); }   // in-place residual like attn.proj / mlp.fc2
        if (tile == 7) return bench_launch2<192, 128, 2, 2, 0>(split, p, st);
        if (tile == 8) return bench_launch2<128, 192, 2, 2, 0>(split, p, st);
        if (tile == 9) return bench_launch2<128, 128, 2, 2, 0>(split, p, st);
#else
        if (tile > 1) return set_err("bench: tile %d is an experiment (build with -DSTA_BENCH_EXPERIMENTS); product tiles: 0 auto, 1, 6, 21, 22, +100 = in-place residual", tile);
#endif
        h->gemm_variant = tile == 1 ? 1 : 0;
        int r = launch_gemm<A_DENSE, EPI_F32>(h, p, st);
        h->gemm_variant = keep;
        return r;
    };
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) CHK(once());
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) CHK(once());
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipGetLastError());
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    // effective shader clock during this kernel (DVFS: the chip clocks to its power budget): a few extra launches
    // with the in-kernel probe on (s_memtime vs the constant 100 MHz s_memrealtime), sampled on every 64th block
    HIPCHK(hipMemsetAsync(clk, 0, 16, st));
    p.clk_dbg = clk;
    for (int i = 0; i < 3; ++i) CHK(once());
    p.clk_dbg = nullptr;
    unsigned long long hc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hc, clk, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    g_bench_ghz = hc[1] ? (float)((double)hc[0] / ((double)hc[1] / 100e6) * 1e-9) : 0.f;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return 0;
}


// In-kernel timeline of ONE launch of the product's GEMM for this shape (tools/gemm_stamps.py): every workgroup stores four
// s_memrealtime stamps (100 MHz: 10 ns) - entry, first K tile landed, main loop done, epilogue stores acknowledged.
// resid != 0: the in-place residual form (attn.proj / mlp.fc2: at SLAM scale K slices to slabs).  out[0..9] = workgroups,
// span of the kernel (first entry -> last exit), median entry->first-tile, median loop, median epilogue, spread of the entries,
// spread of the exits, HIP-event duration of the same launch, K slices, median whole workgroup - all in microseconds.
extern "C" int sta_bench_gemm_stamps(sta_handle* h, int M, int N, int K, int resid, double* out, unsigned long long* raw, int raw_cap, void* stream) {
    REQUIRE(h && out && M > 0 && N > 0 && K > 0, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    int64_t bytes = ((int64_t)M * K + (int64_t)N * K) * 4 + (int64_t)M * N * 4 + N * 4 + (int64_t)8192 * 32 + (1 << 16);
    CHK(ensure_ws(h, bytes, st));
    h->dry = false;
    Bump ws = cur_bump(h);
    Planes A = ws.act(M, K, true);
    Lin Wt; Wt.N = N; Wt.K = K; Wt.w = ws.act(N, K, true);
    Wt.bias = (float*)ws.take((int64_t)N * 4);
    float* C = (float*)ws.take((int64_t)M * N * 4);
    const int cap = 8192;
    unsigned long long* stamps = (unsigned long long*)ws.take((int64_t)cap * 32);
    REQUIRE(!ws.overflow && h->prec != STA_PREC_F16, "internal: bench workspace overflow / f16x3 only");
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, A.hi, (int64_t)M * K * 2, 1u, 1.0f);
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, Wt.w.hi, (int64_t)N * K * 2, 3u, 0.03f);
    HIPCHK(hipMemsetAsync(Wt.bias, 0, (size_t)N * 4, st));
    HIPCHK(hipMemsetAsync(C, 0, (size_t)M * N * 4, st));
    GemmParams p = gp_dense(A, K, Wt, M);
    p.range = h->range;
    p.C32 = C; p.ldc = N; p.ldr = N; p.zero_page = h->zero_page;
    if (resid) { p.resid = C; p.slab = h->cur->slab; }
    int ks = 0;
    // resid == 2: through gemm_f32, i.e. with the specialised in-place residual epilogue (EPI_F32R) at throughput scale
    auto launch = [&](GemmParams& q) -> int {
        if (resid == 2 && !small_grid(h, M, N)) { q.slab = nullptr; return launch_gemm<A_DENSE, EPI_F32R>(h, q, st, &ks); }
        return launch_gemm<A_DENSE, EPI_F32>(h, q, st, &ks);
    };
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) CHK(launch(p));
    HIPCHK(hipMemsetAsync(stamps, 0, (size_t)cap * 32, st));
    p.stamps = stamps;
    CHK(launch(p));       // warm (code path with stamps)
    HIPCHK(hipMemsetAsync(stamps, 0, (size_t)cap * 32, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventRecord(e0, st));
    CHK(launch(p));
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> hs((size_t)cap * 4);
    HIPCHK(hipMemcpy(hs.data(), stamps, (size_t)cap * 32, hipMemcpyDeviceToHost));
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (raw) memcpy(raw, hs.data(), (size_t)(raw_cap < cap ? raw_cap : cap) * 32);
    std::vector<double> pro, loop, epi, whole;
    unsigned long long t0min = ~0ull, t0max = 0, t3min = ~0ull, t3max = 0;
    for (int b = 0; b < cap; ++b) {
        const unsigned long long* q = &hs[(size_t)b * 4];
        if (!q[3]) continue;
        pro.push_back((double)(q[1] - q[0]) * 0.01); loop.push_back((double)(q[2] - q[1]) * 0.01); epi.push_back((double)(q[3] - q[2]) * 0.01);
        whole.push_back((double)(q[3] - q[0]) * 0.01);
        if (q[0] < t0min) t0min = q[0]; if (q[0] > t0max) t0max = q[0];
        if (q[3] < t3min) t3min = q[3]; if (q[3] > t3max) t3max = q[3];
    }
    REQUIRE(!pro.empty(), "no stamps recorded (this shape did not run on a gemm2 family)");
    auto med = [](std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    out[0] = (double)pro.size(); out[1] = (double)(t3max - t0min) * 0.01; out[2] = med(pro); out[3] = med(loop); out[4] = med(epi);
    out[5] = (double)(t0max - t0min) * 0.01; out[6] = (double)(t3max - t3min) * 0.01; out[7] = ms * 1e3; out[8] = ks; out[9] = med(whole);
    return 0;
}

// The attention kernel alone on random operands: `iters` back-to-back launches between two events.  pose: the decoder form
// (AttnParams::pose, nq == nk patch tokens).  (`which` is reserved for kernel variants under test; 0 = the product kernel.)
extern "C" int sta_bench_attention(sta_handle* h, int S, int heads, int nq, int nk, int pose, int iters, int which, float* ms_out, void* stream) {
    REQUIRE(h && ms_out && iters > 0 && S > 0 && heads > 0 && nq > 0 && nk > 0, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int nmax = (nq > nk ? nq : nk) + (pose ? 1 : 0), npad = rup(nmax, 64);
    const int64_t hsz = (int64_t)S * heads * npad * 64, M = (int64_t)S * nq + (pose ? S : 0);
    CHK(ensure_ws(h, (3 * hsz + M * heads * 64) * 4 + (1 << 16), st));
    h->dry = false;
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, true); o.k = ws.planes(hsz, true); o.vt = ws.planes(hsz, true);
    Planes ao = ws.act(M, heads * 64, true);
    REQUIRE(!ws.overflow, "internal: bench workspace overflow");
    if (!split) { o.q.lo = o.k.lo = o.vt.lo = nullptr; ao.lo = nullptr; }
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, o.q.hi, hsz * 2, 5u, 1.0f);
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, o.k.hi, hsz * 2, 7u, 1.0f);
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, o.vt.hi, hsz * 2, 9u, 1.0f);
    REQUIRE(which == 0, "sta_bench_attention: no alternative kernel in this build");
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    int rc = 0;
    for (int i = 0; i < 2 && rc == 0; ++i) rc = run_attn(h, o, ao, heads * 64, S, heads, nq, nk, 0, st, pose != 0);
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters && rc == 0; ++i) rc = run_attn(h, o, ao, heads * 64, S, heads, nq, nk, 0, st, pose != 0);
    HIPCHK(hipEventRecord(e1, st));
    if (rc != 0) return rc;
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return 0;
}
// The two-group attention launch alone (run_attn_mixed) on random operands: ms per launch over `iters` back-to-back launches.
extern "C" int sta_bench_attention_mixed(sta_handle* h, int S1, int S2, int heads, int nq_a, int nk_a, int nq_b, int nk_b, int kv_shift,
                                         int iters, float* ms_out, void* stream) {
    REQUIRE(h && ms_out && iters > 0 && S1 > 0 && S2 >= 0 && heads > 0 && nq_a > 0 && nk_a > 0 && (S2 == 0 || (nq_b > 0 && nk_b > 0)), "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int S = S1 + S2;
    const int nmax = std::max(std::max(nq_a, nk_a), S2 ? std::max(nq_b, nk_b) : 0), npad = rup(nmax + 1, 64);
    const int64_t hsz = (int64_t)S * heads * npad * 64, M = (int64_t)S1 * (nq_a + 1) + (int64_t)S2 * (nq_b + 1);
    CHK(ensure_ws(h, (3 * hsz + M * heads * 64) * 4 + (1 << 16), st));
    h->dry = false;
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, true); o.k = ws.planes(hsz, true); o.vt = ws.planes(hsz, true);
    Planes ao = ws.act(M, heads * 64, true);
    REQUIRE(!ws.overflow, "internal: bench workspace overflow");
    if (!split) { o.q.lo = o.k.lo = o.vt.lo = nullptr; ao.lo = nullptr; }
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, o.q.hi, hsz * 2, 5u, 1.0f);
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, o.k.hi, hsz * 2, 7u, 1.0f);
    hipLaunchKernelGGL(fill_rand_f16_kernel, dim3(2048), dim3(256), 0, st, o.vt.hi, hsz * 2, 9u, 1.0f);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    int rc = 0;
    for (int i = 0; i < 2 && rc == 0; ++i) rc = run_attn_mixed(h, o, ao, heads * 64, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, kv_shift, st);
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters && rc == 0; ++i) rc = run_attn_mixed(h, o, ao, heads * 64, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, kv_shift, st);
    HIPCHK(hipEventRecord(e1, st));
    if (rc != 0) return rc;
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    return 0;
}
#endif   // STA_TEST_HOOKS
