// Kernel-level test entry points (declared in include/sta_mi355_debug.h).  They wrap single
// kernels of the product path with fp32 device tensors in/out so the GPU parity tests can compare
// each kernel with a plain fp32 reference of the same op.  Not used by the product path.

// experiment switch 4 (tests): the debug GEMM / convolution / ConvT / bilinear entries run in the DPT head's f16mx arithmetic
// (f16mx rows in, f16mx weights, f16mx rows out) - what precision f16x3h does inside the head
static bool dbg_mx(const sta_handle* h) { return h->opt[4] == 1 && (h->mx_mask & CLS_HEAD) != 0; }
// experiment switch 4 == 2 (tests, precision f16x3m): the debug GEMM runs the MLP's f16mx path - via_f16 + GELU: mlp.fc1's epilogue
// writing f16mx rows from f16x3 inputs; fp32 output (+ residual): mlp.fc2 = f16mx rows in, f16mx weights, fp32 epilogues
static bool dbg_mx_mlp(const sta_handle* h) { return h->opt[4] == 2 && (h->mx_mask & CLS_FC2) != 0; }

static int dbg_planes_to_f32(sta_handle* h, const Planes& p, int64_t ibstride_rows, int nb, int rows, int C, float* out, hipStream_t st) {
    int64_t total = (int64_t)nb * rows * C;
    int blocks = (int)((total + 255) / 256); if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(planes_to_f32_kernel, dim3(blocks), dim3(256), 0, st, p.hi, p.lo, ibstride_rows, rows, C, total, out, p.rp, p.mx ? 1 : 0);
    HIPCHK(hipGetLastError());
    return 0;
}

// 0xFF (an fp16 NaN pattern) into what the kernel under test must overwrite: an element it never wrote reads back as NaN instead
// of as whatever the shared workspace held - often the correct values of the previous, identically shaped test.
static int dbg_poison(void* ptr, int64_t bytes, hipStream_t st) {
    HIPCHK(hipMemsetAsync(ptr, 0xFF, (size_t)bytes, st));
    return 0;
}
// ... the blocked planes of Bump::act(rows, cols, split) (output planes that are not also an input)
static int dbg_poison_act(const Planes& p, int64_t rows, int64_t cols, hipStream_t st) {
    return dbg_poison(p.hi, rows * ((cols + 31) & ~int64_t(31)) * (p.lo ? 4 : 2), st);
}
// ... the row-major Q / K / V^T planes of Bump::planes(elems, split)
static int dbg_poison_planes(const Planes& p, int64_t elems, hipStream_t st) {
    CHK(dbg_poison(p.hi, elems * 2, st));
    if (p.lo) CHK(dbg_poison(p.lo, elems * 2, st));
    return 0;
}

static int dbg_make_lin(sta_handle* h, Bump& ws, const float* w, const float* bias, int N, int K, int mode,
                        int d0, int d1, int d2, int d3, Lin& L, hipStream_t st, bool mx = false, int cls = CLS_HEAD) {
    L.N = N; L.K = K; L.w = ws.act(N, K, true); L.bias = const_cast<float*>(bias);
    int64_t n = (int64_t)N * K;
    int blocks = (int)((n + 255) / 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(repack_weight_kernel, dim3(blocks), dim3(256), 0, st, w, L.w.hi, L.w.lo, n, mode, d0, d1, d2, d3, (int64_t)N, (int64_t)K, (int64_t)0, 0, h->range);
    if (mx) {   // f16mx copy (the DPT head's layers in precision f16x3h)
        L.cls = cls;
        L.wmx = ws.act(N, K, true);
        hipLaunchKernelGGL(repack_weight_kernel, dim3(blocks), dim3(256), 0, st, w, L.wmx.hi, L.wmx.lo, n, mode, d0, d1, d2, d3, (int64_t)N, (int64_t)K, (int64_t)0, 1, h->range);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// out[M,N] = act(A[M,K] W[N,K]^T + bias) ; via_f16 != 0 routes through the fp16-plane epilogue.
extern "C" int sta_debug_gemm(sta_handle* h, const float* A, const float* W, const float* bias, int M, int N, int K,
                              int act, int via_f16, const float* resid, float* out, void* stream) {
    REQUIRE(h && A && W && out, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    // experiment switch 4 (tests): the debug GEMM runs in the DPT head's f16mx arithmetic (plane epilogue only: the head's 1x1
    // convolutions); same rule as use_mx(): an f16mx kernel needs N % 64 == 0
    const bool mlp = dbg_mx_mlp(h) && N % 64 == 0;
    const bool mx = (dbg_mx(h) && via_f16 && N % 64 == 0) || (mlp && !via_f16);
    CHK(ensure_ws(h, ((int64_t)M * K + (int64_t)2 * N * K + (int64_t)M * N) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes a = ws.act(M, K, split);
    Lin L; CHK(dbg_make_lin(h, ws, W, bias, N, K, 0, N, K, 1, 1, L, st, mx, mlp ? CLS_FC2 : CLS_HEAD));
    CHK(run_rows_to_planes(h, A, (int64_t)M * K, 1, M, K, a, st, 0, mx));
    a.mx = mx;
    if (via_f16) {
        Planes o = ws.act(M, N, split);
        o.mx = (mx && act != ACT_GELU) || (mlp && act == ACT_GELU);
        REQUIRE(!ws.overflow, "debug ws overflow");
        CHK(gemm_f16(h, a, L, M, o, act, st, o.mx));
        CHK(dbg_planes_to_f32(h, o, 0, 1, M, N, out, st));
    } else {
        REQUIRE(!ws.overflow, "debug ws overflow");
        if (resid && resid != out) HIPCHK(hipMemcpyAsync(out, resid, (size_t)M * N * 4, hipMemcpyDeviceToDevice, st));
        CHK(gemm_f32(h, a, L, M, out, N, resid ? out : nullptr, st));
    }
    return 0;
}

// QKV projection + RoPE epilogue.  x [S*ntok, K], W [3C, K]; outputs fp32 [S, heads, ntok, 64] each.
extern "C" int sta_debug_qkv_rope(sta_handle* h, const float* x, const float* W, const float* bias, int S, int ntok, int K, int C,
                                  int wp, int has_pose_tok, float* q, float* k, float* v, void* stream) {
    REQUIRE(h && x && W && q && k && v, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    // has_pose_tok == 2: the decoder's row order - x = [S*ntok patch rows | S pose rows], the buffers hold ntok + 1 tokens
    // per sequence with the pose token LAST (decode_impl)
    const bool tail_pose = has_pose_tok == 2;
    if (tail_pose) has_pose_tok = 0;
    const int M = S * ntok + (tail_pose ? S : 0), heads = C / 64, npad = rup(ntok + (tail_pose ? 1 : 0), 64);
    int hp = (ntok - has_pose_tok + wp - 1) / wp;
    CHK(ensure_rope(h, hp > wp ? hp : wp));
    int64_t hsz = (int64_t)S * heads * npad * 64;
    const bool mx = false;
    CHK(ensure_ws(h, ((int64_t)M * K + (int64_t)6 * C * K + 3 * hsz) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes a = ws.act(M, K, split);
    Lin L; CHK(dbg_make_lin(h, ws, W, bias, 3 * C, K, 0, 3 * C, K, 1, 1, L, st, mx));
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, split); o.k = ws.planes(hsz, split); o.vt = ws.planes(hsz, split);
    REQUIRE(!ws.overflow, "debug ws overflow");
    HIPCHK(hipMemsetAsync(o.vt.hi, 0, hsz * 2, st)); if (split) HIPCHK(hipMemsetAsync(o.vt.lo, 0, hsz * 2, st));
    CHK(run_rows_to_planes(h, x, (int64_t)M * K, 1, M, K, a, st, 0, mx));
    {
        TailHint tail(h, tail_pose ? S : 0);
        CHK(gemm_qkv(h, a, L, M, C, C, C, o, ntok, heads, wp, has_pose_tok, st, tail_pose ? S * ntok : 0));
    }
    const int ntok_o = ntok + (tail_pose ? 1 : 0);
    CHK(dbg_planes_to_f32(h, o.q, npad, S * heads, ntok_o, 64, q, st));
    CHK(dbg_planes_to_f32(h, o.k, npad, S * heads, ntok_o, 64, k, st));
    // Vt [S*heads, 64, npad] -> v [S*heads, ntok, 64]: read back as [S*heads*64 rows, npad] then transpose on host
    CHK(dbg_planes_to_f32(h, o.vt, 0, 1, S * heads * 64, npad, v, st));   // caller passes a [S*heads*64*npad] buffer
    return 0;
}

// The decoder's paired QKV launch (gemm_qkv_pair: attn.qkv + cross_attn.projk|projv) on inputs in the decoder's row order,
// x_a / x_b = [S*ntok patch rows | S pose rows]: a = qkv (nq = nk = nv = C), b = projk|projv (nq = 0, nk = nv = C).  Outputs
// hold ntok + 1 tokens per sequence, the pose token last: q_a, k_a, k_b fp32 [S, C/64, ntok + 1, 64]; vt_a, vt_b the
// transposed buffers [S*C/64*64, roundup(ntok + 1, 64)] (padding zeroed before the launch).
extern "C" int sta_debug_qkv_pair(sta_handle* h, const float* x_a, const float* w_a, const float* bias_a, const float* x_b,
                                  const float* w_b, const float* bias_b, int S, int ntok, int K, int C, int wp,
                                  float* q_a, float* k_a, float* vt_a, float* k_b, float* vt_b, void* stream) {
    REQUIRE(h && x_a && w_a && bias_a && x_b && w_b && bias_b && q_a && k_a && vt_a && k_b && vt_b, "bad argument");
    REQUIRE(S > 0 && ntok > 0 && wp > 0 && ntok % wp == 0 && C % 64 == 0 && K % GEMM_BK == 0, "bad shape");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int M = S * ntok + S, heads = C / 64, nt = ntok + 1, npad = rup(nt, 64);
    CHK(ensure_rope(h, ntok / wp > wp ? ntok / wp : wp));
    const int64_t hsz = (int64_t)S * heads * npad * 64;
    CHK(ensure_ws(h, ((int64_t)2 * M * K + (int64_t)2 * 5 * C * K + 6 * hsz) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes a = ws.act(M, K, split), b = ws.act(M, K, split);
    Lin La, Lb;
    CHK(dbg_make_lin(h, ws, w_a, bias_a, 3 * C, K, 0, 3 * C, K, 1, 1, La, st));
    CHK(dbg_make_lin(h, ws, w_b, bias_b, 2 * C, K, 0, 2 * C, K, 1, 1, Lb, st));
    QKVOut oa, ob; oa.npad = ob.npad = npad;
    oa.q = ws.planes(hsz, split); oa.k = ws.planes(hsz, split); oa.vt = ws.planes(hsz, split);
    ob.q = ws.planes(hsz, split); ob.k = ws.planes(hsz, split); ob.vt = ws.planes(hsz, split);
    REQUIRE(!ws.overflow, "debug ws overflow");
    for (const Planes* v : {&oa.vt, &ob.vt}) { HIPCHK(hipMemsetAsync(v->hi, 0, hsz * 2, st)); if (split) HIPCHK(hipMemsetAsync(v->lo, 0, hsz * 2, st)); }
    CHK(run_rows_to_planes(h, x_a, (int64_t)M * K, 1, M, K, a, st));
    CHK(run_rows_to_planes(h, x_b, (int64_t)M * K, 1, M, K, b, st));
    {
        TailHint tail(h, S);
        GemmParams pa, pb;
        CHK(gp_qkv(h, pa, a, La, M, C, C, C, oa, ntok, heads, wp, 0, S * ntok));
        CHK(gp_qkv(h, pb, b, Lb, M, 0, C, C, ob, ntok, heads, wp, 0, S * ntok));
        CHK(gemm_qkv_pair(h, pa, pb, st));
    }
    CHK(dbg_planes_to_f32(h, oa.q, npad, S * heads, nt, 64, q_a, st));
    CHK(dbg_planes_to_f32(h, oa.k, npad, S * heads, nt, 64, k_a, st));
    CHK(dbg_planes_to_f32(h, ob.k, npad, S * heads, nt, 64, k_b, st));
    CHK(dbg_planes_to_f32(h, oa.vt, 0, 1, S * heads * 64, npad, vt_a, st));
    CHK(dbg_planes_to_f32(h, ob.vt, 0, 1, S * heads * 64, npad, vt_b, st));
    return 0;
}

// The plan (gemm_plan) of the handle's last launch_gemm or paired QKV launch (family 7): out[8] = {family, bm, bn, m_tail,
// tiles_m, tiles_n, ksplit, slab_ks}.
extern "C" int sta_debug_last_gemm_plan(sta_handle* h, int* out) {
    REQUIRE(h && out, "bad argument");
    plan_out(h->last_plan, out);
    return 0;
}

// q,k,v fp32 [S, heads, n*, 64] -> out fp32 [S, nq, heads*64]
extern "C" int sta_debug_attention(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads,
                                   int nq, int nk, int kv_shift, float* out, void* stream) {
    REQUIRE(h && q && k && v && out, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int nmax = nq > nk ? nq : nk, npad = rup(nmax, 64);
    int64_t hsz = (int64_t)S * heads * npad * 64;
    CHK(ensure_ws(h, (3 * hsz + (int64_t)S * nq * heads * 64) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, split); o.k = ws.planes(hsz, split); o.vt = ws.planes(hsz, split);
    Planes ao = ws.act((int64_t)S * nq, heads * 64, split);
    REQUIRE(!ws.overflow, "debug ws overflow");
    // V^T padding stays ZERO: that is the kernel's documented contract (a masked key has p = 0, and 0 * NaN would be NaN; the
    // QKV epilogue's buffers are memset the same way).  Everything else the kernel must not read or must overwrite is poisoned:
    // both planes of the K padding (masked keys must never leak), the Q rows in [nq, npad), the output planes.
    HIPCHK(hipMemsetAsync(o.vt.hi, 0, hsz * 2, st)); if (split) HIPCHK(hipMemsetAsync(o.vt.lo, 0, hsz * 2, st));
    CHK(dbg_poison_planes(o.k, hsz, st));
    CHK(dbg_poison_planes(o.q, hsz, st));
    CHK(dbg_poison_act(ao, (int64_t)S * nq, heads * 64, st));
    CHK(run_rows_to_planes(h, q, (int64_t)nq * 64, S * heads, nq, 64, o.q, st, npad));
    CHK(run_rows_to_planes(h, k, (int64_t)nk * 64, S * heads, nk, 64, o.k, st, npad));
    hipLaunchKernelGGL(pack_vt_kernel, dim3((unsigned)(((int64_t)S * heads * nk * 64 + 255) / 256)), dim3(256), 0, st,
                       v, S * heads, nk, npad, o.vt.hi, o.vt.lo, h->range);
    HIPCHK(hipGetLastError());
    CHK(run_attn(h, o, ao, heads * 64, S, heads, nq, nk, kv_shift, st));
    CHK(dbg_planes_to_f32(h, ao, 0, 1, S * nq, heads * 64, out, st));
    return 0;
}

// Decoder form of the attention kernel (AttnParams::pose): q,k,v fp32 [S, heads, n + 1, 64] with the pose token LAST ->
// out fp32 [S*n + S, heads*64] in the decoder's row order (patch rows sequence-major, then the S pose rows).
extern "C" int sta_debug_attention_pose(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads,
                                        int n, int kv_shift, float* out, void* stream) {
    REQUIRE(h && q && k && v && out && n > 0, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int nt = n + 1, npad = rup(nt, 64);
    int64_t hsz = (int64_t)S * heads * npad * 64;
    const int64_t M = (int64_t)S * nt;
    CHK(ensure_ws(h, (3 * hsz + M * heads * 64) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, split); o.k = ws.planes(hsz, split); o.vt = ws.planes(hsz, split);
    Planes ao = ws.act(M, heads * 64, split);
    REQUIRE(!ws.overflow, "debug ws overflow");
    // V^T padding stays ZERO (the kernel's contract: 0 * NaN, see sta_debug_attention); both planes of the K padding, the Q rows
    // in [n + 1, npad) and the output planes are poisoned
    HIPCHK(hipMemsetAsync(o.vt.hi, 0, hsz * 2, st)); if (split) HIPCHK(hipMemsetAsync(o.vt.lo, 0, hsz * 2, st));
    CHK(dbg_poison_planes(o.k, hsz, st));
    CHK(dbg_poison_planes(o.q, hsz, st));
    CHK(dbg_poison_act(ao, M, heads * 64, st));
    CHK(run_rows_to_planes(h, q, (int64_t)nt * 64, S * heads, nt, 64, o.q, st, npad));
    CHK(run_rows_to_planes(h, k, (int64_t)nt * 64, S * heads, nt, 64, o.k, st, npad));
    hipLaunchKernelGGL(pack_vt_kernel, dim3((unsigned)(((int64_t)S * heads * nt * 64 + 255) / 256)), dim3(256), 0, st,
                       v, S * heads, nt, npad, o.vt.hi, o.vt.lo, h->range);
    HIPCHK(hipGetLastError());
    CHK(run_attn(h, o, ao, heads * 64, S, heads, n, n, kv_shift, st, true));
    CHK(dbg_planes_to_f32(h, ao, 0, 1, (int)M, heads * 64, out, st));
    return 0;
}

// The two-group form (attn_mixed_kernel / run_attn_mixed).  Group a: S1 sequences, q_a fp32 [S1, heads, nq_a + 1, 64], k_a / v_a
// [S1, heads, nk_a + 1, 64], pose token LAST; group b the same with S2, nq_b, nk_b (S2 == 0: q_b, k_b, v_b may be NULL).  k / v of
// a sequence are the keys IT READS: the entry stores those of sequence s at buffer sequence (s + kv_shift) % (S1 + S2), where the
// kernel looks for them.  out fp32 [S1*nq_a + S1 + S2*nq_b + S2, heads*64]: per group the patch rows sequence-major, then its pose
// rows.  Poisoning as in sta_debug_attention_pose: V^T padding zero; K padding, dead Q rows and the output planes 0xFF.
extern "C" int sta_debug_attention_mixed(sta_handle* h, const float* q_a, const float* k_a, const float* v_a, const float* q_b,
                                         const float* k_b, const float* v_b, int S1, int S2, int heads, int nq_a, int nk_a,
                                         int nq_b, int nk_b, int kv_shift, float* out, void* stream) {
    REQUIRE(h && q_a && k_a && v_a && out && S1 > 0 && S2 >= 0 && heads > 0 && nq_a > 0 && nk_a > 0, "bad argument");
    REQUIRE(S2 == 0 || (q_b && k_b && v_b && nq_b > 0 && nk_b > 0), "bad argument (second group)");
    REQUIRE(kv_shift >= 0 && kv_shift < S1 + S2, "bad kv_shift");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int S = S1 + S2;
    const int nmax = std::max(std::max(nq_a, nk_a), S2 ? std::max(nq_b, nk_b) : 0), npad = rup(nmax + 1, 64);
    const int64_t seq = (int64_t)heads * npad * 64, hsz = S * seq;
    const int64_t M = (int64_t)S1 * (nq_a + 1) + (int64_t)S2 * (nq_b + 1);
    CHK(ensure_ws(h, (3 * hsz + M * heads * 64) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, split); o.k = ws.planes(hsz, split); o.vt = ws.planes(hsz, split);
    Planes ao = ws.act(M, heads * 64, split);
    REQUIRE(!ws.overflow, "debug ws overflow");
    HIPCHK(hipMemsetAsync(o.vt.hi, 0, hsz * 2, st)); if (split) HIPCHK(hipMemsetAsync(o.vt.lo, 0, hsz * 2, st));
    CHK(dbg_poison_planes(o.k, hsz, st));
    CHK(dbg_poison_planes(o.q, hsz, st));
    CHK(dbg_poison_act(ao, M, heads * 64, st));
    auto at = [&](const Planes& p, int64_t s) { Planes r = p; r.hi = p.hi + s * seq; if (p.lo) r.lo = p.lo + s * seq; return r; };
    for (int s = 0; s < S; ++s) {
        const bool inb = s >= S1;
        const int sl = inb ? s - S1 : s, nqt = (inb ? nq_b : nq_a) + 1, nkt = (inb ? nk_b : nk_a) + 1, skv = (s + kv_shift) % S;
        const float* q = (inb ? q_b : q_a) + (int64_t)sl * heads * nqt * 64;
        const float* k = (inb ? k_b : k_a) + (int64_t)sl * heads * nkt * 64;
        const float* v = (inb ? v_b : v_a) + (int64_t)sl * heads * nkt * 64;
        CHK(run_rows_to_planes(h, q, (int64_t)nqt * 64, heads, nqt, 64, at(o.q, s), st, npad));
        CHK(run_rows_to_planes(h, k, (int64_t)nkt * 64, heads, nkt, 64, at(o.k, skv), st, npad));
        const Planes vt = at(o.vt, skv);
        hipLaunchKernelGGL(pack_vt_kernel, dim3((unsigned)(((int64_t)heads * nkt * 64 + 255) / 256)), dim3(256), 0, st,
                           v, heads, nkt, npad, vt.hi, vt.lo, h->range);
        HIPCHK(hipGetLastError());
    }
    CHK(run_attn_mixed(h, o, ao, heads * 64, S1, S2, heads, nq_a, nk_a, nq_b, nk_b, kv_shift, st));
    CHK(dbg_planes_to_f32(h, ao, 0, 1, (int)M, heads * 64, out, st));
    return 0;
}

// The per-sequence form (attn_varlen_kernel / run_attn_varlen).  nq / nk: HOST arrays [S].  q fp32: sequence after sequence
// [heads, nq[s] + 1, 64]; k / v: [heads, nk[s] + 1, 64], pose token LAST.  k / v of a sequence are the keys IT READS: the entry stores
// those of sequence s at buffer sequence (s + kv_shift) % S, where the kernel looks for them.  out fp32 [sum(nq[s] + 1), heads*64]:
// per sequence its patch rows, then its pose row.  Poisoning as in sta_debug_attention_mixed: V^T padding zero; K padding, dead Q
// rows and the output planes 0xFF.  Directly behind the output planes lies a guard block of 64 rows, every byte 0x3C, which is
// returned as rows [sum(nq[s] + 1), + 64) of out: a store to an output row at or past the launch's last one lands in the next column
// block (a wrong row of the output) or, from the last column block, in the guard.
extern "C" int sta_debug_attn_varlen(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads,
                                     const int* nq, const int* nk, int kv_shift, float* out, void* stream) {
    REQUIRE(h && q && k && v && out && nq && nk && S > 0 && S <= ATT_MAX_SEQ && heads > 0, "bad argument");
    REQUIRE(kv_shift >= 0 && kv_shift < S, "bad kv_shift");
    int nmax = 0; int64_t M = 0;
    for (int s = 0; s < S; ++s) { REQUIRE(nq[s] > 0 && nk[s] > 0, "bad argument (sequence %d)", s); nmax = std::max(nmax, std::max(nq[s], nk[s])); M += nq[s] + 1; }
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int npad = rup(nmax + 1, 64);
    const int64_t seq = (int64_t)heads * npad * 64, hsz = S * seq;
    const int G = 64;                                                   // guard rows
    CHK(ensure_ws(h, (3 * hsz + (M + G) * heads * 64) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, split); o.k = ws.planes(hsz, split); o.vt = ws.planes(hsz, split);
    Planes ao = ws.act(M + G, heads * 64, split);                       // one allocation: the output planes of M rows, then the guard's of G rows
    ao.rp = M;
    Planes guard = slice_rows(ao, M * (heads * 64 / 32)); guard.rp = G;
    REQUIRE(!ws.overflow, "debug ws overflow");
    HIPCHK(hipMemsetAsync(o.vt.hi, 0, hsz * 2, st)); if (split) HIPCHK(hipMemsetAsync(o.vt.lo, 0, hsz * 2, st));
    CHK(dbg_poison_planes(o.k, hsz, st));
    CHK(dbg_poison_planes(o.q, hsz, st));
    CHK(dbg_poison_act(ao, M, heads * 64, st));
    HIPCHK(hipMemsetAsync(guard.hi, 0x3C, (size_t)G * heads * 64 * (split ? 4 : 2), st));
    auto at = [&](const Planes& p, int64_t s) { Planes r = p; r.hi = p.hi + s * seq; if (p.lo) r.lo = p.lo + s * seq; return r; };
    for (int s = 0; s < S; ++s) {
        const int nqt = nq[s] + 1, nkt = nk[s] + 1, skv = (s + kv_shift) % S;
        CHK(run_rows_to_planes(h, q, (int64_t)nqt * 64, heads, nqt, 64, at(o.q, s), st, npad));
        CHK(run_rows_to_planes(h, k, (int64_t)nkt * 64, heads, nkt, 64, at(o.k, skv), st, npad));
        const Planes vt = at(o.vt, skv);
        hipLaunchKernelGGL(pack_vt_kernel, dim3((unsigned)(((int64_t)heads * nkt * 64 + 255) / 256)), dim3(256), 0, st,
                           v, heads, nkt, npad, vt.hi, vt.lo, h->range);
        HIPCHK(hipGetLastError());
        q += (int64_t)heads * nqt * 64; k += (int64_t)heads * nkt * 64; v += (int64_t)heads * nkt * 64;
    }
    CHK(run_attn_varlen(h, o, ao, heads * 64, S, heads, nq, nk, kv_shift, st));
    CHK(dbg_planes_to_f32(h, ao, 0, 1, (int)M, heads * 64, out, st));
    CHK(dbg_planes_to_f32(h, guard, 0, 1, G, heads * 64, out + M * heads * 64, st));
    return 0;
}

// The rotation step of sta_decode_varlen alone.  n: HOST array [S] of token counts.  bufs: nbuf (<= 3) fp32 device buffers
// [S*heads + 1][npad][64], npad = roundup(max(n) + 1, 64): the decoder's Q / K layout plus ONE guard block behind the last head of
// the last sequence.  EVERY row, the guard's too, is split to planes, rotated in place and returned as hi + lo, so a row the kernel
// must not touch comes back as it went in.  pos_i32: device int32 [sum(n)*2] (y, x), packed, clamped to [-1, pos_max] into a copy first.
extern "C" int sta_debug_rope_varlen(sta_handle* h, float* const* bufs, int nbuf, int S, int heads, const int* n, const int* pos_i32,
                                     int pos_max, void* stream) {
    REQUIRE(h && bufs && pos_i32 && n && nbuf >= 1 && nbuf <= 3 && S > 0 && S <= SEQ_MAX && heads > 0, "bad argument");
    REQUIRE(pos_max >= 0 && pos_max < (1 << 20), "bad argument (pos_max %d)", pos_max);
    for (int b = 0; b < nbuf; ++b) REQUIRE(bufs[b], "null buffer %d", b);
    SeqTable t; memset(&t, 0, sizeof t);
    t.S = S;
    int nmax = 0;
    for (int s = 0; s < S; ++s) { REQUIRE(n[s] > 0 && n[s] < (1 << 20), "bad argument (sequence %d)", s); t.tok0[s + 1] = t.tok0[s] + n[s]; nmax = std::max(nmax, n[s]); }
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int npad = rup(nmax + 1, 64);
    const int64_t hsz = ((int64_t)S * heads + 1) * npad * 64;          // with the guard block
    const int64_t np = (int64_t)t.tok0[S] * 2;
    CHK(ensure_rope(h, pos_max + 1));
    CHK(ensure_ws(h, nbuf * hsz * 4 + np * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes pl[3]; const Planes* pp[3];
    for (int b = 0; b < nbuf; ++b) { pl[b] = ws.planes(hsz, split); pp[b] = &pl[b]; }
    int* pos = (int*)ws.take(np * 4);
    REQUIRE(!ws.overflow, "debug ws overflow");
    hipLaunchKernelGGL(rope_tokens_table_kernel<int>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st,
                       pos_i32, pos_i32, np, (int64_t)0, pos_max, pos, (float2*)nullptr, (int64_t)0);
    HIPCHK(hipGetLastError());
    for (int b = 0; b < nbuf; ++b) CHK(run_rows_to_planes(h, bufs[b], (int64_t)npad * 64, S * heads + 1, npad, 64, pl[b], st, npad));
    CHK(rope_varlen_launch(h, pp, nbuf, t, heads, npad, pos, st));
    for (int b = 0; b < nbuf; ++b) CHK(dbg_planes_to_f32(h, pl[b], npad, S * heads + 1, npad, 64, bufs[b], st));
    return 0;
}

// The encoder form of the per-sequence attention (run_attn_encv): n HOST array [S]; q / k / v fp32, sequence after sequence
// [heads, n[s], 64], NO pose token; every sequence reads its own keys.  npad = roundup(max(n), 64), so a sequence with n[s] == npad
// fills its blocks exactly.  out fp32 [sum(n) + 64, heads*64]: the packed rows, then the guard block behind the output planes (every
// byte 0x3C on entry).  Poisoning as in sta_debug_attn_varlen; the Q / K / V^T allocations carry one more (sequence, head) block than the
// launch uses - K and Q poisoned, V^T zero - so the row behind the last head of the last sequence is poison, not another tensor.
extern "C" int sta_debug_attn_encv(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads, const int* n,
                                   float* out, void* stream) {
    REQUIRE(h && q && k && v && out && n && S > 0 && S <= ATT_MAX_SEQ && heads > 0, "bad argument");
    int nmax = 0; int64_t M = 0;
    for (int s = 0; s < S; ++s) { REQUIRE(n[s] > 0, "bad argument (sequence %d)", s); nmax = std::max(nmax, n[s]); M += n[s]; }
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int npad = rup(nmax, 64);
    const int64_t seq = (int64_t)heads * npad * 64, hsz = S * seq + (int64_t)npad * 64;      // with the spare block
    const int G = 64;                                                   // guard rows
    CHK(ensure_ws(h, (3 * hsz + (M + G) * heads * 64) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, split); o.k = ws.planes(hsz, split); o.vt = ws.planes(hsz, split);
    Planes ao = ws.act(M + G, heads * 64, split);
    ao.rp = M;
    Planes guard = slice_rows(ao, M * (heads * 64 / 32)); guard.rp = G;
    REQUIRE(!ws.overflow, "debug ws overflow");
    HIPCHK(hipMemsetAsync(o.vt.hi, 0, hsz * 2, st)); if (split) HIPCHK(hipMemsetAsync(o.vt.lo, 0, hsz * 2, st));
    CHK(dbg_poison_planes(o.k, hsz, st));
    CHK(dbg_poison_planes(o.q, hsz, st));
    CHK(dbg_poison_act(ao, M, heads * 64, st));
    HIPCHK(hipMemsetAsync(guard.hi, 0x3C, (size_t)G * heads * 64 * (split ? 4 : 2), st));
    auto at = [&](const Planes& p, int64_t s) { Planes r = p; r.hi = p.hi + s * seq; if (p.lo) r.lo = p.lo + s * seq; return r; };
    for (int s = 0; s < S; ++s) {
        CHK(run_rows_to_planes(h, q, (int64_t)n[s] * 64, heads, n[s], 64, at(o.q, s), st, npad));
        CHK(run_rows_to_planes(h, k, (int64_t)n[s] * 64, heads, n[s], 64, at(o.k, s), st, npad));
        const Planes vt = at(o.vt, s);
        hipLaunchKernelGGL(pack_vt_kernel, dim3((unsigned)(((int64_t)heads * n[s] * 64 + 255) / 256)), dim3(256), 0, st,
                           v, heads, n[s], npad, vt.hi, vt.lo, h->range);
        HIPCHK(hipGetLastError());
        q += (int64_t)heads * n[s] * 64; k += (int64_t)heads * n[s] * 64; v += (int64_t)heads * n[s] * 64;
    }
    CHK(run_attn_encv(h, o, ao, heads * 64, S, heads, n, st));
    CHK(dbg_planes_to_f32(h, ao, 0, 1, (int)M, heads * 64, out, st));
    CHK(dbg_planes_to_f32(h, guard, 0, 1, G, heads * 64, out + M * heads * 64, st));
    return 0;
}

// The QKV finisher of sta_encode_varlen alone (qkv_finish_kernel, VARLEN form).  n: HOST array [S]; slab: device fp32 [sum(n), 3E], E =
// heads*64 (q | k | v columns); bias: device fp32 [3E] or NULL; pos_i32: device int32 [sum(n)*2] (y, x), packed, clamped to [0, pos_max]
// into a copy first.  q / k: fp32 device buffers [S*heads + 1][npad][64], vt: [S*heads + 1][64][npad], npad = roundup(max(n), 64) - the
// encoder's layout plus ONE guard block behind each.  EVERY element, the guards' too, is split to planes, the kernel runs on the planes,
// and everything is returned as hi + lo: what the kernel must not touch - rows [n[s], npad) of Q / K, columns [n[s], npad) of V^T (the
// entry does NOT zero them), the guards - comes back as it went in.
extern "C" int sta_debug_qkv_finish_varlen(sta_handle* h, const float* slab, const float* bias, const int* pos_i32, int S, int heads,
                                           const int* n, int pos_max, float* q, float* k, float* vt, void* stream) {
    REQUIRE(h && slab && pos_i32 && n && q && k && vt && S > 0 && S <= SEQ_MAX && heads > 0, "bad argument");
    REQUIRE(pos_max >= 0 && pos_max < (1 << 20), "bad argument (pos_max %d)", pos_max);
    SeqTable t; memset(&t, 0, sizeof t);
    t.S = S;
    int nmax = 0;
    for (int s = 0; s < S; ++s) { REQUIRE(n[s] > 0 && n[s] < (1 << 20), "bad argument (sequence %d)", s); t.tok0[s + 1] = t.tok0[s] + n[s]; nmax = std::max(nmax, n[s]); }
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int npad = rup(nmax, 64);
    const int64_t hsz = ((int64_t)S * heads + 1) * npad * 64;          // with the guard block
    const int64_t np = (int64_t)t.tok0[S] * 2;
    CHK(ensure_rope(h, pos_max + 1));
    CHK(ensure_ws(h, 3 * hsz * 4 + np * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    QKVOut o; o.npad = npad; o.q = ws.planes(hsz, split); o.k = ws.planes(hsz, split); o.vt = ws.planes(hsz, split);
    int* pos = (int*)ws.take(np * 4);
    REQUIRE(!ws.overflow, "debug ws overflow");
    hipLaunchKernelGGL(rope_tokens_table_kernel<int>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st,
                       pos_i32, pos_i32, np, (int64_t)0, pos_max, pos, (float2*)nullptr, (int64_t)0);
    HIPCHK(hipGetLastError());
    float* io[3] = {q, k, vt}; const Planes* pl[3] = {&o.q, &o.k, &o.vt};
    for (int b = 0; b < 3; ++b) CHK(run_rows_to_planes(h, io[b], hsz, 1, (int)(hsz / 64), 64, *pl[b], st));      // flat: both layouts are [.][64] rows
    CHK(qkv_finish_varlen(h, slab, bias, heads * 64, heads, t, o, pos, st));
    for (int b = 0; b < 3; ++b) CHK(dbg_planes_to_f32(h, *pl[b], 0, 1, (int)(hsz / 64), 64, io[b], st));
    return 0;
}

// The gather of sta_encode_varlen alone.  imgs / H / W / n: HOST arrays [B] as in sta_encode_varlen (u8hwc != 0: uint8 HWC frames);
// pos_i32: device int32 [sum(n)*2] (y, x), packed, ALREADY inside each entry's grid.  out: fp32 [sum(n), 768], the patch rows the
// patch-embed GEMM reads, hi + lo; the planes are poisoned first.  which = 0: the VARLEN form, one launch over all entries; which = 1:
// the equal-count form of the same kernel (sta_encode_tokens'), one launch per entry on its rows.
extern "C" int sta_debug_patch_gather_varlen(sta_handle* h, const void* const* imgs, int u8hwc, const int* H, const int* W, const int* pos_i32,
                                             const int* n, int B, int which, float* out, void* stream) {
    REQUIRE(h && imgs && H && W && pos_i32 && n && out && B >= 1 && B <= SEQ_MAX && (which == 0 || which == 1), "bad argument");
    EncEntries e; memset(&e, 0, sizeof e);
    e.t.S = B;
    for (int b = 0; b < B; ++b) {
        REQUIRE(imgs[b] && n[b] > 0 && n[b] < (1 << 20) && H[b] > 0 && W[b] > 0 && H[b] % 16 == 0 && W[b] % 16 == 0, "bad argument (entry %d)", b);
        REQUIRE(!u8hwc || ((uintptr_t)imgs[b] & 15) == 0, "u8 HWC image must be 16-byte aligned (entry %d)", b);
        e.img[b] = imgs[b]; e.H[b] = H[b]; e.W[b] = W[b]; e.t.tok0[b + 1] = e.t.tok0[b] + n[b];
    }
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int64_t M = e.t.tok0[B];
    CHK(ensure_ws(h, M * 768 * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes patches = ws.act(M, 768, split);
    REQUIRE(!ws.overflow, "debug ws overflow");
    CHK(dbg_poison_act(patches, M, 768, st));
    const int per = u8hwc ? 16 : 48;
    if (which == 0) {
        const int blocks = (int)((M * per + 255) / 256);
        if (u8hwc) {
            if (split) hipLaunchKernelGGL((patch_gather_tokens_u8hwc_kernel<true, EncEntries>), dim3(blocks), dim3(256), 0, st, (const uint8_t*)nullptr, pos_i32, 0, 0, 0, 0, patches.hi, patches.lo, M, h->range, e);
            else hipLaunchKernelGGL((patch_gather_tokens_u8hwc_kernel<false, EncEntries>), dim3(blocks), dim3(256), 0, st, (const uint8_t*)nullptr, pos_i32, 0, 0, 0, 0, patches.hi, patches.lo, M, h->range, e);
        } else if (split) hipLaunchKernelGGL((patch_gather_tokens_kernel<true, EncEntries>), dim3(blocks), dim3(256), 0, st, (const float*)nullptr, pos_i32, 0, 0, 0, 0, patches.hi, patches.lo, M, h->range, e);
        else hipLaunchKernelGGL((patch_gather_tokens_kernel<false, EncEntries>), dim3(blocks), dim3(256), 0, st, (const float*)nullptr, pos_i32, 0, 0, 0, 0, patches.hi, patches.lo, M, h->range, e);
        HIPCHK(hipGetLastError());
    } else {
        for (int b = 0; b < B; ++b) {
            const int blocks = (int)(((int64_t)n[b] * per + 255) / 256);
            f16* hi = patches.hi + (int64_t)e.t.tok0[b] * (split ? 64 : 32);          // row tok0[b] of every column block (blk_off)
            const int* pb = pos_i32 + (int64_t)e.t.tok0[b] * 2;
            if (u8hwc) {
                if (split) hipLaunchKernelGGL(patch_gather_tokens_u8hwc_kernel<true>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)imgs[b], pb, 1, n[b], H[b], W[b], hi, patches.lo, M, h->range);
                else hipLaunchKernelGGL(patch_gather_tokens_u8hwc_kernel<false>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)imgs[b], pb, 1, n[b], H[b], W[b], hi, patches.lo, M, h->range);
            } else if (split) hipLaunchKernelGGL(patch_gather_tokens_kernel<true>, dim3(blocks), dim3(256), 0, st, (const float*)imgs[b], pb, 1, n[b], H[b], W[b], hi, patches.lo, M, h->range);
            else hipLaunchKernelGGL(patch_gather_tokens_kernel<false>, dim3(blocks), dim3(256), 0, st, (const float*)imgs[b], pb, 1, n[b], H[b], W[b], hi, patches.lo, M, h->range);
            HIPCHK(hipGetLastError());
        }
    }
    CHK(dbg_planes_to_f32(h, patches, 0, 1, (int)M, 768, out, st));
    return 0;
}

// The rotation step of sta_decode_tokens alone.  bufs: nbuf (<= 3) fp32 device buffers [S1 + S2][heads][npad][64], npad =
// roundup(max(ntok_a, ntok_b) + 1, 64): EVERY row is split to planes (the rows past a sequence's pose token too), rotated in place and
// returned as hi + lo, so a row the kernel must not touch comes back as it went in.  pos_i32: device int32 [S1*ntok_a*2 | S2*ntok_b*2]
// (y, x), clamped to [-1, pos_max] into a copy first.  which = 0: rope_tokens_kernel, one launch; 1: rope_planes_kernel per buffer and side.
extern "C" int sta_debug_rope_tokens(sta_handle* h, float* const* bufs, int nbuf, int S1, int S2, int heads, int ntok_a, int ntok_b,
                                     const int* pos_i32, int pos_max, int which, void* stream) {
    REQUIRE(h && bufs && pos_i32 && nbuf >= 1 && nbuf <= 3 && S1 > 0 && S2 > 0 && heads > 0 && ntok_a > 0 && ntok_b > 0, "bad argument");
    REQUIRE(pos_max >= 0 && pos_max < (1 << 20) && (which == 0 || which == 1), "bad argument (pos_max %d, which %d)", pos_max, which);
    for (int b = 0; b < nbuf; ++b) REQUIRE(bufs[b], "null buffer %d", b);
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int S = S1 + S2, npad = rup(std::max(ntok_a, ntok_b) + 1, 64);
    const int64_t hsz = (int64_t)S * heads * npad * 64;
    const int64_t n1 = (int64_t)S1 * ntok_a * 2, n2 = (int64_t)S2 * ntok_b * 2;
    CHK(ensure_rope(h, pos_max + 1));
    CHK(ensure_ws(h, nbuf * hsz * 4 + (n1 + n2) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes pl[3]; const Planes* pp[3];
    for (int b = 0; b < nbuf; ++b) { pl[b] = ws.planes(hsz, split); pp[b] = &pl[b]; }
    int* pos = (int*)ws.take((n1 + n2) * 4);
    REQUIRE(!ws.overflow, "debug ws overflow");
    hipLaunchKernelGGL(rope_tokens_table_kernel<int>, dim3((unsigned)((n1 + n2 + 255) / 256)), dim3(256), 0, st,
                       pos_i32, pos_i32 + n1, n1, n2, pos_max, pos, (float2*)nullptr, (int64_t)0);
    HIPCHK(hipGetLastError());
    for (int b = 0; b < nbuf; ++b) CHK(run_rows_to_planes(h, bufs[b], (int64_t)npad * 64, S * heads, npad, 64, pl[b], st, npad));
    CHK(rope_tokens_launch(h, pp, nbuf, S1, S2, heads, npad, ntok_a, ntok_b, pos, which == 1, st));
    for (int b = 0; b < nbuf; ++b) CHK(dbg_planes_to_f32(h, pl[b], npad, S * heads, npad, 64, bufs[b], st));
    return 0;
}

// The rotation step of sta_encode_tokens alone.  bufs: nbuf (<= 2) fp32 device buffers [S*heads + 1][npad][64], npad = roundup(ntok, 64)
// with NO pose row: the encoder's Q / K layout plus ONE guard block of npad x 64 behind the last head of the last sequence.  Every row,
// the guard's too, is split to planes, rotated in place and returned as hi + lo, so a row the kernel must not touch comes back as it
// went in.  pos_i32: device int32 [S*ntok*2] (y, x) in [0, pos_max].  pose = 0: rope_tokens_kernel<., false>, the launch of
// encode_tokens_impl; pose = 1: the decoder's pose-row form on the same buffers (ntok + 1 rows per (sequence, head): with ntok a
// multiple of 64 it writes row 0 of the next head and the guard - what the flag exists to prevent).
extern "C" int sta_debug_rope_enc_tokens(sta_handle* h, float* const* bufs, int nbuf, int S, int heads, int ntok, const int* pos_i32,
                                         int pos_max, int pose, void* stream) {
    REQUIRE(h && bufs && pos_i32 && nbuf >= 1 && nbuf <= 2 && S > 0 && heads > 0 && ntok > 0, "bad argument");
    REQUIRE(pos_max >= 0 && pos_max < (1 << 20) && (pose == 0 || pose == 1), "bad argument (pos_max %d, pose %d)", pos_max, pose);
    for (int b = 0; b < nbuf; ++b) REQUIRE(bufs[b], "null buffer %d", b);
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int npad = rup(ntok, 64);
    const int64_t hsz = ((int64_t)S * heads + 1) * npad * 64;          // with the guard block
    const int64_t n = (int64_t)S * ntok * 2;
    CHK(ensure_rope(h, pos_max + 1));
    CHK(ensure_ws(h, nbuf * hsz * 4 + n * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes pl[2]; const Planes* pp[2];
    for (int b = 0; b < nbuf; ++b) { pl[b] = ws.planes(hsz, split); pp[b] = &pl[b]; }
    int* pos = (int*)ws.take(n * 4);
    REQUIRE(!ws.overflow, "debug ws overflow");
    hipLaunchKernelGGL(rope_tokens_table_kernel<int>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       pos_i32, pos_i32, n, (int64_t)0, pos_max, pos, (float2*)nullptr, (int64_t)0);
    HIPCHK(hipGetLastError());
    for (int b = 0; b < nbuf; ++b) CHK(run_rows_to_planes(h, bufs[b], (int64_t)npad * 64, S * heads + 1, npad, 64, pl[b], st, npad));
    if (pose) {       // the decoder's form needs ntok + 1 <= npad of ITS layout; here the extra row is the next block's row 0 (inside the guarded allocation)
        RopeTokParams p;
        for (int b = 0; b < 3; ++b) { p.hi[b] = pl[b < nbuf ? b : 0].hi; p.lo[b] = pl[b < nbuf ? b : 0].lo; }
        p.S1 = S; p.S2 = 0; p.heads = heads; p.npad = npad; p.ntok_a = ntok; p.ntok_b = 0;
        p.pos = pos; p.tab = h->rope_tab; p.rng = h->range;
        const dim3 grid((unsigned)(((int64_t)S * (ntok + 1) * heads * 4 + 255) / 256), nbuf);
        if (split) hipLaunchKernelGGL(rope_tokens_kernel<true>, grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL(rope_tokens_kernel<false>, grid, dim3(256), 0, st, p);
        HIPCHK(hipGetLastError());
    } else {
        CHK(rope_tokens_launch(h, pp, nbuf, S, 0, heads, npad, ntok, 0, pos, false, st, false));
    }
    for (int b = 0; b < nbuf; ++b) CHK(dbg_planes_to_f32(h, pl[b], npad, S * heads + 1, npad, 64, bufs[b], st));
    return 0;
}

// A/B switches of the product's round-4 choices (tools/ab_option.py, ab_slam.py, ab_replay.py; 0 everywhere = product behaviour):
//   1 = 1: small-grid K slices by the old rule ceil(256 / tiles)          2 = 1: small-grid GEMMs always on 4 waves (> 1: the lone-grid limit)
//   4 = 1: debug GEMM entry points in the f16mx arithmetic                5 = 1: attention without the 4-stage prefetch schedule
//   6 = 1: no side lanes, 2: side lanes even under a multi-stream caller  7 = 1: bilinear one output row per workgroup
//   3 = 1: sta_decode_tokens rotates by per-buffer rope_planes_kernel launches (eight per layer) instead of rope_tokens_kernel (two)
//   8 = 1: sta_encode_varlen runs its QKV GEMM once PER SEQUENCE (fused epilogue, identity table) plus one no-pose rope_varlen_kernel launch
//          per layer, as decode_varlen_impl does, instead of one dense GEMM and the varlen finisher (tools/encode_varlen_bench.py)
extern "C" int sta_debug_set_option(sta_handle* h, int idx, int value) {
    REQUIRE(h && idx >= 0 && idx < 9, "bad argument");
    h->opt[idx] = value;
    return 0;
}

// Row-tail hint of the dense GEMMs (GemmParams::m_tail; decode_impl sets it to the number of pose-token rows): sticky
// until reset to 0.  Lets the kernel tests run sta_debug_gemm with skinny tail blocks.
extern "C" int sta_debug_set_tail_hint(sta_handle* h, int rows) {
    REQUIRE(h && rows >= 0 && rows <= 32, "bad argument");
    h->tail_hint = rows;
    return 0;
}

// x NHWC fp32 [n,H,W,Cin], w [Co,Cin,3,3] fp32 (reference layout), out NHWC fp32 [n,Ho,Wo,Co]; resid / resid2 (may be NULL; resid2
// only with resid): the residual planes of the epilogue, as the refinenet fusion passes them (conv3(..., &r[k], &path))
static int dbg_conv3(sta_handle* h, const float* x, const float* w, const float* bias, int n, int H, int W, int Cin, int Co,
                     int stride, int relu_in, int act, const float* resid, const float* resid2, float* out, void* stream) {
    REQUIRE(h && x && w && out, "bad argument");
    REQUIRE(n > 0 && H > 0 && W > 0 && Cin > 0 && Co > 0 && (stride == 1 || stride == 2) && (resid || !resid2), "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    int64_t ein = (int64_t)n * H * W * Cin, eout = (int64_t)n * Ho * Wo * Co;
    CHK(ensure_ws(h, (ein + (int64_t)2 * Co * Cin * 9 + 3 * eout) * 4 + (1 << 16), st));      // (two packed copies of the weight in the f16mx arithmetic)
    Bump ws = cur_bump(h);
    Planes xi = ws.act((int64_t)n * H * W, Cin, split), o = ws.act((int64_t)n * Ho * Wo, Co, split), r = ws.act((int64_t)n * Ho * Wo, Co, split);
    Planes r2 = ws.act((int64_t)n * Ho * Wo, Co, split);
    const bool mx = dbg_mx(h) && Co % 64 == 0;
    xi.mx = o.mx = r.mx = r2.mx = mx;
    Lin L; CHK(dbg_make_lin(h, ws, w, bias, Co, Cin * 9, 1, Co, Cin, 3, 3, L, st, mx));
    REQUIRE(!ws.overflow, "debug ws overflow");
    CHK(run_rows_to_planes(h, x, ein, 1, n * H * W, Cin, xi, st, 0, mx));
    if (resid) CHK(run_rows_to_planes(h, resid, eout, 1, n * Ho * Wo, Co, r, st, 0, mx));
    if (resid2) CHK(run_rows_to_planes(h, resid2, eout, 1, n * Ho * Wo, Co, r2, st, 0, mx));
    CHK(dbg_poison_act(o, (int64_t)n * Ho * Wo, Co, st));
    CHK(conv3(h, xi, n, H, W, Cin, L, stride, relu_in != 0, act, o, resid ? &r : nullptr, resid2 ? &r2 : nullptr, st));
    CHK(dbg_planes_to_f32(h, o, 0, 1, n * Ho * Wo, Co, out, st));
    return 0;
}
extern "C" int sta_debug_conv3x3(sta_handle* h, const float* x, const float* w, const float* bias, int n, int H, int W, int Cin, int Co,
                                 int stride, int relu_in, int act, const float* resid, float* out, void* stream) {
    return dbg_conv3(h, x, w, bias, n, H, W, Cin, Co, stride, relu_in, act, resid, nullptr, out, stream);
}
extern "C" int sta_debug_conv3x3_r2(sta_handle* h, const float* x, const float* w, const float* bias, int n, int H, int W, int Cin, int Co,
                                    int stride, int relu_in, int act, const float* resid, const float* resid2, float* out, void* stream) {
    return dbg_conv3(h, x, w, bias, n, H, W, Cin, Co, stride, relu_in, act, resid, resid2, out, stream);
}

// The fused DPT tail (conv3_head: head.2 3x3 128 -> 128 + ReLU + head.4 1x1 128 -> 4 + point-map / confidence activations) on
// x NHWC fp32 [n,H,W,128]; w2 [128,128,3,3], b2 [128], w4 [4,128], b4 [4] fp32.  The first nA images go to (ptsA [nA,H,W,3],
// confA [nA,H,W]), the rest to (ptsB, confB).  head.4's rows are scaled as sta_finalize_weights scales them (head4_row_scales).
// Fails when conv3_head_ok is false (small grids, forced implicit-GEMM families): the unfused path is never taken here.
extern "C" int sta_debug_conv3_head(sta_handle* h, const float* x, const float* w2, const float* b2, const float* w4, const float* b4,
                                    int n, int H, int W, int nA, float* ptsA, float* confA, float* ptsB, float* confB, void* stream) {
    REQUIRE(h && x && w2 && b2 && w4 && b4 && n > 0 && H > 0 && W > 0 && nA >= 0 && nA <= n, "bad argument");
    REQUIRE((nA == 0 || (ptsA && confA)) && (nA == n || (ptsB && confB)), "bad argument (outputs)");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    const int64_t npix = (int64_t)n * H * W, ein = npix * 128;
    REQUIRE(npix < ((int64_t)1 << 31) / 128, "too many pixels");
    CHK(ensure_ws(h, (ein + (int64_t)2 * 128 * 128 * 9) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act(npix, 128, split);
    const bool mx = dbg_mx(h);
    xi.mx = mx;
    Lin L; CHK(dbg_make_lin(h, ws, w2, b2, 128, 128 * 9, 1, 128, 128, 3, 3, L, st, mx));
    REQUIRE(!ws.overflow, "debug ws overflow");
    REQUIRE(conv3_head_ok(h, L, npix), "the fused tail does not run at %lld pixels under tile family %d (conv3_head_ok)", (long long)npix, h->gemm_variant);
    F32Lin L4; L4.w = const_cast<float*>(w4); L4.b = const_cast<float*>(b4);
    std::vector<float> w4h(4 * 128);
    HIPCHK(hipMemcpyAsync(w4h.data(), w4, w4h.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // the row scales of THIS head.4 for the duration of the call: the handle's own (its loaded weights') come back on every path out
    struct ScaleGuard {
        float* dst; float keep[4];
        explicit ScaleGuard(float* d) : dst(d) { for (int o = 0; o < 4; ++o) keep[o] = d[o]; }
        ~ScaleGuard() { for (int o = 0; o < 4; ++o) dst[o] = keep[o]; }
    } restore_scales(h->head4_scale);
    head4_row_scales(w4h.data(), h->head4_scale);
    CHK(run_rows_to_planes(h, x, ein, 1, (int)npix, 128, xi, st, 0, mx));
    const int64_t pa = (int64_t)nA * H * W, pb = npix - pa;
    if (pa) { CHK(dbg_poison(ptsA, pa * 12, st)); CHK(dbg_poison(confA, pa * 4, st)); }
    if (pb) { CHK(dbg_poison(ptsB, pb * 12, st)); CHK(dbg_poison(confB, pb * 4, st)); }
    return conv3_head(h, xi, n, H, W, 128, L, L4, ptsA, confA, nA, ptsB, confB, st);
}

// x NHWC fp32 [n,H,W,C], w [C,C,k,k] (ConvTranspose2d layout), out NHWC fp32 [n,kH,kW,C]
extern "C" int sta_debug_convt(sta_handle* h, const float* x, const float* w, const float* bias, int n, int H, int W, int C, int k,
                               float* out, void* stream) {
    REQUIRE(h && x && w && bias && out, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    int64_t ein = (int64_t)n * H * W * C, eout = ein * k * k;
    CHK(ensure_ws(h, (ein + (int64_t)2 * C * C * k * k + eout) * 4 + (int64_t)C * k * k * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act((int64_t)n * H * W, C, split), o = ws.act((int64_t)n * H * W * k * k, C, split);
    float* eb = (float*)ws.take((int64_t)C * k * k * 4);
    const bool mx = dbg_mx(h) && (k * k * C) % 64 == 0;
    xi.mx = o.mx = mx;
    Lin L; CHK(dbg_make_lin(h, ws, w, eb, k * k * C, C, 2, C, C, k, k, L, st, mx));
    REQUIRE(!ws.overflow, "debug ws overflow");
    hipLaunchKernelGGL(expand_bias_kernel, dim3((C * k * k + 255) / 256), dim3(256), 0, st, bias, eb, C, k * k);
    CHK(run_rows_to_planes(h, x, ein, 1, n * H * W, C, xi, st, 0, mx));
    CHK(dbg_poison_act(o, (int64_t)n * H * W * k * k, C, st));
    CHK(gemm_convt(h, xi, L, n, H, W, k, C, o, st));
    CHK(dbg_planes_to_f32(h, o, 0, 1, n * H * k * W * k, C, out, st));
    return 0;
}

// x NHWC fp32 [n,H,W,C] -> out NHWC fp32 [n,Hc,Wc,C] (bilinear x2, align_corners, cropped)
extern "C" int sta_debug_up2(sta_handle* h, const float* x, int n, int H, int W, int C, int Hc, int Wc, float* out, void* stream) {
    REQUIRE(h && x && out && C % 8 == 0, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    int64_t ein = (int64_t)n * H * W * C, eout = (int64_t)n * Hc * Wc * C;
    CHK(ensure_ws(h, (ein + eout) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act((int64_t)n * H * W, C, split), o = ws.act((int64_t)n * Hc * Wc, C, split);
    xi.mx = o.mx = dbg_mx(h);
    CHK(run_rows_to_planes(h, x, ein, 1, n * H * W, C, xi, st, 0, xi.mx));
    CHK(dbg_poison_act(o, (int64_t)n * Hc * Wc, C, st));
    CHK(run_up2(h, xi, n, H, W, C, Hc, Wc, o, st));
    CHK(dbg_planes_to_f32(h, o, 0, 1, n * Hc * Wc, C, out, st));
    return 0;
}

// LayerNorm rows [M,C] with (g,b) -> fp32 (direct) and through the fp16 planes
extern "C" int sta_debug_layernorm(sta_handle* h, const float* x, const float* g, const float* b, int M, int C, float eps,
                                   float* out32, float* out_planes, void* stream) {
    REQUIRE(h && x && g && b && out32 && out_planes && C % 4 == 0 && C <= 1024, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    CHK(ensure_ws(h, (int64_t)M * C * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes o = ws.act(M, C, split);
    LNp n; n.g = const_cast<float*>(g); n.b = const_cast<float*>(b);
    CHK(dbg_poison_act(o, M, C, st));
    float keep = h->cfg.ln_eps; h->cfg.ln_eps = eps;
    int r = run_ln(h, x, M, C, n, o, nullptr, nullptr, out32, st);
    h->cfg.ln_eps = keep;
    CHK(r);
    CHK(dbg_planes_to_f32(h, o, 0, 1, M, C, out_planes, st));
    return 0;
}

// The residual stream step of every transformer layer, exactly as the forward pass issues it (gemm_resid_ln): x[M,N] += A[M,K] W[N,K]^T
// + bias IN PLACE, then the LayerNorm(s) of the new x into fp16 planes.  g1 == NULL: only the add (no planes are written); g2 == NULL:
// one affine set.  Below the small-grid predicate the K slices go through the handle's own slab buffer and resid_ln_kernel sums them;
// which path ran is read from sta_debug_last_gemm_plan (slab_ks > 1), not from here.  out1 / out2 (may be NULL): the values the two
// plane sets carry, fp32 [M,N]; both plane sets are filled with 0xFF first, so a set the call must not write reads back as NaN.
extern "C" int sta_debug_gemm_resid_ln(sta_handle* h, const float* A, const float* W, const float* bias, float* x, int M, int N, int K,
                                       const float* g1, const float* b1, const float* g2, const float* b2, float eps,
                                       float* out1, float* out2, void* stream) {
    REQUIRE(h && A && W && bias && x && M > 0 && N > 0 && K > 0, "bad argument");
    REQUIRE(N % 4 == 0 && N <= 1024 && K % GEMM_BK == 0, "bad shape (N %% 4 == 0, N <= 1024, K %% %d == 0)", GEMM_BK);
    REQUIRE((g1 != nullptr) == (b1 != nullptr) && (g2 != nullptr) == (b2 != nullptr) && (g1 || !g2), "bad affine sets (g2 only with g1)");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    CHK(ensure_ws(h, ((int64_t)M * K + (int64_t)N * K + (int64_t)2 * M * rup(N, 32)) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes a = ws.act(M, K, split), o1 = ws.act(M, N, split), o2 = ws.act(M, N, split);
    Lin L; CHK(dbg_make_lin(h, ws, W, bias, N, K, 0, N, K, 1, 1, L, st));
    REQUIRE(!ws.overflow, "debug ws overflow");
    CHK(run_rows_to_planes(h, A, (int64_t)M * K, 1, M, K, a, st));
    CHK(dbg_poison_act(o1, M, N, st));
    CHK(dbg_poison_act(o2, M, N, st));
    LNp la, lb; la.g = const_cast<float*>(g1); la.b = const_cast<float*>(b1); lb.g = const_cast<float*>(g2); lb.b = const_cast<float*>(b2);
    float keep = h->cfg.ln_eps; h->cfg.ln_eps = eps;
    int r = gemm_resid_ln(h, a, L, M, x, N, g1 ? &la : nullptr, g1 ? &o1 : nullptr, g2 ? &lb : nullptr, g2 ? &o2 : nullptr, st);
    h->cfg.ln_eps = keep;
    CHK(r);
    if (out1) CHK(dbg_planes_to_f32(h, o1, 0, 1, M, N, out1, st));
    if (out2) CHK(dbg_planes_to_f32(h, o2, 0, 1, M, N, out2, st));
    return 0;
}

// final 1x1 conv (128->4) + postprocess on an NHWC fp32 feature map [npix,128]
extern "C" int sta_debug_head_final(sta_handle* h, const float* x, const float* w, const float* bias, int64_t npix,
                                    float* pts, float* conf, void* stream) {
    REQUIRE(h && x && w && bias && pts && conf, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const bool split = h->prec != STA_PREC_F16;
    CHK(ensure_ws(h, npix * 128 * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act(npix, 128, split);
    CHK(run_rows_to_planes(h, x, npix * 128, 1, (int)npix, 128, xi, st));
    int blocks = (int)((npix * 16 + 255) / 256); if (blocks > 16384) blocks = 16384;
    if (split) hipLaunchKernelGGL(head_final_kernel<true>, dim3(blocks), dim3(256), 0, st, xi.hi, xi.lo, (int64_t)0, npix, npix, w, bias, pts, conf);
    else hipLaunchKernelGGL(head_final_kernel<false>, dim3(blocks), dim3(256), 0, st, xi.hi, xi.lo, (int64_t)0, npix, npix, w, bias, pts, conf);
    HIPCHK(hipGetLastError());
    return 0;
}

// nearest-rotation (SVD orthogonalisation) of B 3x3 matrices, fp32 in/out (device pointers)
__global__ void dbg_rot_kernel(const float* m, float* r, int B) {
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double M[3][3], R[3][3];
    for (int i = 0; i < 3; ++i) {
        float a = m[b * 9 + i * 3], c = m[b * 9 + i * 3 + 1], d = m[b * 9 + i * 3 + 2];
        float nrm = fmaxf(sqrtf(a * a + c * c + d * d), 1e-12f);
        M[i][0] = a / nrm; M[i][1] = c / nrm; M[i][2] = d / nrm;
    }
    nearest_rotation(M, R);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r[b * 9 + i * 3 + j] = (float)R[i][j];
}
extern "C" int sta_debug_svd_orthogonalize(sta_handle* h, const float* m, float* r, int B, void* stream) {
    REQUIRE(h && m && r, "bad argument");
    DEV_SCOPE(h->device);
    hipLaunchKernelGGL(dbg_rot_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, m, r, B);
    HIPCHK(hipGetLastError());
    return 0;
}

// The gather of sta_regress_views_tokens alone (gather_tokens_varlen_kernel).  srcs / hp / wp / win / cnt: HOST arrays over S <= 32
// sequences (S even: the first half is side i, the second side j, as in the entry); idx_i / idx_j: the packed device int64 index
// arrays of the two halves.  feat_out fp32 [sum(n), E], pos_out int32 [sum(n), 2]: written by the one launch, nothing else is touched.
extern "C" int sta_debug_gather_tokens(sta_handle* h, const float* const* srcs, const int* hp, const int* wp, const int* win, const int* cnt,
                                       const int64_t* idx_i, const int64_t* idx_j, int S, int E, float* feat_out, int* pos_out, void* stream) {
    REQUIRE(h && srcs && hp && wp && win && feat_out && pos_out, "bad argument");
    REQUIRE(S >= 2 && S <= SEQ_MAX && S % 2 == 0 && E >= 4 && E % 4 == 0, "bad argument (S %d, E %d)", S, E);
    REQUIRE(((uintptr_t)feat_out & 15) == 0 && ((uintptr_t)pos_out & 7) == 0, "misaligned output");
    DEV_SCOPE(h->device);
    TokenSel g; int mh[SEQ_MAX], mw[SEQ_MAX];
    const int64_t* const idx_side[2] = {idx_i, idx_j};
    CHK(build_token_sel(srcs, hp, wp, win, cnt, idx_side, S, &g, mh, mw));
    return launch_gather_tokens(g, E, feat_out, pos_out, (hipStream_t)stream);
}

// The pose head with its samples named by a row table (pose_layer_rows_kernel in front of the unchanged layers): sample b reads row
// rows[b] (HOST int64 [k], k <= 16) of tok, rows of tok_stride floats.
extern "C" int sta_debug_pose_rows(sta_handle* h, const float* tok, int64_t tok_stride, const int64_t* rows, int k, float* pose, float* conf, void* stream) {
    REQUIRE(h && h->finalized, "handle not ready");
    REQUIRE(tok && rows && pose && conf && k >= 1 && k <= 16, "bad argument");
    REQUIRE(tok_stride % 4 == 0 && ((uintptr_t)tok & 15) == 0, "tok must be 16-byte aligned with a stride that is a multiple of 4 floats");
    DEV_SCOPE(h->device);
    PoseRows pr;
    for (int e = 0; e < 16; ++e) { pr.row[e] = e < k ? rows[e] : 0; REQUIRE(pr.row[e] >= 0, "negative row"); }
    hipStream_t st = (hipStream_t)stream;
    return plan_and_run(h, st, [&](Bump& ws) { return pose_impl(h, ws, tok, k, tok_stride, pose, conf, st, nullptr, nullptr, 0, &pr); });
}

// ------------------------------------------------------------------------------------------ varlen DPT head: kernel-level hooks
// The varlen siblings of sta_debug_conv3x3_r2 / _conv3_head / _convt / _up2: B <= 32 entries of different size in ONE launch, inputs
// and outputs packed entry-major (entry b: H[b] x W[b] pixels, NHWC fp32).  H / W (/ Hc / Wc): HOST arrays.  guard (device, 4096 B, may
// be NULL): receives the 4096 bytes that lie right behind the output planes in the workspace, filled with 0xA5 before the launch - a
// store past the last packed row of the last channel block lands there.
#define DBG_GUARD_BYTES 4096
static int dbg_vl_check(sta_handle* h, int B, const int* H, const int* W) {
    REQUIRE(h && H && W && B >= 1 && B <= SEQ_MAX, "bad argument");
    REQUIRE(h->prec != STA_PREC_F16, "the varlen forms have no precision-f16 kernels");
    for (int b = 0; b < B; ++b) REQUIRE(H[b] >= 1 && W[b] >= 1, "bad argument (entry %d is %d x %d)", b, H[b], W[b]);
    return 0;
}
// (o: the output planes, allocated LAST before this call: the guard starts at their last byte + 1, inside the allocator's slack and
//  alignment gap, so a store one row past the last packed row of the last channel block lands in it)
static int dbg_guard_arm(Bump& ws, const Planes& o, int64_t rows, int64_t cols, char** g, hipStream_t st) {
    char* end = (char*)o.hi + rows * ((cols + 31) & ~int64_t(31)) * (o.lo ? 4 : 2);
    char* tail = (char*)ws.take(DBG_GUARD_BYTES + 1024);
    REQUIRE(!ws.overflow, "debug ws overflow");
    REQUIRE(end <= tail && tail - end <= 1024, "internal: the guard does not follow the output planes");
    *g = end;
    HIPCHK(hipMemsetAsync(end, 0xA5, DBG_GUARD_BYTES, st));
    return 0;
}
static int dbg_guard_read(const char* g, void* out, hipStream_t st) {
    if (out) HIPCHK(hipMemcpyAsync(out, g, DBG_GUARD_BYTES, hipMemcpyDeviceToDevice, st));
    return 0;
}
extern "C" int sta_debug_conv3x3_varlen(sta_handle* h, const float* x, const float* w, const float* bias, int B, const int* H, const int* W,
                                        int Cin, int Co, int stride, int relu_in, int act, const float* resid, const float* resid2,
                                        float* out, void* guard, void* stream) {
    CHK(dbg_vl_check(h, B, H, W));
    REQUIRE(x && w && out && Cin > 0 && Co > 0 && (stride == 1 || stride == 2) && (resid || !resid2), "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    int ho[SEQ_MAX], wo[SEQ_MAX];
    for (int b = 0; b < B; ++b) { ho[b] = (H[b] - 1) / stride + 1; wo[b] = (W[b] - 1) / stride + 1; }
    const VlGeo g = vl_geo(B, H, W, ho, wo);
    const int64_t pin = g.in0[B], pout = g.out0[B];
    CHK(ensure_ws(h, (pin * Cin + (int64_t)2 * Co * Cin * 9 + 3 * pout * Co) * 4 + (1 << 17), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act(pin, Cin, true), r = ws.act(pout, Co, true), r2 = ws.act(pout, Co, true);
    const bool mx = dbg_mx(h) && Co % 64 == 0;
    Lin L; CHK(dbg_make_lin(h, ws, w, bias, Co, Cin * 9, 1, Co, Cin, 3, 3, L, st, mx));
    Planes o = ws.act(pout, Co, true);
    char* gd; CHK(dbg_guard_arm(ws, o, pout, Co, &gd, st));
    xi.mx = o.mx = r.mx = r2.mx = mx;
    CHK(run_rows_to_planes(h, x, pin * Cin, 1, (int)pin, Cin, xi, st, 0, mx));
    if (resid) CHK(run_rows_to_planes(h, resid, pout * Co, 1, (int)pout, Co, r, st, 0, mx));
    if (resid2) CHK(run_rows_to_planes(h, resid2, pout * Co, 1, (int)pout, Co, r2, st, 0, mx));
    CHK(dbg_poison_act(o, pout, Co, st));
    CHK(conv3_vl(h, xi, g, Cin, L, stride, relu_in != 0, act, o, resid ? &r : nullptr, resid2 ? &r2 : nullptr, st));
    CHK(dbg_planes_to_f32(h, o, 0, 1, (int)pout, Co, out, st));
    return dbg_guard_read(gd, guard, st);
}
// the fused tail on packed pixels (conv3_head_vl: implicit GEMM on 192x128 tiles; fails on a small grid, as sta_debug_conv3_head does)
extern "C" int sta_debug_conv3_head_varlen(sta_handle* h, const float* x, const float* w2, const float* b2, const float* w4, const float* b4,
                                           int B, const int* H, const int* W, float* pts, float* conf, void* stream) {
    CHK(dbg_vl_check(h, B, H, W));
    REQUIRE(x && w2 && b2 && w4 && b4 && pts && conf, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const VlGeo g = vl_geo(B, H, W, H, W);
    const int64_t npix = g.in0[B];
    CHK(ensure_ws(h, (npix * 128 + (int64_t)2 * 128 * 128 * 9) * 4 + (1 << 16), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act(npix, 128, true);
    const bool mx = dbg_mx(h);
    xi.mx = mx;
    Lin L; CHK(dbg_make_lin(h, ws, w2, b2, 128, 128 * 9, 1, 128, 128, 3, 3, L, st, mx));
    REQUIRE(!ws.overflow, "debug ws overflow");
    REQUIRE((auto_family(h) && !small_grid(h, npix, 128)) || h->gemm_variant == 8, "the fused varlen tail does not run at %lld pixels under tile family %d", (long long)npix, h->gemm_variant);
    F32Lin L4; L4.w = const_cast<float*>(w4); L4.b = const_cast<float*>(b4);
    std::vector<float> w4h(4 * 128);
    HIPCHK(hipMemcpyAsync(w4h.data(), w4, w4h.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    struct ScaleGuard {
        float* dst; float keep[4];
        explicit ScaleGuard(float* d) : dst(d) { for (int o = 0; o < 4; ++o) keep[o] = d[o]; }
        ~ScaleGuard() { for (int o = 0; o < 4; ++o) dst[o] = keep[o]; }
    } restore_scales(h->head4_scale);
    head4_row_scales(w4h.data(), h->head4_scale);
    CHK(run_rows_to_planes(h, x, npix * 128, 1, (int)npix, 128, xi, st, 0, mx));
    CHK(dbg_poison(pts, npix * 12, st)); CHK(dbg_poison(conf, npix * 4, st));
    return conv3_head_vl(h, xi, g, 128, L, L4, pts, conf, st);
}
extern "C" int sta_debug_convt_varlen(sta_handle* h, const float* x, const float* w, const float* bias, int B, const int* H, const int* W,
                                      int C, int k, float* out, void* guard, void* stream) {
    CHK(dbg_vl_check(h, B, H, W));
    REQUIRE(x && w && bias && out && C > 0 && (k == 2 || k == 4), "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    int ho[SEQ_MAX], wo[SEQ_MAX];
    for (int b = 0; b < B; ++b) { ho[b] = k * H[b]; wo[b] = k * W[b]; }
    const VlGeo g = vl_geo(B, H, W, ho, wo);
    const int64_t pin = g.in0[B], pout = g.out0[B];
    CHK(ensure_ws(h, (pin * C + (int64_t)2 * C * C * k * k + pout * C) * 4 + (int64_t)C * k * k * 4 + (1 << 17), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act(pin, C, true);
    float* eb = (float*)ws.take((int64_t)C * k * k * 4);
    const bool mx = dbg_mx(h) && (k * k * C) % 64 == 0;
    Lin L; CHK(dbg_make_lin(h, ws, w, eb, k * k * C, C, 2, C, C, k, k, L, st, mx));
    Planes o = ws.act(pout, C, true);
    char* gd; CHK(dbg_guard_arm(ws, o, pout, C, &gd, st));
    xi.mx = o.mx = mx;
    hipLaunchKernelGGL(expand_bias_kernel, dim3((C * k * k + 255) / 256), dim3(256), 0, st, bias, eb, C, k * k);
    CHK(run_rows_to_planes(h, x, pin * C, 1, (int)pin, C, xi, st, 0, mx));
    CHK(dbg_poison_act(o, pout, C, st));
    CHK(gemm_convt_vl(h, xi, L, g, k, C, o, st));
    CHK(dbg_planes_to_f32(h, o, 0, 1, (int)pout, C, out, st));
    return dbg_guard_read(gd, guard, st);
}
extern "C" int sta_debug_up2_varlen(sta_handle* h, const float* x, int B, const int* H, const int* W, int C, const int* Hc, const int* Wc,
                                    float* out, void* guard, void* stream) {
    CHK(dbg_vl_check(h, B, H, W));
    REQUIRE(x && out && Hc && Wc && C % 8 == 0, "bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const VlGeo g = vl_geo(B, H, W, Hc, Wc);
    const int64_t pin = g.in0[B], pout = g.out0[B];
    CHK(ensure_ws(h, (pin + pout) * C * 4 + (1 << 17), st));
    Bump ws = cur_bump(h);
    Planes xi = ws.act(pin, C, true), o = ws.act(pout, C, true);
    char* gd; CHK(dbg_guard_arm(ws, o, pout, C, &gd, st));
    xi.mx = o.mx = dbg_mx(h);
    CHK(run_rows_to_planes(h, x, pin * C, 1, (int)pin, C, xi, st, 0, xi.mx));
    CHK(dbg_poison_act(o, pout, C, st));
    CHK(run_up2_vl(h, xi, g, C, o, st));
    CHK(dbg_planes_to_f32(h, o, 0, 1, (int)pout, C, out, st));
    return dbg_guard_read(gd, guard, st);
}
// Host only: the packing of the varlen head's six levels for B entries of hp[b] x wp[b] patches.  Level 0 .. 5 = (ceil(h/2), ceil(w/2)),
// (h, w), (2h, 2w), (4h, 4w), (8h, 8w), (16h, 16w).  off [6][B + 1]: first packed pixel of each entry, and the level's size; hw [6][B][2].
// ntiles [6] and tiles [cap][3] (both may be NULL): the halo-tiled convolution's tile map of every level, level after level - tile t of a
// level -> (entry, y0, x0), 8 rows x 32 pixels, from vl_tile (sta_common.h), the function the kernel decodes its block index with.
extern "C" int sta_debug_dpt_varlen_plan(int B, const int* hp, const int* wp, long long* off, int* hw, int* ntiles, int* tiles, int cap) {
    REQUIRE(hp && wp && off && hw && B >= 1 && B <= SEQ_MAX && (!tiles || (ntiles && cap >= 0)), "bad argument");
    int64_t used = 0;
    for (int k = 0; k < 6; ++k) {
        int lh[SEQ_MAX], lw[SEQ_MAX];
        for (int b = 0; b < B; ++b) {
            REQUIRE(hp[b] >= 1 && wp[b] >= 1, "bad argument (entry %d)", b);
            lh[b] = k == 0 ? (hp[b] - 1) / 2 + 1 : hp[b] << (k - 1); lw[b] = k == 0 ? (wp[b] - 1) / 2 + 1 : wp[b] << (k - 1);
            hw[(k * B + b) * 2] = lh[b]; hw[(k * B + b) * 2 + 1] = lw[b];
        }
        int64_t a = 0;
        for (int b = 0; b < B; ++b) { off[k * (B + 1) + b] = a; a += (int64_t)lh[b] * lw[b]; }
        off[k * (B + 1) + B] = a;
        REQUIRE(a < ((int64_t)1 << 31), "too many rows at level %d", k);
        if (ntiles) {
            const VlGeo g = vl_geo(B, lh, lw, lh, lw);
            const int nt = vl_tiles(g, 8);
            ntiles[k] = nt;
            if (tiles) {
                REQUIRE(used + nt <= cap, "tile map: %lld tiles do not fit the %d given", (long long)(used + nt), cap);
                for (int t = 0; t < nt; ++t) { int* o = tiles + (used + t) * 3; vl_tile(g, 8, t, o[0], o[1], o[2]); }
            }
            used += nt;
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ workspace independence (tests/test_workspace_gpu.py)
// The product entry points run on whatever the previous call left in the stream's scratch (StreamCtx: the workspace contract).  These
// hooks let a test put a known byte pattern there in front of a call, and look behind the call's planned peak afterwards.
static StreamCtx* dbg_find_ctx(sta_handle* h, hipStream_t st) {
    for (auto& c : h->ctx) if (c.st == st) return &c;
    return nullptr;
}
// bytes of ws[lo, hi) that differ from `byte`: res[0] += their number, res[1] = min of their offsets
__global__ void dbg_tail_scan_kernel(const unsigned char* ws, int64_t lo, int64_t hi, unsigned char byte, unsigned long long* res) {
    for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (int64_t)gridDim.x * blockDim.x)
        if (ws[i] != byte) { atomicAdd(&res[0], 1ull); atomicMin(&res[1], (unsigned long long)i); }
}

// `byte` into every byte of the scratch of `stream`'s context: ws[0, ws_cap), skbuf, slab and (where allocated) side_skbuf, enqueued
// on `stream`.  Fails when the stream has no context yet, or a split-phase scheduler call is pending on it (phase B reads phase A's
// workspace: filling it there would break a call that keeps the contract).
extern "C" int sta_debug_workspace_fill(sta_handle* h, void* stream, int byte) {
    REQUIRE(h && byte >= 0 && byte <= 255, "sta_debug_workspace_fill: bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    StreamCtx* c = dbg_find_ctx(h, st);
    REQUIRE(c, "sta_debug_workspace_fill: this stream has no scratch context (no call has run on it)");
    REQUIRE(!c->rv_open, "sta_debug_workspace_fill: a split-phase scheduler call is pending on this stream (its workspace is live until _finish)");
    if (c->ws && c->ws_cap > 0) HIPCHK(hipMemsetAsync(c->ws, byte, (size_t)c->ws_cap, st));
    if (c->skbuf) HIPCHK(hipMemsetAsync(c->skbuf, byte, (size_t)SKBUF_ELEMS * 4, st));
    if (c->slab) HIPCHK(hipMemsetAsync(c->slab, byte, (size_t)SKBUF_ELEMS * 4, st));
    if (c->side_skbuf) HIPCHK(hipMemsetAsync(c->side_skbuf, byte, (size_t)SKBUF_ELEMS * 4, st));
    return 0;
}

// out[0] ws_cap, out[1] the planned peak of the last plan_and_run call on the context, out[2] / [3] / [4] bytes of skbuf / slab /
// side_skbuf (0: not allocated), out[5] 1 while a split-phase scheduler call is pending, out[6] / [7] 0.
extern "C" int sta_debug_workspace_info(sta_handle* h, void* stream, int64_t out[8]) {
    REQUIRE(h && out, "sta_debug_workspace_info: bad argument");
    StreamCtx* c = dbg_find_ctx(h, (hipStream_t)stream);
    REQUIRE(c, "sta_debug_workspace_info: this stream has no scratch context (no call has run on it)");
    out[0] = c->ws_cap; out[1] = c->plan_peak;
    out[2] = c->skbuf ? SKBUF_ELEMS * 4 : 0; out[3] = c->slab ? SKBUF_ELEMS * 4 : 0; out[4] = c->side_skbuf ? SKBUF_ELEMS * 4 : 0;
    out[5] = c->rv_open ? 1 : 0; out[6] = out[7] = 0;
    return 0;
}

// The bytes of ws[planned peak + 4096, ws_cap) that differ from `byte` (ensure_ws is asked for peak + 4096: that slack belongs to the
// call): *n_bad their number, *first_bad the offset of the first one in ws (-1: none).  One scan kernel on `stream` with a 16-byte
// result of its own (not from the workspace); synchronises the stream.
extern "C" int sta_debug_workspace_tail(sta_handle* h, void* stream, int byte, int64_t* n_bad, int64_t* first_bad) {
    REQUIRE(h && n_bad && first_bad && byte >= 0 && byte <= 255, "sta_debug_workspace_tail: bad argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    StreamCtx* c = dbg_find_ctx(h, st);
    REQUIRE(c, "sta_debug_workspace_tail: this stream has no scratch context (no call has run on it)");
    const int64_t lo = c->plan_peak + 4096, hi = c->ws_cap;
    *n_bad = 0; *first_bad = -1;
    if (!c->ws || lo >= hi) return 0;
    unsigned long long* res = nullptr;
    unsigned long long host[2] = {0ull, ~0ull};
    HIPCHK(hipMalloc((void**)&res, 16));
    hipError_t e = hipMemcpyAsync(res, host, 16, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        int64_t blocks = (hi - lo + 255) / 256; if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(dbg_tail_scan_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const unsigned char*)c->ws, lo, hi, (unsigned char)byte, res);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host, res, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(res);
    if (e != hipSuccess) return set_err("sta_debug_workspace_tail failed: %s", hipGetErrorString(e));
    *n_bad = (int64_t)host[0]; *first_bad = host[0] ? (int64_t)host[1] : -1;
    return 0;
}

#ifdef STA_WAVE_SKEW      // libsta_mi355_skew.so only (sta_skew.h; tests/test_skew_gpu.py)
// The wave-skew configuration of THIS library's kernels.  wave_mask: bit w = wave w of every workgroup is delayed (bit 16: measure the
// barrier intervals instead, nothing is delayed); point_lo / point_hi: bit (id & 63) selects skew point id; repeat: s_sleep 127 per
// hit.  Resets the hit counter, the largest interval and the measuring mode's slots.  Synchronous on the null stream.
extern "C" int sta_debug_set_wave_skew(unsigned wave_mask, unsigned point_lo, unsigned point_hi, unsigned repeat) {
    REQUIRE(wave_mask <= 0x1ffffu && repeat <= 4096u, "sta_debug_set_wave_skew: bad argument");
    StaSkewCfg c;
    c.wave_mask = wave_mask; c.point_lo = point_lo; c.point_hi = point_hi; c.repeat = repeat; c.hits = 0; c.max_gap = 0;
    memset(c.seen, 0, sizeof(c.seen));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_sta_skew), &c, sizeof(c)));
    void* last = nullptr;
    HIPCHK(hipGetSymbolAddress(&last, HIP_SYMBOL(g_sta_skew_last)));
    HIPCHK(hipMemset(last, 0, sizeof(unsigned long long) * STA_SKEW_SLOTS));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}
// out[34]: out[0] skew points hit by selected waves since the last sta_debug_set_wave_skew; out[1] the largest interval between two
// consecutive points of one wave in the measuring mode, in ticks of the 100 MHz clock; out[2 .. 33] bit id = point id was hit (ids
// below 2048).  Synchronous on the null stream.
extern "C" int sta_debug_wave_skew_hits(unsigned long long* out) {
    REQUIRE(out, "sta_debug_wave_skew_hits: null output");
    StaSkewCfg c;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(&c, HIP_SYMBOL(g_sta_skew), sizeof(c)));
    out[0] = c.hits; out[1] = c.max_gap;
    for (int w = 0; w < STA_SKEW_IDS / 64; ++w) out[2 + w] = (unsigned long long)c.seen[2 * w] | ((unsigned long long)c.seen[2 * w + 1] << 32);
    return 0;
}
#endif
