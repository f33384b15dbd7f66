// Orchestration of the STA forward: encoder, cross-view decoder, pose head, DPT head (each a function over one stream's bump
// workspace: the same code runs once dry to size the workspace and once for real, plan_and_run).  Included by sta_api.hip.
// The encoder and the decoder each have ONE allocation function and ONE layer loop (encoder_layers / decoder_layers) that own every
// row-wise launch; a ROUTE (whole frames, token subsets, one token count per entry) is a function that prepares the input rows and
// hands the loop callables for what knows the sequence structure: the QKV producers, the rotation and the attention launch.

// o's Q / K / V^T planes advanced by `off` elements: a whole number of sequences of the shared npad (per-side / per-sequence QKV GEMMs)
static QKVOut qkv_at(const QKVOut& o, int64_t off) {
    QKVOut q = o;
    for (Planes* p : {&q.q, &q.k, &q.vt}) { p->hi += off; if (p->lo) p->lo += off; }
    return q;
}

// ------------------------------------------------------------------------------------------ encoder
struct EncPlanes { Planes patches, lnp, ao, f1; float* qkv32 = nullptr; QKVOut qkv; };
// The encoder's activation planes for M rows in nseq sequences of npad rows; qkv32: also fp32 rows [M, 3E] for a dense QKV GEMM
// (encode_varlen_impl).  Real pass: checks the workspace and zeroes the V^T padding.
static int enc_planes(sta_handle* h, Bump& ws, int M, int nseq, int npad, bool qkv32, EncPlanes& P, hipStream_t st) {
    const sta_config& c = h->cfg;
    const bool split = h->prec != STA_PREC_F16;
    const int E = c.enc_embed_dim;
    P.patches = ws.act(M, 768, split);
    P.lnp = ws.act(M, E, split);
    P.ao = ws.act(M, E, split);
    P.f1 = ws.act(M, (int64_t)E * c.mlp_ratio, split);
    P.f1.mx = c.enc_depth > 0 && use_mx(h, h->enc[0].fc2);          // precision f16x3m: mlp.fc1's GELU epilogue writes f16mx rows for mlp.fc2
    if (qkv32) P.qkv32 = (float*)ws.take((int64_t)M * 3 * E * 4);
    P.qkv.npad = npad;
    const int64_t hsz = (int64_t)nseq * c.enc_num_heads * npad * 64;
    P.qkv.q = ws.planes(hsz, split); P.qkv.k = ws.planes(hsz, split); P.qkv.vt = ws.planes(hsz, split);
    if (h->dry) return 0;
    REQUIRE(!ws.overflow, "internal: encode workspace overflow");
    const Planes* z[1] = {&P.qkv.vt};
    return zero_planes(z, 1, hsz, split, st);
}
// One patch-gather launch: launch(u8, split) is called with two std::bool_constant tags, the frame format and the call's precision
template <class F>
static int gather_dispatch(bool u8hwc, bool split, F&& launch) {
    if (u8hwc) { if (split) launch(std::true_type{}, std::true_type{}); else launch(std::true_type{}, std::false_type{}); }
    else if (split) launch(std::false_type{}, std::true_type{});
    else launch(std::false_type{}, std::false_type{});
    HIPCHK(hipGetLastError());
    return 0;
}
// Patch embedding of the gathered rows, then every Block.  step(b): lnp -> Q / K / V^T (rotated) -> attention of every sequence in ao.
template <class Step>
static int encoder_layers(sta_handle* h, const EncPlanes& P, int M, float* feat, hipStream_t st, Step&& step) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim;
    CHK(gemm_f32(h, P.patches, h->patch, M, feat, E, nullptr, st));
    // every in-place residual GEMM is issued together with the LayerNorm that reads its result (gemm_resid_ln)
    if (c.enc_depth > 0) CHK(run_ln(h, feat, M, E, h->enc[0].n1, P.lnp, nullptr, nullptr, nullptr, st));
    for (int i = 0; i < c.enc_depth; ++i) {
        const EncBlk& b = h->enc[i];
        CHK(step(b));
        CHK(gemm_resid_ln(h, P.ao, b.proj, M, feat, E, &b.n2, &P.lnp, nullptr, nullptr, st));
        CHK(gemm_f16(h, P.lnp, b.fc1, M, P.f1, ACT_GELU, st, P.f1.mx));
        if (i + 1 < c.enc_depth) CHK(gemm_resid_ln(h, P.f1, b.fc2, M, feat, E, &h->enc[i + 1].n1, &P.lnp, nullptr, nullptr, st));
        else CHK(gemm_resid_ln(h, P.f1, b.fc2, M, feat, E, nullptr, nullptr, nullptr, nullptr, st));
    }
    return 0;
}

// imgs: nsets pointers of B images each -> feat [nsets*B, N, E] (fp32, caller memory = residual stream)
static int encode_impl(sta_handle* h, Bump& ws, const void* const* imgs, bool u8hwc, int nsets, int B, int H, int W,
                       float* feat, hipStream_t st) {
    const sta_config& c = h->cfg;
    const bool split = h->prec != STA_PREC_F16;
    const int E = c.enc_embed_dim, Hh = c.enc_num_heads, hp = H / 16, wp = W / 16, N = hp * wp;
    const int n = nsets * B, M = n * N;
    EncPlanes P;
    CHK(enc_planes(h, ws, M, n, rup(N, 64), false, P, st));
    if (h->dry) return 0;
    for (int sidx = 0; sidx < nsets; ++sidx) {
        const int64_t row0 = (int64_t)sidx * B * N;
        CHK(gather_dispatch(u8hwc, split, [&](auto u8, auto sp) {
            const int blocks = (int)(((int64_t)B * N * (decltype(u8)::value ? 16 : 48) + 255) / 256);
            if constexpr (decltype(u8)::value) hipLaunchKernelGGL(patch_gather_u8hwc_kernel<decltype(sp)::value>, dim3(blocks), dim3(256), 0, st, (const uint8_t*)imgs[sidx], B, H, W, P.patches.hi, P.patches.lo, row0, (int64_t)M, h->range);
            else hipLaunchKernelGGL(patch_gather_kernel<decltype(sp)::value>, dim3(blocks), dim3(256), 0, st, (const float*)imgs[sidx], B, H, W, P.patches.hi, P.patches.lo, row0, (int64_t)M, h->range);
        }));
    }
    return encoder_layers(h, P, M, feat, st, [&](const EncBlk& b) -> int {
        CHK(gemm_qkv(h, P.lnp, b.qkv, M, E, E, E, P.qkv, N, Hh, wp, 0, st));
        return run_attn(h, P.qkv, P.ao, E, n, Hh, N, N, 0, st);
    });
}

// The gather launch of a token-subset route, M rows.  V = NoEntries: B x N tokens of one frame size; V = EncEntries: the table's.
template <class V = NoEntries>
static int gather_tokens(sta_handle* h, const void* img, bool u8hwc, int B, int N, int H, int W, const EncPlanes& P, int M, hipStream_t st, const V& ent = V{}) {
    return gather_dispatch(u8hwc, h->prec != STA_PREC_F16, [&](auto u8, auto sp) {
        const int blocks = (int)(((int64_t)M * (decltype(u8)::value ? 16 : 48) + 255) / 256);
        if constexpr (decltype(u8)::value) hipLaunchKernelGGL((patch_gather_tokens_u8hwc_kernel<decltype(sp)::value, V>), dim3(blocks), dim3(256), 0, st, (const uint8_t*)img, h->rope_pos, B, N, H, W, P.patches.hi, P.patches.lo, (int64_t)M, h->range, ent);
        else hipLaunchKernelGGL((patch_gather_tokens_kernel<decltype(sp)::value, V>), dim3(blocks), dim3(256), 0, st, (const float*)img, h->rope_pos, B, N, H, W, P.patches.hi, P.patches.lo, (int64_t)M, h->range, ent);
    });
}

// The encoder on a TOKEN SUBSET (sta_encode_tokens): N tokens per image, token t of image b = the patch at pos[b][t] = (y, x), which is
// also its RoPE position - the reference's module code on the gathered patch embeddings (patch_embed, then every Block with the
// gathered positions: sta_model.py:163-174, sta_blocks.py:129-148,166-169).  M = B*N rows: the gather reads the selected patches
// only, every QKV epilogue sees the grid 1 x N and rotates by the identity table (h->rope_foreign), one rope_tokens_kernel<., false>
// launch per layer rotates Q and K from the positions table, attention runs with nq = nk = N.
// h->rope_pos: the int32 table [B][N][2] inside the grid (enc_tokens_table_kernel).
static int encode_tokens_impl(sta_handle* h, Bump& ws, const void* img, bool u8hwc, int B, int H, int W, int N, float* feat, hipStream_t st) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim, Hh = c.enc_num_heads;
    const int M = B * N, npad = rup(N, 64);
    EncPlanes P;
    CHK(enc_planes(h, ws, M, B, npad, false, P, st));
    if (h->dry) return 0;
    CHK(gather_tokens(h, img, u8hwc, B, N, H, W, P, M, st));
    return encoder_layers(h, P, M, feat, st, [&](const EncBlk& b) -> int {
        CHK(gemm_qkv(h, P.lnp, b.qkv, M, E, E, E, P.qkv, N, Hh, N, 0, st));          // the grid 1 x N, identity table
        CHK(rope_enc_tokens(h, P.qkv.q, P.qkv.k, B, Hh, npad, N, st));
        return run_attn(h, P.qkv, P.ao, E, B, Hh, N, N, 0, st);
    });
}

// The encoder on a batch whose ENTRIES differ in token count and frame size (sta_encode_varlen): entry s has its own frame e.img[s] of
// e.H[s] x e.W[s] pixels and n_s = tok0[s + 1] - tok0[s] tokens at its own positions.  Batch entries never interact in the reference
// (attention is per sample), so entry s is what encode_tokens_impl returns for it alone at B = 1.  Rows are packed, M = sum n_s, sequence
// s the rows [tok0[s], tok0[s + 1]); nothing is padded.  What knows the sequence structure, per layer: (1) the QKV GEMM, dense over all
// rows, fp32 + bias into a workspace [M, 3E] (its fused epilogue cannot write Q / K / V^T across sequence boundaries);
// (2) qkv_finish_kernel's VARLEN form: rotation by each sequence's slice of the positions table, Q / K [S][heads][npad][64], V^T
// [S][heads][64][npad], npad = roundup(max n_s, 64), no pose row; (3) attn_varlen_kernel in the encoder form (run_attn_encv).
// Experiment switch 8: (1) + (2) as S gemm_qkv calls (identity table) + one no-pose rope_varlen_kernel launch, decode_varlen_impl's way.
// h->rope_pos: the int32 table [M][2], each entry clamped into its own grid (enc_varlen_table_kernel).  One lane, outside sta_reserve.
static int encode_varlen_impl(sta_handle* h, Bump& ws, const EncEntries& e, bool u8hwc, float* feat, hipStream_t st) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim, Hh = c.enc_num_heads, S = e.t.S;
    const bool per_seq = h->opt[8] == 1;
    int n[SEQ_MAX], nmax = 0;
    for (int s = 0; s < S; ++s) { n[s] = e.t.tok0[s + 1] - e.t.tok0[s]; nmax = std::max(nmax, n[s]); }
    const int M = e.t.tok0[S], npad = rup(nmax, 64);
    const int64_t ssz = (int64_t)Hh * npad * 64;       // one sequence
    EncPlanes P;
    CHK(enc_planes(h, ws, M, S, npad, !per_seq, P, st));
    if (h->dry) return 0;
    CHK(gather_tokens(h, nullptr, u8hwc, 0, 0, 0, 0, P, M, st, e));
    return encoder_layers(h, P, M, feat, st, [&](const EncBlk& b) -> int {
        if (per_seq) {
            for (int s = 0; s < S; ++s)          // the grid 1 x n_s, identity table: exactly the launch of a B = 1 sta_encode_tokens call
                CHK(gemm_qkv(h, slice_rows(P.lnp, e.t.tok0[s]), b.qkv, n[s], E, E, E, qkv_at(P.qkv, s * ssz), n[s], Hh, n[s], 0, st));
            const Planes* rot[2] = {&P.qkv.q, &P.qkv.k};
            CHK(rope_varlen_launch(h, rot, 2, e.t, Hh, npad, h->rope_pos, st, false));
        } else {
            CHK(gemm_f32(h, P.lnp, b.qkv, M, P.qkv32, 3 * E, nullptr, st));
            CHK(qkv_finish_varlen(h, P.qkv32, nullptr, E, Hh, e.t, P.qkv, h->rope_pos, st));
        }
        return run_attn_encv(h, P.qkv, P.ao, E, S, Hh, n, st);
    });
}

// ------------------------------------------------------------------------------------------ decoder
// Row order of the decoder's residual stream x (fp32, [2B*N + 2B, D]) and of every plane buffer derived from it (decode_impl):
//     rows [0, 2B*N)        patch tokens, sequence-major (sequence s = side * B + b, token t: row s*N + t)
//     rows [2B*N, 2B*N+2B)  the pose tokens of the 2B sequences
// (the reference prepends the pose token to every sequence, sta_model.py:206-213: M = 2B x (N + 1) interleaved rows.  Token
// order is immaterial to every layer - linears and LayerNorm are row-wise, attention is permutation-equivariant - and with
// the pose rows LAST the patch rows tile exactly: at 512x384, B = 8: 12288 = 64 x 192 rows + a 16-row tail that the GEMMs
// serve with skinny tail blocks (GemmParams::m_tail) and the attention kernel with its pose path (AttnParams::pose),
// instead of a 65th tile row, a 7th query block and a 13th key tile everywhere.)
struct DecPlanes { Planes fp, a1, ay, ao, f1; float* emb = nullptr; QKVOut qkv, cqkv; };
// The decoder's activation planes: fp_rows patch-feature rows, M rows of x in nseq sequences of npad rows; emb: also fp32 rows
// [fp_rows, D] for the packed patch embedding (decode_varlen_impl).  Real pass: checks the workspace and zeroes both V^T paddings.
static int dec_planes(sta_handle* h, Bump& ws, int64_t fp_rows, int M, int nseq, int npad, bool emb, DecPlanes& P, hipStream_t st) {
    const sta_config& c = h->cfg;
    const bool split = h->prec != STA_PREC_F16;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim;
    P.fp = ws.act(fp_rows, E, split);
    if (emb) P.emb = (float*)ws.take(fp_rows * D * 4);
    P.a1 = ws.act(M, D, split);
    P.ay = ws.act(M, D, split);
    P.ao = ws.act(M, D, split);
    P.f1 = ws.act(M, (int64_t)D * c.mlp_ratio, split);
    P.f1.mx = c.dec_depth > 0 && use_mx(h, h->dec[0].fc2);
    P.qkv.npad = P.cqkv.npad = npad;          // cross attention (cqkv): its K / V^T are produced while the self-attention set is live
    const int64_t hsz = (int64_t)nseq * c.dec_num_heads * npad * 64;
    P.qkv.q = ws.planes(hsz, split); P.qkv.k = ws.planes(hsz, split);
    P.cqkv.q = ws.planes(hsz, split); P.cqkv.k = ws.planes(hsz, split);
    P.qkv.vt = ws.planes(hsz, split); P.cqkv.vt = ws.planes(hsz, split);      // back to back: one fill zeroes both paddings
    if (h->dry) return 0;
    REQUIRE(!ws.overflow, "internal: decode workspace overflow");
    const Planes* z[2] = {&P.qkv.vt, &P.cqkv.vt};
    return zero_planes(z, 2, hsz, split, st);
}
// Every decoder Block on the M rows of x (in a1 / ay: the LayerNorm pair of the layer input).  The route supplies
//   self_step(b, i):   a1 -> self Q / K / V^T, ay -> the cross K / V^T, rotation, self attention of every sequence into ao
//   cross_step(b, i):  a1 -> the cross Q, rotation, cross attention of every sequence into ao
//   emit(idx, src):    the rows after layer idx (0: decoder input) to wherever the caller wants them
//   final_dst(idx, x): where dec_norm of the last layer's rows goes before it is emitted (x: in place), nullptr if nobody wants them
template <class Self, class Cross, class Emit, class FinalDst>
static int decoder_layers(sta_handle* h, const DecPlanes& P, int M, float* x, hipStream_t st,
                          Self&& self_step, Cross&& cross_step, Emit&& emit, FinalDst&& final_dst) {
    const sta_config& c = h->cfg;
    const int D = c.dec_embed_dim;
    CHK(emit(0, x));
    // norm1(x) and norm_y(x) from one read: y of one side == x of the other (sta_model.py:231-235); qkv and projk|projv:
    // one class, one plane format.  Layer i+1's pair is issued with layer i's mlp.fc2 (gemm_resid_ln).
    if (c.dec_depth > 0) CHK(run_ln(h, x, M, D, h->dec[0].n1, P.a1, &h->dec[0].ny, &P.ay, nullptr, st));
    for (int i = 0; i < c.dec_depth; ++i) {
        const DecBlk& b = h->dec[i];
        CHK(self_step(b, i));
        CHK(gemm_resid_ln(h, P.ao, b.proj, M, x, D, &b.n2, &P.a1, nullptr, nullptr, st));
        CHK(cross_step(b, i));
        CHK(gemm_resid_ln(h, P.ao, b.cproj, M, x, D, &b.n3, &P.a1, nullptr, nullptr, st));
        CHK(gemm_f16(h, P.a1, b.fc1, M, P.f1, ACT_GELU, st, P.f1.mx));
        if (i + 1 < c.dec_depth) {
            const DecBlk& nb = h->dec[i + 1];
            CHK(gemm_resid_ln(h, P.f1, b.fc2, M, x, D, &nb.n1, &P.a1, &nb.ny, &P.ay, st));
            CHK(emit(i + 1, x));
        } else {   // final_x[-1] = dec_norm(final_x[-1])  (sta_model.py:241-242)
            CHK(gemm_resid_ln(h, P.f1, b.fc2, M, x, D, nullptr, nullptr, nullptr, nullptr, st));
            if (float* dst = final_dst(i + 1, x)) {
                Planes none;
                CHK(run_ln(h, x, M, D, h->dec_norm, none, nullptr, nullptr, dst, st));
                CHK(emit(i + 1, dst));
            }
        }
    }
    return 0;
}
// final_dst of the routes that emit through a kernel: x is dead after the last layer, normalise it in place
static float* final_in_place(float* const* want1, float* const* want2, int idx, float* x) {
    return (want1 && want1[idx]) || (want2 && want2[idx]) ? x : nullptr;
}

// Outputs through the `want` tables, after layer i (i = 0: decoder input):
//   ref_layout:  want1[i] / want2[i] = [B, N+1, D] per side in the reference's token order (pose token first), or NULL
//   otherwise:   want1[i] = the whole x in the row order above (internal consumers: sta_forward_pair, sta_regress_views)
struct TailHint { sta_handle* h; TailHint(sta_handle* h_, int t) : h(h_) { h->tail_hint = t; } ~TailHint() { h->tail_hint = 0; } };
static int decode_impl(sta_handle* h, Bump& ws, const float* feat1, const float* feat2, int B, int hp, int wp,
                       float* x, float* const* want1, float* const* want2, bool ref_layout, hipStream_t st) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim, Hh = c.dec_num_heads;
    const int N = hp * wp, Np = N + 1, S = 2 * B, M = S * Np, Mp = S * N, npad = rup(Np, 64);
    DecPlanes P;
    CHK(dec_planes(h, ws, (int64_t)S * N, M, S, npad, false, P, st));
    if (h->dry) return 0;

    if (feat2 == feat1 + (size_t)B * N * E) {          // both sides in one buffer (sta_forward_pair, the scheduler): one launch
        CHK(run_rows_to_planes(h, feat1, (int64_t)N * E, 2 * B, N, E, P.fp, st));
    } else {
        CHK(run_rows_to_planes(h, feat1, (int64_t)N * E, B, N, E, P.fp, st));
        CHK(run_rows_to_planes(h, feat2, (int64_t)N * E, B, N, E, slice_rows(P.fp, (int64_t)B * N), st));
    }
    CHK(gemm_f32(h, P.fp, h->dec_embed, Mp, x, D, nullptr, st));
    float* xpose = x + (size_t)Mp * D;
    hipLaunchKernelGGL(fill_pose_token_kernel, dim3((S * D + 255) / 256), dim3(256), 0, st, xpose, S, 1, D, h->pose_tok);
    HIPCHK(hipGetLastError());
    auto emit = [&](int idx, const float* src) -> int {
        if (!ref_layout) {
            if (want1 && want1[idx] && want1[idx] != src) HIPCHK(hipMemcpyAsync(want1[idx], src, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
            return 0;
        }
        for (int side = 0; side < 2; ++side) {
            float* dst = side == 0 ? (want1 ? want1[idx] : nullptr) : (want2 ? want2[idx] : nullptr);
            if (!dst) continue;
            const int64_t total4 = (int64_t)B * Np * D / 4;
            int blocks = (int)((total4 + 255) / 256); if (blocks > 8192) blocks = 8192;
            hipLaunchKernelGGL(emit_tokens_kernel, dim3(blocks), dim3(256), 0, st, src, side * B, B, N, D, (int64_t)Mp, dst);
            HIPCHK(hipGetLastError());
        }
        return 0;
    };
    TailHint tail(h, S);                 // every dense GEMM below: the last S rows are the pose-token rows
    LaneJoin join_on_exit{h, st, false};          // armed by the first layer that forks
    bool forked = false;                 // this layer's cross K / V^T run on the side stream
    return decoder_layers(h, P, M, x, st,
        [&](const DecBlk& b, int i) -> int {
            // self-attention q,k,v and the cross-attention k,v of the OTHER side depend only on the layer input: one launch.
            // (They write disjoint buffers: qkv / cqkv.)
            // Below the paired launch's scale (two launches + two split-K finishers) the cross-attention K / V run on the context's
            // SIDE stream under the self-attention chain (qkv, attention, proj + norm2, cross q) and join before the cross attention.
            GemmParams pq, pkv;
            CHK(gp_qkv(h, pq, P.a1, b.qkv, M, D, D, D, P.qkv, N, Hh, wp, 0, Mp));
            CHK(gp_qkv(h, pkv, P.ay, b.ckv, M, 0, D, D, P.cqkv, N, Hh, wp, 0, Mp));
            forked = lanes_on(h) && !qkv_pair_one_launch(h, pq, pkv);
            if (forked) {
                CHK(ensure_side(h));
                join_on_exit.armed = true;
                hipEvent_t* ev = h->cur->side_ev + 2 * (i & 1);
                HIPCHK(hipEventRecord(ev[0], st));
                HIPCHK(hipStreamWaitEvent(h->cur->side, ev[0], 0));
                {
                    Lane lane(h, 1);
                    CHK((launch_gemm<A_DENSE, EPI_QKV>(h, pkv, h->cur->side)));
                }
                HIPCHK(hipEventRecord(ev[1], h->cur->side));
                CHK((launch_gemm<A_DENSE, EPI_QKV>(h, pq, st)));
            } else {
                CHK(gemm_qkv_pair(h, pq, pkv, st));
            }
            if (h->rope_foreign) {        // sta_decode_pos: the epilogues above rotated by the identity; every sequence's q / k by its own positions now
                CHK(rope_fix(h, P.qkv.q, S, Hh, npad, N, st)); CHK(rope_fix(h, P.qkv.k, S, Hh, npad, N, st)); CHK(rope_fix(h, P.cqkv.k, S, Hh, npad, N, st));
            }
            return run_attn(h, P.qkv, P.ao, D, S, Hh, N, N, 0, st, true);
        },
        [&](const DecBlk& b, int i) -> int {
            CHK(gemm_qkv(h, P.a1, b.cq, M, D, 0, 0, P.cqkv, N, Hh, wp, 0, st, Mp));
            CHK(rope_fix(h, P.cqkv.q, S, Hh, npad, N, st));
            if (forked) HIPCHK(hipStreamWaitEvent(st, h->cur->side_ev[2 * (i & 1) + 1], 0));
            return run_attn(h, P.cqkv, P.ao, D, S, Hh, N, N, B, st, true);
        },
        emit,
        [&](int idx, float* xin) -> float* {          // not ref_layout: straight into the caller's buffer, emit then has nothing to copy
            const bool wanted = (want1 && want1[idx]) || (ref_layout && want2 && want2[idx]);
            return !wanted ? nullptr : ref_layout ? xin : want1[idx];
        });
}

// ------------------------------------------------------------------------------------------ decoder, two token counts
// The decoder on a view pair of DIFFERENT resolution: side 1 has N1 = hp1 x wp1 patch tokens, side 2 N2 = hp2 x wp2 (the reference's
// module code takes them: cross attention accepts any memory length, sta_blocks.py:193-205; sta_model.py:177-244 is shape-agnostic).
// Row order of x (fp32, [B*(N1+1) + B*(N2+1), D]) and of every plane buffer derived from it: each side is decode_impl's layout with
// S = B, and the two sides are adjacent:
//     [B*N1 patch rows of side 1 | B pose rows of side 1 | B*N2 patch rows of side 2 | B pose rows of side 2]
// No TailHint (the pose rows are not the last rows of the launch: gemm_plan drops the row tail, as for any caller without a hint).
// What knows the sequence structure: the QKV / cross-K|V / cross-Q GEMMs run once PER SIDE on that side's contiguous row
// range (own ntok, wp, pose_base = B*Nx; Q / K / V^T planes advanced by B sequences of the shared npad) - the hot GEMMs' EPI_QKV is
// untouched -, attention is the two-group launch (run_attn_mixed): kv_shift = 0 for the self attention of both sides, kv_shift = B
// with (nq, nk) = (N1, N2) | (N2, N1) for the cross attention of both directions.  One lane (no side stream), outside
// sta_reserve's coverage.  Equal grids are served too (the same route: tests compare it with decode_impl).  Positions: each side's
// patch grid (sta_decode_mixed), or the caller's (sta_decode_tokens: each side enters as the grid 1 x Nx, the QKV epilogues rotate by
// the identity table - h->rope_foreign - and rope_tokens rotates the Q / K buffers of both groups from the positions table, two
// launches per layer).
// want1[i] [B, N1+1, D] / want2[i] [B, N2+1, D] in the reference's token order (pose token first), or NULL.
static int decode_mixed_impl(sta_handle* h, Bump& ws, const float* feat1, const float* feat2, int B, int hp1, int wp1, int hp2, int wp2,
                             float* x, float* const* want1, float* const* want2, hipStream_t st) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim, Hh = c.dec_num_heads;
    const int Nn[2] = {hp1 * wp1, hp2 * wp2}, wps[2] = {wp1, wp2};
    const int Mp[2] = {B * Nn[0], B * Nn[1]};                        // patch rows of a side = its pose_base
    const int R[2] = {Mp[0] + B, Mp[1] + B}, row0[2] = {0, R[0]};    // rows of a side, its first row
    const int M = R[0] + R[1], npad = rup((Nn[0] > Nn[1] ? Nn[0] : Nn[1]) + 1, 64);
    const int64_t ssz = (int64_t)B * Hh * npad * 64;                 // B sequences = one side
    DecPlanes P;
    CHK(dec_planes(h, ws, (int64_t)Mp[0] + Mp[1], M, 2 * B, npad, false, P, st));
    if (h->dry) return 0;

    for (int side = 0; side < 2; ++side) {
        const Planes fps = slice_rows(P.fp, side ? Mp[0] : 0);
        float* xs = x + (size_t)row0[side] * D;
        CHK(run_rows_to_planes(h, side ? feat2 : feat1, (int64_t)Nn[side] * E, B, Nn[side], E, fps, st));
        CHK(gemm_f32(h, fps, h->dec_embed, Mp[side], xs, D, nullptr, st));
        hipLaunchKernelGGL(fill_pose_token_kernel, dim3((B * D + 255) / 256), dim3(256), 0, st, xs + (size_t)Mp[side] * D, B, 1, D, h->pose_tok);
        HIPCHK(hipGetLastError());
    }
    auto emit = [&](int idx, const float* src) -> int {
        for (int side = 0; side < 2; ++side) {
            float* dst = side == 0 ? (want1 ? want1[idx] : nullptr) : (want2 ? want2[idx] : nullptr);
            if (!dst) continue;
            const int64_t total4 = (int64_t)B * (Nn[side] + 1) * D / 4;
            int blocks = (int)((total4 + 255) / 256); if (blocks > 8192) blocks = 8192;
            hipLaunchKernelGGL(emit_tokens_kernel, dim3(blocks), dim3(256), 0, st, src + (size_t)row0[side] * D, 0, B, Nn[side], D, (int64_t)Mp[side], dst);
            HIPCHK(hipGetLastError());
        }
        return 0;
    };
    // one QKV-epilogue GEMM per side: rows [row0, row0 + R) of A -> the side's B sequences of the Q / K / V^T buffers
    auto qkv_sides = [&](const Planes& A, const Lin& W, int nq, int nk, int nv, const QKVOut& o) -> int {
        for (int side = 0; side < 2; ++side)
            CHK(gemm_qkv(h, slice_rows(A, row0[side]), W, R[side], nq, nk, nv, qkv_at(o, side * ssz), Nn[side], Hh, wps[side], 0, st, Mp[side]));
        return 0;
    };
    return decoder_layers(h, P, M, x, st,
        [&](const DecBlk& b, int) -> int {
            CHK(qkv_sides(P.a1, b.qkv, D, D, D, P.qkv));
            CHK(qkv_sides(P.ay, b.ckv, 0, D, D, P.cqkv));         // K / V of a side's OWN tokens: the other side's queries read them (kv_shift = B)
            // sta_decode_tokens: the epilogues above rotated by the identity; both groups' q / k by their own positions now (one launch)
            const Planes* rot[3] = {&P.qkv.q, &P.qkv.k, &P.cqkv.k};
            CHK(rope_tokens(h, rot, 3, B, B, Hh, npad, Nn[0], Nn[1], st));
            return run_attn_mixed(h, P.qkv, P.ao, D, B, B, Hh, Nn[0], Nn[0], Nn[1], Nn[1], 0, st);
        },
        [&](const DecBlk& b, int) -> int {
            CHK(qkv_sides(P.a1, b.cq, D, 0, 0, P.cqkv));
            const Planes* rot[1] = {&P.cqkv.q};
            CHK(rope_tokens(h, rot, 1, B, B, Hh, npad, Nn[0], Nn[1], st));
            return run_attn_mixed(h, P.cqkv, P.ao, D, B, B, Hh, Nn[0], Nn[1], Nn[1], Nn[0], B, st);
        },
        emit, [&](int idx, float* xin) { return final_in_place(want1, want2, idx, xin); });
}

// ------------------------------------------------------------------------------------------ decoder, one token count per entry
// _decode_stereo on a batch whose entries have DIFFERENT token counts (sta_decode_varlen): entry b has n1[b] tokens on side 1 and
// n2[b] on side 2.  Batch entries never interact in the reference (sta_model.py:177-244; attention is per sample), so entry b is
// what a B = 1 call on it alone returns.  Sequences: s = b for side 1, B + b for side 2 (S = 2B <= 32), counts in a SeqTable that
// travels in the kernel arguments (the counts are host values: nothing is copied to the device, nothing is synchronised).
// Row order of x and every plane buffer derived from it: packed, no padded rows,
//     [n_0 patch rows | pose row] [n_1 patch rows | pose row] ... for s = 0 .. S - 1      (sequence s starts at row tok0[s] + s)
// What knows the sequence structure: the QKV / cross-K|V / cross-Q GEMMs run once PER SEQUENCE on its contiguous rows with the
// existing EPI_QKV (one sequence of ntok = n_s, pose_base = n_s: exactly the launch of a B = 1 sta_decode_tokens call; Q / K / V^T
// planes advanced by s sequences of the shared npad); the rotation is rope_varlen_kernel from the packed positions table; attention is
// the per-sequence launch (run_attn_varlen: kv_shift = 0 self attention of all sequences, kv_shift = B both cross directions).  One
// lane, outside sta_reserve's coverage.  want1[i] [sum(n1) + B, D] / want2[i] [sum(n2) + B, D]: entry by entry, pose token first, or NULL.
static int decode_varlen_impl(sta_handle* h, Bump& ws, const float* feat1, const float* feat2, const SeqTable& t, int B,
                              float* x, float* const* want1, float* const* want2, hipStream_t st) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim, Hh = c.dec_num_heads, S = 2 * B;
    int n[SEQ_MAX], nmax = 0;
    for (int s = 0; s < S; ++s) { n[s] = t.tok0[s + 1] - t.tok0[s]; nmax = std::max(nmax, n[s]); }
    const int Mp = t.tok0[S], Mp1 = t.tok0[B], M = Mp + S, npad = rup(nmax + 1, 64);
    const int64_t ssz = (int64_t)Hh * npad * 64;       // one sequence
    auto row0 = [&](int s) { return (int64_t)t.tok0[s] + s; };
    DecPlanes P;
    CHK(dec_planes(h, ws, Mp, M, S, npad, true, P, st));
    if (h->dry) return 0;

    // patch embedding of all tokens in one GEMM on the packed rows, then into the row order above with the pose tokens
    CHK(run_rows_to_planes(h, feat1, (int64_t)Mp1 * E, 1, Mp1, E, P.fp, st));
    CHK(run_rows_to_planes(h, feat2, (int64_t)(Mp - Mp1) * E, 1, Mp - Mp1, E, slice_rows(P.fp, Mp1), st));
    CHK(gemm_f32(h, P.fp, h->dec_embed, Mp, P.emb, D, nullptr, st));
    auto blocks_for = [](int64_t total4) { int64_t b = (total4 + 255) / 256; return (int)(b > 8192 ? 8192 : b); };
    hipLaunchKernelGGL(place_tokens_varlen_kernel, dim3(blocks_for((int64_t)M * D / 4)), dim3(256), 0, st, P.emb, t, D, h->pose_tok, x);
    HIPCHK(hipGetLastError());
    auto emit = [&](int idx, const float* src) -> int {
        for (int side = 0; side < 2; ++side) {
            float* dst = side == 0 ? (want1 ? want1[idx] : nullptr) : (want2 ? want2[idx] : nullptr);
            if (!dst) continue;
            const int64_t rows = row0(side * B + B) - row0(side * B);
            hipLaunchKernelGGL(emit_tokens_varlen_kernel, dim3(blocks_for(rows * D / 4)), dim3(256), 0, st, src, t, side * B, B, D, dst);
            HIPCHK(hipGetLastError());
        }
        return 0;
    };
    // one QKV-epilogue GEMM per sequence: its n_s + 1 rows of A -> its sequence of the Q / K / V^T buffers
    auto qkv_seqs = [&](const Planes& A, const Lin& W, int nq, int nk, int nv, const QKVOut& o) -> int {
        for (int s = 0; s < S; ++s)
            CHK(gemm_qkv(h, slice_rows(A, row0(s)), W, n[s] + 1, nq, nk, nv, qkv_at(o, s * ssz), n[s], Hh, n[s], 0, st, n[s]));
        return 0;
    };
    int nx[SEQ_MAX];                                    // cross attention: sequence s reads the keys of the other side's entry
    for (int s = 0; s < S; ++s) nx[s] = n[(s + B) % S];
    auto rope = [&](const Planes* const* bufs, int nbuf) -> int { return rope_varlen_launch(h, bufs, nbuf, t, Hh, npad, h->rope_pos, st); };
    return decoder_layers(h, P, M, x, st,
        [&](const DecBlk& b, int) -> int {
            CHK(qkv_seqs(P.a1, b.qkv, D, D, D, P.qkv));
            CHK(qkv_seqs(P.ay, b.ckv, 0, D, D, P.cqkv));         // K / V of a sequence's OWN tokens: the other side's queries read them (kv_shift = B)
            const Planes* rot[3] = {&P.qkv.q, &P.qkv.k, &P.cqkv.k};      // the epilogues above rotated by the identity
            CHK(rope(rot, 3));
            return run_attn_varlen(h, P.qkv, P.ao, D, S, Hh, n, n, 0, st);
        },
        [&](const DecBlk& b, int) -> int {
            CHK(qkv_seqs(P.a1, b.cq, D, 0, 0, P.cqkv));
            const Planes* rot[1] = {&P.cqkv.q};
            CHK(rope(rot, 1));
            return run_attn_varlen(h, P.cqkv, P.ao, D, S, Hh, n, nx, B, st);
        },
        emit, [&](int idx, float* xin) { return final_in_place(want1, want2, idx, xin); });
}

// ------------------------------------------------------------------------------------------ pose head
// pose2 / conf2 (optional): the last B - split samples write there (the two sides of a pair: one set of four launches)
// rows (optional, B <= 16): sample b is row rows->row[b] of tok (rows of `stride` floats) instead of row b - pose_layer_rows_kernel
static int pose_impl(sta_handle* h, Bump& ws, const float* tok, int B, int64_t stride, float* pose, float* conf, hipStream_t st,
                     float* pose2 = nullptr, float* conf2 = nullptr, int split = 0, const PoseRows* rows = nullptr) {
    const int D = h->cfg.dec_embed_dim, Hd = 512;
    float* f0 = (float*)ws.take((int64_t)B * Hd * 4);
    float* f1 = (float*)ws.take((int64_t)B * Hd * 4);
    if (h->dry) return 0;
    REQUIRE(!ws.overflow, "internal: pose workspace overflow");
    PoseParams p;
    p.tok = tok; p.tok_stride = stride; p.D = D; p.Hd = Hd;
    p.w0 = h->pm0.w; p.b0 = h->pm0.b; p.w1 = h->pm1.w; p.b1 = h->pm1.b; p.w2 = h->pm2.w; p.b2 = h->pm2.b;
    p.wt = h->pt.w; p.bt = h->pt.b; p.wr = h->pr.w; p.br = h->pr.b; p.wc = h->pc.w; p.bc = h->pc.b;
    p.pose = pose; p.conf = conf; p.pose2 = pose2; p.conf2 = conf2; p.split = split;
    dim3 grid(Hd / 4, B);
    if (rows) hipLaunchKernelGGL(pose_layer_rows_kernel, grid, dim3(256), 0, st, tok, stride, *rows, p.w0, p.b0, f0, D, Hd, 1);
    else hipLaunchKernelGGL(pose_layer_kernel, grid, dim3(256), 0, st, tok, stride, p.w0, p.b0, f0, D, Hd, 1);
    hipLaunchKernelGGL(pose_layer_kernel, grid, dim3(256), 0, st, f0, (int64_t)Hd, p.w1, p.b1, f1, Hd, Hd, 1);
    hipLaunchKernelGGL(pose_layer_kernel, grid, dim3(256), 0, st, f1, (int64_t)Hd, p.w2, p.b2, f0, Hd, Hd, 1);
    hipLaunchKernelGGL(pose_final_kernel, dim3(B), dim3(256), 0, st, p, f0);
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ DPT head
struct RcuTmp { Planes t, y; };
static int run_rcu(sta_handle* h, const Planes& x, int n, int Hh, int Ww, const RCU& u, const Planes& tmp,
                   const Planes& out, const Planes* extra, hipStream_t st) {
    // out = x + conv2(relu(conv1(relu(x)))) [+ extra]   (dpt_block.py:121-142, 196-204)
    CHK(conv3(h, x, n, Hh, Ww, 256, u.c1, 1, true, ACT_RELU, tmp, nullptr, nullptr, st));
    CHK(conv3(h, tmp, n, Hh, Ww, 256, u.c2, 1, false, ACT_NONE, out, &x, extra, st));
    return 0;
}

// outputs: first nA images -> (ptsA, confA), remaining -> (ptsB, confB)
static int dpt_impl(sta_handle* h, Bump& ws, const float* enc, int64_t enc_bs,
                    const float* h1, int64_t h1_bs, const float* h2, int64_t h2_bs, const float* h3, int64_t h3_bs,
                    int n, int H, int W, float* ptsA, float* confA, int nA, float* ptsB, float* confB, hipStream_t st) {
    const sta_config& c = h->cfg;
    const bool split = h->prec != STA_PREC_F16;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim, hp = H / 16, wp = W / 16, N = hp * wp;
    const int M = n * N;
    // precision f16mx: every DPT buffer is in the f16mx row format, except the input of act_postprocess[0]
    // (N = 96: no f16mx kernel for that one GEMM, it reads f16x3 rows and WRITES f16mx rows)
    const bool dmx = (h->mx_mask & CLS_HEAD) != 0;
    auto act = [&](int64_t rows, int64_t cols, bool mx) { Planes q = ws.act(rows, cols, split); q.mx = mx; return q; };
    // Two lanes (round 4).  The head is a chain - level 3 (1/32 scale) -> refinenet4 -> refinenet3 -> refinenet2 -> refinenet1 -> head -
    // with three side branches feeding it: the reassembly of levels 2, 1, 0 (rows -> planes, act_postprocess, layer_rn) and the first
    // convolution of each refinenet's resConfUnit1, which reads only that level.  The 14 side-branch launches run on the context's
    // SIDE stream under the chain: fork at entry, one event per level (2, 1, 0) that the chain waits on right before it consumes
    // that level.  At SLAM scale every kernel of the head is a fraction of a round of workgroups and a launch costs as much as the
    // kernel (tools/model_stamps.py: 10 - 25 us of event time around 5 - 17 us of work): 5-edge scheduler call -5.8 %, one pair
    // @512x384 +2.3 %; at the benchmark's 8 pairs the side kernels fill the chain's partial rounds (+0.8 %).  Same kernels, same
    // split-K slices (the side lane has its own scratch): bit-identical to the one-lane order (tests/test_gpu_parity.py).
    // sta_debug_set_option(h, 6, 1) switches the lane off (A/B: tools/ab_option.py 6 1 0); the whole-model timing modes (stage timing, per-launch timing of every GEMM, stamps) run one lane.
    const bool two = lanes_on(h);
    hipStream_t sb = st;                                                  // the side branches' stream
    if (two) {
        CHK(ensure_side(h));
        sb = h->cur->side;
        HIPCHK(hipEventRecord(h->cur->side_ev[3], st));
        HIPCHK(hipStreamWaitEvent(sb, h->cur->side_ev[3], 0));
    }
    LaneJoin join_on_exit{h, st, two};
    Planes t0 = act(M, E, use_mx(h, h->act0_0)), t1 = act(M, D, dmx);
    Planes t2 = act(M, D, dmx), t3 = act(M, D, dmx);
    // act_postprocess (dpt_block.py:356-410)
    Planes a0 = act(M, 96, dmx), l0 = act((int64_t)M * 16, 96, dmx);
    Planes a1 = act(M, 192, dmx), l1 = act((int64_t)M * 4, 192, dmx);
    Planes l2 = act(M, 384, dmx);
    Planes a3 = act(M, 768, dmx);
    const int h3s = (hp - 1) / 2 + 1, w3s = (wp - 1) / 2 + 1;
    Planes l3 = act((int64_t)n * h3s * w3s, 768, dmx);
    // layer_rn (3x3, no bias) -> 256 channels at 4x, 2x, 1x, 1/2x
    const int Hs[4] = {4 * hp, 2 * hp, hp, h3s}, Ws[4] = {4 * wp, 2 * wp, wp, w3s};
    const int Cs[4] = {96, 192, 384, 768};
    Planes lin[4] = {l0, l1, l2, l3}, r[4], c1o[4];          // c1o[k]: relu(conv1(relu(r[k]))) of refinenet k's resConfUnit1 (k < 3)
    for (int k = 0; k < 4; ++k) {
        r[k] = act((int64_t)n * Hs[k] * Ws[k], 256, dmx);
        if (k < 3) c1o[k] = act((int64_t)n * Hs[k] * Ws[k], 256, dmx);
    }
    REQUIRE(!ws.overflow, "internal: dpt workspace overflow (stage 1)");
    {   // level 3 opens the chain
        CHK(run_rows_to_planes(h, h3, h3_bs, n, N, D, t3, st, 0, t3.mx));
        CHK(gemm_f16(h, t3, h->act3_0, M, a3, ACT_NONE, st, a3.mx));
        CHK(conv3(h, a3, n, hp, wp, 768, h->act3_1, 2, false, ACT_NONE, l3, nullptr, nullptr, st));
        CHK(conv3(h, l3, n, Hs[3], Ws[3], Cs[3], h->rn[3], 1, false, ACT_NONE, r[3], nullptr, nullptr, st));
    }
    {   // side branches, in the order the chain consumes them: level 2, 1, 0
        Lane lane(h, two ? 1 : 0);
        for (int k = 2; k >= 0; --k) {
            if (k == 2) {
                CHK(run_rows_to_planes(h, h2, h2_bs, n, N, D, t2, sb, 0, t2.mx));
                CHK(gemm_f16(h, t2, h->act2_0, M, l2, ACT_NONE, sb, l2.mx));
            } else if (k == 1) {
                CHK(run_rows_to_planes(h, h1, h1_bs, n, N, D, t1, sb, 0, t1.mx));
                CHK(gemm_f16(h, t1, h->act1_0, M, a1, ACT_NONE, sb, a1.mx));
                CHK(gemm_convt(h, a1, h->act1_1, n, hp, wp, 2, 192, l1, sb));
            } else {
                CHK(run_rows_to_planes(h, enc, enc_bs, n, N, E, t0, sb, 0, t0.mx));
                CHK(gemm_f16(h, t0, h->act0_0, M, a0, ACT_NONE, sb, a0.mx));
                CHK(gemm_convt(h, a0, h->act0_1, n, hp, wp, 4, 96, l0, sb));
            }
            CHK(conv3(h, lin[k], n, Hs[k], Ws[k], Cs[k], h->rn[k], 1, false, ACT_NONE, r[k], nullptr, nullptr, sb));
            CHK(conv3(h, r[k], n, Hs[k], Ws[k], 256, h->ref[k].u1.c1, 1, true, ACT_RELU, c1o[k], nullptr, nullptr, sb));
            if (two) HIPCHK(hipEventRecord(h->cur->side_ev[k], sb));
        }
    }
    // refinenet4 .. refinenet1.  out_conv (1x1) commutes with the bilinear upsample (both linear, the
    // interpolation weights sum to 1), so it runs BEFORE the x2 upsample at 1/4 of the FLOPs.
    Planes path;   // upsampled output of the previous stage
    int ph = 0, pw = 0;
    for (int k = 3; k >= 0; --k) {
        const Refine& rf = h->ref[k];
        const int hh = Hs[k], ww = Ws[k];
        const int64_t el = (int64_t)n * hh * ww;
        Planes tmp = act(el, 256, dmx), cur = r[k];
        if (k < 3) {
            REQUIRE(ph == hh && pw == ww, "internal: refinenet size mismatch %dx%d vs %dx%d", ph, pw, hh, ww);
            Planes sum = act(el, 256, dmx);
            REQUIRE(!ws.overflow, "internal: dpt workspace overflow (fusion)");
            if (two) HIPCHK(hipStreamWaitEvent(st, h->cur->side_ev[k], 0));
            // path + RCU1(layer) = path + r[k] + conv2(c1o[k])   (dpt_block.py:121-142, 196-204)
            CHK(conv3(h, c1o[k], n, hh, ww, 256, rf.u1.c2, 1, false, ACT_NONE, sum, &r[k], &path, st));
            cur = sum;
        }
        Planes y = act(el, 256, dmx), z = act(el, 256, dmx);
        REQUIRE(!ws.overflow, "internal: dpt workspace overflow (rcu2)");
        CHK(run_rcu(h, cur, n, hh, ww, rf.u2, tmp, y, nullptr, st));
        CHK(gemm_f16(h, y, rf.out, n * hh * ww, z, ACT_NONE, st, z.mx));
        // upsample x2 (align_corners) ; refinenet4 output is cropped to the layers[2] size (dpt_head.py:58)
        int oh = 2 * hh, ow = 2 * ww;
        if (k == 3) { if (oh > Hs[2]) oh = Hs[2]; if (ow > Ws[2]) ow = Ws[2]; }
        Planes up = act((int64_t)n * oh * ow, 256, dmx);
        REQUIRE(!ws.overflow, "internal: dpt workspace overflow (up)");
        CHK(run_up2(h, z, n, hh, ww, 256, oh, ow, up, st));
        path = up; ph = oh; pw = ow;
    }
    // head: 3x3 256->128, up x2, 3x3 128->128 + ReLU, 1x1 128->4 + postprocess (dpt_block.py:316-324)
    Planes h0 = act((int64_t)n * ph * pw, 128, dmx);
    Planes h0u = act((int64_t)n * H * W, 128, dmx);
    const bool fused_tail = conv3_head_ok(h, h->head2, (int64_t)n * H * W);     // the [pixels,128] map of head.2 stays on chip
    Planes h2o; if (!fused_tail) h2o = act((int64_t)n * H * W, 128, dmx);
    REQUIRE(!ws.overflow, "internal: dpt workspace overflow (head)");
    REQUIRE(2 * ph == H && 2 * pw == W, "internal: head size mismatch");
    CHK(conv3(h, path, n, ph, pw, 256, h->head0, 1, false, ACT_NONE, h0, nullptr, nullptr, st));
    CHK(run_up2(h, h0, n, ph, pw, 128, H, W, h0u, st));
    if (fused_tail) return conv3_head(h, h0u, n, H, W, 128, h->head2, h->head4, ptsA, confA, nA, ptsB, confB, st);
    CHK(conv3(h, h0u, n, H, W, 128, h->head2, 1, false, ACT_RELU, h2o, nullptr, nullptr, st));
    for (int part = 0; part < 2 && !h->dry; ++part) {
        int i0 = part == 0 ? 0 : nA, cnt = part == 0 ? (nA < n ? nA : n) : n - nA;
        if (cnt <= 0) continue;
        float* pp = part == 0 ? ptsA : ptsB; float* cp = part == 0 ? confA : confB;
        int64_t npix = (int64_t)cnt * H * W;
        const int64_t pix0 = (int64_t)i0 * H * W;
        int blocks = (int)((npix * 16 + 255) / 256); if (blocks > 16384) blocks = 16384;
        if (split) hipLaunchKernelGGL(head_final_kernel<true>, dim3(blocks), dim3(256), 0, st, h2o.hi, h2o.lo, pix0, h2o.rp, npix, h->head4.w, h->head4.b, pp, cp, h2o.mx ? 1 : 0);
        else hipLaunchKernelGGL(head_final_kernel<false>, dim3(blocks), dim3(256), 0, st, h2o.hi, h2o.lo, pix0, h2o.rp, npix, h->head4.w, h->head4.b, pp, cp, 0);
        HIPCHK(hipGetLastError());
    }
    return 0;
}


// ------------------------------------------------------------------------------------------ DPT head, one patch rectangle per entry
// dpt_impl on B <= SEQ_MAX entries of DIFFERENT size in one call (sta_head_pts_varlen): entry b is hp[b] x wp[b] patches, and what
// dpt_impl computes for it alone at (16 hp[b], 16 wp[b]).  Nothing is padded and no pixel reads another entry's pixels.  At each of the
// head's six resolutions - (ceil(h/2), ceil(w/2)), (h, w), (2h, 2w), (4h, 4w), (8h, 8w), (16h, 16w) - the pixels of all entries are
// packed entry-major, row-major inside an entry; what dpt_impl derives from one (H, W) - h3s / w3s, the crop of refinenet4's x2
// output to (h, w), the align_corners ratios - is per entry, in the VlGeo table of each launch (kernel arguments; host values:
// nothing is copied to the device, nothing is synchronised).  The same launch sequence as dpt_impl, one launch per step: the row-wise
// steps (rows -> planes through the row table, every 1x1 GEMM, the split-K finisher, head_final_kernel) run once over the packed rows
// as they are; the geometry-decoding steps run their varlen forms (conv3_vl, gemm_convt_vl, run_up2_vl).  Tile families: the cost
// model on the packed M of each level (the halo-tiled family 8, whose cost the model counts per image size, only where it is forced).  One lane.
// enc_row / hook_row: first patch row of entry b in enc / in each hook buffer.  out_pix: pixel offset of entry b in pts / conf, or
// nullptr = packed (256 x the patches before it).
static int dpt_varlen_impl(sta_handle* h, Bump& ws, const float* enc, const int64_t* enc_row, const float* h1, const float* h2, const float* h3,
                           const int64_t* hook_row, const int* hp, const int* wp, int B, float* pts, float* conf, const int64_t* out_pix, hipStream_t st) {
    const sta_config& c = h->cfg;
    const bool split = h->prec != STA_PREC_F16;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim;
    const bool dmx = (h->mx_mask & CLS_HEAD) != 0;
    auto act = [&](int64_t rows, int64_t cols, bool mx) { Planes q = ws.act(rows, cols, split); q.mx = mx; return q; };
    // the six levels: index 0 .. 3 as dpt_impl's Hs / Ws (4x, 2x, 1x, 1/2x), 4 = 8x, 5 = 16x
    int lh[6][SEQ_MAX], lw[6][SEQ_MAX], ch[SEQ_MAX], cw[SEQ_MAX];
    int64_t P[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < B; ++b) {
        const int hh = hp[b], ww = wp[b];
        lh[0][b] = 4 * hh; lw[0][b] = 4 * ww; lh[1][b] = 2 * hh; lw[1][b] = 2 * ww; lh[2][b] = hh; lw[2][b] = ww;
        lh[3][b] = (hh - 1) / 2 + 1; lw[3][b] = (ww - 1) / 2 + 1;
        lh[4][b] = 8 * hh; lw[4][b] = 8 * ww; lh[5][b] = 16 * hh; lw[5][b] = 16 * ww;
        for (int k = 0; k < 6; ++k) P[k] += (int64_t)lh[k][b] * lw[k][b];
        ch[b] = std::min(2 * lh[3][b], hh); cw[b] = std::min(2 * lw[3][b], ww);      // refinenet4's x2 output, cropped (dpt_head.py:58)
    }
    const int M = (int)P[2];
    auto same = [&](int k) { return vl_geo(B, lh[k], lw[k], lh[k], lw[k]); };
    auto step = [&](int ki, int ko) { return vl_geo(B, lh[ki], lw[ki], lh[ko], lw[ko]); };
    RowSrc re, rh; memset(&re, 0, sizeof re); memset(&rh, 0, sizeof rh);
    re.t.S = rh.t.S = B;
    { int acc = 0; for (int b = 0; b < B; ++b) { re.t.tok0[b] = rh.t.tok0[b] = acc; re.src_row[b] = enc_row[b]; rh.src_row[b] = hook_row[b]; acc += hp[b] * wp[b]; } re.t.tok0[B] = rh.t.tok0[B] = acc; }

    Planes t0 = act(M, E, use_mx(h, h->act0_0)), t1 = act(M, D, dmx), t2 = act(M, D, dmx), t3 = act(M, D, dmx);
    Planes a0 = act(M, 96, dmx), l0 = act(P[0], 96, dmx);
    Planes a1 = act(M, 192, dmx), l1 = act(P[1], 192, dmx);
    Planes l2 = act(M, 384, dmx), a3 = act(M, 768, dmx), l3 = act(P[3], 768, dmx);
    const int Cs[4] = {96, 192, 384, 768};
    Planes lin[4] = {l0, l1, l2, l3}, r[4], c1o[4];
    for (int k = 0; k < 4; ++k) {
        r[k] = act(P[k], 256, dmx);
        if (k < 3) c1o[k] = act(P[k], 256, dmx);
    }
    REQUIRE(!ws.overflow, "internal: dpt workspace overflow (stage 1)");
    // reassembly, in dpt_impl's order: level 3 (1x1, then 3x3 stride 2), 2 (1x1), 1 (1x1, ConvT k = 2), 0 (1x1, ConvT k = 4); layer_rn
    CHK(run_rows_to_planes_src(h, h3, rh, D, t3, st, t3.mx));
    CHK(gemm_f16(h, t3, h->act3_0, M, a3, ACT_NONE, st, a3.mx));
    CHK(conv3_vl(h, a3, step(2, 3), 768, h->act3_1, 2, false, ACT_NONE, l3, nullptr, nullptr, st));
    CHK(conv3_vl(h, l3, same(3), Cs[3], h->rn[3], 1, false, ACT_NONE, r[3], nullptr, nullptr, st));
    for (int k = 2; k >= 0; --k) {
        if (k == 2) {
            CHK(run_rows_to_planes_src(h, h2, rh, D, t2, st, t2.mx));
            CHK(gemm_f16(h, t2, h->act2_0, M, l2, ACT_NONE, st, l2.mx));
        } else if (k == 1) {
            CHK(run_rows_to_planes_src(h, h1, rh, D, t1, st, t1.mx));
            CHK(gemm_f16(h, t1, h->act1_0, M, a1, ACT_NONE, st, a1.mx));
            CHK(gemm_convt_vl(h, a1, h->act1_1, step(2, 1), 2, 192, l1, st));
        } else {
            CHK(run_rows_to_planes_src(h, enc, re, E, t0, st, t0.mx));
            CHK(gemm_f16(h, t0, h->act0_0, M, a0, ACT_NONE, st, a0.mx));
            CHK(gemm_convt_vl(h, a0, h->act0_1, step(2, 0), 4, 96, l0, st));
        }
        CHK(conv3_vl(h, lin[k], same(k), Cs[k], h->rn[k], 1, false, ACT_NONE, r[k], nullptr, nullptr, st));
        CHK(conv3_vl(h, r[k], same(k), 256, h->ref[k].u1.c1, 1, true, ACT_RELU, c1o[k], nullptr, nullptr, st));
    }
    // refinenet4 .. refinenet1 (out_conv before the x2 upsample, as in dpt_impl)
    Planes path;
    for (int k = 3; k >= 0; --k) {
        const Refine& rf = h->ref[k];
        const VlGeo g = same(k);
        const int64_t el = P[k];
        Planes tmp = act(el, 256, dmx), cur = r[k];
        if (k < 3) {
            Planes sum = act(el, 256, dmx);
            REQUIRE(!ws.overflow, "internal: dpt workspace overflow (fusion)");
            REQUIRE(h->dry || path.rp == el, "internal: refinenet size mismatch at level %d", k);
            CHK(conv3_vl(h, c1o[k], g, 256, rf.u1.c2, 1, false, ACT_NONE, sum, &r[k], &path, st));
            cur = sum;
        }
        Planes y = act(el, 256, dmx), z = act(el, 256, dmx);
        REQUIRE(!ws.overflow, "internal: dpt workspace overflow (rcu2)");
        CHK(conv3_vl(h, cur, g, 256, rf.u2.c1, 1, true, ACT_RELU, tmp, nullptr, nullptr, st));
        CHK(conv3_vl(h, tmp, g, 256, rf.u2.c2, 1, false, ACT_NONE, y, &cur, nullptr, st));
        CHK(gemm_f16(h, y, rf.out, (int)el, z, ACT_NONE, st, z.mx));
        // k == 3: 2 h3s x 2 w3s cropped to (h, w); the other levels land on the next level's size: lh[k - 1] (k = 0: level 4, 8x)
        const VlGeo ug = k == 3 ? vl_geo(B, lh[3], lw[3], ch, cw) : step(k, k == 0 ? 4 : k - 1);
        Planes up = act(ug.out0[B], 256, dmx);
        REQUIRE(!ws.overflow, "internal: dpt workspace overflow (up)");
        if (k == 3) for (int b = 0; b < B; ++b) REQUIRE(ch[b] == lh[2][b] && cw[b] == lw[2][b], "internal: refinenet4 crop of entry %d", b);
        CHK(run_up2_vl(h, z, ug, 256, up, st));
        path = up;
    }
    // head: 3x3 256 -> 128 at 8x, up x2, 3x3 128 -> 128 + ReLU, 1x1 128 -> 4 + postprocess
    Planes h0 = act(P[4], 128, dmx), h0u = act(P[5], 128, dmx);
    bool packed_out = true;
    if (out_pix) { int64_t o = 0; for (int b = 0; b < B; ++b) { packed_out = packed_out && out_pix[b] == o; o += (int64_t)lh[5][b] * lw[5][b]; } }
    // the fused tail on the packed pixels (conv3_head_ok's rule: implicit GEMM on 192x128, the halo form where forced), packed outputs
    const bool fused_tail = packed_out && h->head2.N == 128 && ((auto_family(h) && !small_grid(h, P[5], h->head2.N)) || h->gemm_variant == 8);
    // (planning pass: always with the [pixels, 128] map of the unfused tail - the scheduler plans with every edge accepted, i.e. packed
    //  outputs, and runs with whatever was accepted: a rejected edge in front of an accepted one leaves a gap, and the tail unfused)
    Planes h2o; if (!fused_tail || h->dry) h2o = act(P[5], 128, dmx);
    REQUIRE(!ws.overflow, "internal: dpt workspace overflow (head)");
    CHK(conv3_vl(h, path, same(4), 256, h->head0, 1, false, ACT_NONE, h0, nullptr, nullptr, st));
    CHK(run_up2_vl(h, h0, step(4, 5), 128, h0u, st));
    if (fused_tail) return conv3_head_vl(h, h0u, same(5), 128, h->head2, h->head4, pts + (out_pix ? out_pix[0] * 3 : 0), conf + (out_pix ? out_pix[0] : 0), st);
    CHK(conv3_vl(h, h0u, same(5), 128, h->head2, 1, false, ACT_RELU, h2o, nullptr, nullptr, st));
    if (h->dry) return 0;
    // head_final_kernel: once over all packed pixels, or once per run of entries whose outputs are contiguous (out_pix with gaps)
    const VlGeo g5 = same(5);
    for (int b0 = 0; b0 < B;) {
        int b1 = b0 + 1;
        int64_t o0 = out_pix ? out_pix[b0] : g5.out0[b0];
        while (b1 < B && (out_pix ? out_pix[b1] : (int64_t)g5.out0[b1]) == o0 + (g5.out0[b1] - g5.out0[b0])) ++b1;
        const int64_t pix0 = g5.out0[b0], npix = g5.out0[b1] - g5.out0[b0];
        int blocks = (int)((npix * 16 + 255) / 256); if (blocks > 16384) blocks = 16384;
        hipLaunchKernelGGL(head_final_kernel<true>, dim3(blocks), dim3(256), 0, st, h2o.hi, h2o.lo, pix0, h2o.rp, npix, h->head4.w, h->head4.b, pts + o0 * 3, conf + o0, h2o.mx ? 1 : 0);
        HIPCHK(hipGetLastError());
        b0 = b1;
    }
    return 0;
}
