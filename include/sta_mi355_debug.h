/*
 * sta_mi355_debug.h - kernel-level TEST and micro-benchmark entry points.  They are NOT part of the product ABI: the
 * product library libsta_mi355.so exports include/sta_mi355.h only; these symbols exist in libsta_mi355_test.so, the same
 * translation unit compiled with -DSTA_TEST_HOOKS (vista_slam_amd/build.py builds both; tests/ and tools/ load the second).
 *
 * Each sta_debug_* function runs exactly one product kernel (the same template instantiation the product path
 * launches) on fp32 device tensors so that tests/ can compare it with a plain fp32 reference of the
 * same op (reference ops cited per function).  Nothing in the product path calls these.
 * All pointers are device pointers unless noted; return 0 / negative + sta_last_error().
 */
#ifndef STA_MI355_DEBUG_H
#define STA_MI355_DEBUG_H
#include "sta_mi355.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Force the GEMM tile family: 0 = automatic (product behaviour), 1 = 128x128 register-staged kernel,
 * 2 = 256-row direct-to-LDS kernels, 3 = 192-row ones (whenever N % 128 == 0), 4 = 192x128 everywhere, 8 = the halo-tiled
 * 3x3 convolution kernel (conv3h.h) wherever it is legal (stride 1, Cout 128 / 256), 9 = automatic WITHOUT that kernel
 * (same-box A/B), 10 / 11 = automatic with the small-grid family switched off / extended to 4x its threshold (process-wide;
 * tools/tile_table.py only).  Lets the tests cover the families on small shapes. */
STA_API int sta_set_gemm_variant(sta_handle* h, int variant);

/* The tile family launch_gemm's cost model picks for a GEMM / convolution (pure host function, no handle, no GPU:
 * tests/test_tile_table.py replays profiles/r03_tile_table.txt through it).  amode: 0 dense, 1 3x3 convolution; epi: 0 f32,
 * 1 f16 planes, 2 qkv, 3 convT, 4 gelu, 5 f32 in-place residual, 6 fused head; M without the pose-token tail rows; split: 1 for
 * the f16x3 / f16x3h precisions; cstride / Ho / Wo: convolutions only (0 otherwise).  Returns 1, 2, 3, 5, 6 or 8
 * (sta_launch.inc: pick_family). */
STA_API int sta_debug_pick_family(int amode, int epi, long long M, int N, int K, int split, int cstride, int Ho, int Wo);

/* Is there a kernel for this loader / epilogue / tile family / arithmetic (pure host function; sta_launch.inc: gemm_has_kernel -
 * what gemm_plan asks before it returns a plan and what launch_gemm's dispatch instantiates by)?  amode, epi as above; family
 * 1 .. 8 (7, the paired launch, is no launch_gemm kernel: 0); mx: f16mx rows and weights; split: 1 for the split precisions;
 * N = Cout and cstride decide for the halo-tiled family 8 and the fused head only.  Returns 1 or 0. */
STA_API int sta_debug_gemm_has_kernel(int amode, int epi, int family, int mx, int split, int N, int cstride);

/* The launch plan of a dense GEMM / convolution (pure host function, no handle, no GPU; sta_launch.inc: gemm_plan, what
 * launch_gemm runs): tile family after the forced-family mapping and the f16mx remaps, its tile, the pose-token row tail the
 * skinny tail blocks compute, and the K slices.  M_all: every row, tail rows included; precision: STA_PREC_*; mx: f16mx rows and
 * weights (what use_mx() decides); tail_hint: the decoder's pose-token rows (0: none); forced_variant: as sta_set_gemm_variant
 * (0..4, 8, 9).  out[8] = {family, bm, bn, m_tail, tiles_m, tiles_n, ksplit, slab_ks}; the main tiles cover rows
 * [0, M_all - m_tail).  Fails when the plan would name a kernel that does not exist.  epi 5 below the small-grid predicate (where the
 * product never launches that epilogue): the plan of gemm_resid_ln's launch there - the fp32 epilogue in place with the handle's
 * slab, slab_ks > 1 when its K slices are left to resid_ln_kernel (N % 64 == 0, N <= 1024, forced_variant 0 or 9).
 * Refused as well: a (loader, epilogue) pair launch_gemm is not built for - amode 1 with an epilogue other than 1 / 6, amode 0 with
 * epilogue 6 (sta_debug_gemm_has_kernel says 0 for every family). */
STA_API int sta_debug_gemm_plan(int amode, int epi, int M_all, int N, int K, int precision, int mx, int tail_hint, int forced_variant, int* out);

/* The launch plan of a 3x3 convolution (pure host function: gemm_plan with the implicit-GEMM loader and the image geometry, so
 * that the halo-tiled family 8 is a candidate).  epi: 1 plane epilogue, 6 fused DPT tail; M = images x Ho x Wo output pixels,
 * N = Cout, K = 9 Cin; cstride 1 | 2; head_gemm: experiment switch 0 (the fused tail as an implicit GEMM from 2^21 pixels on).
 * out[8] as sta_debug_gemm_plan; family 8: bm = 256 = 8 rows x 32 pixels of one image, tiles_m = images x ceil(Ho / 8) x
 * ceil(Wo / 32). */
STA_API int sta_debug_conv_plan(int epi, int M, int N, int K, int precision, int mx, int forced_variant, int cstride, int Ho, int Wo,
                        int head_gemm, int* out);

/* The same record for the handle's LAST launch_gemm or paired QKV launch (family 7, bm x bn = 192 x 128, tiles_n = both halves'
 * column tiles). */
STA_API int sta_debug_last_gemm_plan(sta_handle* h, int* out);

/* The paired QKV launch's decision (pure host function): out[2] = {1: one launch (gemm2_pair_kernel) / 0: two, m_tail of both
 * halves}.  Both halves have M rows and the same K; N_a / N_b their widths, mx_a / mx_b their arithmetic. */
STA_API int sta_debug_qkv_pair_plan(int precision, int M, int N_a, int N_b, int K, int mx_a, int mx_b, int tail_hint, int forced_variant, int* out);

/* The decoder's attn.qkv + cross_attn.projk|projv pair through gemm_qkv_pair, pose-token tail hint S.  x_a, x_b [S*ntok + S, K]
 * in the decoder's row order (patch rows sequence-major, then the S pose rows); w_a [3C,K] (q|k|v), w_b [2C,K] (k|v).  q_a, k_a,
 * k_b out [S,C/64,ntok+1,64] with the pose token last; vt_a, vt_b out [S*C/64*64, roundup(ntok+1,64)] (transposed V, zero
 * padding).  ntok % wp == 0 (the patch grid is ntok/wp x wp). */
STA_API int sta_debug_qkv_pair(sta_handle* h, const float* x_a, const float* w_a, const float* bias_a, const float* x_b,
                       const float* w_b, const float* bias_b, int S, int ntok, int K, int C, int wp,
                       float* q_a, float* k_a, float* vt_a, float* k_b, float* vt_b, void* stream);

/* nn.Linear (+GELU/ReLU, +residual): out[M,N] = act(A[M,K] W[N,K]^T + bias) (+resid).
 * act: 0 none, 1 erf-GELU, 2 ReLU.  via_f16 != 0 uses the fp16-plane epilogue (sta_blocks.py:73-79). */
STA_API int sta_debug_gemm(sta_handle* h, const float* A, const float* W, const float* bias, int M, int N, int K,
                   int act, int via_f16, const float* resid, float* out, void* stream);

/* qkv = Linear(x); RoPE2D(q), RoPE2D(k) (sta_blocks.py:132-138, pos_embed.py:169-185).
 * x [S*ntok,K], W [3C,K]; q,k out [S,C/64,ntok,64]; v out is the TRANSPOSED buffer
 * [S*C/64*64, roundup(ntok,64)] exactly as the attention kernel consumes it.
 * has_pose_tok: 0 none, 1 = token 0 of every sequence (reference order), 2 = the decoder's row order: x = [S*ntok patch rows |
 * S pose rows], outputs hold ntok + 1 tokens per sequence with the pose token last (roundup(ntok + 1, 64) columns of V^T). */
STA_API int sta_debug_qkv_rope(sta_handle* h, const float* x, const float* W, const float* bias, int S, int ntok, int K, int C,
                       int wp, int has_pose_tok, float* q, float* k, float* v, void* stream);

/* softmax(q k^T / 8) v, K/V taken from sequence (s+kv_shift)%S (sta_blocks.py:143,201-205).
 * q [S,heads,nq,64], k,v [S,heads,nk,64] -> out [S,nq,heads*64]. */
STA_API int sta_debug_attention(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads,
                        int nq, int nk, int kv_shift, float* out, void* stream);

/* The decoder form of the same kernel: q, k, v [S,heads,n+1,64] with the pose token LAST (as a key it is folded into the
 * initial softmax state, as a query it is served by the pose blocks) -> out [S*n + S, heads*64] in the decoder's row order
 * (patch rows sequence-major, then the S pose rows).  sta_blocks.py:129-148,201-205 on n + 1 tokens. */
STA_API int sta_debug_attention_pose(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads,
                             int n, int kv_shift, float* out, void* stream);

/* Both attention entries fill, before they pack their inputs, the output planes, both planes of the K padding and the Q rows
 * past the last query with 0xFF (fp16 NaN patterns): an output element the kernel did not write, or a padded key or query it
 * read, shows up as NaN.  The V^T padding is zero, as the kernel's contract requires.  sta_debug_conv3x3 / _conv3x3_r2 / _convt /
 * _up2 / _layernorm poison their output planes the same way, sta_debug_conv3_head its four fp32 outputs. */

/* The launch plan of the attention kernel (pure host function, no handle, no GPU; sta_launch.inc: attn_plan, what run_attn
 * runs).  pose: decoder form (token nq == nk is the pose token); split: 1 for the f16x3 precisions; no_prefetch: option 5.
 * out[11] = {pose mode (0 none, 1 side blocks, 2 spare row of the last query block), prefetch (4-stage schedule) flag, LDS
 * stages, LDS bytes, grid, pose blocks, query blocks, ntiles, nfull, tail stage, pose-query scratch bytes}.  tail stage: -1 when
 * nk % 64 == 0; under prefetch the tail tile's index (its LDS stage); in the double-buffered loop tile index & 1. */
STA_API int sta_debug_attn_plan(int S, int heads, int nq, int nk, int pose, int split, int no_prefetch, int* out);

/* Two-group form of the decoder's attention (attention.h: attn_mixed_kernel; the decoder on view pairs of different resolution):
 * S1 sequences of nq_a queries over nk_a keys and S2 sequences of nq_b over nk_b, pose token LAST in every q / k / v
 * ([S, heads, n + 1, 64]).  k / v of a sequence are the keys it reads; the entry stores them at buffer sequence
 * (s + kv_shift) % (S1 + S2).  out [S1*nq_a + S1 + S2*nq_b + S2, heads*64]: per group the patch rows, then the pose rows.
 * Poisons like sta_debug_attention_pose. */
STA_API int sta_debug_attention_mixed(sta_handle* h, const float* q_a, const float* k_a, const float* v_a, const float* q_b,
                                      const float* k_b, const float* v_b, int S1, int S2, int heads, int nq_a, int nk_a,
                                      int nq_b, int nk_b, int kv_shift, float* out, void* stream);
/* Its launch plan (pure host function; sta_launch.inc: attn_mixed_plan): out[20] = {LDS stages, LDS bytes, grid, query-block
 * workgroups of group a, then per group {pose mode, prefetch, pose blocks, query blocks per (sequence, head), ntiles, nfull, tail
 * stage, pose scratch bytes}}; the record of the handle's last two-group launch; and the kernel's workgroup map: out[3*b + 0..2] =
 * (sequence, head, query block) of query-block workgroup b. */
STA_API int sta_debug_attn_mixed_plan(int S1, int S2, int heads, int nq_a, int nk_a, int nq_b, int nk_b, int split, int no_prefetch, int* out);
STA_API int sta_debug_last_attn_mixed_plan(sta_handle* h, int* out);
STA_API int sta_debug_attn_mixed_block_map(int S1, int S2, int heads, int qblocks_a, int qblocks_b, int* out);

/* Per-sequence form of the decoder's attention (attention.h: attn_varlen_kernel; sta_decode_varlen): S <= 32 sequences, sequence s
 * with nq[s] queries over nk[s] keys (HOST arrays).  q: sequence after sequence [heads, nq[s] + 1, 64]; k / v: [heads, nk[s] + 1, 64],
 * pose token LAST.  k / v of a sequence are the keys it reads; the entry stores them at buffer sequence (s + kv_shift) % S.  out
 * [sum(nq[s] + 1) + 64, heads*64]: per sequence its patch rows, then its pose row; the last 64 rows return a guard block that lies
 * directly behind the output planes, every byte 0x3C on entry.  Poisons like sta_debug_attention_pose. */
STA_API int sta_debug_attn_varlen(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads,
                                  const int* nq, const int* nk, int kv_shift, float* out, void* stream);
/* Its launch plan (pure host function; sta_launch.inc: attn_varlen_plan): out[7 + 11*S] = {S, LDS stages, LDS bytes, grid,
 * query-block workgroups, pose blocks, output rows, then per sequence {pose mode, prefetch, pose blocks, query blocks per head,
 * ntiles, nfull, tail stage, pose scratch bytes, first logical query-block id, first pose block, first output row}}; the record of
 * the handle's last per-sequence launch; and the kernel's workgroup map: out[3*b + 0..2] = (sequence, head, query block) of
 * query-block workgroup b. */
STA_API int sta_debug_attn_varlen_plan(int S, int heads, const int* nq, const int* nk, int split, int no_prefetch, int* out);
STA_API int sta_debug_last_attn_varlen_plan(sta_handle* h, int* out);
STA_API int sta_debug_attn_varlen_block_map(int S, int heads, const int* nq, const int* nk, int* out);

/* Encoder form of the per-sequence attention (sta_encode_varlen: attn_varlen_kernel under attn_encv_plan): S <= 32 sequences, sequence s
 * with n[s] queries over its own n[s] keys (HOST array), NO pose token.  q / k / v: sequence after sequence [heads, n[s], 64].  The
 * buffers are the encoder's, npad = roundup(max(n), 64): n[s] may equal npad.  out [sum(n) + 64, heads*64]: the packed rows, then a guard
 * block that lies directly behind the output planes, every byte 0x3C on entry.  Poisons like sta_debug_attn_varlen. */
STA_API int sta_debug_attn_encv(sta_handle* h, const float* q, const float* k, const float* v, int S, int heads, const int* n,
                                float* out, void* stream);
/* Its launch plan (pure host function; sta_launch.inc: attn_encv_plan) in the record of sta_debug_attn_varlen_plan - pose mode, pose
 * blocks, pose scratch and first pose block are 0, output rows are packed n[s] per sequence -; the record of the handle's last such
 * launch; and the kernel's workgroup map: out[3*b + 0..2] = (sequence, head, query block) of query-block workgroup b. */
STA_API int sta_debug_attn_encv_plan(int S, int heads, const int* n, int split, int no_prefetch, int* out);
STA_API int sta_debug_last_attn_encv_plan(sta_handle* h, int* out);
STA_API int sta_debug_attn_encv_block_map(int S, int heads, const int* n, int* out);

/* The QKV finisher of sta_encode_varlen alone (qkv_finish_kernel, VARLEN form): n HOST array [S] of token counts; slab device fp32
 * [sum(n), 3*heads*64] = the q | k | v rows a dense QKV GEMM left; bias device fp32 [3*heads*64] or NULL; pos_i32 device int32
 * [sum(n)*2] of (y, x), packed, clamped to [0, pos_max].  q / k: fp32 [S*heads + 1][npad][64], vt: fp32 [S*heads + 1][64][npad], npad =
 * roundup(max(n), 64) - the encoder's Q / K / V^T layout and ONE guard block behind each; every element (the guards' too) is split to fp16
 * planes inside, the kernel writes the planes and everything is returned as hi + lo.  Rows [n[s], npad) of Q / K, columns [n[s], npad)
 * of V^T (NOT zeroed by this entry) and the guards are not touched. */
STA_API int sta_debug_qkv_finish_varlen(sta_handle* h, const float* slab, const float* bias, const int* pos_i32, int S, int heads,
                                        const int* n, int pos_max, float* q, float* k, float* vt, void* stream);

/* The gather of sta_encode_varlen alone: imgs / H / W / n HOST arrays [B] as in sta_encode_varlen (u8hwc != 0: uint8 HWC frames);
 * pos_i32 device int32 [sum(n)*2] of (y, x), packed, already inside each entry's grid; out fp32 [sum(n), 768] = the patch rows as
 * hi + lo.  which = 0: the varlen form (one launch); 1: sta_encode_tokens' form of the same kernel, one launch per entry. */
STA_API int sta_debug_patch_gather_varlen(sta_handle* h, const void* const* imgs, int u8hwc, const int* H, const int* W,
                                          const int* pos_i32, const int* n, int B, int which, float* out, void* stream);

/* The gather of sta_regress_views_tokens alone (gather_tokens_varlen_kernel): S <= 32 sequences (S even: the first half is side i,
 * the second side j).  srcs [S] device pointers to cached frames [hp[s]*wp[s], E] fp32, 16-byte aligned; hp / wp [S]; win [S][4] =
 * (y0, x0, h, w) in patches, h * w == 0 = index list of cnt[s] tokens; idx_i / idx_j: packed device int64 indices of the index-list
 * sequences of each half, in sequence order (out-of-grid values are clamped).  All arrays but idx_* are HOST arrays.  feat_out fp32
 * [sum(n), E] and pos_out int32 [sum(n), 2] of (y, x): the packed rows in sequence order. */
STA_API int sta_debug_gather_tokens(sta_handle* h, const float* const* srcs, const int* hp, const int* wp, const int* win, const int* cnt,
                                    const int64_t* idx_i, const int64_t* idx_j, int S, int E, float* feat_out, int* pos_out, void* stream);

/* sta_head_pose with the samples named by a HOST row table: sample b (b < k <= 16) is row rows[b] of tok (rows of tok_stride floats).
 * Bit-identical to sta_head_pose on a stacked copy of those rows. */
STA_API int sta_debug_pose_rows(sta_handle* h, const float* tok, int64_t tok_stride, const int64_t* rows, int k, float* pose, float* conf,
                                void* stream);

/* The rotation step of sta_decode_varlen alone (rope_varlen_kernel): n HOST array [S] of token counts.  bufs[b] (nbuf 1..3): fp32
 * [S*heads + 1][npad][64], npad = roundup(max(n) + 1, 64) - the decoder's Q / K layout and ONE guard block behind it; every row (the
 * guard's too) is split to fp16 planes inside, the buffer is rotated IN PLACE and everything is returned as hi + lo.  Token index n[s]
 * of sequence s is its pose token (position -1), rows (n[s], npad) are not touched.  pos_i32: device int32 [sum(n)*2] of (y, x),
 * packed, clamped to [-1, pos_max]. */
STA_API int sta_debug_rope_varlen(sta_handle* h, float* const* bufs, int nbuf, int S, int heads, const int* n, const int* pos_i32,
                                  int pos_max, void* stream);

/* The rotation step of sta_decode_tokens alone: 2-D RoPE from a positions table on nbuf (1..3) head-major buffers for two groups
 * of sequences with different token counts.  bufs[b]: fp32 [S1 + S2][heads][npad][64], npad = roundup(max(ntok_a, ntok_b) + 1, 64);
 * every row is split to fp16 planes inside, rotated IN PLACE and returned as hi + lo.  Sequences [0, S1) hold ntok_a tokens,
 * sequences [S1, S1 + S2) ntok_b; token index ntok of a sequence is its pose token (position -1), rows (ntok, npad) are not
 * touched.  pos_i32: device int32 [S1*ntok_a*2 | S2*ntok_b*2] of (y, x), clamped to [-1, pos_max].  which = 0: rope_tokens_kernel
 * (one launch); which = 1: rope_planes_kernel launched per buffer and per side. */
STA_API int sta_debug_rope_tokens(sta_handle* h, float* const* bufs, int nbuf, int S1, int S2, int heads, int ntok_a, int ntok_b,
                                  const int* pos_i32, int pos_max, int which, void* stream);

/* The rotation step of sta_encode_tokens alone: the encoder's Q / K layout has NO pose row.  bufs[b] (nbuf 1..2): fp32
 * [S*heads + 1][npad][64], npad = roundup(ntok, 64) - the S*heads blocks of the buffer and ONE guard block behind them; every row
 * (the guard's too) is split to fp16 planes inside, the buffer is rotated IN PLACE and everything is returned as hi + lo.  pos_i32:
 * device int32 [S*ntok*2] of (y, x) in [0, pos_max].  pose = 0: the launch of sta_encode_tokens (exactly ntok rows per (sequence,
 * head)); pose = 1: the decoder's pose-row form of the same kernel on the same buffers (ntok + 1 rows: with ntok a multiple of 64 it
 * writes row 0 of the next head and of the guard). */
STA_API int sta_debug_rope_enc_tokens(sta_handle* h, float* const* bufs, int nbuf, int S, int heads, int ntok, const int* pos_i32,
                                      int pos_max, int pose, void* stream);

/* The same record for the handle's LAST attention launch. */
STA_API int sta_debug_last_attn_plan(sta_handle* h, int* out);

/* out[b] = logical (sequence, head, query block) id of query-block workgroup b of a grid of nwg (attention.h: attn_block_map,
 * the function the kernel calls). */
STA_API int sta_debug_attn_block_map(int nwg, int* out);

/* Switches of the tests / tools (0 everywhere = product behaviour; see tools/ab_option.py; settable as STA_OPT<idx> in the
 * environment at sta_create only in -DSTA_BENCH_EXPERIMENTS builds).  idx 4 = 1: sta_debug_gemm (plane epilogue) / conv3x3 /
 * convt / up2 run in the DPT head's f16mx arithmetic (f16mx rows in and out, f16mx weights) when the handle's precision is
 * f16x3h - the kernels that precision uses inside the head.  A/B switches of round-4 choices: 1 = 1 small-grid K slices by the
 * old rule; 2 = 1 small-grid GEMMs always on 4 waves; 5 = 1 attention without the 4-stage prefetch schedule; 6 = 1 no side
 * lanes (2: always); 7 = 1 bilinear one output row per workgroup; 3 = 1 sta_decode_tokens rotates Q / K by per-buffer
 * rope_planes_kernel launches (one per buffer and side: eight per decoder layer) instead of the two rope_tokens_kernel launches;
 * 8 = 1 sta_encode_varlen runs its QKV GEMM once per sequence with the fused epilogue plus one no-pose rope_varlen_kernel launch per
 * layer (sta_decode_varlen's way) instead of one dense GEMM and the varlen finisher. */
STA_API int sta_debug_set_option(sta_handle* h, int idx, int value);

/* Row-tail hint for the dense GEMMs (what the decoder sets to its 2B pose-token rows): the last `rows` (<= 32) rows of the
 * following sta_debug_gemm calls are computed by skinny tail blocks when the shape qualifies.  Sticky; 0 resets. */
STA_API int sta_debug_set_tail_hint(sta_handle* h, int rows);

/* nn.Conv2d 3x3 pad 1 stride 1|2 on NHWC data, weights in the reference [Co,Cin,3,3] layout;
 * optional ReLU on the input, activation on the output, residual add (dpt_block.py:94-142). */
STA_API int sta_debug_conv3x3(sta_handle* h, const float* x, const float* w, const float* bias, int n, int H, int W, int Cin, int Co,
                      int stride, int relu_in, int act, const float* resid, float* out, void* stream);

/* The same with the second residual of the refinenet fusion (out = act(conv) + resid + resid2; resid2 only with resid). */
STA_API int sta_debug_conv3x3_r2(sta_handle* h, const float* x, const float* w, const float* bias, int n, int H, int W, int Cin, int Co,
                         int stride, int relu_in, int act, const float* resid, const float* resid2, float* out, void* stream);

/* The fused DPT tail as ONE kernel (dpt_block.py:316-324 + postprocess.py:10-62): head.2 (3x3, 128 -> 128) + ReLU + head.4 (1x1,
 * 128 -> 4) + point-map / confidence activations on x NHWC [n,H,W,128].  w2 [128,128,3,3], b2 [128], w4 [4,128], b4 [4]; head.4's
 * rows are scaled by powers of two exactly as sta_finalize_weights does.  Images [0, nA) -> ptsA [nA,H,W,3], confA [nA,H,W]; the
 * rest -> ptsB, confB (an empty side may be NULL); all four are filled with 0xFF first.  Runs the halo form under forced family 8
 * and, above the small-grid predicate (>= 36673 pixels), what the cost model picks under 0 / the implicit-GEMM form under 9; FAILS
 * where the product would take the unfused path. */
STA_API int sta_debug_conv3_head(sta_handle* h, const float* x, const float* w2, const float* b2, const float* w4, const float* b4,
                         int n, int H, int W, int nA, float* ptsA, float* confA, float* ptsB, float* confB, void* stream);

/* nn.ConvTranspose2d kernel=stride=k on NHWC data, weights [C,C,k,k] (dpt_block.py:369-390). */
STA_API int sta_debug_convt(sta_handle* h, const float* x, const float* w, const float* bias, int n, int H, int W, int C, int k,
                    float* out, void* stream);

/* F.interpolate(scale_factor=2, bilinear, align_corners=True), NHWC, cropped to Hc x Wc. */
STA_API int sta_debug_up2(sta_handle* h, const float* x, int n, int H, int W, int C, int Hc, int Wc, float* out, void* stream);

/* nn.LayerNorm(eps) rows; out32 = direct fp32 output, out_planes = value carried by the fp16 planes. */
STA_API int sta_debug_layernorm(sta_handle* h, const float* x, const float* g, const float* b, int M, int C, float eps,
                        float* out32, float* out_planes, void* stream);

/* The residual stream step of a transformer layer as the forward pass issues it (sta_launch.inc: gemm_resid_ln; sta_blocks.py:
 * x = x + proj(...) followed by the next norm): x[M,N] += A[M,K] W[N,K]^T + bias IN PLACE, then up to two LayerNorm(eps) affine
 * sets of the new x into fp16 planes.  g1 == NULL: only the add; g2 == NULL: one set (g2 only with g1).  Below the small-grid
 * predicate the K slices go to the handle's own slab buffer and resid_ln_kernel sums them before it normalises; above it the
 * in-place GEMM is followed by ln_kernel.  Which ran: sta_debug_last_gemm_plan (slab_ks > 1).  out1 / out2 (may be NULL): the
 * values carried by the two plane sets, fp32 [M,N]; both sets are filled with 0xFF before the call, so a set that must not be
 * written reads back as NaN.  N % 4 == 0, N <= 1024, K % 32 == 0. */
STA_API int sta_debug_gemm_resid_ln(sta_handle* h, const float* A, const float* W, const float* bias, float* x, int M, int N, int K,
                            const float* g1, const float* b1, const float* g2, const float* b2, float eps,
                            float* out1, float* out2, void* stream);

/* head.4 (1x1 128->4) + postprocess (postprocess.py:10-62) on [npix,128] features. */
STA_API int sta_debug_head_final(sta_handle* h, const float* x, const float* w, const float* bias, int64_t npix,
                         float* pts, float* conf, void* stream);

/* PoseHead_small.svd_orthogonalize (pose_head.py:38-57) of B row-major 3x3 matrices. */
STA_API int sta_debug_svd_orthogonalize(sta_handle* h, const float* m, float* r, int B, void* stream);

/* Per-launch record of the timed dominant-kernel family since sta_kernel_timing(h, 1): algorithmic FLOPs, HIP-event
 * duration (ms) and tile family of up to `cap` launches (superseded by sta_kernel_timing_dump_shapes, sta_mi355.h). */
STA_API int sta_kernel_timing_dump(sta_handle* h, int cap, double* flops, float* ms, int* variant, int* n_out);

/* In-kernel stamps of EVERY GEMM / convolution launch of the calls made since sta_kernel_timing(h, 4) (= mode 2 + stamps; the
 * first 512 launches, 2048 workgroups each): per launch out6 = {workgroups, span, median entry -> first K tile, median main loop,
 * median epilogue, spread of the exits} in us; pairs with sta_kernel_timing_dump_shapes (same launch order). */
STA_API int sta_kernel_stamps_dump(sta_handle* h, int cap, double* out6, int* n_out);

/* In-kernel timeline of ONE launch of the product's GEMM for M x N x K (tools/gemm_stamps.py): every workgroup stores four
 * 100 MHz stamps (entry, first K tile landed, main loop done, epilogue acknowledged).  resid != 0: the in-place residual form
 * (at SLAM scale: K slices to slabs).  out[10] (us): workgroups, kernel span (first entry -> last exit), median entry -> first
 * tile, median main loop, median epilogue, spread of the entries, spread of the exits, HIP-event duration of the same launch,
 * K slices, median lifetime of a workgroup.  resid == 2: the specialised in-place residual epilogue of the throughput families.
 * raw_host (may be NULL): the four stamps of the first raw_cap workgroups (block id order; block b runs on XCD b % 8). */
STA_API int sta_bench_gemm_stamps(sta_handle* h, int M, int N, int K, int resid, double* out, unsigned long long* raw_host, int raw_cap, void* stream);

/* Time `iters` back-to-back launches of the dominant GEMM kernel (M x N x K, this handle's
 * precision, random operands) with hipEvents on `stream`; average ms per launch in *ms_out.
 * tile: 0 = product selection, 1 = 128x128, 2 = 256x256, 3 = 256x128.  ablation (tile 2/3 only,
 * bench-only kernel variants): 0 none, 1 no DMA in the K loop, 2 DMA+barriers only, 3 MFMA only. */
STA_API int sta_bench_gemm(sta_handle* h, int M, int N, int K, int iters, int tile, int ablation, float* ms_out, void* stream);
/* Effective shader clock (GHz) observed inside the kernel of the last sta_bench_gemm call (s_memtime cycles per
 * 100 MHz s_memrealtime tick, sampled on every 64th workgroup): the chip clocks to its power budget (DVFS). */
STA_API float sta_bench_gemm_last_ghz(void);
/* The attention kernel alone on random operands (tools): ms per launch over `iters` back-to-back launches.  pose != 0: the
 * decoder form (nq == nk patch tokens + the pose token).  which: reserved for kernel variants under test, pass 0. */
STA_API int sta_bench_attention(sta_handle* h, int S, int heads, int nq, int nk, int pose, int iters, int which, float* ms_out, void* stream);
/* The two-group launch alone (attn_mixed_kernel, see sta_debug_attention_mixed for the arguments): ms per launch. */
STA_API int sta_bench_attention_mixed(sta_handle* h, int S1, int S2, int heads, int nq_a, int nk_a, int nq_b, int nk_b, int kv_shift,
                                      int iters, float* ms_out, void* stream);

/* The varlen DPT head (sta_head_pts_varlen), kernel by kernel: B <= 32 entries of different size in ONE launch, inputs and outputs
 * packed entry-major (entry b: H[b] x W[b] pixels, NHWC fp32).  H / W / Hc / Wc: HOST arrays.  Arguments otherwise as
 * sta_debug_conv3x3_r2 / _conv3_head / _convt / _up2.  guard (device, 4096 bytes, may be NULL) receives the 4096 bytes that start at the
 * byte behind the output planes' last row, filled with 0xA5 before the launch.  Precision f16 is refused.  sta_debug_conv3_head_varlen: the fused tail as an
 * implicit GEMM on 192x128 tiles, or the halo form under forced family 8; fails on a small grid (fewer than 192 tiles) and under
 * another forced family, as the head itself falls back to conv + head_final there. */
STA_API int sta_debug_conv3x3_varlen(sta_handle* h, const float* x, const float* w, const float* bias, int B, const int* H, const int* W,
                                     int Cin, int Co, int stride, int relu_in, int act, const float* resid, const float* resid2,
                                     float* out, void* guard, void* stream);
STA_API int sta_debug_conv3_head_varlen(sta_handle* h, const float* x, const float* w2, const float* b2, const float* w4, const float* b4,
                                        int B, const int* H, const int* W, float* pts, float* conf, void* stream);
STA_API int sta_debug_convt_varlen(sta_handle* h, const float* x, const float* w, const float* bias, int B, const int* H, const int* W,
                                   int C, int k, float* out, void* guard, void* stream);
STA_API int sta_debug_up2_varlen(sta_handle* h, const float* x, int B, const int* H, const int* W, int C, const int* Hc, const int* Wc,
                                 float* out, void* guard, void* stream);
/* Host only: the packing of the varlen head's six levels - level 0 .. 5 = (ceil(h/2), ceil(w/2)), (h, w), (2h, 2w), (4h, 4w), (8h, 8w),
 * (16h, 16w).  off [6][B + 1]: first packed pixel of every entry, then the level's size; hw [6][B][2]: the entry's (rows, columns).
 * ntiles [6], tiles [cap][3] (both may be NULL): the tile map of the halo-tiled convolution at every level, level after level: tile ->
 * (entry, y0, x0), tiles of 8 rows x 32 pixels of one entry, decoded by the function the kernel uses; -1 when cap is too small. */
STA_API int sta_debug_dpt_varlen_plan(int B, const int* hp, const int* wp, long long* off, int* hw, int* ntiles, int* tiles, int cap);

/* Workspace independence (tests/test_workspace_gpu.py).  The product entry points run on whatever the previous call on the stream left
 * in its scratch context (workspace, the two split-K scratches, the side lane's scratch); their outputs must not depend on it.
 * sta_debug_workspace_fill: enqueue `byte` (0 .. 255) over ALL of that scratch on `stream`; -1 when the stream has no context yet or a
 * split-phase scheduler call (sta_regress_views[_tokens]_begin) is pending on it.
 * sta_debug_workspace_info: out[0] workspace capacity, out[1] the planned peak of the last call on the context, out[2] / [3] / [4] bytes
 * of the split-K scratch, the slab scratch and the side lane's scratch (0: not allocated), out[5] 1 while a split-phase call is
 * pending, out[6], out[7] 0.
 * sta_debug_workspace_tail: the bytes of workspace [planned peak + 4096, capacity) that differ from `byte`: their number and the
 * offset of the first (-1: none).  Runs on `stream` and synchronises it; touches nothing inside the workspace. */
STA_API int sta_debug_workspace_fill(sta_handle* h, void* stream, int byte);
STA_API int sta_debug_workspace_info(sta_handle* h, void* stream, int64_t out[8]);
STA_API int sta_debug_workspace_tail(sta_handle* h, void* stream, int byte, int64_t* n_bad, int64_t* first_bad);

#ifdef STA_WAVE_SKEW
#include "sta_mi355_skew.h"      /* two more entries, of libsta_mi355_skew.so alone (the wave-skew schedule tests) */
#endif

#ifdef __cplusplus
}
#endif
#endif
