/*
 * sta_mi355.h - C ABI of the MI355X-native Symmetric Two-view Association (STA) frontend.
 *
 * Drop-in boundary for ONE hot path of ViSTA-SLAM: the STA forward pass.  Every entry point
 * below replaces a Python method of the reference `SymmetricTwoViewAssociation`
 * (vista_slam/sta_model/sta_model.py) or its only native sub-boundary (curope):
 *
 *   sta_create / sta_load_tensor / sta_finalize_weights
 *        <- STA() + load_state_dict(ckpt['model'], strict=True) + .to(device).eval()
 *           (vista_slam/slam.py:95-106).  Tensor names == reference state_dict keys.
 *   sta_encode        <- _encode_image(image, true_shape, normalize=False)   (sta_encode_tokens: on a token subset)
 *                        (sta_model.py:163-174, called from slam.py:144)
 *   sta_decode        <- _decode_stereo(feat1, feat2, pos1, pos2)   (positions = the patch grid; sta_decode_pos: any positions)
 *                        (sta_model.py:177-244, called from slam.py:162; N1 != N2 tokens: sta_decode_mixed on two patch
 *                        grids, sta_decode_tokens on token subsets with any positions, sta_decode_varlen with one token count per batch entry)
 *   sta_head_pose     <- head_pose_s(tok[:,0,:])        (heads/pose_head.py:109-120, slam.py:165)
 *   sta_head_pts      <- head_pts(list14, true_shape)   (heads/dpt_head.py:34-66 +
 *                        heads/postprocess.py:10-62 + utils/misc.py:36-78, slam.py:179-180)
 *   sta_forward_pair  <- forward({'main_view','neighbor_views':[b],'loop_views':[]})
 *                        (sta_model.py:247-291)
 *   sta_rope2d_inplace<- curope.rope_2d(tokens, positions, base, fwd)
 *                        (pos_embed/curope/curope.cpp:49-65, kernels.cu:84-108)
 *
 * Conventions
 *   - Plain C types only.  All *_dev pointers are device (HBM) pointers owned by the caller
 *     (the Python shim passes torch-ROCm tensor .data_ptr()).  The library owns only weights
 *     and an internal workspace per caller stream; a workspace grows on the first call of a new shape
 *     and is then reused (no allocation in steady state).
 *   - All work is enqueued on the caller-supplied hipStream_t (`stream`, passed as void*);
 *     no host synchronisation inside, so ordering with surrounding torch ops is preserved.
 *   - Return value: 0 on success, negative on error; sta_last_error() returns a thread-local
 *     message.  A handle is not thread-safe (one host thread at a time; several STREAMS are fine, see
 *     "Streams and concurrency" below); one handle per device.
 *   - Images are NCHW fp32 in [-1,1]; H and W must be multiples of 16.  Portrait frames (H > W) are tokenised row-major
 *     as they are (PatchEmbedDust3R, patch_embed.py:15-26) and every per-pixel output of this ABI is in IMAGE orientation
 *     [.., H, W, ..].  The reference's head wrapper returns portrait outputs as transposed VIEWS of exactly that memory
 *     (`transposed(head(decout, (H, W)))`, utils/misc.py:60-61,81); the Python shim applies the same swapaxes(1, 2), and
 *     sta_regress_views evaluates the shared intrinsics the way the reference does on those views (see there).
 *   - Token tensors are row-major fp32: encoder [B, N, enc_dim], decoder [B, N+1, dec_dim]
 *     (row 0 of every decoder sequence is the pose token, sta_model.py:206-219).
 */
#ifndef STA_MI355_H
#define STA_MI355_H

#include <stdint.h>

/* Every entry point carries STA_API = default ELF visibility; the library itself is compiled with -fvisibility=hidden, so its
 * dynamic symbol table is these declarations and nothing else (no kernel launch stubs, no helper functions:
 * tests/test_cabi_symbols.py compares `nm -D` with this header). */
#ifndef STA_API
#define STA_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sta_handle sta_handle;

/* Arithmetic policy of every GEMM / attention contraction (fp32 accumulate always).
 * gfx950 has no TF32/XF32 MFMA (the reference runs TF32: sta_model.py:5). */
enum {
    STA_PREC_F16   = 1,  /* fp16 x fp16 -> fp32 MFMA, one product  (10-bit mantissa == TF32 class) */
    STA_PREC_F16X3 = 3,  /* 2-term fp16 split of both operands, 3 products (~21-bit, fp32 class)   */
    /* (4 was STA_PREC_F16MX, rounds 1-2: every linear / convolution with its two correction products as ONE block-scaled fp8
     *  MFMA.  +10 % but above the 1e-3 bar on five of the ten stress goldens; retired in round 3, the value is rejected.) */
    STA_PREC_F16X3H = 5, /* f16x3 in the transformer (encoder, decoder, attention, embeddings, pose head); the DPT
                          * head's convolutions in the f16mx arithmetic: fp16 main product + ONE block-scaled fp8 MFMA that
                          * carries both correction products (activation bytes e5m2, weight bytes e4m3: GEMM error ~2e-5, 2 instead of 3 MFMA
                          * units).  The head is
                          * feed-forward and is not followed by any attention layer, so that error is not amplified */
    STA_PREC_F16X3M = 6  /* f16x3h + mlp.fc2 of both transformers in the f16mx arithmetic (mlp.fc1's GELU epilogue writes the
                          * f16mx rows).  Whether this or F16X3H is the default is decided by the written rule of DESIGN.md
                          * section 2 ("a layer class ships in f16mx iff ...") on the measured precision table, not by taste */
};

enum { STA_DTYPE_F32 = 0, STA_DTYPE_F16 = 1, STA_DTYPE_F64 = 2 };   /* weights: F32 only; sta_rope2d_inplace_dtype: all three */

typedef struct sta_config {
    int32_t patch_size;     /* 16 */
    int32_t enc_embed_dim;  /* 1024 */
    int32_t enc_depth;      /* 24 */
    int32_t enc_num_heads;  /* 16  (head_dim must be 64) */
    int32_t dec_embed_dim;  /* 768 */
    int32_t dec_depth;      /* 12  (> 9, heads/dpt_head.py:102) */
    int32_t dec_num_heads;  /* 12 */
    int32_t mlp_ratio;      /* 4 */
    float   rope_base;      /* 100.0 ('RoPE100', sta_model.py:44) */
    float   ln_eps;         /* 1e-6  (sta_model.py:43) */
    int32_t precision;      /* STA_PREC_* */
} sta_config;

/* Fill `cfg` with the reference constructor defaults (sta_model.py:33-52). */
STA_API void sta_default_config(sta_config* cfg);

STA_API int sta_create(const sta_config* cfg, int device, sta_handle** out);
STA_API int sta_destroy(sta_handle* h);

/* Change the arithmetic policy after creation (weights hold both split planes). */
STA_API int sta_set_precision(sta_handle* h, int precision);

/* Bit-reproducible mode.  At SLAM scale (a few hundred rows) the GEMMs and the low-resolution DPT convolutions split K
 * over workgroups.  Since round 2 every product path combines the slices in a FIXED order (each slice stores its partial
 * tile to its own fp32 slab; resid_ln_kernel / qkv_finish_kernel / splitk_finish_kernel sum them), so repeated runs of the
 * same binary give identical bits by default.  One fp32-atomics split-K form is left (in-place residual GEMMs reached
 * outside the fused GEMM + LayerNorm call, e.g. with a forced tile family): on != 0 disables it, at no cost on the product
 * path.  (Why it matters: a borderline `pose_conf < rel_pose_thres` decision, slam.py:169, must not flip run to run.)
 * Default: off. */
STA_API int sta_set_deterministic(sta_handle* h, int on);

/* Streams and concurrency.  Every call enqueues on the caller's stream; the handle keeps ONE scratch context (workspace +
 * split-K buffers) PER STREAM it has been called on, created on the first call on that stream (at most 8 live contexts: a
 * ninth stream takes over the least recently used one behind a device synchronisation).  Calls on
 * different streams therefore never share scratch memory and may overlap on the GPU - the intended use is the SLAM loop's
 * own independence: sta_encode of keyframe i+1 (add_view, slam.py:142-151, 258) on a second stream under
 * sta_regress_views of keyframe i (slam.py:263-277); at 224x224, batch 1 each of them alone leaves most of the chip idle
 * between its ~200 dependent dispatches.  Host-side the handle is still single-threaded (one call at a time).
 * Inside one call the library forks an internal SIDE stream off the caller's stream for the branches that do not lie on the
 * call's critical chain (DPT head: the reassembly of levels 0-2 under the level-3 / refinenet chain; decoder at SLAM scale:
 * the cross-attention K / V under the self-attention) and joins it back before the call's last kernels: the caller sees
 * ordinary stream order.  Same kernels, bit-identical results.
 * (Rounds 2-3 had sta_set_concurrency(h, n): batch slices of ONE forward on library-owned streams.  It stopped paying once
 * the epilogues no longer serialised - -1 % at the headline configuration in round 3 - and was removed in round 4.)
 *
 * sta_set_side_lanes: the application's switch for those internal side streams.  STA_LANES_AUTO (default): on, EXCEPT while
 * the application itself overlaps calls on several streams (another scratch context of this handle was used within its last 8
 * context switches: the chip is then filled across calls and more streams only compete for the runtime's few hardware queues),
 * and except when GPU_MAX_HW_QUEUES is set in the environment (the lanes are tuned for the runtime's default of 4).
 * STA_LANES_OFF / STA_LANES_ON make the schedule independent of either.  Results are bit-identical in all three. */
/* sta_reserve: everything calls of at most these sizes will need on these streams, allocated NOW (no hidden allocation
 * per call).  Without it the library sizes itself lazily - the first call on a new stream creates that stream's scratch context
 * (2 x 16 MiB of split-K scratch; later the side lane's stream, events and 16 MiB), the first call of a larger shape re-allocates
 * the stream's workspace behind a hipDeviceSynchronize, the first scheduler call creates its pinned confidence buffer, a larger
 * patch grid rebuilds the RoPE table.  sta_reserve runs the planning pass of the entry points (the same orchestration code, dry:
 * nothing is launched) and allocates the maximum:
 *   B > 0:          sta_forward_pair[_u8hwc] / sta_encode[_u8hwc] / sta_decode / sta_head_pose / sta_head_pts with batch <= B and
 *                   sta_estimate_intrinsics over <= 2 B maps, frames of H x W;
 *   max_edges > 0:  sta_regress_views[_begin / _finish] with k <= max_edges candidate edges and sta_encode of one H x W frame;
 *   streams[0 .. n_streams): the caller streams the calls will be enqueued on (NULL = the null stream), at most 8 per handle.
 * Afterwards such calls neither allocate nor synchronise the device; sta_alloc_stats proves it: out[0] = device / pinned
 * allocations, frees and stream / event creations, out[1] = device-wide synchronisations the compute entry points have made
 * since sta_create (weight loading, sta_range_report, sta_destroy and the timing tools are not compute entry points).  Not covered
 * (their sizes depend on other arguments): sta_preprocess_frame (tables per source geometry: the first frame of a geometry
 * allocates and synchronises), sta_world_pointcloud (workspace per view count), sta_voxel_downsample (workspace per point count; it
 * synchronises its stream twice like sta_world_pointcloud does once), sta_decode_pos (its RoPE table grows with pos_max and
 * its plan holds the positions table on top of sta_decode's), sta_decode_mixed / sta_decode_tokens (plans per pair of token counts), sta_decode_varlen (a plan per set of counts), sta_encode_tokens[_u8hwc] (a plan per token count),
 * sta_encode_varlen[_u8hwc] (a plan per set of counts; its RoPE table grows with the largest patch grid of a call),
 * sta_regress_views_tokens[_begin] (a plan per set of selections and frame sizes, both phases in it; its RoPE table likewise),
 * sta_view_consistency (pair matrices per view count and window),
 * sta_symmetric_geo_mask (error plane per edge count), sta_geo_valid_mask (error plane per batch) and sta_local_pointclouds /
 * sta_ray_depth (one K^-1 per view). */
STA_API int sta_reserve(sta_handle* h, int B, int H, int W, int max_edges, void* const* streams, int n_streams);
STA_API int sta_alloc_stats(const sta_handle* h, int64_t out[2]);

/* sta_pipeline_streams: n (<= 4) library-owned non-blocking streams that were MEASURED to overlap pairwise on this device.
 * The runtime maps streams onto a few hardware queues and two streams on one queue serialise - which streams those are is not
 * visible through the HIP API (round 4: the same three application streams were reproducibly 20 % slower or faster) - so the
 * library probes: a kernel that spins ~200 us on one stream, a stamp kernel on the other, overlap iff the second started before
 * the first ended; candidates are kept when they overlap every stream kept so far.  The streams belong to the handle: the FIRST
 * call creates and probes all four (a few ms) whatever n is, every later call returns a prefix of the same list - a stream that
 * was handed out stays valid until sta_destroy -, and a failure while probing leaves nothing behind (the next call starts
 * over).  They are meant for the application's lanes: add_view of keyframe i+1 | edges
 * of keyframe i | heads of keyframe i-1 (vista_slam_amd.keyframe_pipeline).  *n_verified_out (may be NULL): how many of the n
 * are verified mutually concurrent (n unless the runtime has fewer usable queues). */
STA_API int sta_pipeline_streams(sta_handle* h, int n, void** streams_out, int* n_verified_out);

#define STA_LANES_AUTO (-1)
#define STA_LANES_OFF 0
#define STA_LANES_ON 1
STA_API int sta_set_side_lanes(sta_handle* h, int mode);

/* sta_set_varlen_heads: how sta_regress_views_tokens / sta_regress_views_tokens_finish run the DPT head, read when the heads are
 * enqueued (at finish time).  The call's workspace is planned at begin time, for the varlen pass only when the switch is on THEN: a
 * caller who never sets it plans and allocates exactly what it did before.  Set it before begin; switching it on between begin and
 * finish makes finish fail with a message (the call is over, the stream serves the next one), switching it off there is served.  0 (default): once per accepted edge and window side (one call for the two sides of an edge whose sides
 * share a shape), as before.  1: the window sides of ALL accepted edges through ONE sta_head_pts_varlen pass that writes straight into
 * the pts / conf layout those entry points define; ranges of rejected edges stay unwritten, the per-edge reductions (depth, the shared
 * K of same-shape pairs) stay per edge.  Same decisions; maps within 1e-4 of mode 0 (tests/test_regress_tokens_varlen_gpu.py).  The three
 * scheduler signatures do not change. */
STA_API int sta_set_varlen_heads(sta_handle* h, int on);

/* Range report.  Activations travel between kernels as fp16 planes (hi + residual), the f16mx arithmetic of the DPT head adds
 * fp8 correction bytes (activations e5m2, weights e4m3): values beyond +-65504 (or NaN) SATURATE when they are written to a
 * plane, activation correction bytes saturate at +-57344, weight bytes at |w| > 28 (the result then degrades towards
 * single-fp16 accuracy for those elements).  Neither can be seen in the outputs, so the writers of every
 * tensor that is NOT a function of a LayerNorm output count them - the input and hook conversions, every plane of the DPT head
 * (which has no normalisation layers: convolutions, transposed convolutions, bilinear), the split-K finishers - and the
 * LayerNorm kernels count non-finite rows of the residual streams: counts[0] = fp16-range events, counts[1] = fp8
 * saturations of THIS handle's calls since the last reset (events = (lane, tile) pairs with at least one such value; the
 * counters live in the handle since round 4 - two handles on one GPU no longer see each other's events; the call
 * synchronises the device).  QKV / attention / mlp.fc1 outputs
 * are bounded by their LayerNorm inputs and are not counted (0.7 % of the step if they were).  A non-zero counts[0] means the
 * forward left the range the parity goldens cover - the reference (fp32) has no such limit.  reset != 0 clears them.
 * counts[0] also includes, permanently, the number of loaded MFMA-operand weight tensors whose EVERY value is below 2^-12 in
 * magnitude (not all zero): such a tensor would enter the matrix pipe as fp16 subnormals (the LOW end of the range). */
STA_API int sta_range_report(sta_handle* h, unsigned long long counts[2], int reset);

/* Number of state_dict entries the handle expects / has received so far. */
STA_API int sta_num_expected_tensors(const sta_handle* h);
STA_API int sta_num_loaded_tensors(const sta_handle* h);

/* Copy one state_dict entry from HOST memory.  `name` is the reference key
 * (e.g. "enc_blocks.3.attn.qkv.weight"); shape must match exactly; unknown names fail
 * (strict=True semantics).  Aliased keys (scratch.layerK_rn / scratch.layer_rn.{K-1}) and the
 * never-executed tensors (enc_norm.*, refinenet4.resConfUnit1.*) are accepted and dropped. */
STA_API int sta_load_tensor(sta_handle* h, const char* name, const void* host_ptr,
                    const int64_t* shape, int ndim, int dtype);

/* Verify every expected tensor arrived (strict) and build the packed fp16 hi/lo planes. */
STA_API int sta_finalize_weights(sta_handle* h);

/* img_dev [B,3,H,W] -> feat_dev [B, N, enc_dim], N = (H/16)*(W/16); no final norm. */
STA_API int sta_encode(sta_handle* h, const float* img_dev, int B, int H, int W,
               float* feat_dev, void* stream);

/* _encode_image(normalize=False) on a TOKEN SUBSET: the encoder counterpart of sta_decode_tokens.  Only the N selected patches of
 * every image are read, embedded and run through the encoder blocks, attending to each other only - what the reference's module code
 * computes for them (patch_embed, gather, then every Block with the gathered positions: sta_model.py:163-174; Block / XFormer_Attention
 * take any token count and rotate q / k by the positions they are handed, sta_blocks.py:129-148,166-169).  It is NOT a slice of
 * sta_encode's output: the tokens left out are not attended to.  img_dev [B,3,H,W] fp32; pos device int64 [B, N, 2] of (y, x) in
 * [0, H/16) x [0, W/16), every batch entry its own, any order, repeats allowed: a position names both the patch that is gathered and
 * the RoPE position of the token.  Values outside the grid are clamped into it (y and x separately; the shim refuses them before the
 * call).  feat_dev [B, N, enc_dim], no final norm, exactly as sta_encode.  Implementation: a gather driven by the positions table,
 * sta_encode's GEMM chain on B*N rows with the identity table in the QKV epilogues, and one launch per layer that rotates the Q and K
 * buffers from the table.  Like sta_decode_mixed / sta_decode_tokens the call runs on one lane and is NOT covered by sta_reserve: the
 * first call of a shape allocates.  Stage and kernel timing see it as they see sta_encode.  Returns -1 with a message for null
 * pointers, N < 1, H / W not multiples of 16, or 2^31 or more rows. */
STA_API int sta_encode_tokens(sta_handle* h, const float* img_dev, const int64_t* pos, int B, int H, int W, int N,
                      float* feat_dev, void* stream);

/* sta_encode_tokens on a batch whose ENTRIES differ in token count and frame size: the encoder in front of sta_decode_varlen.  Batch
 * entries of the reference's encoder never interact (attention is per sample), so entry b is what sta_encode_tokens computes for that
 * entry alone at B = 1 (patch_embed, the gather, every Block with the gathered positions: sta_model.py:163-174,
 * sta_blocks.py:129-148,166-169); nothing is padded and no token attends to another entry's.
 * imgs / H / W / n: HOST arrays [B] (they size the launches and travel in the kernel arguments: the call copies nothing to the device
 * for them and does not synchronise it).  imgs[b]: device pointer to entry b's own frame, fp32 [3, H[b], W[b]]; n[b] >= 1 its token
 * count.  pos: device int64 [sum(n), 2] of (y, x), packed entry-major; entry b's positions live in its own grid H[b]/16 x W[b]/16, any
 * order, repeats allowed, each axis clamped into that grid as in sta_encode_tokens.  feat_dev [sum(n), enc_dim], packed the same way,
 * no final norm.  1 <= B <= 32.
 * Implementation: rows are packed, so the gather, the patch embedding, every LayerNorm, proj, the MLP and the residual epilogues are one
 * launch over all rows.  Per layer the QKV projection is ONE dense GEMM over all rows into an fp32 workspace; a sequence-aware finishing
 * kernel rotates Q / K from the positions table and writes the head-major Q / K / V^T buffers, one sequence after the other; attention
 * is one launch for all sequences, each with its own count and schedule (attn_varlen_kernel, encoder form: no pose token).
 * Like sta_encode_tokens / sta_decode_varlen the call runs on one lane and is NOT covered by sta_reserve: the first call of a set of
 * counts may allocate.  Returns -1 with a message for null pointers, a count below 1, B outside [1, 32], H or W not multiples of 16,
 * or 2^31 or more rows. */
STA_API int sta_encode_varlen(sta_handle* h, const float* const* imgs, const int* H, const int* W, const int64_t* pos, const int* n,
                      int B, float* feat_dev, void* stream);

/* enc_norm (the encoder's final LayerNorm) on `rows` token rows of enc_dim floats: what
 * _encode_image(normalize=True) adds after the blocks (sta_model.py:172-173).  The forward / SLAM paths call
 * _encode_image(normalize=False) (sta_model.py:259,267; slam.py:144), so nothing on the hot path runs this. */
STA_API int sta_encoder_norm(sta_handle* h, const float* feat_dev, int64_t rows, float* out_dev, void* stream);

/* feat1/feat2 [B, N, enc_dim] (N = hp*wp tokens, hp x wp patch grid).
 * out1/out2: arrays of (dec_depth+1) device pointers, each [B, N+1, dec_dim] or NULL to skip
 * that layer.  Index 0 = decoder input (embed + pose token), index i = output of block i,
 * last index has dec_norm applied (sta_model.py:241-242). */
STA_API int sta_decode(sta_handle* h, const float* feat1, const float* feat2, int B, int hp, int wp,
               float* const* out1, float* const* out2, void* stream);

/* _decode_stereo on two views of DIFFERENT resolution: feat1 [B, N1, enc_dim] on an hp1 x wp1 patch grid (N1 = hp1*wp1), feat2
 * [B, N2, enc_dim] on hp2 x wp2 (the reference's module code takes them: cross attention accepts any memory length,
 * sta_blocks.py:193-205).  out1[i] [B, N1+1, dec_dim], out2[i] [B, N2+1, dec_dim]; NULL skips a layer, the last index has dec_norm
 * applied, as in sta_decode.  Patch-grid positions only.  Equal grids are accepted and take the same route (one more QKV launch
 * per projection and no paired QKV launch: sta_decode stays the fast path for them).  sta_head_pts / sta_head_pose take per-call
 * shapes and serve each side.  Not covered by sta_reserve: the first call of a shape pair allocates. */
STA_API int sta_decode_mixed(sta_handle* h, const float* feat1, const float* feat2, int B, int hp1, int wp1, int hp2, int wp2,
                     float* const* out1, float* const* out2, void* stream);

/* _decode_stereo with CALLER positions (sta_model.py:177-244 hands pos1 / pos2 to every decoder block, whose attentions rotate
 * q / k by them: sta_blocks.py:134-137,196-199): pos1 / pos2 are device int64 [B, N, 2] (y, x) as _encode_image returns them,
 * but need not be the patch grid - a window of a larger grid, a permuted token order, repeated positions.  Values must lie in
 * [-1, pos_max] (out-of-range values are clamped); the RoPE table grows to pos_max on first use.  N = tokens per view (both
 * views: the two sides run as one batch).  Implementation: the QKV epilogues of the call rotate by the identity and one small kernel
 * per Q / K buffer rotates it in place from the positions table - the grid form (sta_decode) stays the fast path, and with the patch
 * grid's own positions the two agree to the rounding of one more fp16-plane split (~1e-7), not bit for bit. */
STA_API int sta_decode_pos(sta_handle* h, const float* feat1, const float* feat2, const int64_t* pos1, const int64_t* pos2,
                   int B, int N, int pos_max, float* const* out1, float* const* out2, void* stream);

/* _decode_stereo on TOKEN SUBSETS: caller positions AND unequal token counts, the last input of the reference's _decode_stereo
 * (sta_model.py:177-244; every attention rotates q / k by the positions it is handed, sta_blocks.py:134-137,196-199) - a rectangular
 * window of one view against the whole other view, a pruned token set.  feat1 [B, N1, enc_dim], feat2 [B, N2, enc_dim]; pos1
 * [B, N1, 2], pos2 [B, N2, 2] device int64 (y, x), every batch entry its own.  Values must lie in [-1, pos_max] (out-of-range values
 * are clamped, as in sta_decode_pos; the RoPE table grows to pos_max on first use).  out1[i] [B, N1+1, dec_dim], out2[i]
 * [B, N2+1, dec_dim]; NULL skips a layer, the last index has dec_norm applied.  N1, N2 >= 1 need not be products of a grid; N1 == N2
 * is served by the same route.  Implementation: sta_decode_mixed's row layout and two-group attention with the identity table in the
 * QKV epilogues, then two launches per layer of one kernel that rotates the Q / K buffers of both sides from the positions table.
 * Like sta_decode_mixed the call runs on one lane and is NOT covered by sta_reserve: the first call of a shape pair allocates.
 * Returns -1 with a message for null pointers, N < 1, pos_max outside [0, 2^20) or 2^31 or more decoder rows. */
STA_API int sta_decode_tokens(sta_handle* h, const float* feat1, const float* feat2, const int64_t* pos1, const int64_t* pos2,
                      int B, int N1, int N2, int pos_max, float* const* out1, float* const* out2, void* stream);

/* _decode_stereo on a batch whose ENTRIES have their own token counts: sta_decode_tokens with one (N1, N2) per entry - the pruned
 * token set of every frame, the overlap window of every loop candidate, the edges of one keyframe in one call.  Batch entries of the
 * reference's _decode_stereo never interact (sta_model.py:177-244, sta_blocks.py:129-148,188-208), so entry b is what the reference
 * returns for that entry alone at B = 1; nothing is padded and no token attends to another entry's.
 * n1 / n2: HOST arrays [B], entry b has n1[b] >= 1 tokens on side 1 and n2[b] >= 1 on side 2 (they size the launches and travel in
 * the kernel arguments: the call copies nothing to the device for them and does not synchronise it).  feat1 [sum(n1), enc_dim] and
 * pos1 [sum(n1), 2] (device int64 (y, x)) are packed entry-major; side 2 the same with n2.  Positions must lie in [-1, pos_max]
 * (out-of-range values are clamped, as in sta_decode_tokens; the RoPE table grows to pos_max on first use).  out1[i] is packed
 * [sum(n1) + B, dec_dim]: entry b occupies n1[b] + 1 consecutive rows, pose token first (the reference's order), starting at row
 * sum(n1[0 .. b)) + b; out2[i] the same with n2; NULL skips a layer, the last index has dec_norm applied.  1 <= B <= 16.
 * Implementation: rows are packed, so every row-wise step (LayerNorm, proj, cproj, the MLP, the residual epilogues) is one launch over
 * all rows; the QKV GEMMs run once per (side, entry) with the epilogue of sta_decode_tokens; one kernel per layer and buffer set rotates
 * Q / K from the packed positions table; attention is ONE launch for all 2B sequences, each with its own counts and schedule
 * (attn_varlen_kernel).  Like sta_decode_mixed / sta_decode_tokens the call runs on one lane and is NOT covered by sta_reserve: the first
 * call of a set of counts may allocate.  Returns -1 with a message for null pointers, a count below 1, B outside [1, 16], pos_max
 * outside [0, 2^20) or 2^31 or more decoder rows. */
STA_API int sta_decode_varlen(sta_handle* h, const float* feat1, const float* feat2, const int64_t* pos1, const int64_t* pos2,
                      const int* n1, const int* n2, int B, int pos_max, float* const* out1, float* const* out2, void* stream);

/* tok: B rows of dec_dim floats, consecutive rows `tok_stride` floats apart.
 * pose [B,16] row-major 4x4, conf [B]. */
STA_API int sta_head_pose(sta_handle* h, const float* tok, int B, int64_t tok_stride,
                  float* pose, float* conf, void* stream);

/* DPT pointmap head + postprocess.  enc_feat [B,N,enc_dim] (batch stride enc_bstride floats);
 * hookX point at the FIRST PATCH TOKEN (pose token already skipped) of the decoder outputs
 * selected by hooks [0, d/2+1, 3d/4+1, d+1] (dpt_head.py:112); batch strides in floats.
 * pts [B,H,W,3], conf [B,H,W]. */
STA_API int sta_head_pts(sta_handle* h,
                 const float* enc_feat, int64_t enc_bstride,
                 const float* hook1, int64_t hook1_bstride,
                 const float* hook2, int64_t hook2_bstride,
                 const float* hook3, int64_t hook3_bstride,
                 int B, int H, int W, float* pts, float* conf, void* stream);

/* sta_head_pts on B <= 32 entries whose patch rectangles DIFFER, in one call: entry b is hp[b] x wp[b] patches (hp, wp >= 1), and what
 * sta_head_pts computes for that entry alone at (16 hp[b], 16 wp[b]) - the reference's head_pts on it at B = 1.  Nothing is padded and
 * no pixel reads another entry's pixels (no halo, no bilinear tap, no tile spans two entries): at each of the head's six resolutions
 * the pixels of all entries are packed entry-major, and every launch carries the per-entry geometry in its kernel arguments.
 * enc_row, hook_row, hp, wp, out_pix are HOST arrays [B]; the call copies nothing to the device for them and does not synchronise.
 *   enc_row[b]   first patch row of entry b in enc_feat ([rows, enc_dim], dense rows)
 *   hook_row[b]  first patch row of entry b in EACH hook buffer ([rows, dec_dim], dense rows)
 * - so the packed output of sta_decode_varlen (a pose row in front of each entry) and the scheduler's (edge, side) subsets feed the head
 * in place.  out_pix[b]: pixel offset of entry b in pts (x 3 floats) and conf; NULL = packed, 256 * sum_{b' < b} hp wp.  Outputs are in
 * image orientation, [16 hp, 16 wp].  Tile families come from the cost model on the packed rows of each level; the halo-tiled family 8
 * runs its varlen form where it is forced (sta_set_gemm_variant 8), the register-staged family 1 has none: the automatic choice
 * never takes it here, and forcing it makes the call fail with a message.  Precisions f16x3, f16x3h, f16x3m; plain f16 is refused.  Like
 * the other varlen calls it runs on one lane and is NOT covered by sta_reserve: the first call of a set of shapes may allocate.
 * Returns -1 with a message for null pointers, B outside [1, 32], hp or wp below 1, 2^31 or more rows at any level, features that
 * are not 16-byte aligned. */
STA_API int sta_head_pts_varlen(sta_handle* h, const float* enc_feat, const int64_t* enc_row,
                        const float* hook1, const float* hook2, const float* hook3, const int64_t* hook_row,
                        const int* hp, const int* wp, int B, float* pts, float* conf, const int64_t* out_pix, void* stream);

/* Monolithic two-view forward.  Outputs index 0 = main view (img_a), 1 = support (img_b):
 * pts[k] [B,H,W,3], conf[k] [B,H,W], pose[k] [B,16], pose_conf[k] [B]. */
STA_API int sta_forward_pair(sta_handle* h, const float* img_a, const float* img_b, int B, int H, int W,
                     float* const pts[2], float* const conf[2],
                     float* const pose[2], float* const pose_conf[2], void* stream);

/* Camera-format input (the step before the path): uint8 HWC images [B,H,W,3], 16-byte
 * aligned.  The reference normalisation ImgNorm = ToTensor + Normalize(0.5,0.5)
 * (vista_slam/utils/image.py:13; datasets/slam_images_only.py:19,30) is fused into the patch gather;
 * results are bit-identical to sta_encode / sta_forward_pair on the normalised fp32 NCHW tensor. */
STA_API int sta_encode_u8hwc(sta_handle* h, const uint8_t* img_dev, int B, int H, int W, float* feat_dev, void* stream);
/* sta_encode_tokens on camera-format input [B,H,W,3] uint8 (16-byte aligned) with the fused ImgNorm of sta_encode_u8hwc: bit-identical
 * to sta_encode_tokens on the normalised fp32 NCHW tensor. */
STA_API int sta_encode_tokens_u8hwc(sta_handle* h, const uint8_t* img_dev, const int64_t* pos, int B, int H, int W, int N,
                            float* feat_dev, void* stream);
/* sta_encode_varlen on camera-format frames: imgs[b] [H[b], W[b], 3] uint8, 16-byte aligned; bit-identical to sta_encode_varlen on the
 * normalised fp32 frames. */
STA_API int sta_encode_varlen_u8hwc(sta_handle* h, const uint8_t* const* imgs, const int* H, const int* W, const int64_t* pos, const int* n,
                            int B, float* feat_dev, void* stream);
STA_API int sta_forward_pair_u8hwc(sta_handle* h, const uint8_t* img_a, const uint8_t* img_b, int B, int H, int W,
                           float* const pts[2], float* const conf[2],
                           float* const pose[2], float* const pose_conf[2], void* stream);

/* reductions that consume the path's output for every accepted pair, one fused pass.
 * sta_estimate_intrinsics <- estimate_intrinsic_from_pts3d(pts3d, confidence, shared_intrinsic)
 * (vista_slam/utils/slam_utils.py:8-79; slam.py:184) and, in the same read, depths = pts[...,2]
 * (slam.py:185) and conf.mean() per image (pose_graph.py:37).  shared = 0: K_out [B,3,3]; shared = 1: one K [3,3] over
 * all B images; shared = g >= 2: one K per group of g consecutive images, K_out [B/g,3,3] (g = 2: the two views of a
 * pair).  depth_out [B,H,W] and conf_mean_out [B] may be NULL.
 * sta_estimate_scale <- estimate_scale_with_depth_and_confidence(Di, Dj, ci, cj) (slam_utils.py:168-190),
 * s_out is one device float. */
STA_API int sta_estimate_intrinsics(sta_handle* h, const float* pts, const float* conf, int B, int H, int W, int shared,
                            float* K_out, float* depth_out, float* conf_mean_out, void* stream);
STA_API int sta_estimate_scale(sta_handle* h, const float* Di, const float* Dj, const float* ci, const float* cj, int64_t n,
                       float* s_out, void* stream);

/* input step = SLAM_image_only.process_image (vista_slam/datasets/slam_images_only.py:19-33):
 * `_crop_resize_if_necessary_image_only(rgb, resolution, w_edge, h_edge)` (datasets/base/base_view_graph_dataset.py:
 * 171-225: centre crop with an edge margin, cropping.rescale_image_depthmap LANCZOS rescale to cover the resolution
 * - vista_slam/utils/cropping.py:54-81 -, centre crop to the resolution) followed by ImgNorm (ToTensor +
 * Normalize(0.5,0.5)) and ImgGray (ToTensor + Grayscale).  src: one uint8 RGB frame [Hs,Ws,3] on the device.
 * (res_H, res_W) is the configured resolution (landscape or square, like the reference's `resolution`, which asserts
 * resolution[0] >= resolution[1]); the OUTPUT size (out_H, out_W) is the resolution, transposed when the first crop is
 * portrait (crop height > 1.1 x crop width; base_view_graph_dataset.py:200-205) - sta_preprocess_geometry returns it
 * (host only, no device work) so the caller can size the buffers.  A square crop (0.9 < h/w < 1.1) with a non-square
 * resolution is an error: the reference draws the orientation from an rng there.
 * Outputs (device, any may be NULL): u8_out [out_H,out_W,3] uint8 = the PIL image the reference hands to its
 * transforms, bit-exact to Pillow's 8-bit LANCZOS resampler (feeds sta_encode_u8hwc directly); rgb_out
 * [3,out_H,out_W] fp32 = value['rgb']; gray_out [out_H,out_W] fp32 = value['gray'].  The coefficient tables of one
 * geometry are cached in the handle; a geometry change synchronises `stream` once. */
STA_API int sta_preprocess_geometry(int Hs, int Ws, int res_H, int res_W, int w_edge, int h_edge, int* out_H, int* out_W);
STA_API int sta_preprocess_frame(sta_handle* h, const uint8_t* src, int Hs, int Ws, int res_H, int res_W, int w_edge, int h_edge,
                         uint8_t* u8_out, float* rgb_out, float* gray_out, void* stream);

/* output step of OnlineSLAM.save_data_all (vista_slam/slam.py:338-421).
 * sta_world_pointcloud <- slam.py:396-408: local = K^-1 [x,y,1] * depth * scale (compute_local_pointclouds,
 * vista_slam/utils/slam_utils.py:82-121), world = pose * [local,1], keep conf > conf_thres, colour = (img+1)/2;
 * order = torch boolean-mask order (view-major, row-major).  Inputs (device): depths [N,H,W], scales [N], K [N,3,3],
 * poses [N,4,4], confs [N,H,W], imgs [N,3,H,W] in [-1,1] (slam.imgs; may be NULL -> colour 0).  Outputs (device, any may
 * be NULL, each sized for N*H*W points): pts_out [M,3] fp32, col_out [M,3] fp32, ply_records_out [M,27] bytes = the
 * binary_little_endian vertex records (double x,y,z + uchar r,g,b) Open3D writes for pointcloud.ply.
 * *count_host = M on return (the call synchronises `stream`).
 * sta_mat_to_se3 <- pp.mat2SE3(pose) (slam.py:166): [B,4,4] -> [B,7] (tx,ty,tz,qx,qy,qz,qw), qw >= 0. */
STA_API int sta_world_pointcloud(sta_handle* h, const float* depths, const float* scales, const float* K, const float* poses,
                         const float* confs, const float* imgs, int N, int H, int W, float conf_thres,
                         float* pts_out, float* col_out, uint8_t* ply_records_out, int64_t* count_host, void* stream);
STA_API int sta_mat_to_se3(sta_handle* h, const float* poses, int B, float* se3_out, void* stream);

/* sta_voxel_downsample: the cloud fused on a voxel grid - one row per occupied voxel, the mean of its points and colours.  It is
 * what the reference reaches for Open3D for (eval/eval_recon.py:157-159 voxel_down_sample(0.05)) or avoids by dropping points at
 * random (run.py:41-47); the rows are spatial bins with a per-voxel mean, not a nearest-neighbour structure.
 * Inputs (device): pts [M,3] fp32; col [M,3] fp32 or NULL (colour sums are then 0); M < 2^30; voxel_size finite and > 0;
 * origin = three doubles or NULL; min_points >= 1.
 * Dropping: a point with a non-finite coordinate is dropped and counted in n_dropped.
 * Grid: mn = the per-axis minimum of the kept points (fp32, exact).  origin == NULL: o = double(mn) - voxel_size * 0.5 - the rule
 * Open3D documents for VoxelDownSample, restated from memory: Open3D was not available to check against.  Otherwise o = origin, so
 * that two calls with one origin share one grid.
 * Voxel index per axis: floor((double(p) - o) / voxel_size) - an IEEE fp64 subtraction and division, no multiply-add to contract
 * and no fast-math build flag -, so numpy's float64 gives the same integer, also for a point exactly on a voxel face.  Indices may
 * be negative with an explicit origin; they must fit int32.
 * Limit: the extent index_max - index_min + 1 must be <= 2^21 per axis (a 63-bit key); a wider grid is refused with the extents in
 * the message.
 * Rows: one per occupied voxel with count >= min_points, in ascending lexicographic order of (iz, iy, ix).  Outputs (device, any
 * may be NULL, row outputs sized for M rows): pts_out [V,3] fp32, col_out [V,3] fp32 = the means - sums in fp64, divided by the
 * count in fp64, rounded once to fp32 -, counts_out [V] int32, index_out [V,3] int32 = the absolute voxel indices (ix, iy, iz),
 * inverse_out [M] int32 = the output row of every input point, -1 where the point was dropped or its voxel filtered,
 * ply_records_out [V,27] bytes = sta_world_pointcloud's vertex records of the means (double(fp32 mean), rint(clamp(c,0,1)*255)).
 * count_host[0] = V, count_host[1] = n_dropped.  V = 0 (every point dropped, every voxel below min_points) is not an error; M = 0
 * returns {0, 0} without touching the device.
 * Determinism: no floating-point atomics.  A stable radix sort of (voxel key, input index) puts every voxel's points in ascending
 * input order; a row of at most 1024 points is summed by 64 lanes - lane l adds points l, l + 64, ... in ascending order, then a
 * fixed butterfly -, a longer row by 1024 threads the same way and the 16 wave sums in ascending order.  The order depends on the
 * row's length alone, two calls on one input are bit-identical, inputs whose fp64 sums are exact give the exact mean, and any
 * other input is within one fp32 step of any other order of summation.
 * The call synchronises `stream` twice - after the bounds (the host must see them to refuse a grid and to choose the number of
 * sort passes) and after the row count - and returns with the reduction enqueued: the outputs are complete for whatever runs on
 * `stream` next.  Workspace (the stream's scratch context): about 36 bytes per point - two (key, index) buffers of 12 each, segment
 * and row tables of 12 - plus 1 KiB of histogram per 1024 points and the scan tables. */
STA_API int sta_voxel_downsample(sta_handle* h, const float* pts, const float* col, int64_t M, double voxel_size, const double* origin,
                         int min_points, float* pts_out, float* col_out, int32_t* counts_out, int32_t* index_out, int32_t* inverse_out,
                         uint8_t* ply_records_out, int64_t count_host[2] /* V, n_dropped */, void* stream);

/* geometric consistency of the depth maps the path produced (vista_slam/utils/slam_utils.py; the CODE is the
 * definition where it disagrees with its docstring).  All pointers are device memory; H, W need not be multiples of 16 and
 * H > W is accepted (the kernels have no orientation).  The workspace (pair matrices; error plane, histograms, counters) is
 * taken from the stream's scratch context, which grows - behind one device synchronisation - on the first call of a larger
 * size and never afterwards; apart from that neither call synchronises, allocates or copies to the host.
 * sta_view_consistency <- view_consistency_check(depth, intrinsics, poses, threshold) (slam_utils.py:346-419): every pixel of
 * view i is unprojected (K_i^-1 [x,y,1] d_i), moved to view j (T_j^-1 T_i, poses camera-to-world), projected with K_j
 * (uv = uvw[:2] / uvw[2], the unclamped third coordinate) and compared with depth[j] sampled bilinearly there
 * (grid_sample, align_corners=True, zero padding): agree = |sampled - max(z_j, 1e-6)| < threshold.  count_out [n,H,W] int32 =
 * the number of agreeing views j in [max(0, i-window), min(n, i+window+1)) \ {i}; window = 4 is the reference (its loop, not
 * the +-2 of its docstring).  A point behind view j whose uv falls outside the frame samples 0 and agrees when
 * threshold > 1e-6, as in the reference.  depths [n,H,W], K [n,3,3], poses [n,4,4].
 * sta_symmetric_geo_mask <- compute_symmetric_geo_valid_mask(depths, intri, relative_pose) (slam_utils.py:269-343) for P edges
 * at once, in the layout sta_regress_views writes: depths [P,2,H,W], K [P,3,3] (shared by the pair), rel_pose [P,4,4].
 * Direction 0 warps view 0 by rel_pose into view 1, direction 1 warps view 1 by rel_pose^-1 into view 0; the target pixel is
 * round-half-even(uv), uv = (K p)[:2] / ((K p)[2] + 1e-8); err = |depth_target - z|; thres = 2 * median(err over the pixels that
 * land inside the frame) - torch.median: the LOWER middle element, NaN if any such err is NaN -, 1e10 when none does.
 * mask_out [P,2,H,W] bytes 0/1 = inside && err < thres; thres_out [P,2] (may be NULL) = the thresholds.  The median is an
 * exact device-side selection (four 8-bit radix passes over the fp32 bit patterns).  For portrait frames of
 * sta_regress_views pass the transposed views [P,2,W,H] (the K it returns was computed on those). */
STA_API int sta_view_consistency(sta_handle* h, const float* depths, const float* K, const float* poses, int n, int H, int W,
                         float threshold, int window, int32_t* count_out, void* stream);
STA_API int sta_symmetric_geo_mask(sta_handle* h, const float* depths, const float* K, const float* rel_pose, int P, int H, int W,
                           uint8_t* mask_out, float* thres_out, void* stream);

/* the rest of slam_utils.py - the general two-view check with a quantile threshold, local point clouds and ray
 * depths.  Same rules as f5: device pointers, any H and W (H > W included), workspace from the stream's scratch context (one
 * synchronisation when it first grows), otherwise no allocation, synchronisation or copy to the host; an argument error returns
 * a status and a message and launches nothing.
 * sta_geo_valid_mask <- compute_geo_valid_mask_batched(depth1, depth2, K1, K2, T1, T2, error_thres_rel) (slam_utils.py:193-266):
 * depth1, depth2 [B,H,W], K1, K2 [B,3,3] (only fx, fy, cx, cy are read, as in the reference), T1, T2 [B,4,4] camera-to-world.
 * Pixel (x, y) of view 1 is unprojected ((x - cx1) z / fx1, (y - cy1) z / fy1, z = depth1), moved by T2^-1 T1 (top three rows of
 * each, like the reference's [..., :3]) and projected: u2 = fx2 x2 / z2 + cx2, v2 likewise - the unclamped z2, no epsilon, so a
 * point behind camera 2 projects too.  The target pixel is (int(v2), int(u2)): TRUNCATION toward zero, so u2 in (-1, 0) reads
 * column 0; a coordinate that is not finite or beyond the int32 range is invalid.  err = |z2 - depth2[b, v, u]|;
 * thres = torch.quantile(err of the valid pixels of ALL B images, q), linear interpolation, bit for bit in fp32:
 * rank = q (n - 1), a and b = the floor(rank)-th and ceil(rank)-th smallest, w = rank - floor(rank),
 * thres = w < 0.5 ? fma(w, b - a, a) : fma(-(b - a), 1 - w, b); NaN if any valid err is NaN.  The two order statistics are an
 * exact device-side selection (four 8-bit radix passes, both ranks at once); the launch count does not depend on B.
 * mask_out [B,H,W] bytes 0/1 = valid && err < thres (strict).  thres_out (1 float, may be NULL) = thres; count_out (1 int32, may
 * be NULL) = n, the number of valid pixels.  No valid pixel (torch raises there): count 0, thres NaN, mask all 0.
 * Refused: q outside [0, 1], B*H*W above 16 000 000 (torch.quantile's own limit).
 * sta_local_pointclouds <- compute_local_pointclouds(depths, intrinsics) (slam_utils.py:82-121): out [N,H,W,3] =
 * K^-1 [x, y, 1] * depths[n, y, x]; K is one [3,3] (k_batched = 0) or [N,3,3] (k_batched = 1), inverted once per view in double.
 * sta_ray_depth <- depth_from_pointcloud_dot_batched(pointclouds, intrinsics) (slam_utils.py:124-165): out [B,H,W] = the dot
 * product of pts[b, y, x, :] with the unit ray K^-1 [x, y, 1] / |K^-1 [x, y, 1]|; K as above. */
STA_API int sta_geo_valid_mask(sta_handle* h, const float* depth1, const float* depth2, const float* K1, const float* K2,
                       const float* T1, const float* T2, int B, int H, int W, float q, uint8_t* mask_out, float* thres_out,
                       int32_t* count_out, void* stream);
STA_API int sta_local_pointclouds(sta_handle* h, const float* depths, const float* K, int k_batched, int N, int H, int W,
                          float* out, void* stream);
STA_API int sta_ray_depth(sta_handle* h, const float* pts, const float* K, int k_batched, int B, int H, int W, float* out,
                  void* stream);

/* Token selections from per-pixel maps: the producer of what sta_encode_varlen (index lists), sta_decode_varlen ((y, x) lists) and
 * sta_regress_views_tokens (index lists, windows) take.  B in [1, 32] maps, entry b of its own size H[b] x W[b] (multiples of 16,
 * hp_b x wp_b patches of 16x16 pixels, N_b = hp_b wp_b <= 8192, patch index y wp_b + x), are pooled to one int32 score per patch;
 * a rule selects patches per entry; the selection comes out as an ascending index list, a (y, x) list, a count and a bounding
 * window.  maps, H, W and top_k are HOST arrays read during the call (maps[b]: device memory, contiguous [H_b, W_b]); the geometry
 * travels in the kernel arguments.  Two launches; no copy, no workspace, no allocation, no synchronisation, on the first call as on
 * any later one (sta_alloc_stats does not move).  Everything is integer arithmetic: the result is defined bit for bit.
 * Score (int32 >= 0 per patch, over its 256 pixels):
 *   dtype 0 (uint8 / bool bytes), mode 0: the number of non-zero bytes (255 and 2 count like 1); with invert, of zero bytes.
 *   dtype 1 (float32), mode 0: the number of pixels with v > thres - strict, false for a NaN v and for a NaN thres, true for +inf;
 *     invert negates the predicate, so a NaN pixel counts under invert.
 *   dtype 1, mode 1 (fixed-point sum; thres is ignored): sum of rint(clamp(v, 0, 32767) * 256), rounding half to even; the clamp
 *     takes NaN, -inf and negatives to 0 and +inf to 32767.  The product is exact in fp32 and every term an integer, so the score
 *     does not depend on summation order; its maximum is 256 * 8 388 352 = 2 147 418 112 < 2^31.
 * Rule:
 *   rule 0 (min_score = s >= 0): patch p is selected iff score[p] >= s; with margin = r in [0, 8] the selection is then dilated by r
 *     patches in the Chebyshev metric inside the entry's own grid (a selected patch selects every existing patch with |dy| <= r and
 *     |dx| <= r; nothing crosses the grid border or reaches another entry).  top_k may be NULL.
 *   rule 1 (top_k[b] = k_b in [1, N_b]): exactly k_b patches, those with the largest scores; among equal scores the lower patch
 *     index wins.  min_score is not used (pass 0).
 * Outputs (device memory, the caller's; off_b = sum of N_a over a < b):
 *   score  int32 [sum N_b]      entry b's grid, row-major, at off_b
 *   index  int64 [sum N_b]      slot b starts at off_b: its first n_sel[b] values are the selected patch indices in ASCENDING
 *                               order, the rest of the slot is -1
 *   pos    int64 [sum N_b, 2]   the same slots: (y, x) of every selected patch, -1 in the tail
 *   n_sel  int32 [B]            the counts (k_b under rule 1)
 *   window int32 [B, 4]         (y0, x0, h, w), in patches: the bounding rectangle of the selected patches, after the margin;
 *                               (0, 0, 0, 0) when nothing is selected - an empty selection is a result, not an error
 * Refused (-1 and a message, nothing launched): a null pointer; B outside [1, 32]; H or W below 16 or no multiple of 16;
 * N_b > 8192 (one workgroup keeps an entry's scores and flags in LDS; 8192 patches is a 2048 x 1024 frame); mode 1 with dtype 0 or
 * with invert; rule 1 with margin != 0 or a top_k[b] outside [1, N_b]; min_score < 0; margin outside [0, 8]; a float32 map that is
 * not 4-byte aligned.  A byte map may start at any address (a map that is not 16-byte aligned is read element by element). */
STA_API int sta_select_patches(sta_handle* h, const void* const* maps, const int* H, const int* W, int B,
                               int dtype /*0 uint8, 1 float32*/, int mode /*0 count, 1 fixed-point sum*/, float thres, int invert,
                               int rule /*0 min_score, 1 top_k*/, int min_score, const int* top_k, int margin,
                               int32_t* score, int64_t* index, int64_t* pos, int32_t* n_sel, int32_t* window, void* stream);

/* The keyframe gate: Shi-Tomasi corners on the last keyframe, tracked into the current frame with pyramidal Lucas-Kanade
 * (vista_slam/flow_tracker.py:15-66, which calls OpenCV on the CPU).  The contract RESTATES OpenCV's documented algorithms
 * (pyrDown, goodFeaturesToTrack, calcOpticalFlowPyrLK) in integer and float64 terms; the yardstick is the numpy restatement
 * tests/flow_cases.py, it is NOT cv2, and keyframe decisions can differ from OpenCV's at the margin.
 * Frame: uint8 [H,W] (dtype 0) or fp32 [H,W] in [0,1] (dtype 1), converted as the reference does (run.py:181):
 * uint8(trunc(fp32(g) * 255.0f)).  H, W >= 8 (odd sizes are legal), H * W <= 2^21.  An image read outside its bounds uses periodic
 * reflect-101: m = 2 (n - 1), i = ((i mod m) + m) mod m, i = m - i if i >= n; index 0 for n == 1.
 * Pyramid: level 0 is the uint8 frame; level l + 1 has size ((H_l + 1) / 2, (W_l + 1) / 2) and pixel (y, x) =
 * (sum_ab k[a] k[b] ext(2y + a - 2, 2x + b - 2) + 128) >> 8, k = [1,4,6,4,1]; a level is added while l < max_level (<= 3) and both of
 * its dimensions exceed win.  A pyramid buffer holds its levels at the byte offsets sta_flow_plan reports (256-byte aligned);
 * B frames are pyramid_bytes apart.
 * sta_flow_plan (host only, no GPU): out = {levels, h[4], w[4], offset[4], pyramid_bytes, corner workspace_bytes, 0}.  Returns -1,
 * with the numbers in sta_last_error(), for H or W < 8, H * W > 2^21, B outside [1, 32], win even or outside [3, 21], max_level
 * outside [0, 3], max_corners < 1.
 * sta_flow_pyramid: B frames [B,H,W] -> B pyramids.
 * sta_flow_corners (image = a uint8 [H,W] frame, e.g. level 0 of a pyramid): Sobel 3x3 on the extended image -> gx, gy; box sums of
 * block_size^2 (3, 5 or 7) over the reflect-101 extension of the product maps gx^2, gx gy, gy^2 -> a, b, c (int32);
 * R = (a + c) - isqrt((a - c)^2 + 4 b^2) with the floor square root of the int64 argument.  A pixel is a candidate iff R > 0,
 * double(R) >= quality * double(Rmax), and R equals the maximum of its 3x3 neighbourhood inside the image (ties keep both).  The
 * candidates are ordered by R descending, the lower y * W + x first among equals, and suppressed greedily in that order: one is
 * accepted iff no accepted one lies at dx^2 + dy^2 < min_distance^2 (min_distance in [1, 32]); the first max_corners accepted are
 * written as (x, y) fp32 rows in rank order to corners [max_corners,2], their number to *n_out (device); later rows are not written.
 * workspace: workspace_bytes of device memory, 8-byte aligned, contents free.
 * sta_flow_track: the points pts [n,2] fp32 (x, y) of the frame behind prev_pyramid - any positions, not only corners - into each
 * of the B frames behind next_pyramids.  n = min(*n_dev, n_cap) when n_dev (device) is given - e.g. sta_flow_corners' n_out, so
 * that corners followed by track needs no synchronisation - and n_cap otherwise.  Per point and frame, float64 state, W_BITS = 14,
 * half = (win - 1) / 2, FS = 2^-20, descale(s, k) = (s + 2^(k-1)) >> k, from the top level L down to 0:
 *   p = pts 2^-l - half; the estimate q = pts 2^-L at the top, q <- 2 q below.  ip = floor(p); the level is SKIPPED (estimate
 *   unchanged; at level 0 also status = 0) unless -win <= ip.x < W_l and -win <= ip.y < H_l.  Bilinear weights from the fractions
 *   (al, be) of p: w00 = rint((1-al)(1-be) 2^14), w01 = rint(al (1-be) 2^14), w10 = rint((1-al) be 2^14) (float64 products, half to
 *   even), w11 = 2^14 - w00 - w01 - w10.  Over the win^2 window: I = descale(sum w img, 9), Ix, Iy = descale(sum w grad, 14), grad =
 *   Scharr (3, 10, 3) of the extended level image, 0 at positions outside the level.  A11, A12, A22 = FS x the exact integer sums of
 *   Ix^2, Ix Iy, Iy^2; D = A11 A22 - A12 A12; e = (A11 + A22 - sqrt((A11 - A22)^2 + 4 A12^2)) / (2 win^2); the level is skipped if
 *   e < min_eig or D < 2^-23.  q <- q - half, then up to max_iter rounds: iq = floor(q); outside the bounds above -> status = 0 at
 *   level 0 and the loop ends; J = descale(sum w(q) next_img, 9); b1, b2 = FS x the exact sums of (J - I) Ix, (J - I) Iy;
 *   d = ((A12 b2 - A22 b1) / D, (A12 b1 - A11 b2) / D); q <- q + d; stop if d.d <= eps^2; from the second round on, if
 *   |d.x + dprev.x| < 0.01 and |d.y + dprev.y| < 0.01, q <- q - d / 2 and stop.  After the loop q <- q + half.
 * Every float64 operation is one IEEE operation in the order written.  Outputs (device): next_pts [B,n_cap,2] = float32(q) at level
 * 0, status [B,n_cap] uint8 (a rejection at a coarse level does not clear it, as in OpenCV), rows >= n are not written;
 * stats [B,3] float64 = {n, n_good = points with status 1, sum over them of sqrt(dx^2 + dy^2) in float64 of the fp32 positions}.
 * The mean and the comparison with the threshold are the host's (the reference's mean is float32: a stated difference).
 * None of the three device calls allocates, copies to the host or synchronises. */
STA_API int sta_flow_plan(int H, int W, int B, int win, int max_level, int max_corners, int64_t out[16]);
STA_API int sta_flow_pyramid(sta_handle* h, const void* gray, int dtype /*0 uint8, 1 float32*/, int H, int W, int B, int win, int max_level,
                             uint8_t* pyramid, void* stream);
STA_API int sta_flow_corners(sta_handle* h, const uint8_t* image, int H, int W, int max_corners, double quality, int min_distance,
                             int block_size, void* workspace, int64_t workspace_bytes, float* corners, int32_t* n_out, void* stream);
STA_API int sta_flow_track(sta_handle* h, const uint8_t* prev_pyramid, const uint8_t* next_pyramids, int H, int W, int B, int win,
                           int max_level, const float* pts, const int32_t* n_dev, int n_cap, int max_iter, double eps, double min_eig,
                           float* next_pts, uint8_t* status, double* stats, void* stream);

/* Loop candidates: ORB keypoints and descriptors, a bag-of-words vector from a vocabulary tree, L1 scores against the earlier
 * keyframes (vista_slam/loop_detector.py:14-50, which calls cv2.ORB_create().detectAndCompute and DBoW3 on the CPU).  The contract
 * RESTATES the documented algorithms in integer and float64 terms; the yardstick is the numpy restatement tests/loop_cases.py, it is
 * NOT cv2 / DBoW3.  Stated differences from cv2: 1-degree angle bins (fastAtan2 there); the integer Harris order (float32 there);
 * the blur kernel below (cv2's fixed-point Gaussian there); 11-bit bilinear resizing (INTER_LINEAR_EXACT there); no tie extension at
 * the second cut (retainBest there); and the comparison table is the caller's (OpenCV's learned 256 pairs are not part of this library).
 * Frame, uint8 conversion and reflect-101 are the keyframe gate's (above).  Limits: nlevels in [1, 8], nfeatures in [1, 4096], edge
 * in [22, 64], fast_threshold in [1, 254], H and W > 2 edge, H * W <= 2^21.
 * Scales and sizes (float64, every step one IEEE operation in the order written): s_0 = 1, s_(l+1) = s_l * 1.2; level l has size
 * (rint(H / s_l), rint(W / s_l)); a level whose height or width is <= 2 edge holds no keypoints and is not built (nor is any level
 * above it).  Features per level: f = 1 / 1.2, fp = f multiplied nlevels times into 1, nd = (nfeatures * (1 - f)) / (1 - fp); for
 * l < nlevels - 1: n_l = rint(nd), then nd = nd * f; the last level gets max(nfeatures - sum, 0).  The outputs hold
 * rows = max(nfeatures, sum of n_l) rows (the rounded counts can exceed nfeatures by a few).
 * Level l from level l - 1, bilinear: fx = (x + 0.5) * (W_(l-1) / W_l) - 0.5, sx = floor(fx), a = fx - sx; sx < 0 -> (0, 0);
 * sx >= W_(l-1) - 1 -> (W_(l-1) - 1, 0); c1 = rint(a * 2048), c0 = 2048 - c1, the same for y; pixel = (sum cy cx p + 2^21) >> 22.
 * FAST-9 on the unblurred level, for pixels at least 3 from the border: ring = the 16 Bresenham offsets at radius 3 from (0, -3)
 * clockwise; A = the maximum over the 16 contiguous arcs of 9 of the minimum over the arc of p - ring, Bm the same with ring - p;
 * score = max(A, Bm) - 1; a pixel is a corner iff score >= fast_threshold, a non-corner has score 0.  A corner survives iff its
 * score is STRICTLY greater than its 8 neighbours' scores (ties drop both); only survivors with edge <= x < W_l - edge and
 * edge <= y < H_l - edge go on.  First cut: if more than 2 n_l survive, every survivor whose score is >= the score of the 2 n_l-th
 * largest is kept (ties kept).  Harris on the 7x7 block of the unblurred level centred on the keypoint: Ix = 2 (I(x+1,y) - I(x-1,y))
 * + (I(x+1,y-1) - I(x-1,y-1)) + (I(x+1,y+1) - I(x-1,y+1)), Iy its transpose, a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy,
 * R = 25 (a b - c^2) - (a + b)^2 in int64 (k = 0.04 exactly, OpenCV's positive scale dropped).  Order: R descending, then
 * y * W_l + x ascending; the first n_l are kept, with no tie extension.  Output rows are level-major, in that order within a level;
 * their number goes to *n_out (device), rows at or past it are not written.
 * Orientation on the unblurred level: m10 = sum u I, m01 = sum v I over |v| <= 15, |u| <= umax[|v|], umax = {15,15,15,15,14,14,14,
 * 13,13,12,11,10,9,8,6,3}.  The angle is one of 360 one-degree bins, found with integers from the caller's table
 * trig int32 [720,2] = rint(2^30 (cos, sin)(j * 0.5 degrees)) - the library contains no trigonometry: with d_k = trig[(2k - 1) mod
 * 720] and cross(d, m) = d.x m.y - d.y m.x (int64, m = (m10, m01)), the bin is the smallest k with cross(d_k, m) >= 0 and
 * cross(d_(k+1), m) < 0; bin 0 for m = 0 (and if no k qualifies).
 * Blur per level: B = (sum_ab k[a] k[b] ext(y + a - 3, x + b - 3) + 2^15) >> 16, k = {18,33,49,56,49,33,18}, reflect-101.
 * Descriptor: pattern int8 [256,4] rows (x1, y1, x2, y2), every |value| <= 13 (the caller's to hold; a read is clamped into the
 * level, so a table that breaks the rule cannot read outside it); with (C, S) = trig[2 bin]: rx = (x C - y S + 2^29) >> 30,
 * ry = (x S + y C + 2^29) >> 30 (arithmetic shift = floor); bit i = B(kp + r(x1,y1)) < B(kp + r(x2,y2)), stored in byte i / 8 at
 * bit i % 8.  With edge >= 22 no read leaves the level.
 * sta_orb_plan (host only, no GPU): out = {nlevels, built levels, h[8], w[8], n_l[8], byte offset[8] of a built level in a plane (-1:
 * not built), plane bytes, extraction workspace_bytes, rows, sta_bow_transform's workspace_bytes for `rows` descriptors, 0, 0}.
 * Returns -1, with the numbers in sta_last_error(), for a parameter outside the limits above.
 * sta_orb_extract: image uint8 [H,W] (dtype 0) or fp32 [H,W] (dtype 1); trig, pattern, workspace (8-byte aligned, contents free)
 * on the device.  After the call the workspace begins with the plane of the levels and, plane bytes further, the plane of the blurred
 * levels (each built level at its byte offset); the rest of it is scratch.  Outputs (device): kp int32 [rows,4] = (x, y, level, angle bin) in the level's own pixels, resp int64 [rows] = R,
 * desc uint8 [rows,32], n_out int32.
 *
 * Vocabulary: a k-ary tree, k <= 64, depth <= 10: node_desc uint8 [n,32], child_first int32 [n], child_count int32 [n], word_of
 * int32 [n] (-1 for an inner node), word_weight float64 [n_words]; node 0 is the root, siblings are contiguous, children follow
 * their parent (child_first > the parent's index), a leaf may sit at any depth.
 * sta_bow_transform(desc [n_cap,32], n_dev): n = min(*n_dev, n_cap) (n_cap when n_dev is null).  Per descriptor, from the root: at
 * each node the child with the smallest Hamming distance, the first among equals; at a leaf its word w, dropped when
 * word_weight[w] <= 0.  The vector = the distinct words in ascending order with count_w (int32) and val_w = count_w * weight_w (one
 * float64 multiply), divided by its L1 norm (DBoW's mustNormalize path for L1 scoring); the norm is summed in an order that depends
 * on the number of words alone.  Outputs (device): words, counts int32 [n_cap], vals float64 [n_cap], n_words int32; entries at or
 * past n_words are not written; an empty vector is a result (n_words = 0).  workspace: 4 n_cap bytes.  n_cap in [1, 4104].
 * sta_bow_score: sim[e] float64 = -0.5 * sum over the words common to the query and row rows[e] of the database of
 * (|a - b| - |a|) - |b|  (DBoW's L1 score), e < m, one launch, a fixed summation order: two runs are bit-identical.  The query is
 * (q_words, q_vals, q_n) as sta_bow_transform writes them, in arrays of q_cap entries: min(*q_n, q_cap) words are read, whatever the
 * database's cap is (the two capacities are independent, both in [1, 4104]); the database is db_words int32 [max_views,cap], db_vals float64
 * [max_views,cap], db_n int32 [max_views], rows int32 [m] - all on the device; a row index outside [0, max_views) scores 0.
 * None of the three device calls allocates, copies to the host or synchronises. */
STA_API int sta_orb_plan(int H, int W, int nfeatures, int nlevels, int fast_threshold, int edge, int64_t out[40]);
STA_API int sta_orb_extract(sta_handle* h, const void* image, int dtype /*0 uint8, 1 float32*/, int H, int W, int nfeatures, int nlevels,
                            int fast_threshold, int edge, const int32_t* trig, const int8_t* pattern, void* workspace, int64_t workspace_bytes,
                            int32_t* kp, int64_t* resp, uint8_t* desc, int32_t* n_out, void* stream);
STA_API int sta_bow_transform(sta_handle* h, const uint8_t* desc, const int32_t* n_dev, int n_cap, const uint8_t* node_desc,
                              const int32_t* child_first, const int32_t* child_count, const int32_t* word_of, const double* word_weight,
                              int n_nodes, int n_words, void* workspace, int64_t workspace_bytes, int32_t* words, int32_t* counts, double* vals,
                              int32_t* n_words_out, void* stream);
STA_API int sta_bow_score(sta_handle* h, const int32_t* q_words, const double* q_vals, const int32_t* q_n, int q_cap,
                          const int32_t* db_words, const double* db_vals, const int32_t* db_n, int max_views, int cap, const int32_t* rows, int m,
                          double* sim, void* stream);

/* The Sim(3) pose graph: OnlineSLAM.pose_graph_optimize (vista_slam/slam.py:108-140, pose_graph.py:70-154), there a pypose LM over
 * Sim3 nodes with a dense autograd Jacobian and a dense Cholesky solve.  The contract RESTATES the problem in float64; the yardstick is
 * the numpy restatement tests/pgo_cases.py, it is NOT pypose (which cannot be imported where this library is tested).  Stated
 * differences from the reference: float64 inside (float32 there); inexact steps (PCG to rtol, dense Cholesky there); 7 tangent unknowns
 * per node (pypose differentiates the 8 stored numbers).  The LM constants high / low / up / down / reject, and `decreasing` being
 * relative to f, are restated from memory of pypose's TrustRegion and StopOnPlateau: every one is an argument.
 * Limits: 1 <= n <= 8192 nodes, 1 <= E <= 16384 edges; a violation returns -1 with the numbers in sta_last_error().
 * Group: an element is 8 float64 (tx,ty,tz, qx,qy,qz,qw, s), acting as x -> s R(q) x + t.  Product (s1 R1 t2 + t1, R1 R2, s1 s2),
 * inverse (-(1/s) R^T t, R^T, 1/s); every quaternion written is normalised once and not sign-canonicalised.  A tangent is
 * xi = (tau, phi, sigma) with generator [[sigma I + phi^, tau],[0,0]]; Exp: R = exp(phi^), s = e^sigma, t = W tau,
 * W = C I + A phi^ + B phi^ phi^ with theta = |phi|, C = expm1(sigma) / sigma (1 at sigma = 0) and
 *   theta >= 0.25:  A = Is / theta, B = (C - Ic) / theta^2, Is = (e^sigma (sigma sin - theta cos) + theta) / (sigma^2 + theta^2),
 *                   Ic = (e^sigma (sigma cos + theta sin) - sigma) / (sigma^2 + theta^2);
 *   theta <  0.25:  A = sum_j (-theta^2)^j m_(2j+1) / (2j+1)!, B = sum_j (-theta^2)^j m_(2j+2) / (2j+2)!, j < 6, with the moments
 *                   m_k = int_0^1 u^k e^(u sigma) du from the backward recurrence m_(k-1) = (e^sigma - sigma m_k) / k started at
 *                   m_48 = e^sigma / 49 (no division by sigma: the same branch serves small and large |sigma|).
 * The quaternion of Exp is (k phi, cos(theta/2)), k = sin(theta/2) / theta, or 1/2 - theta^2 / 48 for theta < 1e-4.  Log: q normalised,
 * negated if w < 0 (so |phi| <= pi); phi = f q.xyz, f = 2 atan2(n, w) / n with n = |q.xyz|, or (2/w)(1 - n^2 / (3 w^2)) for n < 1e-4;
 * sigma = log s; tau = W^-1 t by the adjugate.  Ad and ad for the order (tau, phi, sigma):
 *   Ad(T) = [[sR, t^ R, -t],[0, R, 0],[0, 0, 1]],   ad(xi) = [[sigma I + phi^, tau^, -tau],[0, phi^, 0],[0, 0, 0]].
 * Jl(xi) = sum_(k<=32) ad^k / (k+1)! by Horner, column by column: y = e_j + ad y / (k + 1), k = 32 .. 1.
 * sta_sim3_op(op): 0 mul(a, b), 1 inv(a), 2 inv(a) b, 3 Exp(a [count,7]), 4 Log(a) -> out [count,7], 5 retract: Exp(a [count,7]) b where
 * mask (uint8 [count], null = everywhere) is set and a copy of b elsewhere; elements [count,8]; one thread per element.
 * Graph: edge e = (a, b) = edges int32 [E,2] with measurement P_e (poses [E,8]) and weights w_e >= 0 (confs [E,7]) has the residual
 * r_e = Log(P_e X_a^-1 X_b) (the reference's poses @ node1.Inv() @ node2).  An edge is ACTIVE iff a != b, both lie in [0, n) and
 * opt[a] | opt[b] (opt uint8 [n]: the optimised nodes); an inactive edge contributes nothing; an index outside [0, n) sets status bit 1.
 * Under X <- Exp(d) X, with A_e = P_e X_a^-1 and M_e = Jl(r_e)^-1 Ad(A_e) (7x7 elimination with partial pivoting, the first largest
 * entry): dr/dd_b = M_e, dr/dd_a = -M_e.  S_e = M_e^T diag(w_e) M_e, v_e = M_e^T (w_e r_e), c_e = sum w r^2;
 *   f = sum_e c_e,   g_k = sum over the half-edges at k of +-v_e,   (H x)_k = sum over the half-edges at k of +-S_e (x_b - x_a)
 * (+ at k = b, - at k = a; x = 0 at a fixed node).  Nothing is assembled; there is no floating-point atomic.
 * sta_pgo_index: off int32 [n+1], inc int32 [<= 2E] = edge * 2 + side (side 0: the node is a) for the active half-edges at optimised
 * nodes, each node's list ASCENDING by edge; status int32.  One workgroup; workspace 16 E bytes.
 * sta_pgo_linearize: c [E] always; full != 0 also r [E,7], S [E,7,7], v [E,7] (zeros on inactive edges), g [n,7] and the diagonal
 * blocks [n,7,7] = sum of S_e in list order (zeros at fixed nodes); rec = {f, status}: f = the c_e summed as thread t of 1024 takes
 * e = t, t + 1024, ... in order, a shuffle tree per wave, the 16 wave sums in order; status = bit 2 for a non-finite f, ored with
 * *idx_status (sta_pgo_index's, may be null).  The cost-only form (full = 0: off, inc, r, S, v, g, blocks may be null) runs the
 * same instructions: its f is bit-identical to the full form's.
 * sta_pgo_solve: preconditioned CG for (H + D / radius) d = -g, D = diag(clamp(diag H, dmin, dmax)), block-Jacobi preconditioner (per
 * optimised node the 7x7 Cholesky factor of its diagonal block + D_k / radius), x_0 = 0.  Stops at the first of |r_k|_2 <= rtol |g|_2,
 * k = max_iter (bit 4), p^T A p <= 0 or a non-finite scalar (bit 8); a block that is not positive definite is bit 16 (no iteration).
 * ONE workgroup of 1024 threads; node k belongs to thread k mod 1024; dot products sum each thread's rows in ascending order, then the
 * fixed tree above: two runs are bit-identical.  d [n,7] (zeros at fixed nodes); stats float64 [4] = {iterations, |r| / |g| by
 * recurrence, -2 d.g - d.H d (the model decrease), status}.  The products read the UPPER triangle of S_e (S_e is symmetric up to
 * rounding).  Workspace: out[3] of sta_pgo_plan.
 * sta_pgo_plan (host only): out = {off bytes, inc bytes, index workspace bytes, solve workspace bytes, sta_pgo_optimize workspace
 * bytes, n, E, 0}.
 * sta_pgo_optimize: the LM loop, host-driven, on nodes [n,8] in place.  Per outer step (at most `steps`): linearise at X (cost f); up to
 * `reject` trials: solve at the current radius, X' = Exp(d) X on the optimised nodes, f' = f(X'), rho = (f - f') / model decrease
 * (-inf if that is not positive), radius *= up if rho > high, *= down if rho < low, accept iff f' < f.  A step without an accepted
 * trial, or whose accepted trial has f - f' < decreasing * f, raises a count that any other step resets; stop at `patience`.  A
 * non-finite f leaves the nodes unchanged with status bits 2 | 32.  It reads ONE record of 64 bytes back per trial - that is its
 * synchronisation - and allocates nothing; the workspace (256-byte aligned) is the caller's.  info (host, may be null): rows of 8
 * float64 per trial {f, f', rho, radius, PCG iterations, PCG status, |r|/|g|, model decrease}, *n_info rows written.
 * The other four device calls allocate nothing, copy nothing to the host and never synchronise; none takes the stream's scratch. */
STA_API int sta_pgo_plan(int n, int E, int64_t out[8]);
STA_API int sta_sim3_op(sta_handle* h, int op, const double* a, const double* b, const uint8_t* mask, double* out, int64_t count, void* stream);
STA_API int sta_pgo_index(sta_handle* h, const int32_t* edges, const uint8_t* opt, int n, int E, void* workspace, int64_t workspace_bytes,
                          int32_t* off, int32_t* inc, int32_t* status, void* stream);
STA_API int sta_pgo_linearize(sta_handle* h, const double* nodes, const int32_t* edges, const double* poses, const double* confs, const uint8_t* opt,
                              const int32_t* off, const int32_t* inc, const int32_t* idx_status, int n, int E, int full, double* r, double* S, double* v,
                              double* c, double* g, double* blocks, double* rec, void* stream);
STA_API int sta_pgo_solve(sta_handle* h, const int32_t* edges, const uint8_t* opt, const int32_t* off, const int32_t* inc, const double* S, const double* g,
                          const double* blocks, int n, int E, double radius, double dmin, double dmax, double rtol, int max_iter, void* workspace,
                          int64_t workspace_bytes, double* d, double* stats, void* stream);
STA_API int sta_pgo_optimize(sta_handle* h, double* nodes, const int32_t* edges, const double* poses, const double* confs, const uint8_t* opt, int n, int E,
                             double radius, double dmin, double dmax, int steps, int patience, double decreasing, int reject, double high, double low,
                             double up, double down, double pcg_rtol, int pcg_max_iter, void* workspace, int64_t workspace_bytes, double* info,
                             int info_rows, int* n_info, int* status_out, void* stream);

/* The device-resident pose graph: PoseGraphNodes / PoseGraphEdges (vista_slam/pose_graph.py:5-54) and OnlineSLAM.connect_view_i_j
 * (slam.py:191-241), there host lists, a host copy of every node's maps, about a dozen small torch launches per node, .item() round
 * trips and pypose products.  Here the state lives in the caller's device arrays (sta_graph_state; Python: vista_slam_amd/graph.py),
 * allocated once.  The yardstick is the numpy restatement tests/graph_cases.py on the float64 group operations of tests/pgo_cases.py;
 * it is NOT pypose (which cannot be imported where this library is tested).  Stated differences from the reference: float64 state
 * (fp32 there); float64 sums in a fixed order (fp32 torch reductions there); one call per keyframe (one per edge there); the maps of
 * every node stay on the device (host there).
 * sta_graph_state: node poses float64 [max_nodes,8] in the (t, q, s) layout above; edges int64 [max_edges,2]; edge_poses float64
 * [max_edges,8]; edge_confs float64 [max_edges,7]; the map pool depth, conf fp32 [max_nodes,H,W] and intri fp32 [max_nodes,3,3];
 * mean_conf float64 [max_nodes]; per view first_node, best_node int32 [max_views] and best_conf float64 [max_views], max_views =
 * max_view_num + 1 (run.py:209 looks at the view count after the step that exceeds it); partials
 * float64 [32, chunks, 4], scratch of sta_graph_commit.  Every pointer is 16-byte aligned.  The host keeps the structure only: the
 * counts and, per view, the first node (it knows every accept / reject decision from the scheduler's read-back).
 * sta_graph_plan (host only): max_nodes = max_view_num (2 neighbor + loop), max_edges = max_view_num ((2 neighbor + loop - 1) +
 * ((2 neighbor + loop) / 2 + 1)) (slam.py:33-36); refused beyond sta_pgo_plan's limits (8192 nodes, 16384 edges), for H or W that is
 * not a positive multiple of 16, for max_view_num < 1, neighbor < 1 or loop < 0; the numbers are in sta_last_error().  out = {max_nodes,
 * max_edges, chunk (2048 map elements, whatever H W is), chunks = ceil(H W / chunk), poses bytes, edges bytes, edge_poses bytes,
 * edge_confs bytes, pool bytes (depth + conf + intri), mean_conf bytes, tables bytes, partials bytes, their total, max_views, 0, 0}.
 * sta_graph_reset: one launch: poses and edge_poses identity, edges -1, edge_confs 1, first_node = best_node = -1, best_conf = -100.
 * sta_graph_commit: connect_view_i_j for the k <= 16 candidate edges (view_i, view_j[e]) of one keyframe, in order.  Host arguments:
 * the counts before the call, first_i / first_j[e] (the views' first nodes, -1 for none), accepted[e], conf[e]; device: pose[e] 4x4,
 * and for an accepted edge depths[e], confs[e] fp32 [2,H,W] (side 0: view i) and intri[e] [3,3].  An accepted edge makes node n_i
 * then n_j (slam.py:210-215).  Two launches, no allocation, no copy to the host, no synchronisation:
 *   graph_reduce_kernel, grid (chunks, new nodes): one pass over the node's maps copies them to its pool slot and sums, per chunk,
 *     c, and for a view with a first node f: w Dn Df, w Dn Dn with w = max(cn cf, 1e-6), and sqrt(cn cf) (slam.py:224-227,
 *     pose_graph.py:41), every term in float64 from the fp32 inputs (w Dn first, then the second factor).  16-byte loads; a lane sums
 *     its elements in ascending order, a wave by a shuffle tree, the 4 waves in order; the chunk's partial is stored.  When the first
 *     node is made by an earlier edge of the SAME call its maps are read from the call's inputs, never from the slot being filled.
 *   graph_link_kernel, one wave: lane l sums the chunk partials of new node l in ascending chunk order; lane 0 walks the accepted
 *     edges in order: per node mean_conf = sum c / (H W), first_node, best node by strict > ; for a node with a first node f the
 *     scale edge (n, f) with measurement (0, identity, sum w Dn Df / sum w Dn Dn) and weights (2,2,2,2,2,2, sum sqrt / (H W)), and
 *     poses[n] = poses[f] * S; then sim3_ij = (t, q, 1) of pose[e] by sta_mat_to_se3's branch rule evaluated in float64;
 *     poses[n_i] = poses[n_j] * sim3_ij iff view i had no node before this edge; the pose edge (n_i, n_j, sim3_ij, conf x 7).
 *     Products are sta_sim3_op's multiplication, bit for bit.
 * A rejected edge leaves no trace.  Refused (-1): k outside [1, 16], view_j[e] >= view_i or repeated, view_i >= max_views, a first
 * node outside [-1, num_nodes), a missing or misaligned array of an accepted edge, a pool or edge store that would overflow.
 * sta_graph_export: one launch, grid (chunks, n_views): the best node of every view < n_views gathered into poses fp32 [n,4,4]
 * (rotation, translation), scales [n], depths, confs [n,H,W], intrinsics [n,3,3] - the arguments of sta_world_pointcloud; scaled:
 * depth * (float)scale; filter: depth = 0 where conf < thres (get_view, slam.py:313-320).  A view without a node gives zeros. */
typedef struct sta_graph_state {
    int32_t max_nodes, max_edges, max_views, H, W, chunks;
    double* poses;
    int64_t* edges;
    double* edge_poses;
    double* edge_confs;
    float* depth;
    float* conf;
    float* intri;
    double* mean_conf;
    int32_t* first_node;
    int32_t* best_node;
    double* best_conf;
    double* partials;
} sta_graph_state;
STA_API int sta_graph_plan(int max_view_num, int neighbor_edge_num, int loop_edge_num, int H, int W, int64_t out[16]);
STA_API int sta_graph_reset(sta_handle* h, const sta_graph_state* g, void* stream);
STA_API int sta_graph_commit(sta_handle* h, const sta_graph_state* g, int num_nodes, int num_edges, int view_i, int first_i, int k,
                             const int32_t* view_j, const int32_t* first_j, const uint8_t* accepted, const double* conf,
                             const float* const* pose, const float* const* depths, const float* const* confs, const float* const* intri,
                             int* num_nodes_out, int* num_edges_out, void* stream);
STA_API int sta_graph_export(sta_handle* h, const sta_graph_state* g, int n_views, int scaled, int filter, float thres, float* poses,
                             float* scales, float* depths, float* confs, float* intrinsics, void* stream);

/* keyframe scheduler = OnlineSLAM.regress_two_views (vista_slam/slam.py:153-189) for ALL k candidate
 * edges (i, j_e) of a new keyframe i (the neighbour loop slam.py:263-265 and the loop-closure loop :273-277) in one
 * batched launch sequence instead of k sequential B=1 calls, with the reference's early reject kept:
 *   decode (i, j_e) for e < k  ->  pose head on the ij side (slam.py:165)  ->  one k-float D2H read (the reference
 *   synchronises at the same point, slam.py:169)  ->  edge e is REJECTED iff pose_conf[e] < rel_pose_thres and
 *   !adjacent[e] (adjacent[e] = (i - j_e == 1), slam.py:169)  ->  DPT heads for both views of the accepted edges only
 *   ->  shared-per-pair intrinsics and depths (slam.py:182-185).
 * feat_i [N,1024] device, feat_j[e] [N,1024] device (encoder features cached by add_view, slam.py:142-151).
 * pose [k,16] device (pose_ij, 4x4 row-major, every edge).  pose_conf_host [k], slot_host [k], n_accepted: HOST
 * outputs, valid on return (the call synchronises `stream` once): slot_host[e] = -1 for a rejected edge, else the
 * compact index s of edge e in the per-accepted-edge outputs, all device:
 *   pts [n_acc,2,H,W,3] (view order [ij, ji] = torch.cat order of slam.py:182), conf [n_acc,2,H,W],
 *   K [n_acc,3,3] (shared over the pair's two views), depth [n_acc,2,H,W].
 * The buffers must be sized for k edges.  k <= 16.
 * Portrait frames (H > W): pts / conf / depth stay in image orientation [..,H,W,..]; the reference computes K on the
 * transposed views its head wrapper returns (utils/misc.py:60-61), i.e. with u = row - H/2 against X, v = col - W/2
 * against Y and the principal point (H/2, W/2) - K holds exactly that. */
STA_API int sta_regress_views(sta_handle* h, const float* feat_i, const float* const* feat_j, int k,
                      const uint8_t* adjacent, float rel_pose_thres, int H, int W,
                      float* pose, float* pose_conf_host, int* slot_host, int* n_accepted,
                      float* pts, float* conf, float* K, float* depth, void* stream);

/* The same call in two phases, so that the host can enqueue other work between them (e.g. the decode of the NEXT keyframe's
 * edges on another stream while this keyframe's DPT heads run; the next keyframe's edges need only encoder features):
 *   sta_regress_views_begin : gather + batched decode + pose head on `stream`; the k confidences travel to a pinned host
 *                             buffer behind an event.  No host synchronisation.  `pose` [k,16] device as above.
 *   sta_regress_views_finish: waits for that event only, takes the accept / reject decisions (slam.py:169), and enqueues the
 *                             DPT heads + intrinsics + depths of the accepted edges; host outputs valid on return.
 * The pending call owns its stream's scratch context: between begin and finish no other call of this handle may run on
 * THAT stream (it fails loudly); calls on other streams are fine.  sta_regress_views == begin immediately followed by finish. */
STA_API int sta_regress_views_begin(sta_handle* h, const float* feat_i, const float* const* feat_j, int k, int H, int W,
                            float* pose, void* stream);
STA_API int sta_regress_views_finish(sta_handle* h, const uint8_t* adjacent, float rel_pose_thres,
                             float* pose_conf_host, int* slot_host, int* n_accepted,
                             float* pts, float* conf, float* K, float* depth, void* stream);
/* Give up a call that was begun on `stream` (by sta_regress_views_begin or sta_regress_views_tokens_begin) and will not be finished (a host-side error between the phases): waits for
 * phase A's confidence copy, clears the pending state, the stream's scratch context is usable again.  Nothing pending on
 * `stream`: returns 0.  (vista_slam_amd.slam_scheduler.PendingEdges calls it from close() / __del__ / its context manager.) */
STA_API int sta_regress_views_abort(sta_handle* h, void* stream);

/* The keyframe scheduler on TOKEN SUBSETS: sta_regress_views with a SELECTION per edge and side, and every candidate with its own
 * frame size.  feat_i [Ni,E] is keyframe i's cached whole-frame encoding at Hi x Wi, feat_j[e] [Nj_e,E] candidate e's at Hj[e] x
 * Wj[e] (device, 16-byte aligned; Hj / Wj host arrays [k]).  Per side a HOST window array [k][4] = (y0, x0, h, w) in patches of that
 * frame's grid, row-major - the whole frame is (0, 0, hp, wp) -; h * w == 0 makes the side an INDEX LIST of cnt[e] >= 1 int64 indices
 * into the frame's row-major patch grid (any order, repeats allowed, out-of-grid values are clamped into the grid), read from that
 * side's packed DEVICE array idx_*: the lists of the index-list edges follow each other in edge order.  cnt_* (host [k]) is read for
 * index-list sides only; cnt_* / idx_* may be NULL when the side has none.  Selecting means SLICING the cached encoding (the tokens
 * have attended to the whole frame) and the positions are the tokens' (y, x) in their own frame's grid.
 * Edge e is regress_two_views (slam.py:153-189) at B = 1 on the two slices: _decode_stereo, head_pose_s on side i's pose token ->
 * pose [k,16] (device) and pose_conf_host[k]; REJECTED iff pose_conf < rel_pose_thres and !adjacent[e]; for an accepted edge each
 * WINDOW side runs head_pts at the shape (16 h, 16 w); an index-list side has no maps.  Host outputs, valid on return:
 * pose_conf_host[k], accepted_host[k] (0 / 1), n_accepted, k_valid_host[k].
 * pts / conf / depth: ONE device buffer each, the maps of the window sides of ALL k edges in (edge, side) order, so the offsets follow
 * from the shapes the caller passed: a window side of h x w patches occupies 256 h w pixels (x 3 floats in pts), image orientation
 * [16 h, 16 w]; an index-list side occupies nothing.  The ranges of rejected edges are NOT written.  An accepted edge whose two sides
 * are windows of one (h, w) has its two maps adjacent in the reference's [ij, ji] order (slam.py:182) and gets the pair-shared
 * intrinsics K[e] [3,3] with k_valid_host[e] = 1: estimate_intrinsic_from_pts3d of those two maps, i.e. the principal point is the
 * centre of the WINDOW's image (8 w, 8 h), not of the frame; h > w follows the portrait rule of sta_regress_views.  Every other edge
 * has k_valid_host[e] = 0 and K[e] untouched (the reference concatenates the two maps, which two shapes do not allow).
 * Two phases like sta_regress_views_begin / _finish, on the same pending state: a begin of either kind fails while a call of either
 * kind is pending on the stream, a finish of the other kind fails and leaves the call pending, sta_regress_views_abort releases both.
 * One lane of decode; NOT covered by sta_reserve (like sta_decode_varlen: the first call of a set of counts plans and may grow the
 * stream's workspace).  Returns -1 for: null pointers, k outside [1, 16], H or W not a multiple of 16, a window that leaves its
 * grid, a count below 1, features not 16-byte aligned, 2^31 or more decoder rows. */
STA_API int sta_regress_views_tokens(sta_handle* h, const float* feat_i, int Hi, int Wi,
                             const float* const* feat_j, const int* Hj, const int* Wj, int k,
                             const int* win_i, const int* cnt_i, const int64_t* idx_i,
                             const int* win_j, const int* cnt_j, const int64_t* idx_j,
                             const uint8_t* adjacent, float rel_pose_thres,
                             float* pose, float* pose_conf_host, int* accepted_host, int* n_accepted,
                             float* pts, float* conf, float* depth, float* K, int* k_valid_host, void* stream);
STA_API int sta_regress_views_tokens_begin(sta_handle* h, const float* feat_i, int Hi, int Wi,
                                   const float* const* feat_j, const int* Hj, const int* Wj, int k,
                                   const int* win_i, const int* cnt_i, const int64_t* idx_i,
                                   const int* win_j, const int* cnt_j, const int64_t* idx_j,
                                   float* pose, void* stream);
STA_API int sta_regress_views_tokens_finish(sta_handle* h, const uint8_t* adjacent, float rel_pose_thres,
                                    float* pose_conf_host, int* accepted_host, int* n_accepted,
                                    float* pts, float* conf, float* depth, float* K, int* k_valid_host, void* stream);

/* the compact per-pair record of one step's all-gather (vista_slam_amd/parallel.py; what a SLAM consumer
 * reads of a pair, slam.py:165-185), packed from the outputs of sta_forward_pair* in one launch.  Row b of out_dev
 * (rows `row_stride` floats apart, >= 2 * (17 + 2*H*W)) = for view 0 (main) then view 1 (support):
 * pose[16] | pose_conf | depth = pts[..., 2] [H*W] | conf [H*W].  Inputs as sta_forward_pair wrote them (image orientation). */
STA_API int sta_pack_compact(sta_handle* h, const float* const pts[2], const float* const conf[2], const float* const pose[2],
                     const float* const pose_conf[2], int B, int H, int W, float* out_dev, int64_t row_stride, void* stream);

/* In-place 2-D RoPE on fp32 tokens (B,N,Hh,D) with element strides (stride of D must be 1,
 * stride of Hh must be D; same contract as kernels.cu:91-94); pos int64 [B,N,2] contiguous. */
STA_API int sta_rope2d_inplace(float* tokens_dev, int64_t stride_b, int64_t stride_n,
                       const int64_t* pos_dev, int B, int N, int Hh, int D,
                       float base, float fwd, void* stream);
/* The same for the token dtypes curope dispatches on (AT_DISPATCH_FLOATING_TYPES_AND_HALF, kernels.cu:101): STA_DTYPE_F16,
 * STA_DTYPE_F32, STA_DTYPE_F64.  Like the reference kernel (kernels.cu:33-79: float shared memory, float cos / sin) the
 * rotation is evaluated in fp32 whatever the storage type; strides are in ELEMENTS of that type. */
STA_API int sta_rope2d_inplace_dtype(void* tokens_dev, int dtype, int64_t stride_b, int64_t stride_n,
                             const int64_t* pos_dev, int B, int N, int Hh, int D,
                             float base, float fwd, void* stream);

/* Algorithmic FLOPs of one pair at H x W for this handle's config (SURVEY.md 8d closed form). */
STA_API double sta_flops_per_pair(const sta_handle* h, int H, int W);

/* Bytes currently held by the internal workspace / by packed weights. */
STA_API int64_t sta_workspace_bytes(const sta_handle* h);
STA_API int64_t sta_weight_bytes(const sta_handle* h);

/* Per-stage device timing (hipEvent) of the most recent sta_forward_pair when enabled:
 * ms[0]=encode(both views) ms[1]=decode ms[2]=pose heads ms[3]=dpt heads.  Enabling inserts event
 * records on the stream; reading synchronises on the last event. */
STA_API int sta_enable_stage_timing(sta_handle* h, int on);
STA_API int sta_get_stage_ms(sta_handle* h, float ms[4]);

/* Per-launch hipEvent timing of the dominant kernel (gemm_kernel<.., dense, fp32 epilogue>: the
 * proj / fc2 / embed GEMMs) on the stream it is launched on.  enable!=0 resets the counters and
 * starts recording; sta_kernel_timing_read synchronises on the recorded events and returns the
 * number of launches, the summed kernel time, the summed algorithmic FLOPs (2*M*N*K) and bytes.
 * tile_family selects ONE kernel symbol: 1 = gemm_kernel (128x128), 2..5 = gemm2_kernel 256x256,
 * 256x128, 192x256, 192x128; 0 = all of them. */
STA_API int sta_kernel_timing(sta_handle* h, int enable);
STA_API int sta_kernel_timing_read(sta_handle* h, int tile_family, int* launches, double* total_ms, double* total_flops,
                           double* total_algorithmic_bytes);
/* Effective shader clock (GHz) inside the timed launches of the dominant kernel since sta_kernel_timing(h, 1):
 * s_memtime cycles per 100 MHz s_memrealtime tick, summed over every 64th workgroup.  The chip clocks to its power
 * budget, so the MFMA peak actually available to a kernel is 2.5 PF x clock / 2.4 GHz. */
STA_API int sta_kernel_clock_read(sta_handle* h, float* ghz_out);

/* Every GEMM / convolution launch after sta_kernel_timing(h, 2) as a record (bench.py's survey step and roofline block;
 * tools/): shape6 = {M, N, K, epilogue id, A-loader id (0 dense, 1 conv3x3), 1 if the launch ran in the f16mx arithmetic};
 * variant = tile family (1 = 128x128 register-staged, 2 = 256x256 / 16 waves, 3 = 192x256 / 12 waves, 5 = 192x128 / 8 waves,
 * 6 = 128x64 small-grid ring, 7 = gemm2_pair_kernel: two 192x128 GEMMs in one launch, 8 = halo-tiled 3x3 convolution). */
STA_API int sta_kernel_timing_dump_shapes(sta_handle* h, int cap, int* shape6, float* ms, int* variant, int* n_out);
/* Restrict the per-launch timing to ONE kernel symbol {epilogue id, A-loader id, tile family, f16mx flag}; then
 * sta_kernel_timing(h, 3) times every `every`-th launch of that symbol (bench.py: the dominant kernel inside the timed
 * region.  An event pair costs ~9 us of dispatch - tools/probes/boundary_probe.hip: 11.4 vs 2.7 us per launch -, so the
 * timed region samples one launch in four instead of paying that on all 36 per step). */
STA_API int sta_kernel_timing_filter(sta_handle* h, int epilogue, int a_mode, int family, int mx, int every);

STA_API const char* sta_last_error(void);
STA_API const char* sta_version(void);

#ifdef __cplusplus
}
#endif
#endif /* STA_MI355_H */
