// Launch layer of the STA path: tile-family cost model (pick_family), launch_gemm and the GEMM / convolution / LayerNorm / attention
// wrappers the orchestration code calls.  Included by sta_api.hip (one translation unit; needs its types and macros).
// ------------------------------------------------------------------------------------------ tile families
// THE table of tile families: block tile BM x BN, WMS x WNS waves, NSTG stages of the LDS-DMA ring.  plan_tiles, the dispatch of
// launch_gemm, the row-tail rule and the paired launch all read it, so a family's shape is stated here and nowhere else (the
// cost model above pick_family keeps its own measured constants).  The kernels' template arguments are these numbers in this
// order: bench.py and the tools match kernel symbols by them.  Not part of the table, because no family owns them: the 32-pixel
// width of a halo tile (conv3h.h tiles an image in BM / 32 rows x 32 pixels for every Cout), the 32 rows a row tail may have, and
// the chip's 256 CUs (the grid up to which family 6 runs on 8 waves, gemm_plan; the K-slice targets of sg_slices).
struct TileFamily { int id, bm, bn, wms, wns, nstg; };
constexpr TileFamily FAM1{1, GEMM_BM, GEMM_BN, 2, 2, 1};      // gemm.h: 128x128 register-staged, 256 threads (N % 128 != 0)
constexpr TileFamily FAM2{2, 256, 256, 4, 4, 2};
constexpr TileFamily FAM3{3, 192, 256, 3, 4, 2};
constexpr TileFamily FAM5{5, 192, 128, 2, 4, 2};
constexpr TileFamily FAM6{6, 128, 64, 2, 2, 3};               // small grids: 4 waves ...
constexpr TileFamily FAM6_LONE{6, 128, 64, 4, 2, 3};          // ... or 8 where every workgroup is alone on its CU (GemmPlan::lone)
constexpr TileFamily FAM7{7, FAM5.bm, FAM5.bn, FAM5.wms, FAM5.wns, FAM5.nstg};      // two 192x128 GEMMs in one grid (gemm_qkv_pair)
constexpr TileFamily FAM8{8, 256, 256, 4, 4, 0};              // conv3h.h: BM / 32 rows x 32 pixels of one image, Cout = 256 ...
constexpr TileFamily FAM8_N128{8, 256, 128, 4, 4, 0};         // ... and Cout = 128
constexpr TileFamily NO_FAMILY{0, 0, 0, 0, 0, 0};
constexpr int TAIL_BN = 32;                                   // columns of one skinny row-tail block (gemm2.h: gemm2_tail)
constexpr const TileFamily* FAMILIES[] = {&FAM1, &FAM2, &FAM3, &FAM5, &FAM6, &FAM7, &FAM8};
constexpr const TileFamily& tile_family(int id, int N = 0) {      // (the planner's view: family 6 by its 4-wave row, family 8 by Cout)
    if (id == FAM8.id && N == FAM8_N128.bn) return FAM8_N128;
    for (const TileFamily* f : FAMILIES) if (f->id == id) return *f;
    return NO_FAMILY;
}
// THE existence predicate: is there a kernel for this loader / epilogue / tile family / arithmetic?  gemm_plan asks it at run
// time; the dispatch of launch_gemm asks it in `if constexpr`, so what it denies is never instantiated and what it admits
// must compile (tests/test_gemm_dispatch_table.py holds the library's kernel symbols to it).
//   * launch_gemm exists for the six dense epilogues and for the plane and fused-head epilogues of the 3x3 convolution;
//   * f16mx kernels exist for the DPT head's epilogues and (precision f16x3m) for the fp32 / in-place-residual epilogues of dense
//     GEMMs: mlp.fc2.  The latter not on 256x256 (compile time), none on the register-staged family;
//   * the RoPE epilogue exists on the 192x128 / 128x64 / 128x128 tiles only, the fused head on 192x128 and the Cout = 128 halo form;
//   * the 8-wave small-grid form exists in the split arithmetics only;
//   * family 7 is not a launch_gemm kernel (gemm_qkv_pair launches it under qkv_pair_plan).
// Dead rows: (dense, EPI_F32R, family 6), both wave forms, all three arithmetics - five kernels - are admitted and instantiated but
// no caller plans them: gemm_f32 (and sta_bench.inc) launch EPI_F32R only above the small-grid predicate, and family 6 is planned only
// below it.  They stay because this table must describe the kernel list as it is; dropping them is a change of that list.
constexpr bool has_kernel(int amode, int epi, const TileFamily& f, bool mx, bool split) {
    const bool f32 = epi == EPI_F32 || epi == EPI_F32R;
    if (amode == A_CONV3 ? !(epi == EPI_F16 || epi == EPI_HEAD) : !(amode == A_DENSE && epi >= EPI_F32 && epi <= EPI_F32R)) return false;
    if (mx && !(epi == EPI_F16 || epi == EPI_CONVT || epi == EPI_HEAD || f32)) return false;
    switch (f.id) {
        case 1: return !mx && epi != EPI_HEAD;
        case 2: return epi != EPI_QKV && epi != EPI_HEAD && !(mx && f32);
        case 3: return epi != EPI_QKV && epi != EPI_HEAD;
        case 5: return true;
        case 6: return epi != EPI_HEAD && (f.wms == FAM6.wms || split || mx);
        case 8: return amode == A_CONV3 && (epi == EPI_F16 || f.bn == FAM8_N128.bn);
        default: return false;
    }
}
// ... with the shape: the halo form runs stride 1 at Cout = its tile width, the fused head needs all 128 channels in one tile
constexpr bool gemm_has_kernel(int amode, int epi, int family, bool mx, bool split, int N, int cstride) {
    const TileFamily& f = tile_family(family, N);
    return has_kernel(amode, epi, f, mx, split) && (f.id == 8 ? cstride == 1 && N == f.bn : epi != EPI_HEAD || N == f.bn);
}
#ifdef STA_TEST_HOOKS
extern "C" int sta_debug_gemm_has_kernel(int amode, int epi, int family, int mx, int split, int N, int cstride) {
    return gemm_has_kernel(amode, epi, family, mx != 0, split != 0, N, cstride) ? 1 : 0;
}
#endif

// ------------------------------------------------------------------------------------------ launch helpers
// Raises a kernel's dynamic-LDS limit once per device (one bit each: the attribute is set on the current device's copy of the
// function).  The static belongs to the instantiation, i.e. to the kernel.
template <auto Kernel>
static int set_smem_once(int dev, int bytes) {
    static unsigned done = 0;
    if (!(done >> (dev & 31) & 1u)) {
        HIPCHK(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        done |= 1u << (dev & 31);
    }
    return 0;
}
template <bool SPLIT, int AMODE, int EPI, int BM, int BN, int WMS, int WNS, int NSTG = 2, bool MX = false>
static int launch_gemm2(const GemmParams& p, hipStream_t st, int dev = 0, const VlGeo* geo = nullptr) {
    constexpr int smem = gemm2_smem_bytes<SPLIT, BM, BN>(NSTG);
    const int tm = (p.M - p.m_tail + BM - 1) / BM, tn = (p.N + BN - 1) / BN, ks = p.ksplit > 1 ? p.ksplit : 1;
    const int ntail = p.m_tail > 0 ? (p.N + TAIL_BN - 1) / TAIL_BN : 0;     // skinny tail blocks (gemm2_tail), first in the grid
    const dim3 grid((unsigned)(tm * tn * ks + ntail)), block(WMS * WNS * 64);
    if (geo) {      // the varlen form of the same tile family (sta_head_pts_varlen): same grid, the geometry table next to the parameters
        if constexpr (SPLIT && (AMODE == A_CONV3 || EPI == EPI_CONVT)) {
            constexpr auto kern = gemm2_kernel<SPLIT, AMODE, EPI, BM, BN, WMS, WNS, 0, NSTG, MX, VlGeo>;
            CHK(set_smem_once<kern>(dev, smem));
            REQUIRE(p.m_tail == 0, "internal: a varlen launch has no row tail");
            hipLaunchKernelGGL(kern, grid, block, smem, st, p, *geo);
            return 0;
        } else REQUIRE(false, "internal: no varlen form of this GEMM (precision f16, or an epilogue that decodes no geometry)");
    }
    constexpr auto kern = gemm2_kernel<SPLIT, AMODE, EPI, BM, BN, WMS, WNS, 0, NSTG, MX>;
    CHK(set_smem_once<kern>(dev, smem));
    hipLaunchKernelGGL(kern, grid, block, smem, st, p);
    return 0;
}

template <bool SPLIT, int EPI, int BM, int BN, bool MX, int WMS = 4, int WNS = 4>
static int launch_conv3h(const GemmParams& p, hipStream_t st, int dev, const VlGeo* geo = nullptr) {
    constexpr int smem = conv3h_smem_bytes<SPLIT, BM, BN>();
    static_assert(smem <= 160 * 1024, "conv3h: LDS budget");
    if (geo) {      // the varlen form: tiles = the sum of every entry's own tiles
        if constexpr (SPLIT) {
            constexpr auto kv = conv3h_kernel<SPLIT, EPI, BM, BN, WMS, WNS, MX, VlGeo>;
            CHK(set_smem_once<kv>(dev, smem));
            const int64_t tiles = (int64_t)vl_tiles(*geo, BM / 32) * ((p.N + BN - 1) / BN);
            REQUIRE(tiles > 0 && tiles < ((int64_t)1 << 31), "internal: conv3h varlen grid");
            hipLaunchKernelGGL(kv, dim3((unsigned)tiles), dim3(WMS * WNS * 64), smem, st, p, *geo);
            return 0;
        } else REQUIRE(false, "internal: the varlen halo-tiled convolution has no precision-f16 form");
    }
    constexpr auto kern = conv3h_kernel<SPLIT, EPI, BM, BN, WMS, WNS, MX>;
    CHK(set_smem_once<kern>(dev, smem));
    const int n_img = p.M / (p.Ho * p.Wo);
    const int tiles = n_img * ((p.Ho + BM / 32 - 1) / (BM / 32)) * ((p.Wo + 31) / 32) * ((p.N + BN - 1) / BN);
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(WMS * WNS * 64), smem, st, p);
    return 0;
}
// family 1: the register-staged kernel of gemm.h
template <bool SPLIT, int AMODE, int EPI>
static int launch_gemm1(const GemmParams& p, hipStream_t st, int dev) {
    constexpr auto kern = gemm_kernel<SPLIT, AMODE, EPI>;
    if constexpr (SPLIT) CHK(set_smem_once<kern>(dev, gemm_smem_bytes<SPLIT>()));      // (the f16 form fits the default limit)
    const int tm = (p.M + FAM1.bm - 1) / FAM1.bm, tn = (p.N + FAM1.bn - 1) / FAM1.bn;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tm * tn)), dim3(FAM1.wms * FAM1.wns * 64), gemm_smem_bytes<SPLIT>(), st, p);
    return 0;
}

// mode 3 of sta_kernel_timing: does this matching launch carry the event pair?  A 1-in-kevery sample drawn by a multiplicative
// hash of the launch counter, not `counter % kevery`: with 36 matching launches per step and every = 4 the modulo form timed the
// same 9 launch positions of every step (ADVICE r5: a phase-locked sample is biased when the symbol's launches differ by layer
// or by L2 state); the hash has no period that a step's launch count can lock onto.
static inline bool ksample(sta_handle* h) {
    const unsigned k = (unsigned)h->kseen++;
    return h->kevery <= 1 || ((k * 2654435761u) >> 15) % (unsigned)h->kevery == 0;
}
static inline bool auto_family(const sta_handle* h) { return h->gemm_variant == 0 || h->gemm_variant == 9; }

// The ONE small-grid predicate (SLAM scale: 224x224, batch 1..8 -> M = 196..3200 rows; the DPT levels with <= 12288 pixels
// at any scale): below it the 128x64 split-K family runs (launch_gemm), in-place residual GEMMs hand their K slices to
// resid_ln_kernel (gemm_resid_ln), and the specialised throughput epilogues / the paired launch are not used (gemm_f32,
// gemm_qkv_pair).  Threshold measured (profiles/r03_tile_table.txt): with fewer than 192 tiles of 192x128 the 128x64 family is
// 15-40 % faster (162 tiles: 36 vs 45 us; 136: 113 vs 144 us; 128: 113 vs 133 us), from 216 tiles on it is slower.
static inline bool small_grid_m(int mode, int64_t M, int N) {
    if (mode == 1) return false;
    const int64_t t = ((M + 191) / 192) * (int64_t)((N + 127) / 128);
    if (mode == 2) return M <= 2560 || t < 512;
    return M <= 640 || t < 192;
}
// K slices of a small-grid GEMM with tiles_r output tiles: about one workgroup per CU and never more than 256 of them while that
// still splits (256 / tiles_r >= 2: the grid stays "lone" and runs the 8-wave form, launch_gemm); between 128 and 256 tiles a
// GEMM whose K slices would need a finisher kernel of their own (QKV, plane epilogues) is not split at all - the finisher is a
// dispatch (5 - 7 us) for a K loop that two slices shorten by less -, one whose slices are summed by the LayerNorm kernel that
// follows anyway (in-place residual GEMMs) takes two.  Measured against ceil(256 / tiles_r) everywhere: encode -2 %, 5-edge
// scheduler -1.7 %, one pair @224 +3.5 %, one pair @512x384 +1 %.  old_rule (h->opt[1] == 1): the old rule (A/B).
static inline int sg_slices(bool old_rule, int tiles_r, bool own_finisher = false) {
    if (!old_rule) { const int f = 256 / tiles_r; if (f >= 2) return f; if (own_finisher) return 1; }
    return (256 + tiles_r - 1) / tiles_r;
}
static inline bool small_grid(const sta_handle* h, int64_t M, int N) { return small_grid_m(h->small_grid_mode, M, N); }

// Tile-family choice = a quantisation-aware cost model calibrated on profiles/r03_tile_table.txt (tools/tile_table.py: every
// GEMM / convolution shape of the forward at B in {1,2,4,8} x {224x224, 384x512}, in-model HIP-event durations under every forced
// family; tests/test_tile_table.py replays the table through this function).  Every family saturates at the same 300-400
// algorithmic TFLOP/s (the chip is power-bound on this instruction mix, DESIGN.md section 5), so a launch costs
//     rounds x tile area / rate,   rounds = ceil(tiles / 256 CUs),
// `rate` = the family's measured advantage on that class of GEMM at a full grid, x a penalty when the last round is < 90 %
// full (one-workgroup-per-CU families lose more there than 192x128, whose second resident workgroup evens the CUs out):
//   5: 192x128, 8 waves, two workgroups per CU (one block's HBM-bound epilogue hides under the other's main loop): rate 1;
//   3: 192x256, 12 waves, one workgroup per CU, 30 % less L2->LDS traffic per FLOP: +2 % mlp.fc1 (GELU), +4 % the long-K
//      in-place-residual GEMMs (mlp.fc2), +6 % the Cout = 256 convolutions with K >= 1728;
//   2: 256x256, 16 waves: +5 % mlp.fc1, +10 % those convolutions, -10 % the in-place-residual epilogue;
//   8: halo-tiled 3x3 convolution (conv3h.h; 8 x 32-pixel tiles of one image): +12 % at Cout = 256 (x1.47 from three
//      well-filled rounds on), equal at Cout = 128
//      (head.0: ties go to the halo form, which moves 1.3x instead of 6.5x the algorithmic bytes), +12 % with the fused head epilogue (round 6);
//   6: small-grid family (predicate above);  1: 128x128 register-staged kernel: N not a multiple of 128;
//   7 (paired 192x128 launch) is chosen by gemm_qkv_pair.
struct FamilyQuery { int amode, epi; int64_t M; int N, K; int split, cstride, Ho, Wo; int sg_mode; int head_gemm = 0; };      // head_gemm: experiment switch 0 (A/B)
static int pick_family(const FamilyQuery& q) {
    const bool sg = small_grid_m(q.sg_mode, q.M, q.N) && q.N % 64 == 0;
    if (q.N % 128 != 0) return sg ? 6 : 1;
    if (sg) return 6;
    auto cost = [](int64_t tiles, int area, double rate, double pen) {
        const int64_t rounds = (tiles + 255) / 256;
        const double fill = (double)tiles / (double)(rounds * 256);
        return (double)rounds * area / (rate * (fill < 0.9 ? pen : 1.0));
    };
    auto tiles = [&](int bm, int bn) { return ((q.M + bm - 1) / bm) * (int64_t)((q.N + bn - 1) / bn); };
    int best = 5;
    double cbest = cost(tiles(192, 128), 192 * 128, 1.0, 0.96);
    auto consider = [&](int fam, double c) { if (c <= cbest) { cbest = c; best = fam; } };      // ties: the later (larger) family
    if (q.split && q.N % 256 == 0 && q.epi != EPI_QKV) {
        double r3 = 0, r2 = 0;
        if (q.amode == A_DENSE && q.epi == EPI_GELU) { r3 = 1.02; r2 = 1.05; }
        else if (q.amode == A_DENSE && q.epi == EPI_F32R && q.K >= 2048) { r3 = 1.04; r2 = 0.9; }
        else if (q.amode == A_CONV3 && q.N == 256 && q.K >= 2304) { r3 = 1.06; r2 = 1.10; }      // (round 6: not the K = 1728 level any more - 192x128 is 14 % faster there)
        else if (q.amode == A_DENSE && q.epi == EPI_F16) { r3 = 1.0; r2 = 1.0; }      // 1x1 convolutions of the head: quantisation only ...
        if (r3 > 0) {
            // ... except that a one-workgroup-per-CU family in a SINGLE round has nothing to hide its plane epilogue under (K = 256: the
            // epilogue is most of the launch; 49152 x 256 x 256: 41 us on 192x256 against 33 on 192x128, profiles/r06_tile_table.txt)
            const double lone = (q.amode == A_DENSE && q.epi == EPI_F16) ? 0.85 : 1.0;
            consider(3, cost(tiles(192, 256), 192 * 256, tiles(192, 256) <= 256 ? r3 * lone : r3, 0.93));
            consider(2, cost(tiles(256, 256), 256 * 256, tiles(256, 256) <= 256 ? r2 * lone : r2, 0.93));
        }
    }
    if (q.amode == A_CONV3 && (q.epi == EPI_F16 || q.epi == EPI_HEAD) && q.cstride == 1 && (q.N == 128 || q.N == 256) &&
        q.Wo >= 32 && q.M >= 16384 && q.Ho > 0) {
        const int64_t imgs = q.M / ((int64_t)q.Ho * q.Wo);
        const int64_t t8 = imgs * ((q.Ho + 7) / 8) * ((q.Wo + 31) / 32);
        if (q.N == 256) {
            // +12 % per tile against 192x128 in general (a single round: equal to 192x256 within the +-3 % the boxes differ by,
            // which keeps its choice there), 1.47x from three well-filled rounds on (196608 pixels: 539 vs 576 / 640 us)
            const int64_t rounds = (t8 + 255) / 256;
            const double fill = (double)t8 / (double)(rounds * 256);
            // (round 6: in a single round the halo form no longer beats the 256x256 implicit GEMM, whose loop gained more from the
            //  compile-time ReLU - 50176 pixels: 161 - 169 vs 147 - 153 us)
            consider(8, (double)rounds * 256 * 256 / (fill >= 0.7 && rounds >= 3 ? 1.47 : (rounds == 1 ? 1.0 : 1.12)));
        } else {
            // fused DPT tail (round 6, after the transposed-accumulator epilogue; profiles/r06_tile_table.txt): the halo form is 3 - 20 % faster
            // from 100 K to 800 K pixels (one pair @224 ... one pair @512x384: 160 vs 175, 284 vs 314, 254 vs 290 us), equal from 1.5 M
            // pixels on - where it moves 1.25x instead of 6.6x the algorithmic bytes
            // ... and at the benchmark's 3.1 M pixels the implicit-GEMM form, whose second resident workgroup hides the epilogue, is 2.4 - 4.8 %
            // faster again (2043 - 2071 vs 2120 - 2180 us, two boxes) although it moves 6.6x instead of 1.25x the algorithmic bytes
            consider(8, cost(t8, 256 * q.N, q.epi == EPI_HEAD ? (q.M >= (1 << 21) && q.head_gemm ? 0.95 : 1.12) : 1.0, 0.96));
        }
    }
    return best;
}
#ifdef STA_TEST_HOOKS
extern "C" int sta_debug_pick_family(int amode, int epi, long long M, int N, int K, int split, int cstride, int Ho, int Wo) {
    FamilyQuery q{amode, epi, M, N, K, split, cstride, Ho, Wo, 0};
    return pick_family(q);
}
#endif

// ------------------------------------------------------------------------------------------ launch plan
// Everything launch_gemm decides before it launches - tile family, tile size, the pose-token row tail, K slices - as ONE pure host
// function of the shape and the handle's switches: launch_gemm runs exactly this plan, sta_debug_gemm_plan exposes it to the
// host-only sweep (tests/test_gemm_plan.py) and sta_debug_last_gemm_plan reads back the plan of a handle's last launch.
// The plan itself: struct GemmPlan (sta_api.hip, next to the handle that keeps the last one).
struct PlanQuery {
    int amode, epi; int M, N, K;                // M: every row, the tail rows included
    bool split, mx;                             // split: f16x3 / f16x3h / f16x3m;  mx: f16mx rows and weights
    int tail_hint, forced;                      // forced: sta_set_gemm_variant (0 / 9: automatic)
    int sg_mode, head_gemm, old_slices;         // h->small_grid_mode, h->opt[0] == 1, h->opt[1] == 1
    bool deterministic;
    int inplace;                                // EPI_F32 added in place to its residual: 0 no, 1 with a caller slab, 2 without
    int cstride, Ho, Wo;                        // convolutions only
    int lone_opt = 0;                           // h->opt[2]: 1 = never the 8-wave small-grid form, > 1 = its grid limit (A/B)
    int geo_tiles = -1;                         // varlen launch under forced family 8: halo tiles of the entry table (else -1)
};
// geo_tiles >= 0: the row tiles of a varlen halo launch (every entry's own tiles) instead of those of whole images
static GemmPlan plan_tiles(int family, int M, int m_tail, int N, int Ho, int Wo, int geo_tiles = -1) {
    const TileFamily& f = tile_family(family, N);
    GemmPlan g{family, f.bm, f.bn, m_tail, 0, 0, 1, 0};
    if (g.bm == 0) return g;
    const int rows = f.bm / 32;      // family 8: rows x 32 pixels of one image
    if (family == 8) g.tiles_m = geo_tiles >= 0 ? geo_tiles : (int)((int64_t)M / ((int64_t)Ho * Wo) * ((Ho + rows - 1) / rows) * ((Wo + 31) / 32));
    else g.tiles_m = (M - m_tail + g.bm - 1) / g.bm;
    g.tiles_n = (N + g.bn - 1) / g.bn;
    return g;
}
static int gemm_plan(const PlanQuery& q, GemmPlan& out) {
    if (q.geo_tiles >= 0 && q.forced == 8 && gemm_has_kernel(q.amode, q.epi, 8, q.mx, q.split, q.N, q.cstride)) {
        // the halo-tiled family on a varlen launch (forced: the cost model, which counts the tiles of ONE image size, never proposes it
        // there): rows x 32 pixels of one ENTRY per tile, the tiles of all entries in one grid
        out = plan_tiles(8, q.M, 0, q.N, q.Ho, q.Wo, q.geo_tiles);
        return 0;
    }
    // Row tail hint (decode_impl: the 2B pose-token rows after the 2B x N patch rows).  Tile rules below look at the patch
    // rows; the tail is kept only where the FINAL family tiles them exactly and has tail blocks (checked last).
    const bool mx_f32 = q.epi == EPI_F32R || q.epi == EPI_F32;       // mlp.fc2 in the f16mx arithmetic (precision f16x3m)
    int m_tail = 0;
    if (q.amode == A_DENSE && q.tail_hint > 0 && q.tail_hint <= 32 && q.M > q.tail_hint && (!q.mx || mx_f32) && q.N % FAM5.bn == 0 && q.forced != 1) {
        if (!small_grid_m(q.sg_mode, q.M - q.tail_hint, q.N)) m_tail = q.tail_hint;   // throughput scale only (the small-grid family splits K instead)
    }
    const int M = q.M - m_tail;
    // Tile family (pick_family above: cost model calibrated on the measured table); a forced family never displaces the
    // small-grid one, whose split-K plumbing the callers rely on
    const FamilyQuery fq{q.amode, q.epi, M, q.N, q.K, q.split ? 1 : 0, q.cstride, q.Ho, q.Wo, q.sg_mode, q.head_gemm};
    int variant = pick_family(fq);
    if (q.forced == 9 && variant == 8) { FamilyQuery f2 = fq; f2.Wo = 0; variant = pick_family(f2); }     // A/B: no halo kernel
    int ksplit = 1, slab_ks = 0;
    // Small grids (SLAM scale: 224x224, batch 1..8 -> M = 196..3200 rows; the coarse DPT levels at any scale): 128x64 tiles,
    // 3-stage DMA ring, and split-K so that ~256 workgroups stream the weights once instead of 16-64 workgroups looping over
    // all of K.  The K slices go to fp32 SLABS that the next kernel sums (resid_ln_kernel / qkv_finish_kernel /
    // splitk_finish_kernel: fixed order, bit-reproducible) - the product path.  Only an in-place residual GEMM whose caller
    // passed no slab (forced tile families, N > 1024) still adds its slices with fp32 atomics, and not in deterministic mode.
    if (variant == 6) {
        const int tiles_r = ((M + FAM6.bm - 1) / FAM6.bm) * (q.N / FAM6.bn);
        const int tiles = q.deterministic ? (1 << 30) : tiles_r;    // deterministic: no ATOMIC split-K (the slab forms below have a fixed order)
        if (q.amode == A_DENSE && q.epi == EPI_F32 && q.inplace == 1) {
            // the caller finishes the GEMM in the LayerNorm kernel that follows (gemm_resid_ln): slices store partial tiles
            // to slabs instead of atomically adding to the residual stream (the device-scope fp32 atomics of 256 workgroups
            // cost more than the 4-32 K tiles of a slice); fixed summation order -> also taken in deterministic mode
            // (swept at M = 196 / 394 / 1970: a target of 128 / 192 / 256 / 384 / 512 workgroups -> encode 2.50 / 2.40 / 2.38 /
            // 2.49 / 2.55 ms: one workgroup per CU; more slices cost more slab traffic than their shorter K loops save)
            int ks = tiles_r < 256 ? sg_slices(q.old_slices, tiles_r) : 1;
            const int max_ks = q.K / 128;                 // keep >= 4 K tiles per slice
            if (ks > max_ks) ks = max_ks;
            while (ks > 1 && (int64_t)ks * M * q.N > SKBUF_ELEMS) --ks;
            if (ks > 1) { ksplit = ks; slab_ks = ks; }
        } else if (q.amode == A_DENSE && q.epi == EPI_F32 && q.inplace == 2 && tiles < 256) {
            int ks = (256 + tiles - 1) / tiles;
            const int max_ks = q.K / 128;                 // keep >= 4 K tiles per slice
            if (ks > max_ks) ks = max_ks;
            if (ks > 1) ksplit = ks;
        }
        // QKV-epilogue GEMMs (attn.qkv, cross_attn.projq / projk|projv) on small grids: K slices to slabs, qkv_finish_kernel
        // applies bias + RoPE and writes Q / K / V^T (un-split attn.qkv at M = 196: 96 workgroups x 32 K tiles = 25 us)
        if (q.amode == A_DENSE && q.epi == EPI_QKV && tiles_r <= 192 && q.K >= 512) {
            int ks = sg_slices(q.old_slices, tiles_r, true);
            const int max_ks = q.K / 256;                 // keep >= 8 K tiles per slice
            if (ks > max_ks) ks = max_ks;
            while (ks > 1 && (int64_t)ks * M * q.N > SKBUF_ELEMS) --ks;
            if (ks > 1) ksplit = ks;
        }
        // plane-epilogue GEMMs / convs on tiny grids (DPT levels at SLAM scale: 16-64 workgroups looping over K = 2304 ..
        // 6912): split K into fp32 partial sums, a finishing kernel applies bias / activation / residuals.  Worth two
        // extra tiny launches only when the K loop is long and the grid leaves most of the chip idle (swept with atomics: <= 96 /
        // 160 / 256 tiles -> DPT 1.00 / 0.85 / 0.83 ms per view; with slabs, 5-edge scheduler: <= 192 / 256 tiles -> 6.04 / 5.89 ms).  An in-kernel fix-up (last slice finishes the tile behind a
        // device-scope fence + ticket) was 1.7x SLOWER than this: the fence writes back / invalidates the XCD's L2.
        if (q.epi == EPI_F16 && tiles_r <= 256 && q.K >= 1024 && q.N % 4 == 0 && (int64_t)M * q.N <= SKBUF_ELEMS) {
            int ks = sg_slices(q.old_slices, tiles_r, true);
            const int max_ks = q.K / 256;                 // keep >= 8 K tiles per slice
            if (ks > max_ks) ks = max_ks;
            while (ks > 1 && (int64_t)ks * M * q.N > SKBUF_ELEMS) --ks;      // one slab per K slice
            if (ks > 1) ksplit = ks;
        }
    }
    // forced families (tests / tools): 1 = 128x128 register-staged, 2 = 256x256, 3 = 192x256 (both wherever N % 256 == 0 and
    // the epilogue is not the RoPE one), 4 = 192x128 everywhere
    if ((q.forced == 2 || q.forced == 3) && variant != 6 && q.N % FAM5.bn == 0)
        variant = (q.N % FAM2.bn == 0 && q.epi != EPI_QKV) ? q.forced : 5;
    if (q.forced == 4 && variant != 6 && q.N % FAM5.bn == 0) variant = 5;
    if (q.forced == 1) variant = 1;
    // 8 forced (tests): the halo-tiled 3x3 convolution wherever it is legal (stride 1, Cout 128 / 256)
    if (q.amode == A_CONV3 && (q.epi == EPI_F16 || q.epi == EPI_HEAD) && q.cstride == 1 && (q.N == FAM8_N128.bn || q.N == FAM8.bn) && q.forced == 8) variant = 8;
    if (variant != 6) { ksplit = 1; slab_ks = 0; }
    // f16mx arithmetic: no form of the register-staged kernel (use_mx() already requires N % 64 == 0), and the fp32 epilogues
    // have no 256x256 one.  Remapped BEFORE the row tail is checked: the tail must fit the tile the launch really uses.
    if (q.mx && variant == 1) variant = 5;
    if (q.mx && mx_f32 && variant == 2) variant = q.N % FAM3.bn == 0 ? 3 : 5;
    GemmPlan g = plan_tiles(variant, q.M, 0, q.N, q.Ho, q.Wo);
    if (m_tail && g.bm && (q.M - m_tail) % g.bm == 0 && gemm2_has_tail(q.amode, q.epi, g.bm, tile_family(variant, q.N).nstg, q.mx))
        g = plan_tiles(variant, q.M, m_tail, q.N, q.Ho, q.Wo);
    g.ksplit = ksplit; g.slab_ks = slab_ks;
    REQUIRE(gemm_has_kernel(q.amode, q.epi, variant, q.mx, q.split, q.N, q.cstride),
            "internal: no kernel for tile family %d, epilogue %d, f16mx %d, N = %d", variant, q.epi, (int)q.mx, q.N);
    if (variant == 6 && (q.split || q.mx)) {
        // A grid of <= 256 workgroups leaves every workgroup alone on its CU: with 4 waves (one per SIMD) the barrier, the DMA
        // issue, the fragment reads and the MFMAs of a K tile simply add up (ablations, tools/ring_ablate.py: 0.12 + 0.14 + 0.09 +
        // 0.19 = 0.54 us per K tile) - the same tile on 8 waves (two per SIMD, wave tile 32x32) lets one wave's MFMAs run under
        // the other's issue and waits: encode -3.8 %, one pair @224 +4.1 %.  Larger grids (two workgroups per CU already) keep
        // the 4-wave form, whose 64x32 wave tile reads 25 % fewer fragments (8 waves there: -1.2 ... -1.4 %).
        const int sg_grid = g.tiles_m * (q.N / g.bn) * ksplit;
        g.lone = sg_grid <= (q.lone_opt > 1 ? q.lone_opt : 256) && q.lone_opt != 1;
    }
    out = g;
    return 0;
}
static PlanQuery plan_query(const sta_handle* h, int amode, int epi, const GemmParams& p, const VlGeo* geo) {
    PlanQuery q{amode, epi, p.M, p.N, p.K, h->prec != STA_PREC_F16, p.mx != 0, h->tail_hint, h->gemm_variant,
                h->small_grid_mode, h->opt[0] == 1 ? 1 : 0, h->opt[1] == 1 ? 1 : 0, h->deterministic,
                (epi == EPI_F32 && p.resid == p.C32) ? (p.slab ? 1 : 2) : 0, p.cstride, p.Ho, p.Wo, h->opt[2],
                geo && h->gemm_variant == 8 ? vl_tiles(*geo, FAM8.bm / 32) : -1};      // (fewer than 2^31 / 8 tiles: every level has fewer than 2^31 pixels)
    return q;
}
#ifdef STA_TEST_HOOKS
static void plan_out(const GemmPlan& g, int* out) {
    const int v[8] = {g.family, g.bm, g.bn, g.m_tail, g.tiles_m, g.tiles_n, g.ksplit, g.slab_ks};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}
extern "C" int sta_debug_gemm_plan(int amode, int epi, int M_all, int N, int K, int precision, int mx, int tail_hint, int forced_variant, int* out) {
    REQUIRE(out && M_all > 0 && N > 0 && K > 0 && (amode == A_DENSE || amode == A_CONV3), "bad argument");
    REQUIRE(precision == STA_PREC_F16 || precision == STA_PREC_F16X3 || precision == STA_PREC_F16X3H || precision == STA_PREC_F16X3M, "bad precision");
    PlanQuery q{amode, epi, M_all, N, K, precision != STA_PREC_F16, mx != 0, tail_hint, forced_variant, 0, 0, 0, false, 0, 0, 0, 0};
    // epi 5 (in-place residual) BELOW the small-grid predicate: the product never launches EPI_F32R there - the residual GEMMs of the
    // forward go through gemm_resid_ln, which launches the fp32 epilogue in place with the context's slab (its condition, restated;
    // tests/test_row_gpu.py holds the restatement to the last-plan record of real launches): slab_ks of THAT plan is reported
    if (amode == A_DENSE && epi == EPI_F32R && small_grid_m(0, M_all, N) && N % 64 == 0 && N <= 1024 && (forced_variant == 0 || forced_variant == 9)) {
        q.epi = EPI_F32; q.inplace = 1;
    }
    GemmPlan g;
    CHK(gemm_plan(q, g));
    plan_out(g, out);
    return 0;
}
// The same for a 3x3 convolution (A_CONV3; epi 1 plane epilogue, 6 fused head): M = images x Ho x Wo output pixels, K = 9 Cin; with the
// image geometry the halo-tiled family 8 is a candidate.  head_gemm: experiment switch 0.
extern "C" int sta_debug_conv_plan(int epi, int M, int N, int K, int precision, int mx, int forced_variant, int cstride, int Ho, int Wo,
                                   int head_gemm, int* out) {
    REQUIRE(out && M > 0 && N > 0 && K > 0 && (epi == EPI_F16 || epi == EPI_HEAD) && (cstride == 1 || cstride == 2) && Ho > 0 && Wo > 0 &&
            M % (Ho * Wo) == 0, "bad argument");
    REQUIRE(precision == STA_PREC_F16 || precision == STA_PREC_F16X3 || precision == STA_PREC_F16X3H || precision == STA_PREC_F16X3M, "bad precision");
    PlanQuery q{A_CONV3, epi, M, N, K, precision != STA_PREC_F16, mx != 0, 0, forced_variant, 0, head_gemm != 0 ? 1 : 0, 0, false, 0, cstride, Ho, Wo};
    GemmPlan g;
    CHK(gemm_plan(q, g));
    plan_out(g, out);
    return 0;
}
#endif

// Per-launch HIP-event timing (bench / tools): every launch (mode 2), or only the launches of ONE kernel symbol (mode 3,
// sta_kernel_timing_filter: the event pairs break back-to-back dispatch, ~3.5 us each, so the timed region of bench.py carries
// them on the dominant kernel only).  begin() before the launch opens the record (shape, flops, algorithmic bytes, start event),
// end() after it closes it (end event, tile family).
struct KTimer {
    sta_handle* h; hipStream_t st;
    bool timed = false; int family = 0;
    int begin(int epi, int amode, int fam, int mx, int M, int N, int K, double flops, double bytes) {
        family = fam;
        timed = h->ktime && (h->ktime_all || (h->kfilter[0] == epi && h->kfilter[1] == amode && h->kfilter[2] == fam && h->kfilter[3] == mx));
        if (timed && !h->ktime_all && !ksample(h)) timed = false;      // mode 3: a 1-in-kevery sample of the symbol's launches
        if (!timed) return 0;
        if ((int)h->kev.size() < 2 * (h->kn + 1)) {
            hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
            h->kev.push_back(a); h->kev.push_back(b);
        }
        if ((int)h->kflops.size() <= h->kn) h->kflops.resize(h->kn + 1);
        h->kflops[h->kn] = flops;
        if ((int)h->kshape.size() < 6 * (h->kn + 1)) h->kshape.resize(6 * (h->kn + 1));
        { int* q = &h->kshape[6 * h->kn]; q[0] = M; q[1] = N; q[2] = K; q[3] = epi; q[4] = amode; q[5] = mx; }
        if ((int)h->kbytes.size() <= h->kn) h->kbytes.resize(h->kn + 1);
        h->kbytes[h->kn] = bytes;
        HIPCHK(hipEventRecord(h->kev[2 * h->kn], st));
        h->kn++;
        return 0;
    }
    // the record's in-kernel stamp rows (sta_kernel_timing mode 4), or nullptr
    unsigned long long* stamps() const {
        return timed && h->kstamp_on && h->kn <= KSTAMP_LAUNCHES ? h->kstamp + (size_t)(h->kn - 1) * KSTAMP_WG * 4 : nullptr;
    }
    int end() {
        if (!timed) return 0;
        HIPCHK(hipEventRecord(h->kev[2 * (h->kn - 1) + 1], st));
        if ((int)h->kvar.size() < h->kn) h->kvar.resize(h->kn);
        h->kvar[h->kn - 1] = family;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------ dispatch
// One kernel of the table: the predicate decides at compile time whether it exists, the family which launcher it takes.
template <bool SPLIT, bool MX, int AMODE, int EPI, const TileFamily& F>
static int launch_tile(const GemmParams& p, hipStream_t st, int dev, const VlGeo* geo) {
    if constexpr (!has_kernel(AMODE, EPI, F, MX, SPLIT)) {
        // unreachable after gemm_plan succeeded; fails instead of returning 0 with the output unwritten
        return set_err("internal: no kernel for tile family %d (%dx%d, %d waves), epilogue %d, f16mx %d", F.id, F.bm, F.bn, F.wms * F.wns, EPI, (int)MX);
    } else if constexpr (F.id == 8) {
        REQUIRE(geo || ((int64_t)p.Ho * p.Wo > 0 && p.M % (p.Ho * p.Wo) == 0), "internal: conv3h needs whole images");
        REQUIRE(p.N == F.bn && p.cstride == 1, "internal: no halo-tiled convolution for epilogue %d at N = %d", EPI, p.N);
        return launch_conv3h<SPLIT, EPI, F.bm, F.bn, MX, F.wms, F.wns>(p, st, dev, geo);
    } else if constexpr (F.id == 1) {
        REQUIRE(!geo, "internal: tile family %d planned for a varlen launch", F.id);
        return launch_gemm1<SPLIT, AMODE, EPI>(p, st, dev);
    } else {
        REQUIRE(EPI != EPI_HEAD || p.N == F.bn, "internal: fused head epilogue on a tile family without it");
        return launch_gemm2<SPLIT, AMODE, EPI, F.bm, F.bn, F.wms, F.wns, F.nstg, MX>(p, st, dev, geo);
    }
}
// THE arithmetic choice: f16mx rows and weights, the split precisions, plain f16
template <int AMODE, int EPI, const TileFamily& F>
static int launch_family(const GemmParams& p, bool split, hipStream_t st, int dev, const VlGeo* geo) {
    if (p.mx) return launch_tile<true, true, AMODE, EPI, F>(p, st, dev, geo);
    if (split) return launch_tile<true, false, AMODE, EPI, F>(p, st, dev, geo);
    STA_F16ONLY(return (launch_tile<false, false, AMODE, EPI, F>(p, st, dev, geo)));
}
// The finisher of a small-grid GEMM whose K slices went to fp32 partial sums (gemm_plan: ksplit > 1 without slab_ks): bias, RoPE /
// activation and residuals, in a fixed summation order
template <int EPI>
static void finish_split_k(const GemmParams& p, bool split, hipStream_t st) {      // (the caller checks the launch)
    if (EPI == EPI_QKV) {
        const int64_t nthr = (int64_t)p.M * (p.nq + p.nk) + (int64_t)((p.M + 3) / 4) * p.nv;
        const int blocks = (int)((nthr + 255) / 256);
        if (split) hipLaunchKernelGGL(qkv_finish_kernel<true>, dim3(blocks), dim3(256), 0, st, p);
        else hipLaunchKernelGGL(qkv_finish_kernel<false>, dim3(blocks), dim3(256), 0, st, p);
    }
    if (EPI == EPI_F16) {
        const int64_t n4 = (int64_t)p.M * (p.N / 4);
        const int blocks = (int)((n4 + 255) / 256);
        if (split) hipLaunchKernelGGL(splitk_finish_kernel<true>, dim3(blocks), dim3(256), 0, st, p.skbuf, p.ksplit, p.bias, p.M, p.N, p.act, p.R1_hi, p.R2_hi, p.C_hi, p.c_rp, p.r_mx, p.c_mx, p.range);
        else hipLaunchKernelGGL(splitk_finish_kernel<false>, dim3(blocks), dim3(256), 0, st, p.skbuf, p.ksplit, p.bias, p.M, p.N, p.act, p.R1_hi, p.R2_hi, p.C_hi, p.c_rp, 0, 0, p.range);
    }
}
// slab_ks_out: K slices a slab GEMM wrote (0: it did not take the slab path) - the caller's finisher sums exactly those
template <int AMODE, int EPI>
static int launch_gemm(sta_handle* h, const GemmParams& p_in, hipStream_t st, int* slab_ks_out = nullptr, const VlGeo* geo = nullptr) {
    GemmParams p = p_in;
    p.range = h->range;
    if (slab_ks_out) *slab_ks_out = 0;
    p.zero_page = h->zero_page;
    REQUIRE(p.K % GEMM_BK == 0, "GEMM K=%d must be a multiple of %d", p.K, GEMM_BK);
    REQUIRE(p.M > 0 && p.N > 0, "empty GEMM");
    if (AMODE == A_CONV3) REQUIRE(p.Cin % GEMM_BK == 0, "conv Cin=%d must be a multiple of %d", p.Cin, GEMM_BK);
    // the LDS-DMA loaders address a K tile with 32-bit byte offsets (128 B per row of a row block)
    REQUIRE((AMODE != A_DENSE || (int64_t)p.M * 128 < ((int64_t)1 << 32)) && (int64_t)p.N * 128 < ((int64_t)1 << 32),
            "GEMM with M=%d, N=%d exceeds the 32-bit row-offset range of the DMA loaders", p.M, p.N);
    if (AMODE == A_CONV3) REQUIRE((int64_t)p.a_rp * 128 < ((int64_t)1 << 32), "convolution input of %lld pixels exceeds the 32-bit offset range of the tap loader", (long long)p.a_rp);
    if (h->dry) return 0;
    const bool split = h->prec != STA_PREC_F16;
    // varlen launches (geo): every family but the register-staged family 1 has the form; forcing that one is refused here
    REQUIRE(!geo || h->gemm_variant != 1, "tile family %d has no varlen form (sta_head_pts_varlen runs on families 2 / 3 / 5 / 6 / 8)", h->gemm_variant);
    GemmPlan g;
    CHK(gemm_plan(plan_query(h, AMODE, EPI, p, geo), g));
    h->last_plan = g;
    p.m_tail = g.m_tail;
    p.ksplit = g.ksplit;
    if (g.ksplit > 1 && (EPI == EPI_QKV || EPI == EPI_F16)) p.skbuf = lane_skbuf(h);
    if (g.slab_ks == 0) p.slab = nullptr;
    if (slab_ks_out) *slab_ks_out = g.slab_ks;
    KTimer kt{h, st};
    // algorithmic bytes: A and W planes (2 B x planes) read once, C written once (+ residual read)
    CHK(kt.begin(EPI, AMODE, g.family, p.mx, p.M, p.N, p.K, 2.0 * p.M * p.N * p.K,
                 (split ? 4.0 : 2.0) * ((double)p.M * p.K + (double)p.N * p.K) + 4.0 * p.M * p.N * (p.resid ? 2.0 : 1.0)));
    if (kt.timed && g.family == 5) p.clk_dbg = h->clk_buf;   // effective-clock probe (bench only)
    if (unsigned long long* s = kt.stamps()) p.stamps = s;
    // the planned family -> its row of the table
    switch (g.family) {
        case 1: CHK((launch_family<AMODE, EPI, FAM1>(p, split, st, h->device, geo))); break;
        case 2: CHK((launch_family<AMODE, EPI, FAM2>(p, split, st, h->device, geo))); break;
        case 3: CHK((launch_family<AMODE, EPI, FAM3>(p, split, st, h->device, geo))); break;
        case 5: CHK((launch_family<AMODE, EPI, FAM5>(p, split, st, h->device, geo))); break;
        case 6: CHK(g.lone ? (launch_family<AMODE, EPI, FAM6_LONE>(p, split, st, h->device, geo)) : (launch_family<AMODE, EPI, FAM6>(p, split, st, h->device, geo))); break;
        case 8: CHK(g.bn == FAM8_N128.bn ? (launch_family<AMODE, EPI, FAM8_N128>(p, split, st, h->device, geo)) : (launch_family<AMODE, EPI, FAM8>(p, split, st, h->device, geo))); break;
        default: REQUIRE(false, "internal: tile family %d (f16mx %d) has no launch", g.family, p.mx);
    }
    if (g.ksplit > 1) finish_split_k<EPI>(p, split, st);      // (family 6 only)
    HIPCHK(hipGetLastError());
    return kt.end();
}

// mx: A is in the f16mx row format and the f16mx copy of the weight is used (transformer linears in precision f16mx)
static GemmParams gp_dense(const Planes& A, int lda, const Lin& W, int M, bool mx = false) {
    GemmParams p; memset(&p, 0, sizeof p);
    p.A_hi = A.hi; p.A_lo = A.lo; p.lda = lda; p.a_rp = A.rp;
    p.B_hi = mx ? W.wmx.hi : W.w.hi; p.B_lo = mx ? W.wmx.lo : W.w.lo; p.bias = W.bias;
    p.mx = mx ? 1 : 0;
    p.M = M; p.N = W.N; p.K = W.K;
    return p;
}

// out fp32 = A*W^T + bias (+resid), optional row remap
// an f16mx kernel exists for every tile family with N % 64 == 0 (the one exception on the path: act_postprocess[0], N = 96)
static bool use_mx(const sta_handle* h, const Lin& W) { return (h->mx_mask & W.cls) != 0 && W.wmx.hi != nullptr && W.N % 64 == 0; }

static int gemm_f32(sta_handle* h, const Planes& A, const Lin& W, int M, float* out, int ldc,
                    const float* resid, hipStream_t st) {
    GemmParams p = gp_dense(A, W.K, W, M, use_mx(h, W));
    REQUIRE(h->dry || A.mx == (p.mx != 0), "internal: input row format does not match the GEMM's arithmetic (gemm_f32)");
    p.C32 = out; p.ldc = ldc; p.resid = resid; p.ldr = ldc;
    // throughput-scale in-place residual GEMMs (attn.proj, mlp.fc2, cross_attn.proj): specialised epilogue
    if (resid == out && !small_grid(h, M, W.N))
        return launch_gemm<A_DENSE, EPI_F32R>(h, p, st);
    return launch_gemm<A_DENSE, EPI_F32>(h, p, st);
}
// c_mx: the output planes feed an f16mx GEMM (mlp.fc1 -> GELU -> mlp.fc2)
static int gemm_f16(sta_handle* h, const Planes& A, const Lin& W, int M, const Planes& out, int act, hipStream_t st, bool c_mx = false) {
    GemmParams p = gp_dense(A, W.K, W, M, use_mx(h, W));
    p.C_hi = out.hi; p.C_lo = out.lo; p.ldc16 = W.N; p.act = act; p.c_rp = out.rp; p.c_mx = c_mx ? 1 : 0;
    REQUIRE(h->dry || (A.rp >= M && out.rp >= M), "internal: plane rows mismatch in gemm_f16");
    REQUIRE(h->dry || !A.mx || p.mx, "internal: f16mx input rows for a GEMM without an f16mx kernel");
    if (act == ACT_GELU && M > 640) return launch_gemm<A_DENSE, EPI_GELU>(h, p, st);   // mlp.fc1 at throughput scale: compile-time activation, no residual
                                                                                      // planes (small M keeps the generic epilogue and its split-K path)
    return launch_gemm<A_DENSE, EPI_F16>(h, p, st);
}
static int run_ln(sta_handle* h, const float* x, int M, int C, const LNp& a, const Planes& oa, const LNp* b, const Planes* ob,
                  float* o32, hipStream_t st, const float* slab = nullptr, int nslab = 0);
// x += A W^T + b (attn.proj, mlp.fc2, cross_attn.proj) followed by the LayerNorm(s) of x the next GEMM(s) read (la == nullptr:
// none).  Throughput scale: the in-place GEMM, then the LayerNorm kernel.  Small-M regime (SLAM scale): the K slices store
// partial tiles to slabs and the LayerNorm kernel adds them into x before normalising - the same two dispatches without
// the atomics epilogue (13-15 us -> 8 us per GEMM at M = 196), and bit-reproducible.
static int gemm_resid_ln(sta_handle* h, const Planes& A, const Lin& W, int M, float* x, int ld, const LNp* la, const Planes* oa,
                         const LNp* lb, const Planes* ob, hipStream_t st) {
    static const LNp no_ln = {nullptr, nullptr};
    static const Planes no_planes;
    const bool small = small_grid(h, M, W.N) && W.N % 64 == 0 && W.N <= 1024 && auto_family(h) && ld == W.N;
    if (small) {
        GemmParams p = gp_dense(A, W.K, W, M, use_mx(h, W));
        REQUIRE(h->dry || A.mx == (p.mx != 0), "internal: input row format does not match the GEMM's arithmetic (gemm_resid_ln)");
        p.C32 = x; p.ldc = ld; p.resid = x; p.ldr = ld;
        p.slab = h->cur->slab;
        int ks = 0;
        CHK((launch_gemm<A_DENSE, EPI_F32>(h, p, st, &ks)));
        if (ks > 1) return run_ln(h, x, M, W.N, la ? *la : no_ln, oa ? *oa : no_planes, lb, ob, nullptr, st, p.slab, ks);
    } else {
        CHK(gemm_f32(h, A, W, M, x, ld, x, st));
    }
    if (la) return run_ln(h, x, M, W.N, *la, *oa, lb, ob, nullptr, st, nullptr, 0);
    return 0;
}
struct QKVOut { Planes q, k, vt; int npad; };
static int gp_qkv(sta_handle* h, GemmParams& p, const Planes& A, const Lin& W, int M, int nq, int nk, int nv,
                  const QKVOut& o, int ntok, int heads, int wp, int has_pose, int pose_base = 0) {
    p = gp_dense(A, W.K, W, M, use_mx(h, W));
    p.Q_hi = o.q.hi; p.Q_lo = o.q.lo; p.K_hi = o.k.hi; p.K_lo = o.k.lo; p.Vt_hi = o.vt.hi; p.Vt_lo = o.vt.lo;
    p.nq = nq; p.nk = nk; p.nv = nv; p.ntok = ntok; p.npad = o.npad; p.heads = heads; p.wp = wp; p.has_pose_tok = has_pose;
    p.pose_base = pose_base;
    REQUIRE(!(pose_base > 0 && has_pose), "internal: pose_base and has_pose_tok are two layouts of the same thing");
    p.rope_tab = h->rope_foreign ? h->rope_ident : h->rope_tab;      // sta_decode_pos: identity here, rope_fix afterwards
    p.ntok_magic = ntok > 1 ? (unsigned)((1ull << 32) / (unsigned)ntok + 1) : 0u;
    p.wp_magic = wp > 1 ? (unsigned)((1ull << 32) / (unsigned)wp + 1) : 0u;
    REQUIRE(nq + nk + nv == W.N, "qkv segment mismatch");
    return 0;
}
static int gemm_qkv(sta_handle* h, const Planes& A, const Lin& W, int M, int nq, int nk, int nv,
                    const QKVOut& o, int ntok, int heads, int wp, int has_pose, hipStream_t st, int pose_base = 0) {
    GemmParams p;
    CHK(gp_qkv(h, p, A, W, M, nq, nk, nv, o, ntok, heads, wp, has_pose, pose_base));
    return launch_gemm<A_DENSE, EPI_QKV>(h, p, st);
}
// Two QKV-epilogue GEMMs that do not depend on each other as ONE launch (gemm2_pair_kernel) when both run on the 192x128
// family at throughput scale; otherwise two launches.  Decoder: attn.qkv on norm1(x) + cross_attn.projk|projv on norm_y.
// The one decision (a pure host function like gemm_plan; sta_debug_qkv_pair_plan): true = one launch, with the pose-token rows
// of both halves as tail blocks (*m_tail) where the patch rows are whole 192-row tiles.
static bool qkv_pair_plan(bool split, bool auto_fam, int sg_mode, int tail_hint, int M_a, int N_a, int K_a, bool mx_a,
                          int M_b, int N_b, int K_b, bool mx_b, int* m_tail) {
    auto big = [sg_mode](int M, int N) { return N % FAM7.bn == 0 && !small_grid_m(sg_mode, M, N); };
    *m_tail = 0;
    if (!(split && !mx_a && !mx_b && big(M_a, N_a) && big(M_b, N_b) && K_a == K_b && M_a == M_b && auto_fam)) return false;
    const int t = tail_hint;
    if (t > 0 && t <= 32 && M_a > t && (M_a - t) % FAM7.bm == 0 && !small_grid_m(sg_mode, M_a - t, N_a) && !small_grid_m(sg_mode, M_b - t, N_b) &&
        gemm2_has_tail(A_DENSE, EPI_QKV, FAM7.bm, FAM7.nstg, false))
        *m_tail = t;
    return true;
}
static bool qkv_pair_one_launch(const sta_handle* h, const GemmParams& pa, const GemmParams& pb, int* m_tail = nullptr) {
    int mt;
    return qkv_pair_plan(h->prec != STA_PREC_F16, auto_family(h), h->small_grid_mode, h->tail_hint, pa.M, pa.N, pa.K, pa.mx != 0,
                         pb.M, pb.N, pb.K, pb.mx != 0, m_tail ? m_tail : &mt);
}
#ifdef STA_TEST_HOOKS
extern "C" int sta_debug_qkv_pair_plan(int precision, int M, int N_a, int N_b, int K, int mx_a, int mx_b, int tail_hint, int forced_variant, int* out) {
    REQUIRE(out && M > 0 && N_a > 0 && N_b > 0 && K > 0, "bad argument");
    REQUIRE(precision == STA_PREC_F16 || precision == STA_PREC_F16X3 || precision == STA_PREC_F16X3H || precision == STA_PREC_F16X3M, "bad precision");
    out[0] = qkv_pair_plan(precision != STA_PREC_F16, forced_variant == 0 || forced_variant == 9, 0, tail_hint, M, N_a, K, mx_a != 0,
                           M, N_b, K, mx_b != 0, &out[1]) ? 1 : 0;
    return 0;
}
#endif
// Side lanes of the current context (dpt_impl, decode_impl): inside one call the library forks an internal second stream for the
// launches that are off the call's critical chain.  sta_set_side_lanes(h, mode) is the application's switch (include/sta_mi355.h):
//   STA_LANES_OFF / STA_LANES_ON: what they say (results are bit-identical either way);
//   STA_LANES_AUTO (default): on, unless the application itself is overlapping calls on several streams - another scratch context
//     of this handle was used within its last 8 context switches - because the chip is then filled ACROSS calls and the extra
//     internal streams only compete for the runtime's few hardware queues (bench.py slam_replay, three caller streams: 229
//     keyframes/s without side lanes, 189 with them); and off when GPU_MAX_HW_QUEUES is set in the environment (measured with 8:
//     every fork / join between streams on different hardware queues cost ~0.4 ms; the lanes are tuned for the runtime default).
// The whole-model timing modes (stage timing, per-launch timing of every GEMM, stamps) always run one lane.
static bool lanes_on(const sta_handle* h) {
    if (h->rope_foreign) return false;      // sta_decode_pos: one lane (its Q / K fix-ups follow each QKV launch on the call's stream)
    if (h->dry || h->timing || h->ktime_all || h->kstamp_on) return false;     // (the one-kernel timing mode of bench.py stays on the product path: its event pairs sit on each launch's own stream)
    if (h->lanes_mode == STA_LANES_OFF || h->opt[6] == 1) return false;
    if (h->lanes_mode == STA_LANES_ON || h->opt[6] == 2) return true;
    static const bool queues_overridden = getenv("GPU_MAX_HW_QUEUES") != nullptr;
    if (queues_overridden) return false;
    for (const auto& c : h->ctx) if (&c != h->cur && c.last_use + 8 > h->use_clock) return false;
    return true;
}
struct Lane { sta_handle* h; int v; Lane(sta_handle* h_, int v_) : h(h_), v(h_->lane) { h->lane = v_; } ~Lane() { h->lane = v; } };
// Leaves a function that forked the side lane: the caller's stream waits for whatever the side lane still has in flight - also
// on the error paths (an early return must not leave side-lane kernels writing a workspace the next call reuses).
struct LaneJoin {
    sta_handle* h; hipStream_t st; bool armed;
    ~LaneJoin() {
        if (!armed || !h->cur || !h->cur->side) return;
        if (hipEventRecord(h->cur->side_ev[3], h->cur->side) == hipSuccess) (void)hipStreamWaitEvent(st, h->cur->side_ev[3], 0);
    }
};
static int gemm_qkv_pair(sta_handle* h, const GemmParams& pa_in, const GemmParams& pb_in, hipStream_t st) {
    GemmParams pa = pa_in, pb = pb_in;
    pa.range = pb.range = h->range;
    if (h->dry) return 0;
    int m_tail = 0;
    if (!qkv_pair_one_launch(h, pa, pb, &m_tail)) {
        CHK((launch_gemm<A_DENSE, EPI_QKV>(h, pa, st)));
        return launch_gemm<A_DENSE, EPI_QKV>(h, pb, st);
    }
    pa.zero_page = pb.zero_page = h->zero_page;
    pa.ksplit = pb.ksplit = 1;
    pa.m_tail = pb.m_tail = m_tail;       // pose-token rows as skinny tail blocks (GemmParams::m_tail)
    constexpr const TileFamily& F = FAM7;
    const GemmPlan g = plan_tiles(F.id, pa.M, m_tail, pa.N + pb.N, 0, 0);      // (both N are whole tiles, both M equal: qkv_pair_plan)
    h->last_plan = g;
    const int ta = g.tiles_m * (pa.N / F.bn) + (m_tail ? pa.N / TAIL_BN : 0);
    const int tb = g.tiles_m * (pb.N / F.bn) + (m_tail ? pb.N / TAIL_BN : 0);
    KTimer kt{h, st};      // one record: M x (Na + Nb) x K, tile family id 7 = gemm2_pair_kernel
    CHK(kt.begin(EPI_QKV, A_DENSE, F.id, 0, pa.M, pa.N + pb.N, pa.K, 2.0 * pa.M * (pa.N + pb.N) * pa.K,
                 4.0 * (2.0 * pa.M * pa.K + (double)(pa.N + pb.N) * pa.K) + 4.0 * pa.M * (pa.N + pb.N)));
    if (unsigned long long* s = kt.stamps(); s && ta + tb <= KSTAMP_WG) { pa.stamps = s; pb.stamps = s + (size_t)ta * 4; }
    constexpr int smem = gemm2_smem_bytes<true, F.bm, F.bn>(F.nstg);
    constexpr auto kern = gemm2_pair_kernel<true, A_DENSE, EPI_QKV, F.bm, F.bn, F.wms, F.wns>;
    CHK(set_smem_once<kern>(h->device, smem));
    hipLaunchKernelGGL(kern, dim3((unsigned)(ta + tb)), dim3(F.wms * F.wns * 64), smem, st, pa, pb, ta);
    HIPCHK(hipGetLastError());
    return kt.end();
}
static int gemm_convt(sta_handle* h, const Planes& A, const Lin& W, int nimg, int hh, int ww, int k, int cout,
                      const Planes& out, hipStream_t st) {
    GemmParams p = gp_dense(A, W.K, W, nimg * hh * ww, use_mx(h, W));
    REQUIRE(h->dry || A.mx == (p.mx != 0), "internal: ConvT input format mismatch");
    p.C_hi = out.hi; p.C_lo = out.lo; p.ct_k = k; p.ct_cout = cout; p.ct_h = hh; p.ct_w = ww; p.c_rp = out.rp; p.c_mx = out.mx ? 1 : 0;
    return launch_gemm<A_DENSE, EPI_CONVT>(h, p, st);
}
// 3x3 conv, pad 1, NHWC planes
static int conv3(sta_handle* h, const Planes& in, int nimg, int Hi, int Wi, int Cin, const Lin& W, int stride,
                 bool relu_in, int act, const Planes& out, const Planes* r1, const Planes* r2, hipStream_t st) {
    GemmParams p; memset(&p, 0, sizeof p);
    p.A_hi = in.hi; p.A_lo = in.lo; p.a_rp = in.rp;
    p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.cstride = stride; p.relu_in = relu_in ? 1 : 0;
    p.Ho = (Hi + 2 - 3) / stride + 1; p.Wo = (Wi + 2 - 3) / stride + 1;
    const bool mx = use_mx(h, W);
    REQUIRE(h->dry || in.mx == mx, "internal: conv input format mismatch");
    p.mx = mx ? 1 : 0;
    p.B_hi = mx ? W.wmx.hi : W.w.hi; p.B_lo = mx ? W.wmx.lo : W.w.lo; p.bias = W.bias;
    p.M = nimg * p.Ho * p.Wo; p.N = W.N; p.K = W.K;
    REQUIRE(W.K == 9 * Cin, "conv weight K mismatch");
    p.C_hi = out.hi; p.C_lo = out.lo; p.ldc16 = W.N; p.act = act; p.c_rp = out.rp; p.c_mx = out.mx ? 1 : 0;
    REQUIRE(h->dry || ((int64_t)nimg * Hi * Wi == in.rp && out.rp == p.M), "internal: conv plane rows mismatch");
    if (r1) { p.R1_hi = r1->hi; p.R1_lo = r1->lo; p.r_mx = r1->mx ? 1 : 0; REQUIRE(h->dry || r1->rp == out.rp, "internal: residual rows mismatch"); }
    if (r2) { p.R2_hi = r2->hi; p.R2_lo = r2->lo; REQUIRE(h->dry || (r2->rp == out.rp && (!r1 || r1->mx == r2->mx)), "internal: residual rows / format mismatch"); p.r_mx = r2->mx ? 1 : 0; }
    return launch_gemm<A_CONV3, EPI_F16>(h, p, st);
}

// head.2 (3x3 conv 128 -> 128) + ReLU + head.4 (1x1 conv 128 -> 4) + point-map / confidence activations as ONE kernel
// (EPI_HEAD): true when it was launched; false = the caller runs conv3 + head_final_kernel (small grids, forced tile families).
static bool conv3_head_ok(sta_handle* h, const Lin& W, int64_t M) {
    return W.N == 128 && ((auto_family(h) && !small_grid(h, M, W.N)) || h->gemm_variant == 8);
}
static int conv3_head(sta_handle* h, const Planes& in, int nimg, int Hi, int Wi, int Cin, const Lin& W, const F32Lin& W4,
                      float* ptsA, float* confA, int nA, float* ptsB, float* confB, hipStream_t st) {
    GemmParams p; memset(&p, 0, sizeof p);
    p.A_hi = in.hi; p.A_lo = in.lo; p.a_rp = in.rp;
    p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.cstride = 1; p.relu_in = 0; p.Ho = Hi; p.Wo = Wi;
    const bool mx = use_mx(h, W);
    REQUIRE(h->dry || in.mx == mx, "internal: conv input format mismatch");
    p.mx = mx ? 1 : 0;
    p.B_hi = mx ? W.wmx.hi : W.w.hi; p.B_lo = mx ? W.wmx.lo : W.w.lo; p.bias = W.bias;
    p.M = nimg * Hi * Wi; p.N = W.N; p.K = W.K;
    REQUIRE(W.K == 9 * Cin && W.N == 128, "conv weight shape mismatch (fused head)");
    REQUIRE(h->dry || (int64_t)nimg * Hi * Wi == in.rp, "internal: conv plane rows mismatch");
    p.hw4 = W4.w; p.hb4 = W4.b; for (int o = 0; o < 4; ++o) p.hw4_scale[o] = h->head4_scale[o];
    p.hptsA = ptsA; p.hconfA = confA; p.hptsB = ptsB; p.hconfB = confB;
    p.hsplit = (int64_t)(nA < nimg ? nA : nimg) * Hi * Wi;
    return launch_gemm<A_CONV3, EPI_HEAD>(h, p, st);
}

static int run_ln(sta_handle* h, const float* x, int M, int C, const LNp& a, const Planes& oa,
                  const LNp* b, const Planes* ob, float* o32, hipStream_t st,
                  const float* slab, int nslab) {
    if (h->dry) return 0;
    LnParams p; memset(&p, 0, sizeof p);
    p.range = h->range;
    p.slab = slab; p.nslab = nslab; p.xw = const_cast<float*>(x);     // slab split-K: x += sum of the slices first (x is the residual stream)
    p.x = x; p.ldx = C; p.M = M; p.C = C; p.eps = h->cfg.ln_eps;
    p.g1 = a.g; p.b1 = a.b; p.o1_hi = oa.hi; p.o1_lo = oa.lo;
    if (b) { p.g2 = b->g; p.b2 = b->b; p.o2_hi = ob->hi; p.o2_lo = ob->lo; }
    p.o32 = o32; p.ldo32 = C;
    if (slab) {          // residual-GEMM finish + LayerNorm, one block per row
        REQUIRE(C <= 1024 && C % 4 == 0, "internal: slab LayerNorm needs C <= 1024");
        if (h->prec != STA_PREC_F16) hipLaunchKernelGGL(resid_ln_kernel<true>, dim3(M), dim3(256), 0, st, p);
        else hipLaunchKernelGGL(resid_ln_kernel<false>, dim3(M), dim3(256), 0, st, p);
        HIPCHK(hipGetLastError());
        return 0;
    }
    dim3 grid((M + 3) / 4);
    if (h->prec != STA_PREC_F16) hipLaunchKernelGGL(ln_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(ln_kernel<false>, grid, dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    return 0;
}

// pose: token index nq (== nk) of the buffers is the pose token (decoder row order, see decode_impl / AttnParams::pose)
// sta_decode_pos: rotate a Q or K buffer [S][heads][npad][64] in place by the caller's positions (pose token: -1)
static int rope_fix(sta_handle* h, const Planes& qk, int S, int heads, int npad, int ntok, hipStream_t st) {
    if (h->dry || !h->rope_foreign) return 0;
    const int64_t total = (int64_t)S * heads * (ntok + 1) * 32;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (qk.lo) hipLaunchKernelGGL(rope_planes_kernel<true>, grid, dim3(256), 0, st, qk.hi, qk.lo, S, heads, npad, ntok, h->rope_pos, h->rope_tab, h->range);
    else hipLaunchKernelGGL(rope_planes_kernel<false>, grid, dim3(256), 0, st, qk.hi, qk.lo, S, heads, npad, ntok, h->rope_pos, h->rope_tab, h->range);
    HIPCHK(hipGetLastError());
    return 0;
}
// sta_decode_tokens: rotate nbuf (<= 3) Q / K buffers [S1 + S2][heads][npad][64] in place, sequences [0, S1) with ntok_a tokens and
// the table slice pos[0, S1*ntok_a*2), sequences [S1, S1 + S2) with ntok_b tokens and the slice behind it: ONE launch of
// rope_tokens_kernel.  per_buffer (experiment switch 3 / sta_debug_rope_tokens which = 1): the same rotation as 2 * nbuf launches of
// rope_planes_kernel, one per buffer and side - what the entry would cost on the existing kernel (A/B only).
// pose = false (sta_encode_tokens, rope_enc_tokens): buffers without a pose row - ntok rows per (sequence, head), see rope_tokens_kernel.
static int rope_tokens_launch(sta_handle* h, const Planes* const* bufs, int nbuf, int S1, int S2, int heads, int npad, int ntok_a, int ntok_b,
                              const int* pos, bool per_buffer, hipStream_t st, bool pose = true) {
    REQUIRE(nbuf >= 1 && nbuf <= 3 && pos && h->rope_tab, "internal: rope_tokens_launch arguments");
    REQUIRE(pose || !per_buffer, "internal: the per-buffer rotation has the pose-row form only");
    REQUIRE(std::max(S1 > 0 ? ntok_a : 0, S2 > 0 ? ntok_b : 0) + (pose ? 1 : 0) <= npad, "internal: rope_tokens_launch rows exceed npad");
    const bool split = bufs[0]->lo != nullptr;
    if (per_buffer) {
        for (int b = 0; b < nbuf; ++b)
            for (int side = 0; side < 2; ++side) {
                const int S = side ? S2 : S1, ntok = side ? ntok_b : ntok_a;
                const int64_t off = side ? (int64_t)S1 * heads * npad * 64 : 0;
                const int* ps = pos + (side ? (int64_t)S1 * ntok_a * 2 : 0);
                const dim3 grid((unsigned)(((int64_t)S * heads * (ntok + 1) * 32 + 255) / 256));
                if (split) hipLaunchKernelGGL(rope_planes_kernel<true>, grid, dim3(256), 0, st, bufs[b]->hi + off, bufs[b]->lo + off, S, heads, npad, ntok, ps, h->rope_tab, h->range);
                else hipLaunchKernelGGL(rope_planes_kernel<false>, grid, dim3(256), 0, st, bufs[b]->hi + off, (f16*)nullptr, S, heads, npad, ntok, ps, h->rope_tab, h->range);
            }
        HIPCHK(hipGetLastError());
        return 0;
    }
    RopeTokParams p;
    for (int b = 0; b < 3; ++b) { p.hi[b] = bufs[b < nbuf ? b : 0]->hi; p.lo[b] = bufs[b < nbuf ? b : 0]->lo; }
    p.S1 = S1; p.S2 = S2; p.heads = heads; p.npad = npad; p.ntok_a = ntok_a; p.ntok_b = ntok_b;
    p.pos = pos; p.tab = h->rope_tab; p.rng = h->range;
    const int pr = pose ? 1 : 0;
    const int64_t total = ((int64_t)S1 * (ntok_a + pr) + (int64_t)S2 * (ntok_b + pr)) * heads * 4;
    const dim3 grid((unsigned)((total + 255) / 256), nbuf);
    if (!pose) {
        if (split) hipLaunchKernelGGL((rope_tokens_kernel<true, false>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((rope_tokens_kernel<false, false>), grid, dim3(256), 0, st, p);
    } else if (split) hipLaunchKernelGGL(rope_tokens_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(rope_tokens_kernel<false>, grid, dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    return 0;
}
// ... inside a decoder call: nothing unless the call carries caller positions (sta_decode_tokens)
static int rope_tokens(sta_handle* h, const Planes* const* bufs, int nbuf, int S1, int S2, int heads, int npad, int ntok_a, int ntok_b, hipStream_t st) {
    if (h->dry || !h->rope_foreign) return 0;
    return rope_tokens_launch(h, bufs, nbuf, S1, S2, heads, npad, ntok_a, ntok_b, h->rope_pos, h->opt[3] == 1, st);
}

// sta_encode_tokens: the encoder's Q and K buffers [S][heads][npad][64] (npad = roundup(ntok, 64), no pose row) by the call's
// positions table: one launch per layer (blockIdx.y = buffer)
static int rope_enc_tokens(sta_handle* h, const Planes& q, const Planes& k, int S, int heads, int npad, int ntok, hipStream_t st) {
    if (h->dry) return 0;
    REQUIRE(h->rope_foreign && h->rope_pos, "internal: rope_enc_tokens outside sta_encode_tokens");
    const Planes* rot[2] = {&q, &k};
    return rope_tokens_launch(h, rot, 2, S, 0, heads, npad, ntok, 0, h->rope_pos, false, st, false);
}

static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// ------------------------------------------------------------------------------------------ attention launch plans
// Everything a run_attn* decides before it launches its kernel, as pure host functions of the shapes and the switches (like
// gemm_plan): the launcher runs exactly its plan and keeps it in the handle; the sta_debug_attn_*plan hooks expose the plans to the
// host-only sweeps (tests/test_attention*_plan.py) and the sta_debug_last_attn_*plan hooks read back the plan a kernel test ran under.
// The rules of ONE sequence (nq queries over nk keys) live in attn_seq_rule and attn_seq_finish, the LDS of a launch in attn_lds;
// the three builders below differ only in how sequences are laid out in the grid and in the output.
//   pose query: 2 = one more row of the last query block when that block has spare rows (nq = 196: rows 196..255 of the second
//   block are dead anyway - free, and no latency-bound side path at SLAM scale: 12.8 vs 26.1 us for 10 x 12 heads); 1 = one side
//   workgroup per (sequence, head) when the patch queries fill their blocks exactly (nq = 768)
//   prefetch: small grids with <= 4 key tiles run on 4 LDS stages, every K / V^T tile requested up front (attention.h; one
//   workgroup per CU then, which a grid of <= 256 workgroups has anyway); no_prefetch = debug option 5
// R: AttnPlan, AttnMixedPlan::Group or AttnVarlenPlan::Seq (the records the debug hooks serialise share these field names).
// pose_form: the decoder's pose-token form (pose key at token index nk, pose query at token index nq).
template <class R>
static int attn_seq_rule(R& a, int nq, int nk, bool pose_form) {
    a.pose = pose_form ? (nq % 128 != 0 ? 2 : 1) : 0;
    a.qblocks = (nq + (a.pose == 2 ? 1 : 0) + 127) / 128;
    a.ntiles = (nk + ATT_KV - 1) / ATT_KV; a.nfull = nk / ATT_KV;
    // the pose-query blocks park npad scores + 8 + 256 partials (fp32) in the smallest LDS allocation of the kernel; npad >= nk + 1
    // (attn_plan requires nq == nk in the pose form, so nk is also what the fixed launch would compute from nq)
    a.pose_scratch = pose_form ? (rup(nk + 1, 64) + 8 + 256) * 4 : 0;
    REQUIRE(a.pose_scratch <= attn_smem_bytes<false>(), "internal: pose-query scratch exceeds the LDS allocation");
    return 0;
}
// ... once the grid is known.  The prefetch decision uses the grid of the WHOLE launch: it is about how many workgroups share a CU.
// Returns whether the sequence prefetches.
template <class R>
static bool attn_seq_finish(R& a, int nk, int grid, bool no_prefetch) {
    a.prefetch = (nk <= ATT_PREFETCH_TILES * ATT_KV && grid <= 256 && !no_prefetch) ? 1 : 0;
    a.tail_stage = a.nfull == a.ntiles ? -1 : (a.prefetch ? a.nfull : (a.nfull & 1));
    return a.prefetch != 0;
}
// A launch carries the LDS of its hungriest sequence: 4 stages as soon as one prefetches (a double-buffered sequence then simply
// leaves stages 2 and 3 alone; the grid is <= 256 workgroups in that case, one per CU either way).
template <class P>
static void attn_lds(P& m, bool any_prefetch, bool split) {
    m.stages = any_prefetch ? ATT_PREFETCH_TILES : 2;
    m.lds_bytes = split ? attn_smem_bytes<true>(m.stages) : attn_smem_bytes<false>(m.stages);
}

// attn_kernel: S sequences of one shape
static int attn_plan(int S, int heads, int nq, int nk, bool pose, bool split, bool no_prefetch, AttnPlan& out) {
    REQUIRE(S > 0 && heads > 0 && nq > 0 && nk > 0, "empty attention");
    REQUIRE(!pose || nq == nk, "internal: pose-token attention needs nq == nk < npad");
    AttnPlan a{};
    CHK(attn_seq_rule(a, nq, nk, pose));
    a.pose_blocks = a.pose == 1 ? S * heads : 0;
    const int64_t grid = (int64_t)a.qblocks * heads * S + a.pose_blocks;
    REQUIRE(grid < ((int64_t)1 << 31), "attention grid of %lld workgroups", (long long)grid);
    a.grid = (int)grid;
    attn_lds(a, attn_seq_finish(a, nk, a.grid, no_prefetch), split);
    out = a;
    return 0;
}
// attn_mixed_kernel (decode_mixed_impl): group a = S1 sequences of nq_a queries over nk_a keys, group b = S2 sequences of nq_b over
// nk_b, both in the pose-token form
static int attn_mixed_plan(int S1, int S2, int heads, int nq_a, int nk_a, int nq_b, int nk_b, bool split, bool no_prefetch, AttnMixedPlan& out) {
    REQUIRE(S1 > 0 && S2 >= 0 && heads > 0 && nq_a > 0 && nk_a > 0, "empty attention");
    REQUIRE(S2 == 0 || (nq_b > 0 && nk_b > 0), "empty attention (second group)");
    AttnMixedPlan m{};
    const int Sg[2] = {S1, S2}, nq[2] = {nq_a, nq_b}, nk[2] = {nk_a, nk_b};
    int64_t grid = 0;
    for (int i = 0; i < 2; ++i) {
        AttnMixedPlan::Group& a = m.g[i];
        if (Sg[i] == 0) continue;
        CHK(attn_seq_rule(a, nq[i], nk[i], true));
        a.pose_blocks = a.pose == 1 ? Sg[i] * heads : 0;
        grid += (int64_t)a.qblocks * heads * Sg[i] + a.pose_blocks;
    }
    REQUIRE(grid < ((int64_t)1 << 31), "attention grid of %lld workgroups", (long long)grid);
    m.grid = (int)grid;
    m.nwg_a = m.g[0].qblocks * heads * S1;
    bool any = false;
    for (int i = 0; i < 2; ++i)
        if (Sg[i] != 0 && attn_seq_finish(m.g[i], nk[i], m.grid, no_prefetch)) any = true;
    attn_lds(m, any, split);
    out = m;
    return 0;
}
// attn_varlen_kernel: S <= ATT_MAX_SEQ sequences, sequence s with nq[s] queries over nk[s] keys (the caller resolves kv_shift: nk[s]
// is the count of the sequence s reads).  Logical query-block ids and pose blocks are handed out in sequence order; output rows are
// packed per sequence.  pose_form (decode_varlen_impl): [nq patch rows | pose row] per sequence.  !pose_form (encode_varlen_impl,
// nq == nk == n): no pose token anywhere - no pose blocks, no pose scratch, orow0 = the prefix sum of n, and npad may EQUAL n[s]
// (the pose form reads token index nk as the pose key: here that is row 0 of the next head, or the end of the buffer).
static_assert(ATT_MAX_SEQ == SEQ_MAX, "the attention table (attention.h) and the row table (elementwise.h) hold the same sequences of one call");
static int attn_varlen_plan(int S, int heads, const int* nq, const int* nk, bool pose_form, bool split, bool no_prefetch, AttnVarlenPlan& out) {
    REQUIRE(S > 0 && S <= ATT_MAX_SEQ && heads > 0 && nq && nk, "per-sequence attention takes 1 .. %d sequences", ATT_MAX_SEQ);
    AttnVarlenPlan m{};
    m.S = S;
    const int pr = pose_form ? 1 : 0;
    int64_t nwg = 0, npose = 0, orows = 0;
    for (int i = 0; i < S; ++i) {
        REQUIRE(nq[i] > 0 && nk[i] > 0, "empty attention (sequence %d)", i);
        AttnVarlenPlan::Seq& a = m.s[i];
        a.nq = nq[i]; a.nk = nk[i];
        CHK(attn_seq_rule(a, nq[i], nk[i], pose_form));
        a.pose_blocks = a.pose == 1 ? heads : 0;
        REQUIRE(nwg + npose < ((int64_t)1 << 30) && orows < ((int64_t)1 << 31) - nq[i] - pr, "attention launch too large");
        a.blk0 = (int)nwg; a.pose_blk0 = (int)npose; a.orow0 = (int)orows;
        nwg += (int64_t)a.qblocks * heads; npose += a.pose_blocks; orows += (int64_t)nq[i] + pr;
    }
    REQUIRE(nwg + npose < ((int64_t)1 << 31), "attention grid of %lld workgroups", (long long)(nwg + npose));
    m.nwg = (int)nwg; m.pose_blocks = (int)npose; m.grid = (int)(nwg + npose); m.orows = (int)orows;
    bool any = false;
    for (int i = 0; i < S; ++i)
        if (attn_seq_finish(m.s[i], nk[i], m.grid, no_prefetch)) any = true;
    attn_lds(m, any, split);
    out = m;
    return 0;
}
#ifdef STA_TEST_HOOKS
static void attn_plan_out(const AttnPlan& a, int* out) {
    const int v[11] = {a.pose, a.prefetch, a.stages, a.lds_bytes, a.grid, a.pose_blocks, a.qblocks, a.ntiles, a.nfull, a.tail_stage, a.pose_scratch};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}
// out[11] = {pose mode, prefetch, LDS stages, LDS bytes, grid, pose blocks, query blocks, ntiles, nfull, tail stage, pose scratch bytes}
extern "C" int sta_debug_attn_plan(int S, int heads, int nq, int nk, int pose, int split, int no_prefetch, int* out) {
    REQUIRE(out, "bad argument");
    AttnPlan a;
    CHK(attn_plan(S, heads, nq, nk, pose != 0, split != 0, no_prefetch != 0, a));
    attn_plan_out(a, out);
    return 0;
}
extern "C" int sta_debug_last_attn_plan(sta_handle* h, int* out) {
    REQUIRE(h && out, "bad argument");
    attn_plan_out(h->last_attn, out);
    return 0;
}
// out[b] = the logical id (attn_block_map, the function attn_kernel calls) of query-block workgroup b of nwg
extern "C" int sta_debug_attn_block_map(int nwg, int* out) {
    REQUIRE(out && nwg > 0, "bad argument");
    for (int b = 0; b < nwg; ++b) out[b] = attn_block_map(b, nwg);
    return 0;
}
static void attn_mixed_plan_out(const AttnMixedPlan& m, int* out) {
    out[0] = m.stages; out[1] = m.lds_bytes; out[2] = m.grid; out[3] = m.nwg_a;
    for (int i = 0; i < 2; ++i) {
        const AttnMixedPlan::Group& a = m.g[i];
        const int v[8] = {a.pose, a.prefetch, a.pose_blocks, a.qblocks, a.ntiles, a.nfull, a.tail_stage, a.pose_scratch};
        for (int j = 0; j < 8; ++j) out[4 + 8 * i + j] = v[j];
    }
}
// out[20] = {LDS stages, LDS bytes, grid, query-block workgroups of group a, then per group {pose mode, prefetch, pose blocks, query
// blocks, ntiles, nfull, tail stage, pose scratch bytes}}
extern "C" int sta_debug_attn_mixed_plan(int S1, int S2, int heads, int nq_a, int nk_a, int nq_b, int nk_b, int split, int no_prefetch, int* out) {
    REQUIRE(out, "bad argument");
    AttnMixedPlan m;
    CHK(attn_mixed_plan(S1, S2, heads, nq_a, nk_a, nq_b, nk_b, split != 0, no_prefetch != 0, m));
    attn_mixed_plan_out(m, out);
    return 0;
}
extern "C" int sta_debug_last_attn_mixed_plan(sta_handle* h, int* out) {
    REQUIRE(h && out, "bad argument");
    attn_mixed_plan_out(h->last_attn_mixed, out);
    return 0;
}
// The workgroup -> (sequence, head, query block) map of attn_mixed_kernel's query-block workgroups, computed by the arithmetic the
// kernel uses (attn_block_map over both groups' blocks, group a's logical ids first): out[3 * b + {0, 1, 2}] for workgroup b of
// nwg = heads * (S1 * qblocks_a + S2 * qblocks_b).
extern "C" int sta_debug_attn_mixed_block_map(int S1, int S2, int heads, int qblocks_a, int qblocks_b, int* out) {
    REQUIRE(out && S1 > 0 && S2 >= 0 && heads > 0 && qblocks_a > 0 && (S2 == 0 || qblocks_b > 0), "bad argument");
    const int nwg_a = qblocks_a * heads * S1, nwg = nwg_a + qblocks_b * heads * S2;
    for (int b = 0; b < nwg; ++b) {
        int logical = attn_block_map(b, nwg);
        const bool inb = logical >= nwg_a;
        if (inb) logical -= nwg_a;
        const int nqb = inb ? qblocks_b : qblocks_a;
        out[3 * b] = logical / (nqb * heads) + (inb ? S1 : 0); out[3 * b + 1] = (logical / nqb) % heads; out[3 * b + 2] = logical % nqb;
    }
    return 0;
}
static void attn_varlen_plan_out(const AttnVarlenPlan& m, int* out) {
    const int hd[7] = {m.S, m.stages, m.lds_bytes, m.grid, m.nwg, m.pose_blocks, m.orows};
    for (int j = 0; j < 7; ++j) out[j] = hd[j];
    for (int i = 0; i < m.S; ++i) {
        const AttnVarlenPlan::Seq& a = m.s[i];
        const int v[11] = {a.pose, a.prefetch, a.pose_blocks, a.qblocks, a.ntiles, a.nfull, a.tail_stage, a.pose_scratch, a.blk0, a.pose_blk0, a.orow0};
        for (int j = 0; j < 11; ++j) out[7 + 11 * i + j] = v[j];
    }
}
// The workgroup -> (sequence, head, query block) map of attn_varlen_kernel's query-block workgroups under a plan, by the kernel's
// arithmetic (attn_block_map, then the scan over the plan's first logical ids): out[3 * b + {0, 1, 2}] for workgroup b of the plan's nwg.
static void attn_varlen_block_map_out(const AttnVarlenPlan& m, int heads, int* out) {
    for (int b = 0; b < m.nwg; ++b) {
        int logical = attn_block_map(b, m.nwg), s = 0;
        for (int i = 1; i < m.S; ++i) if (m.s[i].blk0 <= logical) s = i;
        logical -= m.s[s].blk0;
        out[3 * b] = s; out[3 * b + 1] = (logical / m.s[s].qblocks) % heads; out[3 * b + 2] = logical % m.s[s].qblocks;
    }
}
// out[7 + 11 * S] = {S, LDS stages, LDS bytes, grid, query-block workgroups, pose blocks, output rows, then per sequence {pose mode,
// prefetch, pose blocks, query blocks, ntiles, nfull, tail stage, pose scratch bytes, first logical id, first pose block, first output row}}
extern "C" int sta_debug_attn_varlen_plan(int S, int heads, const int* nq, const int* nk, int split, int no_prefetch, int* out) {
    REQUIRE(out, "bad argument");
    AttnVarlenPlan m;
    CHK(attn_varlen_plan(S, heads, nq, nk, true, split != 0, no_prefetch != 0, m));
    attn_varlen_plan_out(m, out);
    return 0;
}
extern "C" int sta_debug_last_attn_varlen_plan(sta_handle* h, int* out) {
    REQUIRE(h && out, "bad argument");
    attn_varlen_plan_out(h->last_attn_varlen, out);
    return 0;
}
extern "C" int sta_debug_attn_varlen_block_map(int S, int heads, const int* nq, const int* nk, int* out) {
    REQUIRE(out, "bad argument");
    AttnVarlenPlan m;
    CHK(attn_varlen_plan(S, heads, nq, nk, true, true, false, m));
    attn_varlen_block_map_out(m, heads, out);
    return 0;
}
// the encoder form (pose mode, pose blocks, pose scratch and first pose block are 0 in the record)
extern "C" int sta_debug_attn_encv_plan(int S, int heads, const int* n, int split, int no_prefetch, int* out) {
    REQUIRE(out, "bad argument");
    AttnVarlenPlan m;
    CHK(attn_varlen_plan(S, heads, n, n, false, split != 0, no_prefetch != 0, m));
    attn_varlen_plan_out(m, out);
    return 0;
}
extern "C" int sta_debug_last_attn_encv_plan(sta_handle* h, int* out) {
    REQUIRE(h && out, "bad argument");
    attn_varlen_plan_out(h->last_attn_encv, out);
    return 0;
}
extern "C" int sta_debug_attn_encv_block_map(int S, int heads, const int* n, int* out) {
    REQUIRE(out, "bad argument");
    AttnVarlenPlan m;
    CHK(attn_varlen_plan(S, heads, n, n, false, true, false, m));
    attn_varlen_block_map_out(m, heads, out);
    return 0;
}
#endif

// ------------------------------------------------------------------------------------------ attention launch
// the fields of AttnParams every launch fills the same way (the caller memsets the whole params struct first)
static void attn_params(sta_handle* h, AttnParams& p, const QKVOut& qkv, const Planes& out, int ldo, int S, int heads, int kv_shift) {
    p.range = h->range;
    p.Q_hi = qkv.q.hi; p.Q_lo = qkv.q.lo; p.K_hi = qkv.k.hi; p.K_lo = qkv.k.lo; p.Vt_hi = qkv.vt.hi; p.Vt_lo = qkv.vt.lo;
    p.O_hi = out.hi; p.O_lo = out.lo; p.ldo = ldo;
    p.S = S; p.heads = heads; p.npad = qkv.npad; p.kv_shift = kv_shift;
    p.scale_log2e = 0.125f * 1.44269504088896340736f;
}
// K names one attention kernel: K::fn<SPLIT>() is its instantiation (so that a -DSTA_DEV_FAST build never names the f16 one)
struct AttnK { template <bool SPLIT> static constexpr auto fn() { return &attn_kernel<SPLIT>; } };
struct AttnMixedK { template <bool SPLIT> static constexpr auto fn() { return &attn_mixed_kernel<SPLIT>; } };
struct AttnVarlenK { template <bool SPLIT> static constexpr auto fn() { return &attn_varlen_kernel<SPLIT>; } };
template <class K, class P>
static int launch_attn(sta_handle* h, int grid, int lds_bytes, const P& p, hipStream_t st) {
    if (h->prec != STA_PREC_F16) {
        constexpr auto kernel = K::template fn<true>();
        CHK(set_smem_once<kernel>(h->device, attn_smem_bytes<true>(ATT_PREFETCH_TILES)));
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), lds_bytes, st, p);
    } else {
        STA_F16ONLY(hipLaunchKernelGGL(K::template fn<false>(), dim3((unsigned)grid), dim3(256), lds_bytes, st, p));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int run_attn(sta_handle* h, const QKVOut& qkv, const Planes& out, int ldo, int S, int heads,
                    int nq, int nk, int kv_shift, hipStream_t st, bool pose = false) {
    if (h->dry) return 0;
    REQUIRE(!pose || (nq == nk && nq + 1 <= qkv.npad), "internal: pose-token attention needs nq == nk < npad");
    AttnPlan a;
    CHK(attn_plan(S, heads, nq, nk, pose, h->prec != STA_PREC_F16, h->opt[5] == 1, a));
    h->last_attn = a;
    REQUIRE(!pose || (int64_t)(qkv.npad + 8 + 256) * 4 <= attn_smem_bytes<false>(), "internal: pose-query scratch exceeds the LDS allocation");
    REQUIRE(!pose || qkv.npad % 64 == 0, "internal: pose-query path needs npad % 64 == 0");
    AttnParams p; memset(&p, 0, sizeof p);
    attn_params(h, p, qkv, out, ldo, S, heads, kv_shift);
    p.nq = nq; p.nk = nk; p.pose = a.pose; p.prefetch = a.prefetch;
    return launch_attn<AttnK>(h, a.grid, a.lds_bytes, p, st);
}

// out: [S1*nq_a patch rows | S1 pose rows | S2*nq_b patch rows | S2 pose rows] (decode_mixed_impl's row order), out.rp rows in all
static int run_attn_mixed(sta_handle* h, const QKVOut& qkv, const Planes& out, int ldo, int S1, int S2, int heads,
                          int nq_a, int nk_a, int nq_b, int nk_b, int kv_shift, hipStream_t st) {
    if (h->dry) return 0;
    AttnMixedPlan m;
    CHK(attn_mixed_plan(S1, S2, heads, nq_a, nk_a, nq_b, nk_b, h->prec != STA_PREC_F16, h->opt[5] == 1, m));
    h->last_attn_mixed = m;
    const int nmax = std::max(std::max(nq_a, nk_a), S2 ? std::max(nq_b, nk_b) : 0);
    REQUIRE(nmax + 1 <= qkv.npad && qkv.npad % 64 == 0, "internal: two-group attention needs max(nq, nk) < npad, npad %% 64 == 0");
    REQUIRE(kv_shift >= 0 && kv_shift < S1 + S2, "internal: kv_shift out of range");
    const int64_t orows = (int64_t)S1 * (nq_a + 1) + (int64_t)S2 * (nq_b + 1);
    REQUIRE(out.rp == orows && orows < ((int64_t)1 << 31), "internal: two-group attention output of %lld rows in planes of %lld", (long long)orows, (long long)out.rp);
    AttnMixedParams mp; memset(&mp, 0, sizeof mp);
    attn_params(h, mp.a, qkv, out, ldo, S1 + S2, heads, kv_shift);
    mp.a.nq = nq_a; mp.a.nk = nk_a; mp.a.pose = m.g[0].pose; mp.a.prefetch = m.g[0].prefetch;
    mp.b.S1 = S1;
    mp.b.nq = S2 ? nq_b : nq_a; mp.b.nk = S2 ? nk_b : nk_a; mp.b.pose = S2 ? m.g[1].pose : m.g[0].pose; mp.b.prefetch = m.g[1].prefetch;
    mp.b.orow0 = S1 * (nq_a + 1); mp.b.orows = (int)orows;
    return launch_attn<AttnMixedK>(h, m.grid, m.lds_bytes, mp, st);
}

// attn_varlen_kernel under a plan of either form
static int launch_attn_varlen(sta_handle* h, const QKVOut& qkv, const Planes& out, int ldo, int heads, const AttnVarlenPlan& m, int kv_shift, hipStream_t st) {
    REQUIRE(out.rp == m.orows, "internal: per-sequence attention output of %d rows in planes of %lld", m.orows, (long long)out.rp);
    AttnVarlenParams vp; memset(&vp, 0, sizeof vp);
    attn_params(h, vp.a, qkv, out, ldo, m.S, heads, kv_shift);
    vp.nwg = m.nwg; vp.npose_blocks = m.pose_blocks; vp.orows = m.orows;
    for (int s = 0; s < m.S; ++s) {
        const AttnVarlenPlan::Seq& a = m.s[s];
        vp.seq[s] = AttnSeq{a.nq, a.nk, a.pose, a.prefetch, a.blk0, a.pose_blk0, a.orow0, 0};
    }
    return launch_attn<AttnVarlenK>(h, m.grid, m.lds_bytes, vp, st);
}
// out: [nq[s] patch rows | pose row] per sequence (decode_varlen_impl's row order), out.rp rows in all.  nq[s]: queries of sequence s;
// nk[s]: the keys it reads, which are those of buffer sequence (s + kv_shift) % S.
static int run_attn_varlen(sta_handle* h, const QKVOut& qkv, const Planes& out, int ldo, int S, int heads, const int* nq, const int* nk, int kv_shift, hipStream_t st) {
    if (h->dry) return 0;
    REQUIRE(S > 0 && S <= ATT_MAX_SEQ && kv_shift >= 0 && kv_shift < S, "internal: per-sequence attention arguments");
    int nmax = 0;
    for (int s = 0; s < S; ++s) nmax = std::max(nmax, std::max(nq[s], nk[s]));
    AttnVarlenPlan m;
    CHK(attn_varlen_plan(S, heads, nq, nk, true, h->prec != STA_PREC_F16, h->opt[5] == 1, m));
    h->last_attn_varlen = m;
    REQUIRE(nmax + 1 <= qkv.npad && qkv.npad % 64 == 0, "internal: per-sequence attention needs max(n) < npad, npad %% 64 == 0");
    return launch_attn_varlen(h, qkv, out, ldo, heads, m, kv_shift, st);
}
// out: [n[s] rows] per sequence, packed (encode_varlen_impl's row order), out.rp = sum(n) rows
static int run_attn_encv(sta_handle* h, const QKVOut& qkv, const Planes& out, int ldo, int S, int heads, const int* n, hipStream_t st) {
    if (h->dry) return 0;
    REQUIRE(S > 0 && S <= ATT_MAX_SEQ, "internal: per-sequence attention arguments");
    int nmax = 0;
    for (int s = 0; s < S; ++s) nmax = std::max(nmax, n[s]);
    AttnVarlenPlan m;
    CHK(attn_varlen_plan(S, heads, n, n, false, h->prec != STA_PREC_F16, h->opt[5] == 1, m));
    h->last_attn_encv = m;
    REQUIRE(nmax <= qkv.npad && qkv.npad % 64 == 0, "internal: encoder per-sequence attention needs max(n) <= npad, npad %% 64 == 0");
    return launch_attn_varlen(h, qkv, out, ldo, heads, m, 0, st);
}

// sta_decode_varlen: rotate nbuf (<= 3) Q / K buffers [S][heads][npad][64] in place, sequence s by its slice of the packed positions
// table (SeqTable): one launch of rope_varlen_kernel
// pose = false (sta_encode_varlen's per-sequence QKV route): buffers without a pose row, n_s rows per (sequence, head)
static int rope_varlen_launch(sta_handle* h, const Planes* const* bufs, int nbuf, const SeqTable& t, int heads, int npad, const int* pos, hipStream_t st, bool pose = true) {
    REQUIRE(nbuf >= 1 && nbuf <= 3 && pos && h->rope_tab && t.S >= 1 && t.S <= SEQ_MAX, "internal: rope_varlen_launch arguments");
    const int pr = pose ? 1 : 0;
    for (int s = 0; s < t.S; ++s) REQUIRE(t.tok0[s + 1] - t.tok0[s] >= 1 && t.tok0[s + 1] - t.tok0[s] + pr <= npad, "internal: rope_varlen_launch rows exceed npad");
    RopeVarlenParams p;
    for (int b = 0; b < 3; ++b) { p.hi[b] = bufs[b < nbuf ? b : 0]->hi; p.lo[b] = bufs[b < nbuf ? b : 0]->lo; }
    p.heads = heads; p.npad = npad; p.pos = pos; p.tab = h->rope_tab; p.rng = h->range; p.t = t;
    const int64_t total = ((int64_t)t.tok0[t.S] + t.S * pr) * heads * 4;
    const dim3 grid((unsigned)((total + 255) / 256), nbuf);
    if (!pose) {
        if (bufs[0]->lo) hipLaunchKernelGGL((rope_varlen_kernel<true, false>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((rope_varlen_kernel<false, false>), grid, dim3(256), 0, st, p);
    } else if (bufs[0]->lo) hipLaunchKernelGGL(rope_varlen_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(rope_varlen_kernel<false>, grid, dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    return 0;
}

// sta_encode_varlen: qkv_finish_kernel's VARLEN form on the fp32 rows [tok0[S], 3E] of one dense QKV GEMM (bias: nullptr when the
// GEMM added it).  sum_s ceil(n_s / 64) x heads tiles, times three (Q, K, V).
static int qkv_finish_varlen(sta_handle* h, const float* slab, const float* bias, int E, int heads, const SeqTable& t, const QKVOut& o, const int* pos, hipStream_t st) {
    REQUIRE(slab && pos && h->rope_tab && t.S >= 1 && t.S <= SEQ_MAX && E == heads * 64, "internal: qkv_finish_varlen arguments");
    int64_t tiles = 0;
    for (int s = 0; s < t.S; ++s) {
        const int n = t.tok0[s + 1] - t.tok0[s];
        REQUIRE(n >= 1 && n <= o.npad, "internal: qkv_finish_varlen rows exceed npad");
        tiles += (n + 63) / 64;
    }
    REQUIRE(o.npad % 64 == 0 && tiles * heads < ((int64_t)1 << 31), "internal: qkv_finish_varlen grid");
    QkvVarlenParams p;
    p.slab = slab; p.lds = (int64_t)3 * E; p.bias = bias; p.E = E; p.heads = heads; p.npad = o.npad; p.pos = pos; p.rope_tab = h->rope_tab;
    p.Q_hi = o.q.hi; p.Q_lo = o.q.lo; p.K_hi = o.k.hi; p.K_lo = o.k.lo; p.Vt_hi = o.vt.hi; p.Vt_lo = o.vt.lo;
    p.range = h->range; p.t = t;
    const dim3 grid((unsigned)(tiles * heads), 3);
    if (o.q.lo) hipLaunchKernelGGL((qkv_finish_kernel<true, QkvVarlenParams>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((qkv_finish_kernel<false, QkvVarlenParams>), grid, dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    return 0;
}

static int run_rows_to_planes(sta_handle* h, const float* x, int64_t bstride, int nb, int rows, int C, const Planes& o, hipStream_t st, int64_t obstride = 0, bool mx = false) {
    if (h->dry) return 0;
    int64_t total4 = (int64_t)nb * rows * C / 4;
    int blocks = (int)((total4 + 255) / 256); if (blocks > 8192) blocks = 8192;
    if (h->prec != STA_PREC_F16) hipLaunchKernelGGL(rows_to_planes_kernel<true>, dim3(blocks), dim3(256), 0, st, x, bstride, rows, C, total4, o.hi, o.lo, obstride, o.rp, mx ? 1 : 0, h->range);
    else hipLaunchKernelGGL(rows_to_planes_kernel<false>, dim3(blocks), dim3(256), 0, st, x, bstride, rows, C, total4, o.hi, o.lo, obstride, o.rp, 0, h->range);
    HIPCHK(hipGetLastError());
    return 0;
}

static int run_up2(sta_handle* h, const Planes& in, int n, int Hi, int Wi, int C, int Hc, int Wc, const Planes& out, hipStream_t st) {
    if (h->dry) return 0;
    REQUIRE(in.mx == out.mx && C % 8 == 0, "internal: bilinear format mismatch");
    // four output rows per workgroup from 64 rows on (shared taps: half the tap loads, a third of the L2 fetches); one row per
    // workgroup below that, where the grid would no longer fill the chip - and in precision f16, which has the one-row form only
    // (its grid must be n * Hc workgroups: sized for four rows it left three quarters of the output unwritten)
    const bool split = h->prec != STA_PREC_F16;
    const bool quad = split && Hc >= 64 && (int64_t)n * ((Hc + 3) / 4) >= 512 && h->opt[7] != 1;
    const int blocks = quad ? n * ((Hc + 3) / 4) : n * Hc;
    if (split) {
        if (quad) hipLaunchKernelGGL((bilinear_up2_kernel<true, 4>), dim3(blocks), dim3(256), 0, st, in.hi, in.lo, n, Hi, Wi, C, Hc, Wc, out.hi, out.lo, in.mx ? 1 : 0, h->range);
        else hipLaunchKernelGGL((bilinear_up2_kernel<true, 1>), dim3(blocks), dim3(256), 0, st, in.hi, in.lo, n, Hi, Wi, C, Hc, Wc, out.hi, out.lo, in.mx ? 1 : 0, h->range);
    } else {
        STA_F16ONLY(hipLaunchKernelGGL((bilinear_up2_kernel<false, 1>), dim3(blocks), dim3(256), 0, st, in.hi, in.lo, n, Hi, Wi, C, Hc, Wc, out.hi, out.lo, 0, h->range));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------ varlen DPT head: launch forms
// One launch over the packed pixels of B entries of different size (sta_head_pts_varlen; geometry table: VlGeo, sta_common.h).
// vl_geo: entry b is hi[b] x wi[b] input pixels -> ho[b] x wo[b] output pixels; offsets = prefix sums (host values).
static VlGeo vl_geo(int B, const int* hi, const int* wi, const int* ho, const int* wo) {
    VlGeo g; memset(&g, 0, sizeof g);
    g.B = B;
    int64_t a = 0, o = 0;
    for (int b = 0; b < B; ++b) {
        g.hi[b] = hi[b]; g.wi[b] = wi[b]; g.ho[b] = ho[b]; g.wo[b] = wo[b];
        g.in0[b] = (int)a; g.out0[b] = (int)o;
        a += (int64_t)hi[b] * wi[b]; o += (int64_t)ho[b] * wo[b];
    }
    g.in0[B] = (int)a; g.out0[B] = (int)o;      // (the callers check that every level has fewer than 2^31 rows)
    return g;
}
// 3x3 conv, pad 1, stride 1 or 2, every entry on its own (no tap leaves the entry): conv3 with per-entry geometry
static int conv3_vl(sta_handle* h, const Planes& in, const VlGeo& g, int Cin, const Lin& W, int stride,
                    bool relu_in, int act, const Planes& out, const Planes* r1, const Planes* r2, hipStream_t st) {
    GemmParams p; memset(&p, 0, sizeof p);
    p.A_hi = in.hi; p.A_lo = in.lo; p.a_rp = in.rp;
    p.Cin = Cin; p.cstride = stride; p.relu_in = relu_in ? 1 : 0;       // Hi / Wi / Ho / Wo stay 0: the table has them, and no family that needs ONE image size is chosen
    const bool mx = use_mx(h, W);
    REQUIRE(h->dry || in.mx == mx, "internal: conv input format mismatch");
    p.mx = mx ? 1 : 0;
    p.B_hi = mx ? W.wmx.hi : W.w.hi; p.B_lo = mx ? W.wmx.lo : W.w.lo; p.bias = W.bias;
    p.M = g.out0[g.B]; p.N = W.N; p.K = W.K;
    REQUIRE(W.K == 9 * Cin, "conv weight K mismatch");
    for (int b = 0; b < g.B; ++b)
        REQUIRE(g.ho[b] == (g.hi[b] - 1) / stride + 1 && g.wo[b] == (g.wi[b] - 1) / stride + 1, "internal: varlen conv geometry of entry %d", b);
    for (int b = 0; b < g.B; ++b) REQUIRE(g.wi[b] < (1 << 23), "entry %d is %d pixels wide: the varlen tap loader takes rows of fewer than 2^23 pixels", b, g.wi[b]);
    p.C_hi = out.hi; p.C_lo = out.lo; p.ldc16 = W.N; p.act = act; p.c_rp = out.rp; p.c_mx = out.mx ? 1 : 0;
    REQUIRE(h->dry || (g.in0[g.B] == in.rp && out.rp == p.M), "internal: conv plane rows mismatch");
    if (r1) { p.R1_hi = r1->hi; p.R1_lo = r1->lo; p.r_mx = r1->mx ? 1 : 0; REQUIRE(h->dry || r1->rp == out.rp, "internal: residual rows mismatch"); }
    if (r2) { p.R2_hi = r2->hi; p.R2_lo = r2->lo; REQUIRE(h->dry || (r2->rp == out.rp && (!r1 || r1->mx == r2->mx)), "internal: residual rows / format mismatch"); p.r_mx = r2->mx ? 1 : 0; }
    return launch_gemm<A_CONV3, EPI_F16>(h, p, st, nullptr, &g);
}
// the fused tail (conv3_head) on packed pixels: pixel i of the pack -> pts[3 i], conf[i] (the implied packing only)
static int conv3_head_vl(sta_handle* h, const Planes& in, const VlGeo& g, int Cin, const Lin& W, const F32Lin& W4, float* pts, float* conf, hipStream_t st) {
    GemmParams p; memset(&p, 0, sizeof p);
    p.A_hi = in.hi; p.A_lo = in.lo; p.a_rp = in.rp;
    p.Cin = Cin; p.cstride = 1; p.relu_in = 0;
    const bool mx = use_mx(h, W);
    REQUIRE(h->dry || in.mx == mx, "internal: conv input format mismatch");
    p.mx = mx ? 1 : 0;
    p.B_hi = mx ? W.wmx.hi : W.w.hi; p.B_lo = mx ? W.wmx.lo : W.w.lo; p.bias = W.bias;
    p.M = g.out0[g.B]; p.N = W.N; p.K = W.K;
    REQUIRE(W.K == 9 * Cin && W.N == 128, "conv weight shape mismatch (fused head)");
    REQUIRE(h->dry || g.in0[g.B] == in.rp, "internal: conv plane rows mismatch");
    for (int b = 0; b < g.B; ++b) REQUIRE(g.wi[b] < (1 << 23), "entry %d is %d pixels wide: the varlen tap loader takes rows of fewer than 2^23 pixels", b, g.wi[b]);
    p.hw4 = W4.w; p.hb4 = W4.b; for (int o = 0; o < 4; ++o) p.hw4_scale[o] = h->head4_scale[o];
    p.hptsA = pts; p.hconfA = conf; p.hptsB = nullptr; p.hconfB = nullptr; p.hsplit = p.M;
    return launch_gemm<A_CONV3, EPI_HEAD>(h, p, st, nullptr, &g);
}
// ConvTranspose2d with kernel = stride = k: entry b's hi x wi pixels scatter into ITS k hi x k wi output pixels
static int gemm_convt_vl(sta_handle* h, const Planes& A, const Lin& W, const VlGeo& g, int k, int cout, const Planes& out, hipStream_t st) {
    GemmParams p = gp_dense(A, W.K, W, g.in0[g.B], use_mx(h, W));
    REQUIRE(h->dry || A.mx == (p.mx != 0), "internal: ConvT input format mismatch");
    for (int b = 0; b < g.B; ++b) REQUIRE(g.ho[b] == k * g.hi[b] && g.wo[b] == k * g.wi[b], "internal: varlen ConvT geometry of entry %d", b);
    REQUIRE(h->dry || (out.rp == g.out0[g.B] && A.rp == g.in0[g.B]), "internal: ConvT plane rows mismatch");
    p.C_hi = out.hi; p.C_lo = out.lo; p.ct_k = k; p.ct_cout = cout; p.c_rp = out.rp; p.c_mx = out.mx ? 1 : 0;
    return launch_gemm<A_DENSE, EPI_CONVT>(h, p, st, nullptr, &g);
}
// bilinear x2 (align_corners), entry b: hi x wi -> ho x wo <= 2 hi x 2 wi (the crop); one workgroup per output row of an entry
static int run_up2_vl(sta_handle* h, const Planes& in, const VlGeo& g, int C, const Planes& out, hipStream_t st) {
    if (h->dry) return 0;
    REQUIRE(in.mx == out.mx && C % 8 == 0, "internal: bilinear format mismatch");
    REQUIRE(h->prec != STA_PREC_F16, "internal: the varlen bilinear has no precision-f16 form");
    int64_t rows = 0;
    for (int b = 0; b < g.B; ++b) {
        REQUIRE(g.ho[b] >= 1 && g.wo[b] >= 1 && g.ho[b] <= 2 * g.hi[b] && g.wo[b] <= 2 * g.wi[b], "internal: varlen bilinear geometry of entry %d", b);
        rows += g.ho[b];
    }
    REQUIRE(in.rp == g.in0[g.B] && out.rp == g.out0[g.B], "internal: bilinear plane rows mismatch");
    hipLaunchKernelGGL((bilinear_up2_kernel<true, 1, VlGeo>), dim3((unsigned)rows), dim3(256), 0, st, in.hi, in.lo, g, C, in.rp, out.rp, out.hi, out.lo, in.mx ? 1 : 0, h->range);
    HIPCHK(hipGetLastError());
    return 0;
}
// fp32 rows -> planes through a row table (RowSrc, elementwise.h): one launch for the rows of every entry
static int run_rows_to_planes_src(sta_handle* h, const float* x, const RowSrc& rs, int C, const Planes& o, hipStream_t st, bool mx) {
    if (h->dry) return 0;
    REQUIRE(h->prec != STA_PREC_F16, "internal: the row-table form has no precision-f16 form");
    const int64_t total4 = (int64_t)rs.t.tok0[rs.t.S] * C / 4;
    int blocks = (int)((total4 + 255) / 256); if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL((rows_to_planes_kernel<true, RowSrc>), dim3(blocks), dim3(256), 0, st, x, rs, C, total4, o.hi, o.rp, mx ? 1 : 0, h->range);
    HIPCHK(hipGetLastError());
    return 0;
}

static int ensure_rope(sta_handle* h, int P) {
    if (P <= h->rope_P && h->rope_tab) return 0;
    // cos/sin of pos * base^(-d/16), pos = -1 .. P-1, fp32 like the reference python path (pos_embed.py:127-146)
    std::vector<float> tab((size_t)(P + 1) * 32);
    for (int pi = 0; pi <= P; ++pi)
        for (int d = 0; d < 16; ++d) {
            float inv_freq = 1.0f / powf(h->cfg.rope_base, (float)d / 16.0f);
            float f = (float)(pi - 1) * inv_freq;
            tab[((size_t)pi * 16 + d) * 2 + 0] = cosf(f);
            tab[((size_t)pi * 16 + d) * 2 + 1] = sinf(f);
        }
    HIPCHK(hipDeviceSynchronize()); h->n_devsync++;
    if (h->rope_tab) { HIPCHK(hipFree(h->rope_tab)); h->n_alloc++; }
    HIPCHK(hipMalloc((void**)&h->rope_tab, tab.size() * 4)); h->n_alloc++;
    HIPCHK(hipMemcpy(h->rope_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    h->rope_P = P;
    return 0;
}


