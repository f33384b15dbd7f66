// Entry points of the rows either side of the STA forward (SURVEY.md section 8 rows f1-f4), declared in
// include/sta_mi355.h: f3 input step (sta_preprocess_frame), f4 output step (sta_world_pointcloud, sta_mat_to_se3),
// f1 post-STA reductions (sta_estimate_intrinsics, sta_estimate_scale), f2 keyframe scheduler (sta_regress_views),
// f5 geometric consistency (sta_view_consistency, sta_symmetric_geo_mask).
// Included by sta_api.hip (one translation unit); kernels live in elementwise.h and geo.h.

// ---------------------------------------------------------------------------------------------------------
// f3: input step.  Host side = the integer geometry of _crop_resize_if_necessary_image_only
// (base_view_graph_dataset.py:171-225) and Pillow's coefficient tables (Resample.c precompute_coeffs +
// normalize_coeffs_8bpc), in double like the original; device side = elementwise.h pre_*_kernel.
static double pre_lanczos(double x) {
    auto sinc = [](double v) { if (v == 0.0) return 1.0; v = v * M_PI; return sin(v) / v; };
    if (-3.0 <= x && x < 3.0) return sinc(x) * sinc(x / 3.0);
    return 0.0;
}
// coefficients for output samples [o0, o0+cnt) of an in_size -> out_size resample; returns ksize
static int pre_coeffs(int in_size, int out_size, int o0, int cnt, std::vector<int>& bounds, std::vector<int>& kk) {
    double scale, filterscale;
    filterscale = scale = (double)((float)in_size - 0.0f) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 3.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    bounds.assign((size_t)cnt * 2, 0);
    kk.assign((size_t)cnt * ksize, 0);
    std::vector<double> w(ksize);
    const double ss = 1.0 / filterscale;
    for (int q = 0; q < cnt; ++q) {
        const int xx = o0 + q;
        const double center = 0.0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5); if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5); if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) { w[x] = pre_lanczos((x + xmin - center + 0.5) * ss); ww += w[x]; }
        for (int x = 0; x < xmax; ++x) {
            double v = w[x];
            if (ww != 0.0) v /= ww;
            kk[(size_t)q * ksize + x] = v < 0 ? (int)(-0.5 + v * (1 << 22)) : (int)(0.5 + v * (1 << 22));
        }
        bounds[2 * q] = xmin; bounds[2 * q + 1] = xmax;
    }
    return ksize;
}

// first crop (l, t, cw x ch) and the orientation rule of base_view_graph_dataset.py:200-210: a portrait crop
// (ch > 1.1 cw) transposes the resolution; returns nullptr or the error text
static const char* pre_first_crop(int Hs, int Ws, int res_H, int res_W, int w_edge, int h_edge, int* l_, int* t_, int* cw_, int* ch_,
                                  int* out_H, int* out_W) {
    if (!(Hs > 0 && Ws > 0 && res_H > 0 && res_W > 0 && w_edge >= 0 && h_edge >= 0)) return "bad size";
    if (res_W < res_H) return "resolution must be landscape or square (W >= H); a portrait FRAME transposes it by itself";
    const int cx = (int)(Ws / 2.0), cy = (int)(Hs / 2.0);
    const int mx = cx < Ws - cx ? cx : Ws - cx, my = cy < Hs - cy ? cy : Hs - cy;
    if (!(mx > Ws / 5.0 && my > Hs / 5.0)) return "Bad principal point";
    int l = cx - mx, t = cy - my, r = cx + mx, b = cy + my;
    if (l < w_edge) l = w_edge; if (t < h_edge) t = h_edge;
    if (r > Ws - w_edge) r = Ws - w_edge; if (b > Hs - h_edge) b = Hs - h_edge;
    const int cw = r - l, ch = b - t;
    if (!(cw > 0 && ch > 0)) return "edge margins leave no image";
    if (0.9 < (double)ch / cw && (double)ch / cw < 1.1 && res_W != res_H)
        return "square frame with a non-square resolution: the reference picks the orientation at random";
    const bool portrait = ch > 1.1 * cw;
    *l_ = l; *t_ = t; *cw_ = cw; *ch_ = ch;
    *out_H = portrait ? res_W : res_H; *out_W = portrait ? res_H : res_W;
    return nullptr;
}

extern "C" int sta_preprocess_geometry(int Hs, int Ws, int res_H, int res_W, int w_edge, int h_edge, int* out_H, int* out_W) {
    REQUIRE(out_H && out_W, "null argument");
    int l, t, cw, ch;
    const char* err = pre_first_crop(Hs, Ws, res_H, res_W, w_edge, h_edge, &l, &t, &cw, &ch, out_H, out_W);
    REQUIRE(!err, "%s", err);
    return 0;
}

extern "C" int sta_preprocess_frame(sta_handle* h, const uint8_t* src, int Hs, int Ws, int res_H, int res_W, int w_edge, int h_edge,
                                    uint8_t* u8_out, float* rgb_out, float* gray_out, void* stream) {
    REQUIRE(h && src, "null argument");
    REQUIRE(u8_out || rgb_out || gray_out, "no output requested");
    int l, t, cw, ch, out_H, out_W;
    const char* err = pre_first_crop(Hs, Ws, res_H, res_W, w_edge, h_edge, &l, &t, &cw, &ch, &out_H, &out_W);
    REQUIRE(!err, "%s", err);
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int key[6] = {Hs, Ws, res_H, res_W, w_edge, h_edge};
    if (memcmp(key, h->pre_key, sizeof(key)) != 0) {
        const double sx = (double)out_W / cw, sy = (double)out_H / ch;
        const double scale_final = (sx > sy ? sx : sy) + 1e-8;                       // cropping.py:67
        const int rw = (int)floor(cw * scale_final), rh = (int)floor(ch * scale_final);
        const int l2 = (int)nearbyint(rw / 2.0 - out_W / 2.0), t2 = (int)nearbyint(rh / 2.0 - out_H / 2.0);   // np.round: half to even
        REQUIRE(l2 >= 0 && t2 >= 0 && l2 + out_W <= rw && t2 + out_H <= rh, "internal: final crop outside the rescaled image");
        std::vector<int> bh, kh, bv, kv;
        const int ksh = pre_coeffs(cw, rw, l2, out_W, bh, kh);
        const int ksv = pre_coeffs(ch, rh, t2, out_H, bv, kv);
        const int y_first = bv[0], y_last = bv[2 * (out_H - 1)] + bv[2 * (out_H - 1) + 1];
        for (int y = 0; y < out_H; ++y) bv[2 * y] -= y_first;
        const int64_t total = (int64_t)bh.size() + kh.size() + bv.size() + kv.size();
        HIPCHK(hipDeviceSynchronize()); h->n_devsync++;         // earlier frames (on any stream) may still read the old tables
        if (total > h->pre_cap) {
            if (h->pre_tab) { HIPCHK(hipFree(h->pre_tab)); h->n_alloc++; }
            h->pre_tab = nullptr; h->pre_cap = 0;
            HIPCHK(hipMalloc((void**)&h->pre_tab, (size_t)total * 4)); h->n_alloc++;
            h->pre_cap = total;
        }
        std::vector<int> all; all.reserve(total);
        all.insert(all.end(), bh.begin(), bh.end()); all.insert(all.end(), kh.begin(), kh.end());
        all.insert(all.end(), bv.begin(), bv.end()); all.insert(all.end(), kv.begin(), kv.end());
        HIPCHK(hipMemcpy(h->pre_tab, all.data(), (size_t)total * 4, hipMemcpyHostToDevice));
        const int meta[12] = {l, t, ksh, ksv, y_first, y_last - y_first, (int)bh.size(), (int)kh.size(), (int)bv.size(), (int)kv.size(), 0, 0};
        memcpy(h->pre_meta, meta, sizeof(meta));
        memcpy(h->pre_key, key, sizeof(key));
    }
    const int* m = h->pre_meta;
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        uint8_t* tmp = (uint8_t*)ws.take((int64_t)m[5] * out_W * 4);
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        PreParams p;
        p.src = src; p.Ws = Ws; p.l = m[0]; p.t = m[1]; p.ow = out_W; p.oh = out_H;
        p.bh = h->pre_tab; p.kh = p.bh + m[6]; p.ksh = m[2];
        p.bv = p.kh + m[7]; p.kv = p.bv + m[8]; p.ksv = m[3];
        p.y_first = m[4]; p.y_rows = m[5]; p.tmp = tmp;
        p.out_u8 = u8_out; p.out_rgb = rgb_out; p.out_gray = gray_out;
        const int gx = (out_W + 255) / 256;
        hipLaunchKernelGGL(pre_horizontal_kernel, dim3(gx, p.y_rows), dim3(256), 0, st, p);
        hipLaunchKernelGGL(pre_vertical_kernel, dim3(gx, out_H), dim3(256), 0, st, p);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// ---------------------------------------------------------------------------------------------------------
// f4: output step (slam.py:338-421).
extern "C" int sta_world_pointcloud(sta_handle* h, const float* depths, const float* scales, const float* K, const float* poses,
                                    const float* confs, const float* imgs, int N, int H, int W, float conf_thres,
                                    float* pts_out, float* col_out, uint8_t* ply_records_out, int64_t* count_host, void* stream) {
    REQUIRE(h && depths && scales && K && poses && confs && count_host, "null argument");
    REQUIRE(N > 0 && H > 0 && W > 0, "bad size");
    REQUIRE(pts_out || col_out || ply_records_out, "no output requested");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)N * H * W;
    REQUIRE((total + 255) / 256 < (int64_t)1 << 30, "point cloud too large");
    const int nblk = (int)((total + 255) / 256);
    *count_host = 0;
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        int* counts = (int*)ws.take((int64_t)nblk * 4);
        int64_t* offs = (int64_t*)ws.take((int64_t)(nblk + 1) * 8);
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        CloudParams p;
        p.depth = depths; p.scale = scales; p.K = K; p.pose = poses; p.conf = confs; p.img = imgs;
        p.N = N; p.H = H; p.W = W; p.thres = conf_thres; p.counts = counts; p.offs = offs; p.nblk = nblk;
        p.pts = pts_out; p.col = col_out; p.rec = ply_records_out;
        hipLaunchKernelGGL(cloud_count_kernel, dim3(nblk), dim3(256), 0, st, p);
        vox_scan(st, counts, offs, nblk);
        hipLaunchKernelGGL(cloud_emit_kernel, dim3(nblk), dim3(256), 0, st, p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(count_host, offs + nblk, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    });
}

// Voxel-grid fusion of a cloud (kernels in voxel.h; the contract is in the header).  The host learns the bounds and the dropped
// count after the first two kernels - it must, to refuse an over-wide grid and to choose the number of sort passes - and V before
// the reduction: two copies that synchronise the stream.
static double vox_index_host(double p, double o, double vs) {
#pragma clang fp contract(off)
    const double d = p - o;
    return floor(d / vs);
}
static int vox_bit_length(long long v) { int n = 0; while (v > 0) { ++n; v >>= 1; } return n; }

extern "C" int sta_voxel_downsample(sta_handle* h, const float* pts, const float* col, int64_t M, double voxel_size, const double* origin,
                                    int min_points, float* pts_out, float* col_out, int32_t* counts_out, int32_t* index_out,
                                    int32_t* inverse_out, uint8_t* ply_records_out, int64_t* count_host, void* stream) {
    REQUIRE(h && count_host, "null argument");
    REQUIRE(M >= 0 && M < (int64_t)1 << 30, "voxel_downsample takes fewer than 2^30 points (got %lld)", (long long)M);
    REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0, "voxel_size must be finite and > 0 (got %g)", voxel_size);
    REQUIRE(min_points >= 1, "min_points must be >= 1 (got %d)", min_points);
    if (origin) REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "origin must be finite");
    count_host[0] = 0; count_host[1] = 0;
    if (M == 0) return 0;
    REQUIRE(pts, "null argument");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int m = (int)M;
    const int nb256 = (m + 255) / 256, nbb = nb256 < 1024 ? nb256 : 1024;
    const int long_cap = m / VOX_LONG + 1;
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        float* bpart = (float*)ws.take((int64_t)nbb * 32);
        float* bout = (float*)ws.take(32);
        VoxSort sort; VoxScan hscan, rscan;
        vox_take_sort(ws, m, &sort);
        vox_take_scan(ws, nb256, &hscan);
        vox_take_scan(ws, nb256, &rscan);
        int* const cnt_h = hscan.counts; int64_t* const off_h = hscan.offs;
        int* const cnt_r = rscan.counts; int64_t* const off_r = rscan.offs;
        int* seg = (int*)ws.take((int64_t)(m + 1) * 4);
        int2* rows = (int2*)ws.take((int64_t)m * 8);
        int* n_long = (int*)ws.take(4);
        int* long_rows = (int*)ws.take((int64_t)long_cap * 4);
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        // 1. bounds
        hipLaunchKernelGGL(vox_bounds_kernel, dim3(nbb), dim3(256), 0, st, pts, m, bpart);
        hipLaunchKernelGGL(vox_bounds_final_kernel, dim3(1), dim3(256), 0, st, (const float*)bpart, nbb, bout);
        HIPCHK(hipGetLastError());
        float bh[8];
        HIPCHK(hipMemcpyAsync(bh, bout, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int dropped; memcpy(&dropped, &bh[6], 4);
        const int n = m - dropped;                                  // the kept points: the first n sorted positions
        count_host[1] = dropped;
        if (inverse_out) HIPCHK(hipMemsetAsync(inverse_out, 0xff, (size_t)m * 4, st));      // -1 unless a row claims the point
        if (n == 0) return 0;
        VoxGrid g; g.vs = voxel_size;
        long long ext[3];
        for (int a = 0; a < 3; ++a) {
            {
#pragma clang fp contract(off)
                const double half = voxel_size * 0.5;
                g.o[a] = origin ? origin[a] : (double)bh[a] - half;
            }
            const double lo = vox_index_host((double)bh[a], g.o[a], voxel_size), hi = vox_index_host((double)bh[3 + a], g.o[a], voxel_size);
            REQUIRE(lo >= -2147483648.0 && hi <= 2147483647.0, "voxel index outside int32 on axis %d: [%.17g, %.17g] at voxel_size %g", a, lo, hi,
                    voxel_size);
            g.lo[a] = (int)lo;
            ext[a] = (long long)hi - (long long)lo + 1;
        }
        REQUIRE(ext[0] <= VOX_MAX_EXTENT && ext[1] <= VOX_MAX_EXTENT && ext[2] <= VOX_MAX_EXTENT,
                "voxel grid too wide: %lld x %lld x %lld voxels at voxel_size %g (at most %d per axis)", ext[0], ext[1], ext[2], voxel_size,
                VOX_MAX_EXTENT);
        g.nx = vox_bit_length(ext[0] - 1); g.ny = vox_bit_length(ext[1] - 1);
        const int bits = g.nx + g.ny + vox_bit_length(ext[2] - 1);
        // the all-ones key of a dropped point must differ from every voxel's key in the digits that are sorted: a spare bit in the top
        // digit does it, a key width that fills its digits takes one more pass
        const int passes = (bits + 7) / 8 + (dropped > 0 && bits % 8 == 0 ? 1 : 0);
        // 2. keys  3. sort
        hipLaunchKernelGGL(vox_key_kernel, dim3(nb256), dim3(256), 0, st, pts, m, g, sort.key[0], sort.idx[0]);
        const int r = vox_sort(st, sort, m, passes);
        const unsigned long long* skey = sort.key[r];
        const int* sidx = sort.idx[r];
        // 4. heads, then rows
        const int nbn = (n + 255) / 256;
        hipLaunchKernelGGL(vox_head_count_kernel, dim3(nbn), dim3(256), 0, st, skey, n, cnt_h);
        vox_scan(st, cnt_h, off_h, nbn);
        hipLaunchKernelGGL(vox_head_emit_kernel, dim3(nbn), dim3(256), 0, st, skey, n, (const int64_t*)off_h, nbn, seg);
        HIPCHK(hipMemsetAsync(n_long, 0, 4, st));
        hipLaunchKernelGGL(vox_row_count_kernel, dim3(nbn), dim3(256), 0, st, (const int*)seg, (const int64_t*)(off_h + nbn), min_points, cnt_r);
        vox_scan(st, cnt_r, off_r, nbn);
        hipLaunchKernelGGL(vox_row_emit_kernel, dim3(nbn), dim3(256), 0, st, (const int*)seg, (const int64_t*)(off_h + nbn), min_points,
                           (const int64_t*)off_r, rows, n_long, long_rows);
        HIPCHK(hipGetLastError());
        int64_t V = 0;
        HIPCHK(hipMemcpyAsync(&V, off_r + nbn, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        count_host[0] = V;
        if (V == 0 || !(pts_out || col_out || counts_out || index_out || inverse_out || ply_records_out)) return 0;
        // 5. reduce (stream-ordered: the outputs are complete for whatever the caller enqueues on `stream` next)
        VoxOut o;
        o.pts = pts; o.col = col; o.key = skey; o.idx = sidx; o.rows = rows; o.V = (int)V; o.g = g;
        o.pts_out = pts_out; o.col_out = col_out; o.counts_out = counts_out; o.index_out = index_out; o.inverse_out = inverse_out;
        o.rec = ply_records_out;
        hipLaunchKernelGGL(vox_reduce_kernel, dim3(((int)V + 3) / 4), dim3(256), 0, st, o);
        if (n > VOX_LONG)
            hipLaunchKernelGGL(vox_reduce_long_kernel, dim3(long_cap < 256 ? long_cap : 256), dim3(1024), 0, st, o, (const int*)n_long, (const int*)long_rows);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// ---------------------------------------------------------------------------------------------------------
// f5: geometric consistency of depth maps (slam_utils.py:269-419; kernels in geo.h).  Neither call synchronises or copies to
// the host; the workspace comes from the stream's scratch context like f4's.
extern "C" int sta_view_consistency(sta_handle* h, const float* depths, const float* K, const float* poses, int n, int H, int W,
                                    float threshold, int window, int32_t* count_out, void* stream) {
    REQUIRE(h && depths && K && poses && count_out, "null argument");
    REQUIRE(n >= 1 && H > 0 && W > 0, "bad size");
    REQUIRE(window >= 0, "window must be >= 0 (got %d)", window);
    REQUIRE((int64_t)H * W < (int64_t)1 << 30 && n <= 65535, "depth maps too large");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int w = window < n - 1 ? window : n - 1;             // views further than n - 1 apart do not exist: same votes, bounded table
    const int64_t npair = (int64_t)n * (2 * w + 1);
    REQUIRE(npair < (int64_t)1 << 30, "too many view pairs");
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        GeoPair* pairs = (GeoPair*)ws.take(npair * (int64_t)sizeof(GeoPair));
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        hipLaunchKernelGGL(vote_pairs_kernel, dim3((unsigned)((npair + 63) / 64)), dim3(64), 0, st, K, poses, n, w, pairs);
        hipLaunchKernelGGL(view_consistency_kernel, dim3((H * W + 255) / 256, n), dim3(256), 0, st, depths, pairs, n, H, W, w,
                           threshold, count_out);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

extern "C" int sta_symmetric_geo_mask(sta_handle* h, const float* depths, const float* K, const float* rel_pose, int P, int H, int W,
                                      uint8_t* mask_out, float* thres_out, void* stream) {
    REQUIRE(h && depths && K && rel_pose && mask_out, "null argument");
    REQUIRE(P >= 1 && H > 0 && W > 0, "bad size");
    REQUIRE((int64_t)H * W < (int64_t)1 << 30 && P <= 32767, "depth maps too large");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int hw = H * W, slots = 2 * P, gx = (hw + 255) / 256;
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        GeoPair* pairs = (GeoPair*)ws.take((int64_t)slots * sizeof(GeoPair));
        unsigned* err = (unsigned*)ws.take((int64_t)slots * hw * 4);
        const int64_t zero_bytes = (int64_t)slots * (GEO_STATE + 4 * 256) * 4;      // state + the four histograms, cleared together
        int* state = (int*)ws.take(zero_bytes);
        unsigned* hist = (unsigned*)(state + slots * GEO_STATE);
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        HIPCHK(hipMemsetAsync(state, 0, (size_t)zero_bytes, st));
        hipLaunchKernelGGL(sym_pairs_kernel, dim3((slots + 63) / 64), dim3(64), 0, st, K, rel_pose, P, pairs);
        hipLaunchKernelGGL(geo_warp_kernel, dim3(gx, 2, P), dim3(256), 0, st, depths, pairs, H, W, err, state, hist);
        hipLaunchKernelGGL(geo_pick_kernel, dim3(slots), dim3(64), 0, st, hist, 0, state, thres_out);
        for (int pass = 1; pass < 4; ++pass) {
            unsigned* hp = hist + (int64_t)pass * slots * 256;
            hipLaunchKernelGGL(geo_hist_kernel, dim3(gx, slots), dim3(256), 0, st, err, hw, state, pass, hp);
            hipLaunchKernelGGL(geo_pick_kernel, dim3(slots), dim3(64), 0, st, hp, pass, state, thres_out);
        }
        hipLaunchKernelGGL(geo_mask_kernel, dim3(gx, slots), dim3(256), 0, st, err, hw, state, mask_out);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// f6: the general two-view check, local point clouds and ray depths (slam_utils.py:193-266, 82-165; kernels in geo.h).  Like f5:
// no synchronisation, no copy to the host, workspace from the stream's scratch context.  The mask is ten launches behind one
// memset whatever B is: the quantile is ONE selection over the whole batch.
extern "C" int sta_geo_valid_mask(sta_handle* h, const float* depth1, const float* depth2, const float* K1, const float* K2,
                                  const float* T1, const float* T2, int B, int H, int W, float q, uint8_t* mask_out,
                                  float* thres_out, int32_t* count_out, void* stream) {
    REQUIRE(h && depth1 && depth2 && K1 && K2 && T1 && T2 && mask_out, "null argument");
    REQUIRE(B >= 1 && H > 0 && W > 0, "bad size");
    REQUIRE(q >= 0.f && q <= 1.f, "q must lie in [0, 1] (got %g)", (double)q);          // (a NaN q fails too)
    REQUIRE((int64_t)B * H * W <= 16000000, "B*H*W = %lld is above torch.quantile's limit of 16 000 000 elements", (long long)B * H * W);
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int hw = H * W, total = B * hw, gx = (hw + 255) / 256;
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        GeoPair* pairs = (GeoPair*)ws.take((int64_t)B * sizeof(GeoPair));
        unsigned* err = (unsigned*)ws.take((int64_t)total * 4);
        const int64_t zero_bytes = (GQ_STATE + 256 + 3 * 2 * 256) * 4;              // state + hist0 + three two-rank passes, cleared together
        int* state = (int*)ws.take(zero_bytes);
        unsigned* hist0 = (unsigned*)(state + GQ_STATE);
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        HIPCHK(hipMemsetAsync(state, 0, (size_t)zero_bytes, st));
        hipLaunchKernelGGL(geo_q_pairs_kernel, dim3((B + 63) / 64), dim3(64), 0, st, K1, K2, T1, T2, B, pairs);
        hipLaunchKernelGGL(geo_q_warp_kernel, dim3(B * gx), dim3(256), 0, st, depth1, depth2, pairs, H, W, gx, err, state, hist0);
        hipLaunchKernelGGL(geo_q_pick_kernel, dim3(1), dim3(128), 0, st, hist0, 0, q, state, thres_out, count_out);
        const int gh = (total + 256 * GQ_PER - 1) / (256 * GQ_PER);
        for (int pass = 1; pass < 4; ++pass) {
            unsigned* hp = hist0 + 256 + (pass - 1) * 512;
            hipLaunchKernelGGL(geo_q_hist_kernel, dim3(gh), dim3(256), 0, st, err, total, state, pass, hp);
            hipLaunchKernelGGL(geo_q_pick_kernel, dim3(1), dim3(128), 0, st, hp, pass, q, state, thres_out, count_out);
        }
        hipLaunchKernelGGL(geo_q_mask_kernel, dim3((total + 255) / 256), dim3(256), 0, st, err, total, state, mask_out);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// out = element-wise kernel behind one K^-1 per view (n_k = N or 1 matrices)
template <class Launch>
static int geo_with_kinv(sta_handle* h, const float* K, int k_batched, int N, hipStream_t st, Launch launch) {
    const int nk = k_batched ? N : 1;
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        float* kinv = (float*)ws.take((int64_t)nk * 9 * 4);
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        hipLaunchKernelGGL(geo_kinv_kernel, dim3((nk + 63) / 64), dim3(64), 0, st, K, nk, kinv);
        launch(kinv);
        HIPCHK(hipGetLastError());
        return 0;
    });
}
extern "C" int sta_local_pointclouds(sta_handle* h, const float* depths, const float* K, int k_batched, int N, int H, int W,
                                     float* out, void* stream) {
    REQUIRE(h && depths && K && out, "null argument");
    REQUIRE(N >= 1 && H > 0 && W > 0, "bad size");
    REQUIRE(k_batched == 0 || k_batched == 1, "k_batched must be 0 or 1 (got %d)", k_batched);
    const int64_t hw = (int64_t)H * W, gx = (3 * hw + 255) / 256;
    REQUIRE(hw < (int64_t)1 << 29 && N * gx < (int64_t)1 << 31, "depth maps too large");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    return geo_with_kinv(h, K, k_batched, N, st, [&](const float* kinv) {
        hipLaunchKernelGGL(geo_local_points_kernel, dim3((unsigned)(N * gx)), dim3(256), 0, st, depths, kinv, k_batched, H, W, (int)gx, out);
    });
}
extern "C" int sta_ray_depth(sta_handle* h, const float* pts, const float* K, int k_batched, int B, int H, int W, float* out,
                             void* stream) {
    REQUIRE(h && pts && K && out, "null argument");
    REQUIRE(B >= 1 && H > 0 && W > 0, "bad size");
    REQUIRE(k_batched == 0 || k_batched == 1, "k_batched must be 0 or 1 (got %d)", k_batched);
    const int64_t hw = (int64_t)H * W, gx = (hw + 255) / 256;
    REQUIRE(hw < (int64_t)1 << 29 && B * gx < (int64_t)1 << 31, "point maps too large");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    return geo_with_kinv(h, K, k_batched, B, st, [&](const float* kinv) {
        hipLaunchKernelGGL(geo_ray_depth_kernel, dim3((unsigned)(B * gx)), dim3(256), 0, st, pts, kinv, k_batched, H, W, (int)gx, out);
    });
}

// Token selections from per-pixel maps (kernels in select.h; the contract is in include/sta_mi355.h).  The per-entry geometry is a
// host table that travels in the kernel arguments, like sta_head_pts_varlen's: two launches, no memset, no workspace, no copy, no
// synchronisation - on the first call of a set of shapes as on any later one.
extern "C" int sta_select_patches(sta_handle* h, const void* const* maps, const int* H, const int* W, int B, int dtype, int mode,
                                  float thres, int invert, int rule, int min_score, const int* top_k, int margin, int32_t* score,
                                  int64_t* index, int64_t* pos, int32_t* n_sel, int32_t* window, void* stream) {
    REQUIRE(h && maps && H && W && score && index && pos && n_sel && window, "null argument");
    REQUIRE(B >= 1 && B <= SEQ_MAX, "bad argument (B = %d): sta_select_patches takes 1 .. %d maps", B, SEQ_MAX);
    REQUIRE(dtype == 0 || dtype == 1, "dtype must be 0 (uint8) or 1 (float32) (got %d)", dtype);
    REQUIRE(mode == 0 || mode == 1, "mode must be 0 (count) or 1 (fixed-point sum) (got %d)", mode);
    REQUIRE(rule == 0 || rule == 1, "rule must be 0 (min_score) or 1 (top_k) (got %d)", rule);
    REQUIRE(mode == 0 || dtype == 1, "the fixed-point sum (mode 1) is defined for float32 maps only");
    REQUIRE(mode == 0 || !invert, "invert is refused with the fixed-point sum (mode 1)");
    REQUIRE(margin >= 0 && margin <= SEL_MAX_MARGIN, "margin must lie in [0, %d] (got %d)", SEL_MAX_MARGIN, margin);
    REQUIRE(min_score >= 0, "min_score must be >= 0 (got %d)", min_score);
    if (rule == 1) {
        REQUIRE(top_k, "null argument (top_k)");
        REQUIRE(margin == 0, "margin is refused with top_k (the count would stop being known on the host; got margin = %d)", margin);
    }
    SelGeo g;
    memset(&g, 0, sizeof(g));
    int max_n = 0;
    for (int b = 0; b < B; ++b) {
        REQUIRE(maps[b], "null argument (maps[%d])", b);
        REQUIRE(H[b] >= 16 && W[b] >= 16 && H[b] % 16 == 0 && W[b] % 16 == 0, "entry %d: H and W must be multiples of 16, at least 16 (got %d x %d)", b, H[b], W[b]);
        const int64_t n = (int64_t)(H[b] / 16) * (W[b] / 16);
        REQUIRE(n <= SEL_MAX_PATCHES, "entry %d: %d x %d is %lld patches, above the limit of %d per entry", b, H[b], W[b], (long long)n, SEL_MAX_PATCHES);
        REQUIRE(dtype == 0 || ((uintptr_t)maps[b] & 3) == 0, "entry %d: a float32 map must be 4-byte aligned", b);
        if (rule == 1) REQUIRE(top_k[b] >= 1 && top_k[b] <= n, "entry %d: top_k must lie in [1, %lld] (got %d)", b, (long long)n, top_k[b]);
        g.map[b] = maps[b]; g.H[b] = H[b]; g.W[b] = W[b]; g.k[b] = rule == 1 ? top_k[b] : 0;
        g.off[b + 1] = g.off[b] + (int)n;
        max_n = (int)n > max_n ? (int)n : max_n;
    }
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int want = (max_n + 15) / 16, gx = want < 256 ? want : 256;      // 16 patches per workgroup and step; larger entries stride
    const dim3 grid(gx, B), block(256);
    if (dtype == 0) hipLaunchKernelGGL(patch_score_kernel<SEL_U8>, grid, block, 0, st, g, thres, invert, score);
    else if (mode == 0) hipLaunchKernelGGL(patch_score_kernel<SEL_F32_THRES>, grid, block, 0, st, g, thres, invert, score);
    else hipLaunchKernelGGL(patch_score_kernel<SEL_F32_SUM>, grid, block, 0, st, g, thres, invert, score);
    hipLaunchKernelGGL(patch_select_kernel, dim3(B), block, 0, st, g, rule, min_score, margin, score, index, pos, n_sel, window);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// The keyframe gate (kernels in flow.h; the contract is in include/sta_mi355.h).  sta_flow_plan holds every size and refusal and is
// host only; the three device calls take the caller's buffers, launch on `stream` and return: no allocation, no copy to the host, no
// synchronisation - the corner count stays on the device and sta_flow_track reads it there.
static int64_t flow_align(int64_t v) { return (v + 255) & ~(int64_t)255; }
static int flow_levels(int H, int W, int win, int max_level, FlowLevels* lv) {
    REQUIRE(H >= 8 && W >= 8, "flow: H and W must be at least 8 (got %d x %d)", H, W);
    REQUIRE((int64_t)H * W <= FLOW_MAX_PIXELS, "flow: %d x %d is %lld pixels, above the limit of %d", H, W, (long long)H * W, FLOW_MAX_PIXELS);
    REQUIRE(win >= 3 && win <= FLOW_MAX_WIN && win % 2 == 1, "flow: win must be odd and lie in [3, %d] (got %d)", FLOW_MAX_WIN, win);
    REQUIRE(max_level >= 0 && max_level < FLOW_MAX_LEVELS, "flow: max_level must lie in [0, %d] (got %d)", FLOW_MAX_LEVELS - 1, max_level);
    memset(lv, 0, sizeof(*lv));
    lv->levels = 1; lv->h[0] = H; lv->w[0] = W; lv->off[0] = 0;
    int64_t end = flow_align((int64_t)H * W);
    while (lv->levels - 1 < max_level) {
        const int l = lv->levels, nh = (lv->h[l - 1] + 1) / 2, nw = (lv->w[l - 1] + 1) / 2;
        if (!(nh > win && nw > win)) break;
        lv->h[l] = nh; lv->w[l] = nw; lv->off[l] = end;
        end += flow_align((int64_t)nh * nw);
        lv->levels = l + 1;
    }
    lv->bytes = end;
    return 0;
}
static int flow_idx_bits(int N) { int n = 0; for (long long v = (long long)N - 1; v > 0; v >>= 1) ++n; return n; }
// the corner workspace: R, cell, two key and two payload arrays of one word per pixel, the sort's histogram, three counters
struct FlowWs { int *R, *cell, *idx[2], *hist, *dtot, *counters; unsigned long long* key[2]; int64_t bytes; };
static FlowWs flow_workspace(void* base, int H, int W) {
    const int64_t N = (int64_t)H * W, nbs = (N + VOX_TILE - 1) / VOX_TILE;
    FlowWs w;
    int64_t o = 0;
    auto take = [&](int64_t b) { void* p = (void*)((uintptr_t)base + (uintptr_t)o); o += flow_align(b); return p; };
    w.key[0] = (unsigned long long*)take(N * 8); w.key[1] = (unsigned long long*)take(N * 8);
    w.R = (int*)take(N * 4); w.cell = (int*)take(N * 4);
    w.idx[0] = (int*)take(N * 4); w.idx[1] = (int*)take(N * 4);
    w.hist = (int*)take(256 * nbs * 4); w.dtot = (int*)take(256 * 4); w.counters = (int*)take(16);
    w.bytes = o;
    return w;
}

extern "C" int sta_flow_plan(int H, int W, int B, int win, int max_level, int max_corners, int64_t out[16]) {
    REQUIRE(out, "null argument");
    FlowLevels lv;
    CHK(flow_levels(H, W, win, max_level, &lv));
    REQUIRE(B >= 1 && B <= FLOW_MAX_FRAMES, "flow: 1 .. %d frames per call (got B = %d)", FLOW_MAX_FRAMES, B);
    REQUIRE(max_corners >= 1 && max_corners <= FLOW_MAX_PIXELS, "flow: max_corners must lie in [1, %d] (got %d)", FLOW_MAX_PIXELS, max_corners);
    memset(out, 0, 16 * sizeof(int64_t));
    out[0] = lv.levels;
    for (int l = 0; l < lv.levels; ++l) { out[1 + l] = lv.h[l]; out[5 + l] = lv.w[l]; out[9 + l] = lv.off[l]; }
    out[13] = lv.bytes;
    out[14] = flow_workspace(nullptr, H, W).bytes;
    return 0;
}

extern "C" int sta_flow_pyramid(sta_handle* h, const void* gray, int dtype, int H, int W, int B, int win, int max_level, uint8_t* pyramid,
                                void* stream) {
    REQUIRE(h && gray && pyramid, "null argument");
    REQUIRE(dtype == 0 || dtype == 1, "flow: dtype must be 0 (uint8) or 1 (float32) (got %d)", dtype);
    FlowLevels lv;
    CHK(flow_levels(H, W, win, max_level, &lv));
    REQUIRE(B >= 1 && B <= FLOW_MAX_FRAMES, "flow: 1 .. %d frames per call (got B = %d)", FLOW_MAX_FRAMES, B);
    REQUIRE(dtype == 0 || ((uintptr_t)gray & 3) == 0, "flow: a float32 frame must be 4-byte aligned");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* up = lv.levels > 1 ? pyramid + lv.off[1] : nullptr;
    const dim3 g0((W + 31) / 32, (H + 31) / 32, B);
    if (dtype == 1)
        hipLaunchKernelGGL(flow_pyrdown_kernel<true>, g0, dim3(256), 0, st, gray, (long long)H * W, H, W, pyramid, up, lv.h[1], lv.w[1], lv.bytes);
    else
        hipLaunchKernelGGL(flow_pyrdown_kernel<false>, g0, dim3(256), 0, st, gray, (long long)H * W, H, W, pyramid, up, lv.h[1], lv.w[1], lv.bytes);
    for (int l = 2; l < lv.levels; ++l)
        hipLaunchKernelGGL(flow_pyrdown_kernel<false>, dim3((lv.w[l - 1] + 31) / 32, (lv.h[l - 1] + 31) / 32, B), dim3(256), 0, st,
                           (const void*)(pyramid + lv.off[l - 1]), lv.bytes, lv.h[l - 1], lv.w[l - 1], (uint8_t*)nullptr, pyramid + lv.off[l],
                           lv.h[l], lv.w[l], lv.bytes);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_flow_corners(sta_handle* h, const uint8_t* image, int H, int W, int max_corners, double quality, int min_distance,
                                int block_size, void* workspace, int64_t workspace_bytes, float* corners, int32_t* n_out, void* stream) {
    REQUIRE(h && image && workspace && corners && n_out, "null argument");
    FlowLevels lv;
    CHK(flow_levels(H, W, FLOW_MAX_WIN, 0, &lv));
    REQUIRE(max_corners >= 1 && max_corners <= FLOW_MAX_PIXELS, "flow: max_corners must lie in [1, %d] (got %d)", FLOW_MAX_PIXELS, max_corners);
    REQUIRE(std::isfinite(quality) && quality > 0.0 && quality <= 1.0, "flow: quality must lie in (0, 1] (got %g)", quality);
    REQUIRE(min_distance >= 1 && min_distance <= FLOW_MAX_MIN_DISTANCE, "flow: min_distance must lie in [1, %d] (got %d)", FLOW_MAX_MIN_DISTANCE, min_distance);
    REQUIRE(block_size == 3 || block_size == 5 || block_size == 7, "flow: block_size must be 3, 5 or 7 (got %d)", block_size);
    REQUIRE(((uintptr_t)workspace & 7) == 0, "flow: the workspace must be 8-byte aligned");
    const FlowWs w = flow_workspace(workspace, H, W);
    REQUIRE(workspace_bytes >= w.bytes, "flow: the workspace holds %lld bytes, %d x %d needs %lld", (long long)workspace_bytes, H, W, (long long)w.bytes);
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int N = H * W, nb256 = (N + 255) / 256;
    int* rmax = w.counters; int* n_cand = w.counters + 1;
    HIPCHK(hipMemsetAsync(w.counters, 0, 16, st));
    hipLaunchKernelGGL(flow_response_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, st, image, H, W, block_size / 2, w.R, rmax);
    const int idx_bits = flow_idx_bits(N), bits = FLOW_R_BITS + idx_bits;
    hipLaunchKernelGGL(flow_key_kernel, dim3(nb256), dim3(256), 0, st, (const int*)w.R, H, W, (const int*)rmax, quality, idx_bits, w.key[0], w.idx[0], n_cand);
    // the all-ones key of a pixel that is no candidate must sort behind every candidate: a spare bit in the top digit does it
    const int passes = (bits + 7) / 8 + (bits % 8 == 0 ? 1 : 0);
    const VoxSort sort{{w.key[0], w.key[1]}, {w.idx[0], w.idx[1]}, w.hist, w.dtot};
    const int* sidx = sort.idx[vox_sort(st, sort, N, passes)];
    hipLaunchKernelGGL(flow_rank_kernel, dim3(nb256), dim3(256), 0, st, sidx, N, (const int*)n_cand, w.cell);
    hipLaunchKernelGGL(flow_suppress_kernel, dim3(1), dim3(1024), 0, st, w.cell, sidx, (const int*)n_cand, H, W, min_distance, max_corners, corners, n_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_flow_track(sta_handle* h, const uint8_t* prev_pyramid, const uint8_t* next_pyramids, int H, int W, int B, int win,
                              int max_level, const float* pts, const int32_t* n_dev, int n_cap, int max_iter, double eps, double min_eig,
                              float* next_pts, uint8_t* status, double* stats, void* stream) {
    REQUIRE(h && prev_pyramid && next_pyramids && stats, "null argument");
    FlowTrack a;
    CHK(flow_levels(H, W, win, max_level, &a.lv));
    REQUIRE(B >= 1 && B <= FLOW_MAX_FRAMES, "flow: 1 .. %d frames per call (got B = %d)", FLOW_MAX_FRAMES, B);
    REQUIRE(n_cap >= 0 && n_cap <= FLOW_MAX_PIXELS, "flow: n_cap must lie in [0, %d] (got %d)", FLOW_MAX_PIXELS, n_cap);
    REQUIRE(n_cap == 0 || (pts && next_pts && status), "null argument");
    REQUIRE(max_iter >= 1 && max_iter <= 1000, "flow: max_iter must lie in [1, 1000] (got %d)", max_iter);
    REQUIRE(std::isfinite(eps) && eps >= 0.0 && std::isfinite(min_eig), "flow: eps must be finite and >= 0, min_eig finite");
    a.prev = prev_pyramid; a.next = next_pyramids; a.pts = pts; a.n_dev = n_dev; a.n_cap = n_cap; a.win = win; a.max_iter = max_iter;
    a.eps = eps; a.min_eig = min_eig; a.out = next_pts; a.status = status;
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (n_cap > 0) hipLaunchKernelGGL(flow_track_kernel, dim3(n_cap, B), dim3(64), 0, st, a);
    hipLaunchKernelGGL(flow_stats_kernel, dim3(B), dim3(256), 0, st, pts, n_dev, n_cap, (const float*)next_pts, (const uint8_t*)status, stats);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Loop candidates (kernels in loop.h; the contract is in include/sta_mi355.h).  sta_orb_plan holds every size and refusal and is host
// only; the three device calls take the caller's buffers, launch on `stream` and return: no allocation, no copy to the host, no
// synchronisation - the keypoint and word counts stay on the device.
static int orb_levels(int H, int W, int nfeatures, int nlevels, int fast_threshold, int edge, OrbLevels* lv) {
    REQUIRE(nlevels >= 1 && nlevels <= ORB_MAX_LEVELS, "orb: nlevels must lie in [1, %d] (got %d)", ORB_MAX_LEVELS, nlevels);
    REQUIRE(nfeatures >= 1 && nfeatures <= ORB_MAX_FEATURES, "orb: nfeatures must lie in [1, %d] (got %d)", ORB_MAX_FEATURES, nfeatures);
    REQUIRE(edge >= ORB_MIN_EDGE && edge <= ORB_MAX_EDGE, "orb: edge must lie in [%d, %d] (got %d)", ORB_MIN_EDGE, ORB_MAX_EDGE, edge);
    REQUIRE(fast_threshold >= 1 && fast_threshold <= 254, "orb: fast_threshold must lie in [1, 254] (got %d)", fast_threshold);
    REQUIRE(H > 2 * edge && W > 2 * edge, "orb: H and W must exceed 2 * edge = %d (got %d x %d)", 2 * edge, H, W);
    REQUIRE((int64_t)H * W <= ORB_MAX_PIXELS, "orb: %d x %d is %lld pixels, above the limit of %d", H, W, (long long)H * W, ORB_MAX_PIXELS);
    memset(lv, 0, sizeof(*lv));
    lv->levels = nlevels; lv->edge = edge; lv->thr = fast_threshold;
    // float64, one operation per step (volatile: no step is fused or reassociated)
    volatile double s = 1.0;
    for (int l = 0; l < nlevels; ++l) {
        volatile double qh = (double)H / s, qw = (double)W / s;
        lv->h[l] = (int)std::nearbyint(qh); lv->w[l] = (int)std::nearbyint(qw);
        s = s * 1.2;
    }
    volatile double f = 1.0 / 1.2, fp = 1.0;
    for (int l = 0; l < nlevels; ++l) fp = fp * f;
    volatile double one_f = 1.0 - f, one_fp = 1.0 - fp;
    volatile double nd = (double)nfeatures * one_f;
    nd = nd / one_fp;
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) {
        lv->nfeat[l] = (int)std::nearbyint(nd);
        sum += lv->nfeat[l];
        nd = nd * f;
    }
    lv->nfeat[nlevels - 1] = std::max(nfeatures - sum, 0);
    sum += lv->nfeat[nlevels - 1];
    lv->rows = std::max(nfeatures, sum);
    int64_t end = 0;
    for (int l = 0; l < nlevels; ++l) {
        if (lv->h[l] <= 2 * edge || lv->w[l] <= 2 * edge) break;
        lv->off[l] = end;
        end += flow_align((int64_t)lv->h[l] * lv->w[l]);
        // survivors are strict 3x3 maxima inside the edge: no two are neighbours
        lv->cand_off[l] = lv->cand_total;
        lv->cand_cap[l] = ((lv->h[l] - 2 * edge + 1) / 2) * ((lv->w[l] - 2 * edge + 1) / 2);
        lv->cand_total += lv->cand_cap[l];
        lv->sel_off[l] = lv->slots;
        lv->slots += lv->nfeat[l];
        lv->built = l + 1;
    }
    lv->bytes = end;
    return 0;
}
// the extraction workspace: four level-shaped planes (levels and blurred levels first: the header promises them to the caller; scores,
// survivors), the candidate lists, the slots, the histograms and 16 counters
struct OrbWs { uint8_t *img, *blur, *score, *surv; long long *candR, *selR; int *candP, *selP, *hist, *counters; int64_t bytes; };
static OrbWs orb_workspace(void* base, const OrbLevels& lv) {
    OrbWs w;
    int64_t o = 0;
    auto take = [&](int64_t b) { void* p = (void*)((uintptr_t)base + (uintptr_t)o); o += flow_align(b); return p; };
    w.img = (uint8_t*)take(lv.bytes); w.blur = (uint8_t*)take(lv.bytes); w.score = (uint8_t*)take(lv.bytes); w.surv = (uint8_t*)take(lv.bytes);
    w.candR = (long long*)take((int64_t)lv.cand_total * 8); w.selR = (long long*)take((int64_t)lv.slots * 8);
    w.candP = (int*)take((int64_t)lv.cand_total * 4); w.selP = (int*)take((int64_t)lv.slots * 4);
    w.hist = (int*)take(ORB_MAX_LEVELS * 256 * 4); w.counters = (int*)take(64);
    w.bytes = o;
    return w;
}

extern "C" int sta_orb_plan(int H, int W, int nfeatures, int nlevels, int fast_threshold, int edge, int64_t out[40]) {
    REQUIRE(out, "null argument");
    OrbLevels lv;
    CHK(orb_levels(H, W, nfeatures, nlevels, fast_threshold, edge, &lv));
    memset(out, 0, 40 * sizeof(int64_t));
    out[0] = lv.levels; out[1] = lv.built;
    for (int l = 0; l < lv.levels; ++l) { out[2 + l] = lv.h[l]; out[10 + l] = lv.w[l]; out[18 + l] = lv.nfeat[l]; out[26 + l] = l < lv.built ? lv.off[l] : -1; }
    out[34] = lv.bytes;
    out[35] = orb_workspace(nullptr, lv).bytes;
    out[36] = lv.rows;
    out[37] = flow_align((int64_t)lv.rows * 4);
    return 0;
}

extern "C" int sta_orb_extract(sta_handle* h, const void* image, int dtype, int H, int W, int nfeatures, int nlevels, int fast_threshold, int edge,
                               const int32_t* trig, const int8_t* pattern, void* workspace, int64_t workspace_bytes, int32_t* kp, int64_t* resp,
                               uint8_t* desc, int32_t* n_out, void* stream) {
    REQUIRE(h && image && trig && pattern && workspace && kp && resp && desc && n_out, "null argument");
    REQUIRE(dtype == 0 || dtype == 1, "orb: dtype must be 0 (uint8) or 1 (float32) (got %d)", dtype);
    OrbLevels lv;
    CHK(orb_levels(H, W, nfeatures, nlevels, fast_threshold, edge, &lv));
    REQUIRE(dtype == 0 || ((uintptr_t)image & 3) == 0, "orb: a float32 frame must be 4-byte aligned");
    REQUIRE(((uintptr_t)trig & 3) == 0 && ((uintptr_t)kp & 3) == 0 && ((uintptr_t)n_out & 3) == 0 && ((uintptr_t)resp & 7) == 0,
            "orb: trig, kp and n_out must be 4-byte aligned, resp 8-byte aligned");
    REQUIRE(((uintptr_t)workspace & 7) == 0, "orb: the workspace must be 8-byte aligned");
    const OrbWs w = orb_workspace(workspace, lv);
    REQUIRE(workspace_bytes >= w.bytes, "orb: the workspace holds %lld bytes, %d x %d with %d features over %d levels needs %lld",
            (long long)workspace_bytes, H, W, nfeatures, nlevels, (long long)w.bytes);
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    int* ncand = w.counters; int* cut = w.counters + 8;
    HIPCHK(hipMemsetAsync(w.hist, 0, ORB_MAX_LEVELS * 256 * 4, st));
    HIPCHK(hipMemsetAsync(w.counters, 0, 64, st));
    const int N = H * W;
    if (dtype == 1) hipLaunchKernelGGL(orb_level0_kernel<true>, dim3((N + 255) / 256), dim3(256), 0, st, image, N, w.img);
    else hipLaunchKernelGGL(orb_level0_kernel<false>, dim3((N + 255) / 256), dim3(256), 0, st, image, N, w.img);
    for (int l = 1; l < lv.built; ++l) {
        volatile double ry = (double)lv.h[l - 1] / (double)lv.h[l], rx = (double)lv.w[l - 1] / (double)lv.w[l];
        hipLaunchKernelGGL(orb_resize_kernel, dim3((lv.w[l] + 15) / 16, (lv.h[l] + 15) / 16), dim3(256), 0, st,
                           (const uint8_t*)(w.img + lv.off[l - 1]), lv.h[l - 1], lv.w[l - 1], w.img + lv.off[l], lv.h[l], lv.w[l], (double)ry, (double)rx);
    }
    const dim3 tiles((W + 15) / 16, (H + 15) / 16, lv.built);      // level 0 is the largest
    hipLaunchKernelGGL(orb_fast_kernel, tiles, dim3(256), 0, st, (const uint8_t*)w.img, lv, w.score);
    hipLaunchKernelGGL(orb_nms_kernel, tiles, dim3(256), 0, st, (const uint8_t*)w.score, lv, w.surv, w.hist);
    hipLaunchKernelGGL(orb_cut_kernel, dim3(1), dim3(64), 0, st, (const int*)w.hist, lv, cut);
    hipLaunchKernelGGL(orb_harris_kernel, tiles, dim3(256), 0, st, (const uint8_t*)w.img, (const uint8_t*)w.surv, lv, (const int*)cut, ncand, w.candR, w.candP);
    int max_cap = 1;
    for (int l = 0; l < lv.built; ++l) max_cap = std::max(max_cap, lv.cand_cap[l]);
    hipLaunchKernelGGL(orb_rank_kernel, dim3((max_cap + 255) / 256, lv.built), dim3(256), 0, st, lv, (const int*)ncand, (const long long*)w.candR,
                       (const int*)w.candP, w.selR, w.selP);
    hipLaunchKernelGGL(orb_blur_kernel, tiles, dim3(256), 0, st, (const uint8_t*)w.img, lv, w.blur);
    hipLaunchKernelGGL(orb_describe_kernel, dim3(std::max(lv.slots, 1)), dim3(64), 0, st, (const uint8_t*)w.img, (const uint8_t*)w.blur, lv,
                       (const int*)ncand, (const long long*)w.selR, (const int*)w.selP, (const int*)trig, (const signed char*)pattern, (int*)kp,
                       (long long*)resp, desc, (int*)n_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_bow_transform(sta_handle* h, const uint8_t* desc, const int32_t* n_dev, int n_cap, const uint8_t* node_desc,
                                 const int32_t* child_first, const int32_t* child_count, const int32_t* word_of, const double* word_weight,
                                 int n_nodes, int n_words, void* workspace, int64_t workspace_bytes, int32_t* words, int32_t* counts, double* vals,
                                 int32_t* n_words_out, void* stream) {
    REQUIRE(h && desc && node_desc && child_first && child_count && word_of && word_weight && workspace && words && counts && vals && n_words_out,
            "null argument");
    REQUIRE(n_cap >= 1 && n_cap <= ORB_MAX_ROWS, "bow: n_cap must lie in [1, %d] (got %d)", ORB_MAX_ROWS, n_cap);
    REQUIRE(n_nodes >= 1 && n_words >= 0 && n_words <= n_nodes, "bow: a vocabulary has at least its root and at most one word per node (got %d nodes, %d words)",
            n_nodes, n_words);
    REQUIRE(((uintptr_t)desc & 3) == 0 && ((uintptr_t)node_desc & 3) == 0, "bow: descriptors must be 4-byte aligned");
    REQUIRE(((uintptr_t)workspace & 3) == 0 && workspace_bytes >= (int64_t)n_cap * 4, "bow: the workspace holds %lld bytes, %d descriptors need %lld",
            (long long)workspace_bytes, n_cap, (long long)n_cap * 4);
    REQUIRE(((uintptr_t)vals & 7) == 0 && ((uintptr_t)word_weight & 7) == 0, "bow: vals and word_weight must be 8-byte aligned");
    BowVocab v;
    v.node_desc = node_desc; v.child_first = child_first; v.child_count = child_count; v.word_of = word_of; v.word_weight = word_weight;
    v.n_nodes = n_nodes; v.n_words = n_words;
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    int* wid = (int*)workspace;
    hipLaunchKernelGGL(bow_walk_kernel, dim3((n_cap + 3) / 4), dim3(256), 0, st, desc, (const int*)n_dev, n_cap, v, wid);
    hipLaunchKernelGGL(bow_reduce_kernel, dim3(1), dim3(1024), 0, st, (const int*)wid, n_cap, word_weight, (int*)words, (int*)counts, vals, (int*)n_words_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_bow_score(sta_handle* h, const int32_t* q_words, const double* q_vals, const int32_t* q_n, int q_cap,
                             const int32_t* db_words, const double* db_vals, const int32_t* db_n, int max_views, int cap, const int32_t* rows, int m,
                             double* sim, void* stream) {
    REQUIRE(h && q_words && q_vals && q_n && db_words && db_vals && db_n, "null argument");
    REQUIRE(max_views >= 1 && cap >= 1 && cap <= ORB_MAX_ROWS, "bow: max_views must be positive and cap lie in [1, %d] (got %d, %d)", ORB_MAX_ROWS,
            max_views, cap);
    REQUIRE(q_cap >= 1 && q_cap <= ORB_MAX_ROWS, "bow: q_cap must lie in [1, %d] (got %d)", ORB_MAX_ROWS, q_cap);
    REQUIRE(m >= 0 && m <= (1 << 20), "bow: m must lie in [0, 2^20] (got %d)", m);
    REQUIRE(m == 0 || (rows && sim), "null argument");
    REQUIRE(((uintptr_t)q_vals & 7) == 0 && ((uintptr_t)db_vals & 7) == 0 && ((uintptr_t)sim & 7) == 0, "bow: values and sim must be 8-byte aligned");
    DEV_SCOPE(h->device);
    if (m > 0) hipLaunchKernelGGL(bow_score_kernel, dim3(m), dim3(64), 0, (hipStream_t)stream, (const int*)q_words, q_vals, (const int*)q_n, q_cap,
                                  (const int*)db_words, db_vals, (const int*)db_n, max_views, cap, (const int*)rows, sim);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// The Sim(3) pose graph (kernels in pgo.h; the contract is in include/sta_mi355.h).  sta_pgo_plan holds every size and refusal and is
// host only.  sta_sim3_op, sta_pgo_index, sta_pgo_linearize and sta_pgo_solve take the caller's buffers, launch on `stream` and return:
// no allocation, no copy to the host, no synchronisation.  sta_pgo_optimize is the host-driven LM loop: it reads ONE record of 64
// bytes back per trial step (its synchronisation) and allocates nothing either.
static int pgo_limits(int n, int E) {
    REQUIRE(n >= 1 && n <= PGO_MAX_NODES, "pgo: n must lie in [1, %d] (got %d)", PGO_MAX_NODES, n);
    REQUIRE(E >= 1 && E <= PGO_MAX_EDGES, "pgo: E must lie in [1, %d] (got %d)", PGO_MAX_EDGES, E);
    return 0;
}
// the workspace of sta_pgo_optimize: every buffer of the four device calls, 256-byte aligned, and the record
struct PgoWs { int *off, *inc, *tmp, *idx_status; double *r, *S, *v, *c, *g, *blocks, *d, *trial, *solve, *rec; int64_t bytes; };
static PgoWs pgo_workspace(void* base, int n, int E) {
    PgoWs w;
    int64_t o = 0;
    auto take = [&](int64_t b) { void* p = (void*)((uintptr_t)base + (uintptr_t)o); o += flow_align(b); return p; };
    w.off = (int*)take((int64_t)(n + 1) * 4); w.inc = (int*)take((int64_t)E * 8); w.tmp = (int*)take((int64_t)E * 16); w.idx_status = (int*)take(4);
    w.r = (double*)take((int64_t)E * 56); w.S = (double*)take((int64_t)E * 392); w.v = (double*)take((int64_t)E * 56); w.c = (double*)take((int64_t)E * 8);
    w.g = (double*)take((int64_t)n * 56); w.blocks = (double*)take((int64_t)n * 392); w.d = (double*)take((int64_t)n * 56);
    w.trial = (double*)take((int64_t)n * 64); w.solve = (double*)take((int64_t)pgo_solve_ws_doubles(n, E) * 8); w.rec = (double*)take(64);
    w.bytes = o;
    return w;
}

extern "C" int sta_pgo_plan(int n, int E, int64_t out[8]) {
    REQUIRE(out, "null argument");
    CHK(pgo_limits(n, E));
    out[0] = (int64_t)(n + 1) * 4; out[1] = (int64_t)E * 8; out[2] = (int64_t)E * 16;
    out[3] = (int64_t)pgo_solve_ws_doubles(n, E) * 8; out[4] = pgo_workspace(nullptr, n, E).bytes; out[5] = n; out[6] = E; out[7] = 0;
    return 0;
}

extern "C" int sta_sim3_op(sta_handle* h, int op, const double* a, const double* b, const uint8_t* mask, double* out, int64_t count, void* stream) {
    REQUIRE(h && a && out, "null argument");
    REQUIRE(op >= SIM3_MUL && op <= SIM3_RETRACT, "sim3: op must lie in [0, 5] (got %d)", op);
    REQUIRE(b || op == SIM3_INV || op == SIM3_EXP || op == SIM3_LOG, "sim3: op %d takes two operands", op);
    REQUIRE(count >= 0 && count <= (1 << 24), "sim3: count must lie in [0, 2^24] (got %lld)", (long long)count);
    REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 7) == 0, "sim3: operands must be 8-byte aligned");
    DEV_SCOPE(h->device);
    if (count > 0) hipLaunchKernelGGL(sim3_op_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, op, a, b, mask, out, (long long)count);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_pgo_index(sta_handle* h, const int32_t* edges, const uint8_t* opt, int n, int E, void* workspace, int64_t workspace_bytes,
                             int32_t* off, int32_t* inc, int32_t* status, void* stream) {
    REQUIRE(h && edges && opt && workspace && off && inc && status, "null argument");
    CHK(pgo_limits(n, E));
    REQUIRE(((uintptr_t)workspace & 3) == 0 && workspace_bytes >= (int64_t)E * 16, "pgo: the index workspace holds %lld bytes, %d edges need %lld",
            (long long)workspace_bytes, E, (long long)E * 16);
    DEV_SCOPE(h->device);
    hipLaunchKernelGGL(pgo_index_kernel, dim3(1), dim3(PGO_THREADS), 0, (hipStream_t)stream, (const int*)edges, opt, n, E, (int*)workspace, (int*)off, (int*)inc,
                       (int*)status);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_pgo_linearize(sta_handle* h, const double* nodes, const int32_t* edges, const double* poses, const double* confs, const uint8_t* opt,
                                 const int32_t* off, const int32_t* inc, const int32_t* idx_status, int n, int E, int full, double* r, double* S, double* v,
                                 double* c, double* g, double* blocks, double* rec, void* stream) {
    REQUIRE(h && nodes && edges && poses && confs && opt && c && rec, "null argument");
    REQUIRE(!full || (off && inc && r && S && v && g && blocks), "pgo: the full form needs off, inc, r, S, v, g and blocks");
    CHK(pgo_limits(n, E));
    REQUIRE((((uintptr_t)nodes | (uintptr_t)poses | (uintptr_t)confs | (uintptr_t)r | (uintptr_t)S | (uintptr_t)v | (uintptr_t)c | (uintptr_t)g | (uintptr_t)blocks |
              (uintptr_t)rec) & 7) == 0, "pgo: float64 buffers must be 8-byte aligned");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pgo_linearize_kernel, dim3((E + 63) / 64), dim3(64), 0, st, nodes, (const int*)edges, poses, confs, opt, n, E, full ? 1 : 0, r, S, v, c);
    hipLaunchKernelGGL(pgo_cost_kernel, dim3(1), dim3(PGO_THREADS), 0, st, (const double*)c, E, (const int*)idx_status, rec);
    if (full) hipLaunchKernelGGL(pgo_node_kernel, dim3((n + 63) / 64), dim3(64), 0, st, (const int*)off, (const int*)inc, opt, n, (const double*)S,
                                 (const double*)v, g, blocks);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_pgo_solve(sta_handle* h, const int32_t* edges, const uint8_t* opt, const int32_t* off, const int32_t* inc, const double* S, const double* g,
                             const double* blocks, int n, int E, double radius, double dmin, double dmax, double rtol, int max_iter, void* workspace,
                             int64_t workspace_bytes, double* d, double* stats, void* stream) {
    REQUIRE(h && edges && opt && off && inc && S && g && blocks && workspace && d && stats, "null argument");
    CHK(pgo_limits(n, E));
    REQUIRE(radius > 0 && dmin > 0 && dmax >= dmin, "pgo: radius and dmin must be positive and dmax >= dmin (got %g, %g, %g)", radius, dmin, dmax);
    REQUIRE(rtol >= 0 && max_iter >= 1 && max_iter <= (1 << 20), "pgo: rtol must be >= 0 and max_iter lie in [1, 2^20] (got %g, %d)", rtol, max_iter);
    const int64_t need = (int64_t)pgo_solve_ws_doubles(n, E) * 8;
    REQUIRE(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= need, "pgo: the solve workspace holds %lld bytes, %d nodes and %d edges need %lld",
            (long long)workspace_bytes, n, E, (long long)need);
    REQUIRE((((uintptr_t)S | (uintptr_t)g | (uintptr_t)blocks | (uintptr_t)d | (uintptr_t)stats) & 7) == 0, "pgo: float64 buffers must be 8-byte aligned");
    DEV_SCOPE(h->device);
    hipLaunchKernelGGL(pgo_solve_kernel, dim3(1), dim3(PGO_THREADS), 0, (hipStream_t)stream, (const int*)edges, opt, (const int*)off, (const int*)inc, S, g, blocks,
                       n, E, radius, dmin, dmax, rtol, max_iter, (double*)workspace, d, stats);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_pgo_optimize(sta_handle* h, double* nodes, const int32_t* edges, const double* poses, const double* confs, const uint8_t* opt, int n, int E,
                                double radius, double dmin, double dmax, int steps, int patience, double decreasing, int reject, double high, double low,
                                double up, double down, double pcg_rtol, int pcg_max_iter, void* workspace, int64_t workspace_bytes, double* info,
                                int info_rows, int* n_info, int* status_out, void* stream) {
    REQUIRE(h && nodes && edges && poses && confs && opt && workspace && status_out, "null argument");
    CHK(pgo_limits(n, E));
    REQUIRE(steps >= 1 && steps <= 1000 && patience >= 1 && reject >= 1 && reject <= 1000, "pgo: steps and reject must lie in [1, 1000], patience be positive (got %d, %d, %d)",
            steps, reject, patience);
    REQUIRE(up >= 1 && down > 0 && down <= 1 && high >= low, "pgo: up >= 1, 0 < down <= 1 and high >= low (got %g, %g, %g, %g)", up, down, high, low);
    REQUIRE(!info || (info_rows >= 0 && n_info), "pgo: info needs info_rows >= 0 and n_info");
    const PgoWs w = pgo_workspace(workspace, n, E);
    REQUIRE(((uintptr_t)workspace & 255) == 0 && workspace_bytes >= w.bytes, "pgo: the workspace must be 256-byte aligned and holds %lld bytes, %d nodes and %d edges need %lld",
            (long long)workspace_bytes, n, E, (long long)w.bytes);
    hipStream_t st = (hipStream_t)stream;
    const int64_t solve_bytes = (int64_t)pgo_solve_ws_doubles(n, E) * 8;
    int status = 0, stall = 0, rows = 0;
    if (n_info) *n_info = 0;
    *status_out = 0;
    CHK(sta_pgo_index(h, edges, opt, n, E, w.tmp, (int64_t)E * 16, w.off, w.inc, w.idx_status, stream));
    for (int step = 0; step < steps; ++step) {
        // rec = {solve stats [4], f', its status, f, its status}
        CHK(sta_pgo_linearize(h, nodes, edges, poses, confs, opt, w.off, w.inc, w.idx_status, n, E, 1, w.r, w.S, w.v, w.c, w.g, w.blocks, w.rec + 6, stream));
        bool accepted = false, good = false;
        for (int t = 0; t < reject; ++t) {
            CHK(sta_pgo_solve(h, edges, opt, w.off, w.inc, w.S, w.g, w.blocks, n, E, radius, dmin, dmax, pcg_rtol, pcg_max_iter, w.solve, solve_bytes, w.d, w.rec, stream));
            CHK(sta_sim3_op(h, SIM3_RETRACT, w.d, nodes, opt, w.trial, n, stream));
            CHK(sta_pgo_linearize(h, w.trial, edges, poses, confs, opt, nullptr, nullptr, nullptr, n, E, 0, nullptr, nullptr, nullptr, w.c, nullptr, nullptr, w.rec + 4, stream));
            double rec[8];
            {
                DEV_SCOPE(h->device);
                HIPCHK(hipMemcpyAsync(rec, w.rec, 64, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
            }
            const double f = rec[6], fn = rec[4], mdec = rec[2];
            status |= (int)rec[7] & PGO_ST_INDEX;
            if (!std::isfinite(f)) { *status_out = status | PGO_ST_NONFINITE | PGO_ST_UNCHANGED; if (n_info) *n_info = rows; return 0; }
            const double rho = (mdec > 0 && std::isfinite(fn)) ? (f - fn) / mdec : -INFINITY;
            if (info && rows < info_rows) {
                double* o = info + (size_t)rows * 8;
                o[0] = f; o[1] = fn; o[2] = rho; o[3] = radius; o[4] = rec[0]; o[5] = rec[3]; o[6] = rec[1]; o[7] = mdec;
                ++rows;
            }
            if (rho > high) radius *= up; else if (rho < low) radius *= down;
            if (std::isfinite(fn) && fn < f) {
                accepted = true; good = (f - fn) >= decreasing * f;
                DEV_SCOPE(h->device);
                HIPCHK(hipMemcpyAsync(nodes, w.trial, (size_t)n * 64, hipMemcpyDeviceToDevice, st));
                break;
            }
        }
        stall = (accepted && good) ? 0 : stall + 1;
        if (stall >= patience) break;
    }
    if (n_info) *n_info = rows;
    *status_out = status;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// The device-resident pose graph (kernels in graph.h; the contract is in include/sta_mi355.h).  sta_graph_plan holds every size and
// refusal and is host only; the three device calls take the caller's arrays, launch on `stream` and return.
static int graph_state_ok(const sta_graph_state* g) {
    REQUIRE(g && g->poses && g->edges && g->edge_poses && g->edge_confs && g->depth && g->conf && g->intri && g->mean_conf && g->first_node && g->best_node &&
            g->best_conf && g->partials, "graph: null array in the state");
    REQUIRE(g->max_nodes >= 1 && g->max_nodes <= PGO_MAX_NODES && g->max_edges >= 1 && g->max_edges <= PGO_MAX_EDGES && g->max_views >= 1,
            "graph: the state holds %d nodes, %d edges and %d views (at most %d nodes and %d edges)", g->max_nodes, g->max_edges, g->max_views, PGO_MAX_NODES, PGO_MAX_EDGES);
    REQUIRE(g->H >= 16 && g->W >= 16 && g->H % 16 == 0 && g->W % 16 == 0, "graph: H and W must be positive multiples of 16 (got %d x %d)", g->H, g->W);
    REQUIRE(g->chunks == (g->H * g->W + GRAPH_CHUNK - 1) / GRAPH_CHUNK, "graph: %d chunks for %d x %d maps (expected %d)", g->chunks, g->H, g->W,
            (g->H * g->W + GRAPH_CHUNK - 1) / GRAPH_CHUNK);
    REQUIRE((((uintptr_t)g->poses | (uintptr_t)g->edges | (uintptr_t)g->edge_poses | (uintptr_t)g->edge_confs | (uintptr_t)g->depth | (uintptr_t)g->conf |
              (uintptr_t)g->intri | (uintptr_t)g->mean_conf | (uintptr_t)g->first_node | (uintptr_t)g->best_node | (uintptr_t)g->best_conf | (uintptr_t)g->partials) & 15) == 0,
            "graph: every array of the state must be 16-byte aligned");
    return 0;
}

extern "C" int sta_graph_plan(int max_view_num, int neighbor_edge_num, int loop_edge_num, int H, int W, int64_t out[16]) {
    REQUIRE(out, "null argument");
    REQUIRE(max_view_num >= 1 && neighbor_edge_num >= 1 && loop_edge_num >= 0, "graph: max_view_num and neighbor_edge_num must be positive, loop_edge_num >= 0 (got %d, %d, %d)",
            max_view_num, neighbor_edge_num, loop_edge_num);
    REQUIRE(H >= 16 && W >= 16 && H % 16 == 0 && W % 16 == 0 && (int64_t)H * W <= (1 << 24), "graph: H and W must be positive multiples of 16 with H W <= 2^24 (got %d x %d)", H, W);
    const int64_t per = 2 * (int64_t)neighbor_edge_num + loop_edge_num;
    const int64_t n = (int64_t)max_view_num * per, E = (int64_t)max_view_num * ((per - 1) + (per / 2 + 1));          // slam.py:33-36
    REQUIRE(n <= PGO_MAX_NODES && E <= PGO_MAX_EDGES, "graph: %d views with %d neighbour and %d loop edges need %lld nodes and %lld edges, above the optimiser's limits of %d and %d",
            max_view_num, neighbor_edge_num, loop_edge_num, (long long)n, (long long)E, PGO_MAX_NODES, PGO_MAX_EDGES);
    const int64_t hw = (int64_t)H * W, chunks = (hw + GRAPH_CHUNK - 1) / GRAPH_CHUNK;
    out[0] = n; out[1] = E; out[2] = GRAPH_CHUNK; out[3] = chunks;
    out[4] = n * 64; out[5] = E * 16; out[6] = E * 64; out[7] = E * 56;
    out[8] = n * (2 * hw + 9) * 4; out[9] = n * 8; out[10] = ((int64_t)max_view_num + 1) * 16; out[11] = GRAPH_MAX_CALL_NODES * chunks * 32;
    out[12] = out[4] + out[5] + out[6] + out[7] + out[8] + out[9] + out[10] + out[11]; out[13] = (int64_t)max_view_num + 1; out[14] = out[15] = 0;
    return 0;
}

extern "C" int sta_graph_reset(sta_handle* h, const sta_graph_state* g, void* stream) {
    REQUIRE(h, "null argument");
    CHK(graph_state_ok(g));
    DEV_SCOPE(h->device);
    GraphResetArgs a;
    a.poses = g->poses; a.edge_poses = g->edge_poses; a.edge_confs = g->edge_confs; a.mean_conf = g->mean_conf; a.best_conf = g->best_conf;
    a.edges = (long long*)g->edges; a.first_node = g->first_node; a.best_node = g->best_node;
    a.max_nodes = g->max_nodes; a.max_edges = g->max_edges; a.max_views = g->max_views;
    const int most = std::max(g->max_nodes, std::max(g->max_edges, g->max_views));
    hipLaunchKernelGGL(graph_reset_kernel, dim3((most + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_graph_commit(sta_handle* h, const sta_graph_state* g, int num_nodes, int num_edges, int view_i, int first_i, int k,
                                const int32_t* view_j, const int32_t* first_j, const uint8_t* accepted, const double* conf,
                                const float* const* pose, const float* const* depths, const float* const* confs, const float* const* intri,
                                int* num_nodes_out, int* num_edges_out, void* stream) {
    REQUIRE(h && view_j && first_j && accepted && conf && pose && depths && confs && intri && num_nodes_out && num_edges_out, "null argument");
    CHK(graph_state_ok(g));
    REQUIRE(k >= 1 && k <= GRAPH_MAX_CALL_EDGES, "graph: 1 .. %d candidate edges per call (got %d)", GRAPH_MAX_CALL_EDGES, k);
    REQUIRE(num_nodes >= 0 && num_nodes <= g->max_nodes && num_edges >= 0 && num_edges <= g->max_edges, "graph: counts %d / %d outside the store of %d nodes and %d edges",
            num_nodes, num_edges, g->max_nodes, g->max_edges);
    REQUIRE(view_i >= 1 && view_i < g->max_views, "graph: view i must lie in [1, %d) (got %d)", g->max_views, view_i);
    REQUIRE(first_i >= -1 && first_i < num_nodes, "graph: the first node of view %d must lie in [-1, %d) (got %d)", view_i, num_nodes, first_i);
    const int hw = g->H * g->W;
    GraphReduceArgs ra;
    GraphLinkArgs la;
    int nn = num_nodes, ne = num_edges, jobs = 0;
    const float *i_depth = nullptr, *i_conf = nullptr;      // view i's first node, when an earlier edge of this call made it
    for (int e = 0; e < k; ++e) {
        REQUIRE(view_j[e] >= 0 && view_j[e] < view_i, "graph: edge %d connects view %d to view %d: j must lie in [0, i)", e, view_i, view_j[e]);
        for (int f = 0; f < e; ++f) REQUIRE(view_j[f] != view_j[e], "graph: view %d is a candidate of view %d twice (edges %d and %d)", view_j[e], view_i, f, e);
        REQUIRE(first_j[e] >= -1 && first_j[e] < num_nodes, "graph: the first node of view %d must lie in [-1, %d) (got %d)", view_j[e], num_nodes, first_j[e]);
        if (!accepted[e]) continue;
        REQUIRE(pose[e] && depths[e] && confs[e] && intri[e], "graph: accepted edge %d lacks its pose, maps or intrinsics", e);
        REQUIRE((((uintptr_t)depths[e] | (uintptr_t)confs[e]) & 15) == 0 && (((uintptr_t)pose[e] | (uintptr_t)intri[e]) & 3) == 0, "graph: the maps of edge %d must be 16-byte aligned", e);
        const int scale_edges = (first_i >= 0 ? 1 : 0) + (first_j[e] >= 0 ? 1 : 0);
        REQUIRE(nn + 2 <= g->max_nodes, "graph: the pool of %d nodes is full (edge %d of view %d)", g->max_nodes, e, view_i);
        REQUIRE(ne + scale_edges + 1 <= g->max_edges, "graph: the store of %d edges is full (edge %d of view %d)", g->max_edges, e, view_i);
        const int n_i = nn, n_j = nn + 1;
        GraphNodeJob& ji = ra.job[2 * jobs];
        GraphNodeJob& jj = ra.job[2 * jobs + 1];
        ji.depth = depths[e]; ji.conf = confs[e]; ji.intri = intri[e]; ji.node = n_i; ji.pad = 0;
        jj.depth = depths[e] + hw; jj.conf = confs[e] + hw; jj.intri = intri[e]; jj.node = n_j; jj.pad = 0;
        ji.ref_depth = ji.ref_conf = jj.ref_depth = jj.ref_conf = nullptr;
        if (first_i >= 0) {
            ji.ref_depth = i_depth ? i_depth : g->depth + (size_t)first_i * hw;
            ji.ref_conf = i_conf ? i_conf : g->conf + (size_t)first_i * hw;
        }
        if (first_j[e] >= 0) { jj.ref_depth = g->depth + (size_t)first_j[e] * hw; jj.ref_conf = g->conf + (size_t)first_j[e] * hw; }
        GraphEdgeJob& je = la.job[jobs];
        je.pose = pose[e]; je.conf = conf[e]; je.n_i = n_i; je.n_j = n_j; je.first_i = first_i; je.first_j = first_j[e]; je.view_i = view_i; je.view_j = view_j[e];
        if (first_i < 0) { first_i = n_i; i_depth = depths[e]; i_conf = confs[e]; }
        nn += 2; ne += scale_edges + 1; ++jobs;
    }
    *num_nodes_out = nn; *num_edges_out = ne;
    if (jobs == 0) return 0;
    DEV_SCOPE(h->device);
    ra.pool_depth = g->depth; ra.pool_conf = g->conf; ra.pool_intri = g->intri; ra.partials = g->partials; ra.hw = hw; ra.chunks = g->chunks;
    la.partials = g->partials; la.poses = g->poses; la.edge_poses = g->edge_poses; la.edge_confs = g->edge_confs; la.mean_conf = g->mean_conf; la.best_conf = g->best_conf;
    la.edges = (long long*)g->edges; la.first_node = g->first_node; la.best_node = g->best_node; la.n_jobs = jobs; la.num_edges = num_edges; la.hw = hw; la.chunks = g->chunks;
    hipLaunchKernelGGL(graph_reduce_kernel, dim3(g->chunks, 2 * jobs), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, ra);
    hipLaunchKernelGGL(graph_link_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, la);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_graph_export(sta_handle* h, const sta_graph_state* g, int n_views, int scaled, int filter, float thres, float* poses,
                                float* scales, float* depths, float* confs, float* intrinsics, void* stream) {
    REQUIRE(h && poses && scales && depths && confs && intrinsics, "null argument");
    CHK(graph_state_ok(g));
    REQUIRE(n_views >= 1 && n_views <= g->max_views, "graph: export of %d views from a graph of at most %d", n_views, g->max_views);
    REQUIRE((((uintptr_t)depths | (uintptr_t)confs) & 15) == 0, "graph: the exported maps must be 16-byte aligned");
    DEV_SCOPE(h->device);
    GraphExportArgs a;
    a.node_poses = g->poses; a.pool_depth = g->depth; a.pool_conf = g->conf; a.pool_intri = g->intri; a.best_node = g->best_node;
    a.poses = poses; a.scales = scales; a.depths = depths; a.confs = confs; a.intrinsics = intrinsics;
    a.hw = g->H * g->W; a.max_nodes = g->max_nodes; a.scaled = scaled ? 1 : 0; a.filter = filter ? 1 : 0; a.thres = thres;
    hipLaunchKernelGGL(graph_export_kernel, dim3(g->chunks, n_views), dim3(GRAPH_THREADS), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// f4, continued: pp.mat2SE3
extern "C" int sta_mat_to_se3(sta_handle* h, const float* poses, int B, float* se3_out, void* stream) {
    REQUIRE(h && poses && se3_out && B > 0, "bad argument");
    DEV_SCOPE(h->device);
    hipLaunchKernelGGL(mat_to_se3_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, poses, B, se3_out);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_estimate_intrinsics(sta_handle* h, const float* pts, const float* conf, int B, int H, int W, int shared,
                                       float* K_out, float* depth_out, float* conf_mean_out, void* stream) {
    REQUIRE(h && pts && conf && K_out && B > 0 && H > 0 && W > 0, "bad argument");
    REQUIRE(shared >= 0 && (shared < 2 || B % shared == 0), "shared group size %d does not divide B=%d", shared, B);
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)H * W;
    int nblk = (int)((hw + 256 * 8 - 1) / (256 * 8)); if (nblk > 256) nblk = 256; if (nblk < 1) nblk = 1;
    return plan_and_run(h, st, [&](Bump& ws) -> int {
        double* partial = (double*)ws.take((int64_t)B * nblk * 5 * 8);
        if (h->dry) return 0;
        REQUIRE(!ws.overflow, "internal: workspace overflow");
        hipLaunchKernelGGL(intrinsics_partial_kernel, dim3(nblk, B), dim3(256), 0, st, pts, conf, B, H, W, depth_out, partial, nblk, 0);
        hipLaunchKernelGGL(intrinsics_final_kernel, dim3(1), dim3(64), 0, st, partial, B, nblk, H, W, shared, K_out, conf_mean_out, 0);
        HIPCHK(hipGetLastError());
        return 0;
    });
}

// ---------------------------------------------------------------------------------------------------------
// f2: keyframe scheduler.  OnlineSLAM.step (slam.py:263-277) calls regress_two_views (slam.py:153-189) once per
// candidate edge (i, j): B=1 decode -> pose head (ij only) -> early return when the pose confidence is below
// rel_pose_thres and the views are not adjacent -> DPT on both views -> shared intrinsics + depths.
// Here all k candidate edges of keyframe i are decoded in ONE batched launch sequence, the pose head runs first,
// one k-float D2H read decides acceptance, and the DPT + post-STA reductions run batched over the accepted edges
// only (so the DPT-skip saving of the reference is kept).
static int launch_gather(const GatherChunks& g, int n, int64_t max16, hipStream_t st) {
    int gx = (int)((max16 + 256 * 4 - 1) / (256 * 4)); if (gx < 1) gx = 1; if (gx > 256) gx = 256;
    hipLaunchKernelGGL(gather_chunks_kernel, dim3(gx, n), dim3(256), 0, st, g);
    HIPCHK(hipGetLastError());
    return 0;
}

// Workspace layout of one scheduler call: the same sequence of takes in the planning pass, in phase A (begin) and in phase B
// (finish) - the tensors phase A leaves for phase B live at these offsets of the stream's workspace.
struct RvLayout { float *F, *x, *hk[3], *cdev, *cf, *ch[3]; int64_t mark; };
static RvLayout rv_layout(Bump& ws, int S, int k, int64_t fe, int64_t xe) {
    RvLayout L;
    L.F = (float*)ws.take(S * fe * 4);              // [2k,N,E]: k copies of view i, then the k views j
    L.x = (float*)ws.take(S * xe * 4);
    for (int q = 0; q < 3; ++q) L.hk[q] = (float*)ws.take(S * xe * 4);
    L.cdev = (float*)ws.take(k * 4);
    L.cf = (float*)ws.take(S * fe * 4);             // compacted DPT inputs of the accepted edges
    for (int q = 0; q < 3; ++q) L.ch[q] = (float*)ws.take(S * xe * 4);
    L.mark = ws.off;
    return L;
}
struct RvDims { int hp, wp, N, Np, E, D, S, dd, hidx[3]; int64_t fe, xe, pe; };
static RvDims rv_dims(const sta_handle* h, int k, int H, int W) {
    const sta_config& c = h->cfg;
    RvDims d;
    d.hp = H / 16; d.wp = W / 16; d.N = d.hp * d.wp; d.Np = d.N + 1; d.E = c.enc_embed_dim; d.D = c.dec_embed_dim; d.S = 2 * k;
    d.dd = c.dec_depth;
    d.hidx[0] = d.dd * 2 / 4; d.hidx[1] = d.dd * 3 / 4; d.hidx[2] = d.dd;
    d.fe = (int64_t)d.N * d.E; d.xe = (int64_t)d.Np * d.D; d.pe = (int64_t)d.N * d.D;   // floats per sequence: features, hook incl. pose token, hook patch rows
    return d;
}
// phase A: gather -> batched decode -> pose head on the ij side -> confidences on their way to the host (async, pinned)
static int rv_phase_a(sta_handle* h, Bump& ws, const RvDims& d, const float* feat_i, const float* const* feat_j, int k,
                      float* pose, hipStream_t st) {
    RvLayout L = rv_layout(ws, d.S, k, d.fe, d.xe);
    if (!h->dry) {
        GatherChunks g;
        for (int e = 0; e < k; ++e) {
            g.src[e] = (const uint4*)feat_i; g.dst[e] = (uint4*)(L.F + e * d.fe); g.n16[e] = d.fe / 4;
            g.src[k + e] = (const uint4*)feat_j[e]; g.dst[k + e] = (uint4*)(L.F + (k + e) * d.fe); g.n16[k + e] = d.fe / 4;
        }
        CHK(launch_gather(g, 2 * k, d.fe / 4, st));
    }
    // hooks in the decoder's own row order (decode_impl): [2k*N patch rows, sequence (side*k + e) at row (side*k + e)*N | 2k pose rows]
    std::vector<float*> w1(d.dd + 1, nullptr);
    for (int q = 0; q < 3; ++q) w1[d.hidx[q]] = L.hk[q];
    CHK(decode_impl(h, ws, L.F, L.F + (size_t)k * d.fe, k, d.hp, d.wp, L.x, w1.data(), nullptr, false, st));
    ws.rewind(L.mark);
    CHK(pose_impl(h, ws, L.hk[2] + (size_t)d.S * d.pe, k, (int64_t)d.D, pose, L.cdev, st));       // pose_ij only (slam.py:165): pose rows of side 0
    if (!h->dry) {
        StreamCtx& c = *h->cur;
        HIPCHK(hipMemcpyAsync(c.rv_conf, L.cdev, (size_t)k * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(c.rv_ev, st));
    }
    return 0;
}
// phase B: acceptance on the host (slam.py:169) -> DPT heads + shared intrinsics + depths of the accepted edges.
// `decide` = false in the planning pass (all k edges accepted: the largest workspace).
static int rv_phase_b(sta_handle* h, Bump& ws, const RvDims& d, int k, const uint8_t* adjacent, float rel_pose_thres, int H, int W,
                      float* pose_conf_host, int* slot_host, int* n_accepted, float* pts, float* conf, float* K, float* depth,
                      hipStream_t st) {
    RvLayout L = rv_layout(ws, d.S, k, d.fe, d.xe);
    int na = k;
    if (!h->dry) {
        StreamCtx& c = *h->cur;
        HIPCHK(hipEventSynchronize(c.rv_ev));                  // the reference syncs here too (slam.py:169)
        int slots[16];
        na = 0;
        for (int e = 0; e < k; ++e) {
            pose_conf_host[e] = c.rv_conf[e];
            const bool rej = pose_conf_host[e] < rel_pose_thres && !adjacent[e];   // slam.py:169
            slots[e] = rej ? -1 : na++;
            slot_host[e] = slots[e];
        }
        *n_accepted = na;
        if (na == 0) return 0;
        // accepted edges -> the DPT head's image order, per edge [ij, ji] (slam.py:182): encoder features + the three decoder hooks
        // (patch rows only).  One launch while the 8 chunks per accepted edge fit one chunk table, else one per tensor.
        REQUIRE(d.pe % 4 == 0, "internal: hook slice not 16-byte sized");
        GatherChunks g;
        int m = 0;
        const bool one = 8 * na <= 64;
        for (int q = -1; q < 3; ++q) {
            const float* src = q < 0 ? L.F : L.hk[q];
            float* dst = q < 0 ? L.cf : L.ch[q];
            const int64_t el = q < 0 ? d.fe : d.pe;
            for (int e = 0; e < k; ++e) {
                if (slots[e] < 0) continue;
                const int s0 = 2 * slots[e];
                for (int side = 0; side < 2; ++side) {
                    g.src[m] = (const uint4*)(src + (size_t)(side * k + e) * el); g.dst[m] = (uint4*)(dst + (size_t)(s0 + side) * el); g.n16[m] = el / 4; ++m;
                }
            }
            if (!one) { CHK(launch_gather(g, m, el / 4, st)); m = 0; }
        }
        if (one) CHK(launch_gather(g, m, (d.fe > d.pe ? d.fe : d.pe) / 4, st));
    }
    const int n = 2 * na;
    CHK(dpt_impl(h, ws, L.cf, d.fe, L.ch[0], d.pe, L.ch[1], d.pe, L.ch[2], d.pe, n, H, W, pts, conf, n, nullptr, nullptr, st));
    ws.rewind(L.mark);
    const int64_t hw = (int64_t)H * W;
    int nblk = (int)((hw + 256 * 8 - 1) / (256 * 8)); if (nblk > 256) nblk = 256; if (nblk < 1) nblk = 1;
    double* partial = (double*)ws.take((int64_t)n * nblk * 5 * 8);
    if (h->dry) return 0;
    REQUIRE(!ws.overflow, "internal: workspace overflow");
    hipLaunchKernelGGL(intrinsics_partial_kernel, dim3(nblk, n), dim3(256), 0, st, pts, conf, n, H, W, depth, partial, nblk, H > W);
    hipLaunchKernelGGL(intrinsics_final_kernel, dim3(1), dim3(64), 0, st, partial, n, nblk, H, W, 2, K, (float*)nullptr, H > W);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int sta_regress_views_begin(sta_handle* h, const float* feat_i, const float* const* feat_j, int k, int H, int W,
                                       float* pose, void* stream) {
    REQUIRE(h, "null handle");
    DEV_SCOPE(h->device);
    CHK(check_ready(h, k, H, W));
    REQUIRE(k <= 16, "at most 16 candidate edges per keyframe (got %d)", k);
    REQUIRE(feat_i && feat_j && pose, "null argument");
    for (int e = 0; e < k; ++e) REQUIRE(feat_j[e] && ((uintptr_t)feat_j[e] & 15) == 0, "feat_j[%d] null or not 16-byte aligned", e);
    REQUIRE(((uintptr_t)feat_i & 15) == 0, "feat_i not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const RvDims d = rv_dims(h, k, H, W);
    CHK(ensure_rope(h, d.hp > d.wp ? d.hp : d.wp));
    CHK(stream_ctx(h, st));
    REQUIRE(!h->cur->rv_open, "sta_regress_views_begin: the previous scheduler call on this stream has not been finished");
    if (!h->cur->rv_conf) {
        HIPCHK(hipHostMalloc((void**)&h->cur->rv_conf, 16 * sizeof(float), hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&h->cur->rv_ev, hipEventDisableTiming));
        h->n_alloc += 2;
    }
    // one plan for both phases (phase B sized for k accepted edges), then phase A runs
    int r = plan_and_run(h, st, [&](Bump& ws) -> int {
        if (h->dry) {
            CHK(rv_phase_a(h, ws, d, feat_i, feat_j, k, pose, st));
            ws.rewind(0);
            return rv_phase_b(h, ws, d, k, nullptr, 0.f, H, W, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st);
        }
        return rv_phase_a(h, ws, d, feat_i, feat_j, k, pose, st);
    });
    if (r != 0) return r;
    if (h->reserve_only) return 0;                      // sta_reserve: both phases are planned and allocated, nothing is pending
    StreamCtx& c = *h->cur;
    c.rv_open = true; c.rv_kind = 0; c.rv_k = k; c.rv_H = H; c.rv_W = W;
    return 0;
}

extern "C" int sta_regress_views_finish(sta_handle* h, const uint8_t* adjacent, float rel_pose_thres,
                                        float* pose_conf_host, int* slot_host, int* n_accepted,
                                        float* pts, float* conf, float* K, float* depth, void* stream) {
    REQUIRE(h, "null handle");
    DEV_SCOPE(h->device);
    REQUIRE(adjacent && pose_conf_host && slot_host && n_accepted && pts && conf && K && depth, "null argument");
    hipStream_t st = (hipStream_t)stream;
    CHK(stream_ctx(h, st));
    StreamCtx& c = *h->cur;
    REQUIRE(c.rv_open, "sta_regress_views_finish: no scheduler call was begun on this stream");
    REQUIRE(c.rv_kind == 0, "sta_regress_views_finish: the call pending on this stream was begun with sta_regress_views_tokens_begin: finish it with sta_regress_views_tokens_finish (or abort it)");
    c.rv_open = false;                                  // (also on an error below: the call is over either way)
    const int k = c.rv_k, H = c.rv_H, W = c.rv_W;
    const RvDims d = rv_dims(h, k, H, W);
    *n_accepted = 0;
    h->dry = false;
    Bump ws = cur_bump(h);                              // the workspace phase A planned and filled
    return rv_phase_b(h, ws, d, k, adjacent, rel_pose_thres, H, W, pose_conf_host, slot_host, n_accepted, pts, conf, K, depth, st);
}

// Drop a scheduler call that was begun on `stream` and will never be finished (an exception between the two phases, a dropped
// handle on the host side).  Waits for phase A's copy event so that nothing of it is still in flight into the pinned buffer,
// then clears the pending state: the stream's scratch context is usable (and recyclable) again.  A stream with nothing
// pending is not an error (returns 0): the host-side wrapper calls this from its destructor.
extern "C" int sta_regress_views_abort(sta_handle* h, void* stream) {
    REQUIRE(h, "null handle");
    DEV_SCOPE(h->device);
    hipStream_t st = (hipStream_t)stream;
    for (auto& c : h->ctx) {
        if (c.st != st || !c.rv_open) continue;
        if (c.rv_ev) HIPCHK(hipEventSynchronize(c.rv_ev));
        c.rv_open = false; c.rv_k = 0;
    }
    return 0;
}

extern "C" int sta_regress_views(sta_handle* h, const float* feat_i, const float* const* feat_j, int k,
                                 const uint8_t* adjacent, float rel_pose_thres, int H, int W,
                                 float* pose, float* pose_conf_host, int* slot_host, int* n_accepted,
                                 float* pts, float* conf, float* K, float* depth, void* stream) {
    REQUIRE(adjacent && pose_conf_host && slot_host && n_accepted && pts && conf && K && depth, "null argument");
    CHK(sta_regress_views_begin(h, feat_i, feat_j, k, H, W, pose, stream));
    return sta_regress_views_finish(h, adjacent, rel_pose_thres, pose_conf_host, slot_host, n_accepted, pts, conf, K, depth, stream);
}

// ---------------------------------------------------------------------------------------------------------
// f2 on TOKEN SUBSETS (sta_regress_views_tokens): the scheduler contract above with a SELECTION per edge and side - the whole frame, a
// window of its patch grid, or an index list -, every candidate with its own frame size.  Selecting = slicing the cached whole-frame
// encoding (gather_tokens_varlen_kernel: both packed sides and the positions table in one launch), then ONE varlen decode
// (decode_varlen_impl: sequence e = side i of edge e, k + e = side j), the pose head on the k pose rows of side i through a row table
// (pose_layer_rows_kernel), the k confidences to the host, and for the accepted edges the DPT head per window side at that side's
// token shape: one call with n = 2 where both sides of an edge share a shape (then also the pair-shared intrinsics, slam.py:182-185),
// else one per window side.  The head reads its inputs where the decode left them - a window's rows are contiguous in the packed
// features and in the emitted hooks (pose row first, skipped) -, the two images of an n = 2 call lie one pointer difference apart.
//
// Builds the per-sequence table from the HOST arrays of an entry and checks them.  srcs / hp / wp: [S]; win: [S][4] (y0, x0, h, w),
// h * w == 0 = index list of cnt[s] tokens taken from idx_side[s < S / 2 ? 0 : 1], whose slices follow each other in sequence order.
static int build_token_sel(const float* const* srcs, const int* hp, const int* wp, const int* win, const int* cnt,
                           const int64_t* const idx_side[2], int S, TokenSel* out, int* mh, int* mw) {
    TokenSel& g = *out; memset(&g, 0, sizeof g);
    g.t.S = S;
    int64_t acc = 0, ioff[2] = {0, 0};
    for (int s = 0; s < S; ++s) {
        const int side = s < S / 2 ? 0 : 1, e = s % (S / 2);
        const int y0 = win[4 * s], x0 = win[4 * s + 1], wh = win[4 * s + 2], ww = win[4 * s + 3];
        REQUIRE(srcs[s] && ((uintptr_t)srcs[s] & 15) == 0, "features of edge %d side %d null or not 16-byte aligned", e, side);
        REQUIRE(hp[s] >= 1 && wp[s] >= 1, "bad frame grid %d x %d (edge %d side %d)", hp[s], wp[s], e, side);
        int n;
        if ((int64_t)wh * ww != 0) {
            REQUIRE(wh >= 1 && ww >= 1 && y0 >= 0 && x0 >= 0 && (int64_t)y0 + wh <= hp[s] && (int64_t)x0 + ww <= wp[s],
                    "window (%d, %d, %d, %d) leaves the %d x %d grid (edge %d side %d)", y0, x0, wh, ww, hp[s], wp[s], e, side);
            n = wh * ww; mh[s] = wh; mw[s] = ww;
            g.y0[s] = y0; g.x0[s] = x0; g.ww[s] = ww;
        } else {
            REQUIRE(cnt && cnt[s] >= 1, "bad argument (edge %d side %d: an index list has at least one token)", e, side);
            REQUIRE(idx_side[side], "null index array (edge %d side %d selects by index)", e, side);
            n = cnt[s]; mh[s] = 0; mw[s] = 0;
            g.idx[s] = idx_side[side] + ioff[side]; ioff[side] += n;
        }
        g.src[s] = srcs[s]; g.hp[s] = hp[s]; g.wp[s] = wp[s];
        g.t.tok0[s] = (int)acc; acc += n;
        REQUIRE(acc + S < ((int64_t)1 << 31), "too many decoder rows (%lld or more)", (long long)(acc + S));
    }
    g.t.tok0[S] = (int)acc;
    return 0;
}
static int launch_gather_tokens(const TokenSel& g, int E, float* feat, int* pos, hipStream_t st) {
    int gx = g.t.tok0[g.t.S]; if (gx > 65536) gx = 65536;
    hipLaunchKernelGGL(gather_tokens_varlen_kernel, dim3(gx), dim3(256), 0, st, g, E, feat, pos);
    HIPCHK(hipGetLastError());
    return 0;
}

struct RvtLayout { float *F, *x, *hk[3][2], *cdev; int* rp; float2* ident; int64_t n_ident, mark; };
static RvtLayout rvt_layout(Bump& ws, const SeqTable& t, int k, int E, int D) {
    RvtLayout L;
    const int64_t Mp = t.tok0[2 * k], Mp1 = t.tok0[k];
    int nmax = 0;
    for (int s = 0; s < 2 * k; ++s) nmax = std::max(nmax, t.tok0[s + 1] - t.tok0[s]);
    L.F = (float*)ws.take(Mp * E * 4);                  // packed features: side i's k selections, then side j's
    L.rp = (int*)ws.take(Mp * 2 * 4);
    L.n_ident = (int64_t)(nmax + 2) * 16;               // each sequence is the grid 1 x n: table rows 0 .. max(n) + 1 (sta_decode_varlen)
    L.ident = (float2*)ws.take(L.n_ident * 8);
    L.x = (float*)ws.take((Mp + 2 * k) * D * 4);
    for (int q = 0; q < 3; ++q) {                       // emitted hooks per side, entry by entry, pose row first (decode_varlen_impl)
        L.hk[q][0] = (float*)ws.take((Mp + 2 * k) * D * 4);      // both sides in ONE block of dense rows: the varlen head reads side j through
        L.hk[q][1] = L.hk[q][0] + (size_t)(Mp1 + k) * D;         // row offsets from side i's base (sta_set_varlen_heads)
    }
    L.cdev = (float*)ws.take(k * 4);
    L.mark = ws.off;
    return L;
}
// phase A: gather -> varlen decode -> pose head on the pose rows of side i -> confidences on their way to the host
static int rvt_phase_a(sta_handle* h, Bump& ws, const TokenSel& g, int k, float* pose, hipStream_t st) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim, dd = c.dec_depth;
    const int hidx[3] = {dd * 2 / 4, dd * 3 / 4, dd};
    RvtLayout L = rvt_layout(ws, g.t, k, E, D);
    if (!h->dry) {
        REQUIRE(!ws.overflow, "internal: scheduler workspace overflow");
        CHK(launch_gather_tokens(g, E, L.F, L.rp, st));
        hipLaunchKernelGGL(rope_tokens_table_kernel<int64_t>, dim3((unsigned)((L.n_ident + 255) / 256)), dim3(256), 0, st,
                           (const int64_t*)nullptr, (const int64_t*)nullptr, (int64_t)0, (int64_t)0, 0, L.rp, L.ident, L.n_ident);    // the identity table alone
        HIPCHK(hipGetLastError());
        h->rope_pos = L.rp; h->rope_ident = (const float*)L.ident;
    }
    std::vector<float*> w1(dd + 1, nullptr), w2(dd + 1, nullptr);
    for (int q = 0; q < 3; ++q) { w1[hidx[q]] = L.hk[q][0]; w2[hidx[q]] = L.hk[q][1]; }
    CHK(decode_varlen_impl(h, ws, L.F, L.F + (size_t)g.t.tok0[k] * E, g.t, k, L.x, w1.data(), w2.data(), st));
    ws.rewind(L.mark);
    PoseRows rows;
    for (int e = 0; e < 16; ++e) rows.row[e] = e < k ? (int64_t)g.t.tok0[e] + e : 0;      // pose_ij only (slam.py:165)
    CHK(pose_impl(h, ws, L.hk[2][0], k, (int64_t)D, pose, L.cdev, st, nullptr, nullptr, 0, &rows));
    if (!h->dry) {
        StreamCtx& cx = *h->cur;
        HIPCHK(hipMemcpyAsync(cx.rv_conf, L.cdev, (size_t)k * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(cx.rv_ev, st));
    }
    return 0;
}
// phase B: acceptance on the host -> per accepted edge the DPT head of its window sides, depths, and K where both sides share a shape.
// Map buffers: (edge, side) order over the WINDOW sides of all k edges, offsets from the host-known shapes; what belongs to a rejected
// edge or to no side at all is not written.  Planning pass (dry): every edge accepted.
static int rvt_phase_b(sta_handle* h, Bump& ws, const SeqTable& t, const StreamCtx::RvtState& rs, int k, const uint8_t* adjacent, float rel_pose_thres,
                       float* pose_conf_host, int* accepted_host, int* n_accepted, float* pts, float* conf, float* depth, float* K,
                       int* k_valid_host, hipStream_t st) {
    const sta_config& c = h->cfg;
    const int E = c.enc_embed_dim, D = c.dec_embed_dim;
    RvtLayout L = rvt_layout(ws, t, k, E, D);
    bool acc[16];
    for (int e = 0; e < k; ++e) acc[e] = true;
    if (!h->dry) {
        StreamCtx& cx = *h->cur;
        HIPCHK(hipEventSynchronize(cx.rv_ev));                 // the reference syncs here too (slam.py:169)
        int na = 0;
        for (int e = 0; e < k; ++e) {
            pose_conf_host[e] = cx.rv_conf[e];
            acc[e] = !(pose_conf_host[e] < rel_pose_thres && !adjacent[e]);        // slam.py:169
            accepted_host[e] = acc[e] ? 1 : 0; k_valid_host[e] = 0;
            na += acc[e] ? 1 : 0;
        }
        *n_accepted = na;
    }
    const int Mp1 = t.tok0[k];
    int64_t pix = 0;                                           // pixels of the window sides before this one
    // The switch is read HERE, at finish time.  The workspace was planned at begin time: for the varlen pass only when the switch was on
    // THEN (rs.plan_v) - a caller who never sets it plans, and allocates, what the per-edge route needs and no more.  Switching it on
    // between begin and finish is refused; switching it off is served (the per-edge route is planned always).
    const bool vheads = h->dry ? rs.plan_v != 0 : h->varlen_heads;
    REQUIRE(h->dry || !vheads || rs.plan_v, "sta_set_varlen_heads(h, 1) came after sta_regress_views_tokens_begin: the call's workspace was planned there, for the per-edge heads; set the switch before begin");
    if (vheads) {      // ONE varlen head pass over the window sides of all accepted edges, written straight into the layout below
        int64_t erow[SEQ_MAX], hrow[SEQ_MAX], opix[SEQ_MAX]; int hp[SEQ_MAX], wp[SEQ_MAX], nb = 0;
        int64_t px = 0;
        for (int e = 0; e < k; ++e)
            for (int side = 0; side < 2; ++side) {
                const int s = side ? k + e : e;
                if (rs.mh[s] == 0) continue;
                if (acc[e]) {
                    erow[nb] = t.tok0[s];                                              // L.F: both sides packed, no pose rows
                    hrow[nb] = (int64_t)t.tok0[s] + (side ? k : 0) + e + 1;              // hooks: a pose row in front of every entry, side j behind side i
                    hp[nb] = rs.mh[s]; wp[nb] = rs.mw[s]; opix[nb] = px; ++nb;
                }
                px += (int64_t)256 * rs.mh[s] * rs.mw[s];
            }
        if (nb > 0 && (h->dry || (pts && conf))) {
            ws.rewind(L.mark);
            CHK(dpt_varlen_impl(h, ws, L.F, erow, L.hk[0][0], L.hk[1][0], L.hk[2][0], hrow, hp, wp, nb, pts, conf, opix, st));
        }
    }
    for (int e = 0; e < k; ++e) {
        const int si = e, sj = k + e;
        const bool pair = rs.mh[si] > 0 && rs.mh[si] == rs.mh[sj] && rs.mw[si] == rs.mw[sj];
        const float* enc[2] = {L.F + (size_t)t.tok0[si] * E, L.F + (size_t)t.tok0[sj] * E};
        const float* hk[3][2];
        for (int q = 0; q < 3; ++q) {                          // the side's patch rows of hook q: behind the entry's pose row
            hk[q][0] = L.hk[q][0] + (size_t)(t.tok0[si] + e + 1) * D;
            hk[q][1] = L.hk[q][1] + (size_t)(t.tok0[sj] - Mp1 + e + 1) * D;
        }
        for (int side = 0; side < 2; ++side) {
            const int s = side ? sj : si;
            if (rs.mh[s] == 0) continue;
            const int H = 16 * rs.mh[s], W = 16 * rs.mw[s], n = pair ? 2 : 1;
            const int64_t hw = (int64_t)H * W;
            if (acc[e]) {
                ws.rewind(L.mark);
                if (!vheads || h->dry) CHK(dpt_impl(h, ws, enc[side], enc[1] - enc[0], hk[0][side], hk[0][1] - hk[0][0], hk[1][side], hk[1][1] - hk[1][0],
                             hk[2][side], hk[2][1] - hk[2][0], n, H, W, pts ? pts + pix * 3 : nullptr, conf ? conf + pix : nullptr, n, nullptr, nullptr, st));
                ws.rewind(L.mark);
                int nblk = (int)((hw + 256 * 8 - 1) / (256 * 8)); if (nblk > 256) nblk = 256; if (nblk < 1) nblk = 1;
                double* partial = (double*)ws.take((int64_t)n * nblk * 5 * 8);
                if (!h->dry) {
                    REQUIRE(!ws.overflow, "internal: workspace overflow");
                    hipLaunchKernelGGL(intrinsics_partial_kernel, dim3(nblk, n), dim3(256), 0, st, pts + pix * 3, conf + pix, n, H, W, depth + pix, partial, nblk, H > W);
                    if (pair) {
                        hipLaunchKernelGGL(intrinsics_final_kernel, dim3(1), dim3(64), 0, st, partial, 2, nblk, H, W, 2, K + (size_t)e * 9, (float*)nullptr, H > W);
                        k_valid_host[e] = 1;
                    }
                    HIPCHK(hipGetLastError());
                }
            }
            pix += n * hw;
            if (pair) break;                                   // both sides went in one call
        }
    }
    return 0;
}

// Host arrays of the entry -> per-sequence arrays (s = e side i, k + e side j) for build_token_sel
static int rvt_table(sta_handle* h, const float* feat_i, int Hi, int Wi, const float* const* feat_j, const int* Hj, const int* Wj, int k,
                     const int* win_i, const int* cnt_i, const int64_t* idx_i, const int* win_j, const int* cnt_j, const int64_t* idx_j,
                     TokenSel* g, StreamCtx::RvtState* rs, int* pmax) {
    REQUIRE(k >= 1 && k <= 16, "1 .. 16 candidate edges per keyframe (got %d)", k);
    REQUIRE(feat_i && feat_j && Hj && Wj && win_i && win_j, "null argument");
    const float* srcs[SEQ_MAX]; int hp[SEQ_MAX], wp[SEQ_MAX], win[SEQ_MAX * 4], cnt[SEQ_MAX];
    CHK(check_ready(h, k, Hi, Wi));
    *pmax = std::max(Hi, Wi) / 16;
    for (int e = 0; e < k; ++e) {
        CHK(check_ready(h, k, Hj[e], Wj[e]));
        *pmax = std::max(*pmax, std::max(Hj[e], Wj[e]) / 16);
        srcs[e] = feat_i; hp[e] = Hi / 16; wp[e] = Wi / 16;
        srcs[k + e] = feat_j[e]; hp[k + e] = Hj[e] / 16; wp[k + e] = Wj[e] / 16;
        for (int q = 0; q < 4; ++q) { win[4 * e + q] = win_i[4 * e + q]; win[4 * (k + e) + q] = win_j[4 * e + q]; }
        cnt[e] = cnt_i ? cnt_i[e] : 0; cnt[k + e] = cnt_j ? cnt_j[e] : 0;
    }
    const int64_t* const idx_side[2] = {idx_i, idx_j};
    memset(rs, 0, sizeof *rs);
    CHK(build_token_sel(srcs, hp, wp, win, cnt, idx_side, 2 * k, g, rs->mh, rs->mw));
    for (int s = 0; s < 2 * k; ++s) rs->n[s] = g->t.tok0[s + 1] - g->t.tok0[s];
    return 0;
}

extern "C" int sta_regress_views_tokens_begin(sta_handle* h, const float* feat_i, int Hi, int Wi,
                                              const float* const* feat_j, const int* Hj, const int* Wj, int k,
                                              const int* win_i, const int* cnt_i, const int64_t* idx_i,
                                              const int* win_j, const int* cnt_j, const int64_t* idx_j,
                                              float* pose, void* stream) {
    REQUIRE(h, "null handle");
    DEV_SCOPE(h->device);
    TokenSel g; StreamCtx::RvtState rs; int pmax = 0;
    CHK(rvt_table(h, feat_i, Hi, Wi, feat_j, Hj, Wj, k, win_i, cnt_i, idx_i, win_j, cnt_j, idx_j, &g, &rs, &pmax));
    rs.plan_v = h->varlen_heads ? 1 : 0;
    REQUIRE(pose, "null argument");
    hipStream_t st = (hipStream_t)stream;
    CHK(ensure_rope(h, pmax));
    CHK(stream_ctx(h, st));
    REQUIRE(!h->cur->rv_open, "sta_regress_views_tokens_begin: the previous scheduler call on this stream has not been finished");
    if (!h->cur->rv_conf) {
        HIPCHK(hipHostMalloc((void**)&h->cur->rv_conf, 16 * sizeof(float), hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&h->cur->rv_ev, hipEventDisableTiming));
        h->n_alloc += 2;
    }
    RopeForeign scope(h);
    // one plan for both phases (phase B sized for k accepted edges), then phase A runs
    int r = plan_and_run(h, st, [&](Bump& ws) -> int {
        if (h->dry) {
            CHK(rvt_phase_a(h, ws, g, k, pose, st));
            ws.rewind(0);
            return rvt_phase_b(h, ws, g.t, rs, k, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st);
        }
        return rvt_phase_a(h, ws, g, k, pose, st);
    });
    if (r != 0) return r;
    if (h->reserve_only) return 0;
    StreamCtx& c = *h->cur;
    c.rv_open = true; c.rv_kind = 1; c.rv_k = k; c.rvt = rs;
    return 0;
}

extern "C" int sta_regress_views_tokens_finish(sta_handle* h, const uint8_t* adjacent, float rel_pose_thres,
                                               float* pose_conf_host, int* accepted_host, int* n_accepted,
                                               float* pts, float* conf, float* depth, float* K, int* k_valid_host, void* stream) {
    REQUIRE(h, "null handle");
    DEV_SCOPE(h->device);
    REQUIRE(adjacent && pose_conf_host && accepted_host && n_accepted && pts && conf && depth && K && k_valid_host, "null argument");
    hipStream_t st = (hipStream_t)stream;
    CHK(stream_ctx(h, st));
    StreamCtx& c = *h->cur;
    REQUIRE(c.rv_open, "sta_regress_views_tokens_finish: no scheduler call was begun on this stream");
    REQUIRE(c.rv_kind == 1, "sta_regress_views_tokens_finish: the call pending on this stream was begun with sta_regress_views_begin: finish it with sta_regress_views_finish (or abort it)");
    c.rv_open = false;                                  // (also on an error below: the call is over either way)
    const int k = c.rv_k;
    SeqTable t; memset(&t, 0, sizeof t);
    t.S = 2 * k;
    for (int s = 0; s < 2 * k; ++s) t.tok0[s + 1] = t.tok0[s] + c.rvt.n[s];
    *n_accepted = 0;
    h->dry = false;
    Bump ws = cur_bump(h);                              // the workspace phase A planned and filled
    return rvt_phase_b(h, ws, t, c.rvt, k, adjacent, rel_pose_thres, pose_conf_host, accepted_host, n_accepted, pts, conf, depth, K, k_valid_host, st);
}

extern "C" int sta_regress_views_tokens(sta_handle* h, const float* feat_i, int Hi, int Wi,
                                        const float* const* feat_j, const int* Hj, const int* Wj, int k,
                                        const int* win_i, const int* cnt_i, const int64_t* idx_i,
                                        const int* win_j, const int* cnt_j, const int64_t* idx_j,
                                        const uint8_t* adjacent, float rel_pose_thres,
                                        float* pose, float* pose_conf_host, int* accepted_host, int* n_accepted,
                                        float* pts, float* conf, float* depth, float* K, int* k_valid_host, void* stream) {
    REQUIRE(h, "null handle");
    REQUIRE(adjacent && pose_conf_host && accepted_host && n_accepted && pts && conf && depth && K && k_valid_host, "null argument");
    CHK(sta_regress_views_tokens_begin(h, feat_i, Hi, Wi, feat_j, Hj, Wj, k, win_i, cnt_i, idx_i, win_j, cnt_j, idx_j, pose, stream));
    return sta_regress_views_tokens_finish(h, adjacent, rel_pose_thres, pose_conf_host, accepted_host, n_accepted, pts, conf, depth, K, k_valid_host, stream);
}

// ---------------------------------------------------------------------------------------------------------
// sta_reserve: SURVEY 8(b) "no hidden allocation per call".  Without it the library sizes itself lazily: the first call on a new
// stream creates that stream's scratch context (2 x 16 MiB of split-K scratch, later the side lane's stream, events and 16 MiB),
// the first call of a larger shape re-allocates the stream's workspace behind a hipDeviceSynchronize, the first scheduler call
// creates its pinned confidence buffer, a larger patch grid rebuilds the RoPE table.  sta_reserve does all of that up front for
// the given streams and sizes, by running the PLANNING pass of every entry point (the same orchestration code, dry) and
// allocating the maximum: afterwards calls of at most these sizes on these streams neither allocate nor synchronise the device
// (sta_alloc_stats counts both; tests/test_gpu_parity.py::test_reserve_then_no_allocation_and_no_device_sync).
extern "C" int sta_reserve(sta_handle* h, int B, int H, int W, int max_edges, void* const* streams, int n_streams) {
    REQUIRE(h && h->finalized, "sta_reserve: handle not ready (weights not finalized)");
    REQUIRE(B >= 0 && max_edges >= 0 && max_edges <= 16 && (B > 0 || max_edges > 0), "sta_reserve: bad batch / edge count");
    REQUIRE(n_streams >= 1 && n_streams <= MAX_STREAM_CTX && streams, "sta_reserve: 1 <= n_streams <= %d", MAX_STREAM_CTX);
    DEV_SCOPE(h->device);
    CHK(check_ready(h, B > 0 ? B : 1, H, W));
    {   // every stream needs a scratch context: the ones it already has + the new ones must fit
        int fresh = 0;
        for (int i = 0; i < n_streams; ++i) {
            bool known = false;
            for (auto& c : h->ctx) known |= c.st == (hipStream_t)streams[i];
            for (int j = 0; j < i; ++j) known |= streams[j] == streams[i];
            fresh += known ? 0 : 1;
        }
        REQUIRE((int)h->ctx.size() + fresh <= MAX_STREAM_CTX, "sta_reserve: %d more streams than free scratch contexts (at most %d streams per handle)", fresh, MAX_STREAM_CTX);
    }
    // dry-run arguments: non-null, 16-byte aligned, never dereferenced (the planning pass launches nothing)
    float* const dummy = reinterpret_cast<float*>(uintptr_t(4096));
    struct Guard { sta_handle* h; ~Guard() { h->reserve_only = false; } } guard{h};
    h->reserve_only = true;
    const int hp = H / 16, wp = W / 16, L = h->cfg.dec_depth + 1;
    for (int i = 0; i < n_streams; ++i) {
        void* st = streams[i];
        if (B > 0) {
            float* const two[2] = {dummy, dummy};
            CHK(sta_forward_pair(h, dummy, dummy, B, H, W, two, two, two, two, st));
            CHK(sta_encode(h, dummy, B, H, W, dummy, st));
            std::vector<float*> outs((size_t)L, dummy);
            CHK(sta_decode(h, dummy, dummy + 4, B, hp, wp, outs.data(), outs.data(), st));     // (two separate feature buffers: the larger plan)
            CHK(sta_head_pose(h, dummy, B, (int64_t)h->cfg.dec_embed_dim, dummy, dummy, st));
            CHK(sta_head_pts(h, dummy, 0, dummy, 0, dummy, 0, dummy, 0, B, H, W, dummy, dummy, st));
            CHK(sta_estimate_intrinsics(h, dummy, dummy, 2 * B, H, W, 2, dummy, dummy, dummy, st));
        }
        if (max_edges > 0) {
            std::vector<const float*> fj((size_t)max_edges, dummy);
            CHK(sta_regress_views_begin(h, dummy, fj.data(), max_edges, H, W, dummy, st));
            CHK(sta_encode(h, dummy, 1, H, W, dummy, st));
        }
    }
    return 0;
}
extern "C" int sta_alloc_stats(const sta_handle* h, int64_t out[2]) {
    REQUIRE(h && out, "null argument");
    out[0] = h->n_alloc; out[1] = h->n_devsync;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// Streams for an application that overlaps calls (the three lanes of the keyframe pipeline).  HIP maps streams onto a few
// hardware queues (default 4) and two streams that share a queue run their kernels one after the other: the same three
// torch.cuda.Stream()s were reproducibly "slow" or "fast" (bench.py slam_replay, round 4: 177-183 vs 224-226 keyframes/s) and
// nothing in the HIP API says which.  So the library hands out streams it has MEASURED to overlap: a probe kernel stamps its
// start, spins ~200 us and stamps its end on stream a; the same kernel without the spin is launched on stream b right behind
// it; b overlaps a iff b started before a ended.  Candidates are created one at a time and kept when they overlap every
// stream kept so far.
__global__ void stream_probe_kernel(unsigned long long* out, unsigned long long spin_ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();          // 100 MHz
    out[0] = t0;
    while (__builtin_amdgcn_s_memrealtime() - t0 < spin_ticks) __builtin_amdgcn_s_sleep(8);
    out[1] = __builtin_amdgcn_s_memrealtime();
}
static int streams_overlap(hipStream_t a, hipStream_t b, unsigned long long* dev_stamps, bool* overlap) {
    unsigned long long hs[4];
    int votes = 0;
    for (int rep = 0; rep < 3; ++rep) {
        hipLaunchKernelGGL(stream_probe_kernel, dim3(1), dim3(64), 0, a, dev_stamps, 20000ull);      // 200 us
        hipLaunchKernelGGL(stream_probe_kernel, dim3(1), dim3(64), 0, b, dev_stamps + 2, 0ull);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(a)); HIPCHK(hipStreamSynchronize(b));
        HIPCHK(hipMemcpy(hs, dev_stamps, sizeof hs, hipMemcpyDeviceToHost));
        if (hs[2] < hs[1]) ++votes;                                       // b started before a ended
    }
    *overlap = votes >= 2;
    return 0;
}
extern "C" int sta_pipeline_streams(sta_handle* h, int n, void** streams_out, int* n_verified_out) {
    REQUIRE(h && streams_out && n >= 1 && n <= 4, "sta_pipeline_streams: bad argument (1 <= n <= 4)");
    DEV_SCOPE(h->device);
    constexpr int NMAX = 4;
    // The FIRST call creates and probes the maximum (4) whatever n is, later calls return a prefix of the same list: a stream that
    // was handed out is never destroyed before sta_destroy (a second call with a larger n used to destroy and re-create all of
    // them under the caller's torch.cuda.ExternalStream wrappers and the StreamCtx entries keyed by the old pointers: ADVICE r5).
    // A failure while probing destroys everything and leaves the list EMPTY, so the next call starts over instead of returning
    // unverified streams as if the probe had succeeded.
    if (h->pipe_streams.empty()) {
        unsigned long long* stamps = nullptr;
        HIPCHK(hipMalloc((void**)&stamps, 4 * sizeof(unsigned long long)));
        std::vector<hipStream_t> kept, rejected;
        int rc = 0;
        for (int cand = 0; cand < 16 && (int)kept.size() < NMAX && rc == 0; ++cand) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { rc = set_err("sta_pipeline_streams: stream creation failed"); break; }
            bool ok = true;
            for (hipStream_t k : kept) {
                bool ov = false;
                if (streams_overlap(k, s, stamps, &ov) != 0) { rc = -1; break; }
                if (!ov) { ok = false; break; }
            }
            if (rc == 0 && ok) kept.push_back(s); else rejected.push_back(s);
        }
        hipFree(stamps);
        const int verified = (int)kept.size();
        // fewer than 4 mutually overlapping streams on this runtime (e.g. GPU_MAX_HW_QUEUES=1): fill up with the rejected ones -
        // correct, only not concurrent - and say so through n_verified_out
        while (rc == 0 && (int)kept.size() < NMAX && !rejected.empty()) { kept.push_back(rejected.back()); rejected.pop_back(); }
        for (hipStream_t s : rejected) hipStreamDestroy(s);
        if (rc == 0 && (int)kept.size() < NMAX) rc = set_err("sta_pipeline_streams: could not create %d streams", NMAX);
        if (rc != 0) {
            for (hipStream_t s : kept) hipStreamDestroy(s);
            return rc;
        }
        h->pipe_streams = kept; h->pipe_verified = verified;
    }
    for (int i = 0; i < n; ++i) streams_out[i] = (void*)h->pipe_streams[i];
    if (n_verified_out) *n_verified_out = h->pipe_verified < n ? h->pipe_verified : n;
    return 0;
}

extern "C" int sta_estimate_scale(sta_handle* h, const float* Di, const float* Dj, const float* ci, const float* cj, int64_t n,
                                  float* s_out, void* stream) {
    REQUIRE(h && Di && Dj && ci && cj && s_out && n > 0, "bad argument");
    DEV_SCOPE(h->device);
    hipLaunchKernelGGL(scale_estimate_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, Di, Dj, ci, cj, n, s_out);
    HIPCHK(hipGetLastError());
    return 0;
}


// ---------------------------------------------------------------------------------------------------------
// (e): compact per-pair outputs of sta_forward_pair* for the step's one all-gather, one launch (was a torch.cat of eight
// strided slices in parallel.pack_compact).
extern "C" int sta_pack_compact(sta_handle* h, const float* const pts[2], const float* const conf[2], const float* const pose[2],
                                const float* const pose_conf[2], int B, int H, int W, float* out_dev, int64_t row_stride, void* stream) {
    REQUIRE(h && pts && conf && pose && pose_conf && out_dev && B > 0 && H > 0 && W > 0, "bad argument");
    const int64_t hw = (int64_t)H * W, width = 2 * (17 + 2 * hw);
    REQUIRE(row_stride >= width, "row_stride %lld < record width %lld", (long long)row_stride, (long long)width);
    DEV_SCOPE(h->device);
    PackCompact g;
    for (int v = 0; v < 2; ++v) {
        REQUIRE(pts[v] && conf[v] && pose[v] && pose_conf[v], "null view pointer");
        g.pts[v] = pts[v]; g.conf[v] = conf[v]; g.pose[v] = pose[v]; g.pose_conf[v] = pose_conf[v];
    }
    g.out = out_dev; g.hw = hw; g.row_stride = row_stride;
    int gx = (int)((2 * hw + 256 * 8 - 1) / (256 * 8)); if (gx < 1) gx = 1; if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(pack_compact_kernel, dim3(gx, 2 * B), dim3(256), 0, (hipStream_t)stream, g);
    HIPCHK(hipGetLastError());
    return 0;
}
