// snowgpu_batch.cpp -- the launch sequence of one augment batch, everything on device pointers: which kernel goes to which stream in
// which order, and the scratch it needs.  Every order and every stream choice below is a measurement; the comments say which.
#include "sg_host.h"
#include "sg_launch.h"      // sg_tiles
#include "sg_queue.h"       // the dict queue's layout

static int sync_tables(snowgpu_ctx *ctx)
{
    if (!ctx->tables_dirty) return SNOWGPU_OK;
    const size_t n = std::max<size_t>(ctx->tables.size(), 1);
    if (n > ctx->d_tables_cap) {
        if (ctx->d_tables) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->d_tables); }
        HIPCHK(ctx, hipMalloc((void **)&ctx->d_tables, n * sizeof(SgTable)));
        ctx->d_tables_cap = n;
    }
    std::vector<SgTable> h(n);
    for (size_t i = 0; i < ctx->tables.size(); ++i) h[i] = ctx->tables[i].desc;
    HIPCHK(ctx, hipMemcpy(ctx->d_tables, h.data(), n * sizeof(SgTable), hipMemcpyHostToDevice));
    ctx->tables_dirty = false;
    return SNOWGPU_OK;
}

// Expected flakes per beam for a target at the table's edge ~ K * delta / (2 pi); real sweeps sit well
// below that (flakes in range scale with (d / R0)^2).  The first pass runs with the smallest list that most
// beams fit in -- its LDS footprint decides how many waves hide each other's latency -- and hands the rest
// to the next capacity.
static void choose_tiers(const snowgpu_ctx *ctx, double beam_div_deg, int tiers[4], int *n_tiers)
{
    const double expect = (double)ctx->max_flakes * (beam_div_deg * (SG_PI / 180.0)) / SG_TWO_PI;
    // (measured on the 40 k-flake tables of C1, expect = 19: a 4-entry first pass is 5 % faster than an 8-entry one, a 16-entry one
    // half as fast -- the lists' LDS footprint decides the occupancy of the pass over ALL rows, the tiers only see the long ones)
    int first = expect <= 24.0 ? 4 : (expect <= 48.0 ? 8 : (expect <= 96.0 ? 16 : SG_LCAP));
    if (ctx->first_tier_override == 4 || ctx->first_tier_override == 8 || ctx->first_tier_override == 16 ||
        ctx->first_tier_override == SG_LCAP)
        first = ctx->first_tier_override;
    int n = 0;
    for (int c : {4, 8, 16, SG_LCAP})
        if (c >= first) tiers[n++] = c;
    *n_tiers = n;
}

// dict hand-over buffer of a list-mode tier: entries it holds for a batch of n rows (the rest of the class, if any,
// runs the received-power phase in place)
static int64_t tier_queue_cap(const snowgpu_ctx *ctx, int lmax, int64_t n)
{
    if (ctx->tier_cap_override > 0) return std::min<int64_t>(ctx->tier_cap_override, std::max<int64_t>(n, 1));
    // A buffer for every row while that costs at most 1 GiB per tier: it saves the launch of the in-place fallback pass -- a
    // chip-sized grid that finds nothing to do but sits in the chain of dependent launches a small batch is bound by.  This
    // includes the 1.5 M-row chunks of the host pipeline: 0.33 GB (8 entries) + 0.63 GB (16 entries) per context and compute
    // lane, i.e. about 1 GB per lane of the 288 GB (DESIGN.md section 3 lists it).  Beyond 1 GiB: the fractions below.
    const int64_t slot_bytes = (int64_t)sizeof(double) * (3 * (int64_t)lmax + 2) + 2;
    if (std::max<int64_t>(n, 1) * slot_bytes <= ((int64_t)1 << 30)) return std::max<int64_t>(n, 1);
    const int64_t div = lmax <= 8 ? 4 : (lmax <= 16 ? 16 : 64);
    return std::min<int64_t>(std::max<int64_t>(n, 1), std::max<int64_t>(n / div, 4096));
}

// ---- the batch launch sequence (everything on device pointers) --------------------------------------
static int launch_compaction(snowgpu_ctx *ctx, BatchDev &b, const int32_t *perm, const double *thr, size_t regions, int64_t max_tiles);

int run_batch(snowgpu_ctx *ctx, BatchDev &b)
{
    snowgpu_ctx *R = ctx->root ? ctx->root : ctx;      // a lane computes on the tables / lasers / settings of its root
    if (R->h_las.n <= 0) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_lasers has not been called");
    if (b.beam_div_deg <= 0 || b.beam_div_deg >= 45.0)
        return fail(ctx, SNOWGPU_E_INVALID, "beam divergence must be in (0, 45) degrees");
    int rc = sync_tables(R);
    if (rc) { if (R != ctx) ctx->err = R->err; return rc; }
    const int64_t max_tiles = sg_tiles(b.max_frame);
    const size_t n = (size_t)b.n_total;
    const size_t esz = b.dtype == 0 ? 4 : 8;
    hipStream_t st = b.stream;
    const bool serial = R->serial || b.serial;
    hipStream_t s_aux = serial ? st : ctx->aux, s_aux2 = serial ? st : ctx->aux2, s_aux3 = serial ? st : ctx->aux3;
    HIPCHK(ctx, hipMemsetAsync(b.status, 0, sizeof(int32_t) * 8, st));      // (status[1] = first offending row, -1 = none: set by the first kernel)
    if (n == 0) {
        HIPCHK(ctx, hipMemsetAsync(b.status + 1, 0xff, sizeof(int32_t), st));
        HIPCHK(ctx, hipMemsetAsync(b.out_counts, 0, sizeof(int64_t) * (size_t)b.n_frames, st));
        HIPCHK(ctx, hipMemsetAsync(b.out_stats, 0, sizeof(int64_t) * 3 * (size_t)b.n_frames, st));
        if (b.pack) HIPCHK(ctx, hipMemsetAsync(b.pack->mv_counts, 0, sizeof(int64_t) * (size_t)b.n_frames, st));
        return SNOWGPU_OK;
    }
    // 0. noise-threshold prepass (simulation.py:449-467) unless the caller brought the polynomial.  Only the compaction
    // (the noise-floor decision) needs its result, so it runs on its own stream next to the received-power kernels:
    // bandwidth-bound reductions beside latency-bound persistent waves.
    const double *thr = b.thr_poly;
    bool pre_forked = false;
    // The prepass' per-tile statistics ride on the channel sort's first pass over the rows when the plane is known by then: a
    // caller's plane, or the reference-today plane (a constant).  Estimated planes (least squares, RANSAC) come later, on the
    // prepass stream, and the statistics keep their own pass.
    const bool fuse_stats = !b.thr_poly && !b.defer_thr && !b.perm && (b.plane != nullptr || R->plane_par.method == SG_PLANE_REFERENCE);
    const double *early_plane = b.plane;
    double *lean_part = nullptr;
    if (fuse_stats) {
        if (!early_plane) {
            ENSURE(ctx, ctx->plane_est, (size_t)b.n_frames * 4);
            ENSURE(ctx, ctx->plane_info, (size_t)b.n_frames * 4);
            int pe = sg_plane_run(&ctx->plane_scr, &R->plane_par, b.rows, b.dtype, b.frame_off, nullptr, b.n_frames, b.n_total, b.max_frame,
                                  ctx->plane_est.p, ctx->plane_info.p, st);
            if (pe) return fail(ctx, SNOWGPU_E_HIP, std::string("plane estimate: ") + (pe > 0 ? hipGetErrorString((hipError_t)pe) : "allocation"));
            early_plane = ctx->plane_est.p;
        }
        lean_part = sg_prepass_reserve_tiles(&ctx->prepass, b.n_frames, b.max_frame);
        if (!lean_part) return fail(ctx, SNOWGPU_E_HIP, "prepass: allocation");
    }
    bool hist_early = false;
    // Large batches take the statistics out of the sort again: as a kernel of their own on the prepass stream, behind the histogram fill, they
    // run beside the sort and the scan (the sort's first pass 0.33 -> 0.20 ms on the step's critical path, the scan a little slower for the
    // company: C2 - 0.7 %, C2fire - 0.8 %, C3 - 0.9 % on one box).  Same sums in the same order as inside the sort (k_lean_stats deals the
    // rows to its threads as k_sort_hist does): same bits.  Only with a caller's plane -- nothing on `st` has to make it first.
    const bool stats_early = fuse_stats && !serial && early_plane == b.plane && (R->stats_early < 0 ? b.n_frames > 16 : R->stats_early == 1);
    auto launch_prepass = [&]() -> int {
        HIPCHK(ctx, hipEventRecord(ctx->ev_fork0, st));
        HIPCHK(ctx, hipStreamWaitEvent(s_aux2, ctx->ev_fork0, 0));
        const double *pl = fuse_stats ? early_plane : b.plane;
        if (!pl) {                                  // simulation.py:449 calculate_plane(pc): on the device, by the context's method
            ENSURE(ctx, ctx->plane_est, (size_t)b.n_frames * 4);
            ENSURE(ctx, ctx->plane_info, (size_t)b.n_frames * 4);
            int pe = sg_plane_run(&ctx->plane_scr, &R->plane_par, b.rows, b.dtype, b.frame_off, nullptr, b.n_frames, b.n_total, b.max_frame,
                                  ctx->plane_est.p, ctx->plane_info.p, s_aux2);
            if (pe) return fail(ctx, SNOWGPU_E_HIP, std::string("plane estimate: ") + (pe > 0 ? hipGetErrorString((hipError_t)pe) : "allocation"));
            pl = ctx->plane_est.p;
        }
        int e = sg_prepass_run(&ctx->prepass, b.rows, b.dtype, b.frame_off, b.n_frames, b.n_total, b.max_frame, pl,
                               b.noise_floor, ctx->thr_poly.p, b.status, s_aux2, fuse_stats ? 1 : 0, ctx->srows.p, ctx->frame_unsorted.p, hist_early ? 1 : 0, b.weather);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("prepass: ") + (e > 0 ? hipGetErrorString((hipError_t)e) : "allocation"));
        if (b.out_thr_poly)
            HIPCHK(ctx, hipMemcpyAsync(b.out_thr_poly, ctx->thr_poly.p, sizeof(double) * 3 * (size_t)b.n_frames, hipMemcpyDeviceToDevice, s_aux2));
        HIPCHK(ctx, hipEventRecord(ctx->ev_join0, s_aux2));
        pre_forked = true;
        return SNOWGPU_OK;
    };
    if (!thr && b.defer_thr) {
        // (no prepass here: the caller fits the polynomial from the device half it already has; run_compaction brings it)
    } else if (!thr) {
        ENSURE(ctx, ctx->thr_poly, (size_t)b.n_frames * 3);
        thr = ctx->thr_poly.p;
        if (!serial) {           // the prepass' histogram fill runs on ITS stream, beside the sort
            // Forked from the caller's stream FIRST: the fill is then ordered behind whatever the caller queued before this call (the wet
            // kernels of a fused call fill and read the same histogram on `st`), and a stream capture of this call records it in the graph --
            // issued on a stream that has not joined the capture it ran once, eagerly, and every replay but the first added into a stale
            // histogram.
            HIPCHK(ctx, hipEventRecord(ctx->ev_fork0, st));
            HIPCHK(ctx, hipStreamWaitEvent(s_aux2, ctx->ev_fork0, 0));
            int he = sg_prepass_clear_hist(&ctx->prepass, b.n_frames, s_aux2);
            if (he) return fail(ctx, SNOWGPU_E_HIP, std::string("prepass: ") + (he > 0 ? hipGetErrorString((hipError_t)he) : "allocation"));
            hist_early = true;
            if (fuse_stats && stats_early) {
                int se = sg_prepass_stats_early(&ctx->prepass, b.rows, b.dtype, b.frame_off, b.n_frames, b.max_frame, early_plane, s_aux2);
                if (se) return fail(ctx, SNOWGPU_E_HIP, std::string("prepass statistics: ") + (se > 0 ? hipGetErrorString((hipError_t)se) : "allocation"));
            }
        }
    } else if (b.out_thr_poly) {
        HIPCHK(ctx, hipMemcpyAsync(b.out_thr_poly, thr, sizeof(double) * 3 * (size_t)b.n_frames, hipMemcpyDeviceToDevice, st));
    }
    // 1. channel sort (simulation.py:447).  A frame whose rows come channel-sorted (channel-major sweeps) keeps the identity and is read
    // in place; any other frame (firing order, as in an STF .bin) gets a sorted copy from the sort's second pass.  Either way sorted
    // position g is "row g" of one of the two arrays for everything downstream: no gather through the permutation.
    const int32_t *perm = b.perm;
    ENSURE(ctx, ctx->srows, n * 5 * esz);
    ENSURE(ctx, ctx->frame_unsorted, (size_t)b.n_frames);
    if (!perm) {
        ENSURE(ctx, ctx->tile_hist, (size_t)b.n_frames * (size_t)max_tiles * 256);
        ENSURE(ctx, ctx->tile_base, (size_t)b.n_frames * (size_t)max_tiles * 256);
        ENSURE(ctx, ctx->tile_unsorted, (size_t)b.n_frames * (size_t)max_tiles);
        ENSURE(ctx, ctx->rank, n);
        ENSURE(ctx, ctx->perm, n);
        ENSURE(ctx, ctx->keep, n);                // channel bytes between the two sort passes; flag / keep bytes afterwards
        // (first pass and per-frame scan here; the second pass -- the sorted copy of unsorted frames -- further down, so that the segment
        // builder, which needs the scan only, runs on its side stream beside it)
        int e = sg_launch_sort(b.rows, b.dtype, b.frame_off, b.n_frames, b.n_total, ctx->tile_hist.p, ctx->tile_base.p,
                               ctx->rank.p, ctx->keep.p, ctx->perm.p, b.status, max_tiles, (fuse_stats && !stats_early) ? early_plane : nullptr, (fuse_stats && !stats_early) ? lean_part : nullptr,
                               ctx->tile_unsorted.p, ctx->frame_unsorted.p, ctx->srows.p, b.want_perm ? 1 : 0, 1, st);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("sort launch: ") + hipGetErrorString((hipError_t)e));
        perm = ctx->perm.p;
    } else {
        int e = sg_launch_gather_rows(b.rows, b.dtype, b.frame_off, b.n_frames, b.n_total, b.max_frame, perm, ctx->srows.p, ctx->frame_unsorted.p, b.status, st);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("gather launch: ") + hipGetErrorString((hipError_t)e));
    }
    b.perm_out = const_cast<int32_t *>(perm);
    // 1b. on the side stream: table descriptors per (frame, channel) and the launch order of the pass over all rows -- by flake
    // table (segments of the device sort) unless the caller brought the permutation (no channel histogram
    // then) or table ids are too sparse for the segment builder.
    const int64_t n_ft = (int64_t)b.n_frames * R->h_las.n;
    ENSURE(ctx, ctx->frame_tables, (size_t)n_ft);
    int tiers[4], n_tiers = 0;
    choose_tiers(R, b.beam_div_deg, tiers, &n_tiers);
    const int first_block = sg_beams_block(tiers[0]);
    const bool use_seg = !b.perm && R->tables.size() <= 65536 && b.n_frames <= (1 << 22)
                         && b.n_total < ((int64_t)1 << 31);
    // (a masked batch knows n_total as an upper bound only; the linear order of the pass over all rows reads it as the exact count)
    if (b.mask_map && !use_seg) return fail(ctx, SNOWGPU_E_INVALID, "a masked batch needs the segment order of the pass over all rows: at most 65536 tables and 2^22 frames");
    if (use_seg) {
        const size_t P = (size_t)b.n_frames * 256;
        ENSURE(ctx, ctx->seg_tbl_cnt, (R->tables.size() + 1) * SG_TBL_STRIDE); ENSURE(ctx, ctx->seg_tbl_base, R->tables.size() + 1);
        ENSURE(ctx, ctx->seg_blk, P); ENSURE(ctx, ctx->seg_cnt, P);
        ENSURE(ctx, ctx->seg_frame, P); ENSURE(ctx, ctx->seg_start, P); ENSURE(ctx, ctx->seg_n, 2);
        ENSURE(ctx, ctx->seg_of_blk, ((size_t)((b.n_total + first_block - 1) / first_block) + P) * SG_BLKREC);
        ENSURE(ctx, ctx->chunk_blk, 2);
    }
    // (The pass over all rows is ONE launch.  Cut into several, with k_power of one range beside the scan of the next, it gained
    // nothing: both are bound by the LDS their lists need, so sharing a CU only trades waves.)
    const int64_t total_blocks_ub = (b.n_total + first_block - 1) / first_block + (use_seg ? (int64_t)b.n_frames * 256 : 0);
    // Everything this step counts up from zero lies in ONE block, cleared by one fill (each fill is a launch on the chain between
    // the sort and the scan): per region the queue counter and the SG_MAX_CLASSES tier-list counters; per frame the intensity
    // statistics; the tier lists' lengths, the work-item counters, the row kernels' redo counters.
    static_assert(SG_MAX_CLASSES * sizeof(int32_t) == 2 * sizeof(unsigned long long), "a region's tier counters are two 64-bit words");
    const size_t q_chunk = 8 * (size_t)first_block;
    const size_t regions = std::max<size_t>((size_t)b.n_frames * 256, n / q_chunk + 2);
    const size_t zero_words = 3 * regions + 2 * (size_t)b.n_frames + 8;      // (.. and per frame the compaction's count of finished tiles)
    ENSURE(ctx, ctx->qn, zero_words);
    ENSURE(ctx, ctx->tbase, SG_MAX_CLASSES * regions);
    // A batch of up to four frames builds its segments (and clears the zero block) with ONE block on the caller's stream: no fill, no hop
    // to the side stream and back between the sort and the scan.
    bool seg_small = false;
    if (use_seg) {
        const int se = sg_launch_segments_small(b.frame_off, b.n_frames, ctx->tile_base.p, max_tiles, b.table_ids, R->h_las.n, (int)R->tables.size(), first_block,
                                                ctx->seg_blk.p, ctx->seg_start.p, ctx->seg_cnt.p, ctx->seg_frame.p, ctx->seg_n.p, ctx->seg_of_blk.p,
                                                ctx->chunk_blk.p, R->d_tables, ctx->frame_tables.p, ctx->qn.p, (int64_t)zero_words, st);
        if (se > 0) return fail(ctx, SNOWGPU_E_HIP, std::string("segment launch: ") + hipGetErrorString((hipError_t)se));
        seg_small = se == 0;
    }
    if (!seg_small) {
        HIPCHK(ctx, hipEventRecord(ctx->ev_fork, st));
        HIPCHK(ctx, hipStreamWaitEvent(s_aux, ctx->ev_fork, 0));
        int e = 0;
        if (!use_seg) e = sg_launch_resolve_tables(R->d_tables, (int)R->tables.size(), b.table_ids, n_ft, ctx->frame_tables.p, s_aux);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("table resolve launch: ") + hipGetErrorString((hipError_t)e));
        if (use_seg) {                                // (its first kernel resolves the table descriptors on the way)
            e = sg_launch_segments(b.frame_off, b.n_frames, ctx->tile_base.p, max_tiles, b.table_ids, R->h_las.n, (int)R->tables.size(), first_block,
                                   ctx->seg_tbl_cnt.p, ctx->seg_tbl_base.p, ctx->seg_blk.p, ctx->seg_start.p, ctx->seg_cnt.p, ctx->seg_frame.p,
                                   ctx->seg_n.p, ctx->seg_of_blk.p, ctx->chunk_blk.p, R->d_tables, ctx->frame_tables.p, s_aux);
            if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("segment launch: ") + hipGetErrorString((hipError_t)e));
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev_join, s_aux));
    }
    if (!b.perm) {
        int e = sg_launch_sort(b.rows, b.dtype, b.frame_off, b.n_frames, b.n_total, ctx->tile_hist.p, ctx->tile_base.p,
                               ctx->rank.p, ctx->keep.p, ctx->perm.p, b.status, max_tiles, nullptr, nullptr,
                               ctx->tile_unsorted.p, ctx->frame_unsorted.p, ctx->srows.p, b.want_perm ? 1 : 0, 2, st);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("sort launch: ") + hipGetErrorString((hipError_t)e));
    }
    // 3. beams
    ENSURE(ctx, ctx->rec, n);
    ENSURE(ctx, ctx->rec_q, n);
    ENSURE(ctx, ctx->rng, n * esz);
    ENSURE(ctx, ctx->keep, n);
    ENSURE(ctx, ctx->tier_list, n * (size_t)n_tiers);      // one list per later tier, each as long as the batch (address space) ...
    ENSURE(ctx, ctx->tier_sparse, n * (size_t)n_tiers);    // ... and the same as the scan leaves them: region by region
    ENSURE(ctx, ctx->ctile_cnt, (size_t)b.n_frames * (size_t)max_tiles + 1);
    ENSURE(ctx, ctx->ctile_base, (size_t)b.n_frames * (size_t)max_tiles + 1);
    SgBeamArgs a{};
    a.rows = b.rows; a.frame_off = b.frame_off; a.n_frames = b.n_frames; a.n_total = b.n_total; a.perm = perm;
    a.srows = ctx->srows.p; a.frame_unsorted = ctx->frame_unsorted.p;
    a.uniform_rows = (b.uniform_rows > 0 && b.n_total < ((int64_t)1 << 31)) ? b.uniform_rows : 0;
    a.inv_uniform_rows = a.uniform_rows > 0 ? 1.0f / (float)a.uniform_rows : 0.0f;
    a.las = R->d_las; a.frame_tables = ctx->frame_tables.p;
    a.rgrid = R->d_rgrid; a.beam_div_deg = b.beam_div_deg; a.rec = ctx->rec.p; a.rec_q = ctx->rec_q.p;
    a.status = b.status;
    a.rng = ctx->rng.p;
    a.dbg_count = b.dbg_count; a.dbg_rj = b.dbg_rj; a.dbg_ratio = b.dbg_ratio; a.dbg_cap = b.dbg_cap;
    a.exact_math = R->exact_math;
    // Later capacity tiers = classes of the tier lists; the last class is the global-list tier, whose lists hold a whole
    // table if need be (capped at 8192 flakes in one beam).
    const int n_cls = n_tiers;
    // Small batches (up to four sweeps): a tier holds a few hundred beams -- one or two waves' worth for one beam per lane, a chain of
    // dependent latencies 100 us long -- and the row kernels (snowgpu_rows.hip: G lanes per beam; scan, dict and received power in one
    // pass, no hand-over buffers) finish them in a third of that (0.334 -> 0.306 ms per single sweep); from 16 sweeps on they lose
    // (2-3x the instructions).  SNOWGPU_TIER_ROWS=1 / 0 forces either (tests/test_gpu_parity.py::test_remaining_environment_switches_change_no_byte).
    const bool tier_rows = (R->tier_rows < 0 ? b.n_total <= ((int64_t)1 << 19) : R->tier_rows == 1) && R->tier_cap_override <= 0;
    const int h_lanes = 256;
    const int h_cap = (int)std::min<uint32_t>(std::max<uint32_t>(R->max_flakes, 64u), 8192u);
    a.n_cls = n_cls;
    for (int k = 0; k + 1 < n_cls; ++k) a.cls_cap[k] = tiers[k + 1];
    a.cls_cap[n_cls - 1] = h_cap;
    ENSURE(ctx, ctx->h_lists, (size_t)4 * (size_t)(h_cap + 1) * (size_t)h_lanes);
    a.h_lists = ctx->h_lists.p; a.h_cap = h_cap; a.h_lanes = h_lanes;
    a.tier_list = ctx->tier_list.p; a.tier_stride = b.n_total; a.tier_sparse = ctx->tier_sparse.p;
    if (tier_rows) {
        ENSURE(ctx, ctx->redo_list, n * (size_t)n_tiers);
        a.redo_list = ctx->redo_list.p;
    }
    // Overflow slots: a beam of the pass over all rows that over-fills its LDS list, up to SG_OV_CAP flakes, leaves all of them in
    // the slot of its sorted position, and the tiers up to that capacity run no second scan (400 bytes per sorted position, touched
    // by the few per cent of beams that overflow: 13 GB of address space for a 256-sweep batch, 0.6 GB per chunk of the pipeline).
    const bool use_ov = tiers[0] < SG_OV_CAP && n_cls >= 2 && !tier_rows &&
                        R->tier_cap_override <= 0 && n * SG_OV_STRIDE * sizeof(double) <= ((size_t)40 << 30);
    int64_t tq_caps[SG_MAX_CLASSES] = {0, 0, 0, 0};
    for (int k = 0; k + 1 < n_cls && !tier_rows; ++k) {
        if (use_ov && tiers[k + 1] <= SG_OV_CAP) continue;     // (this class reads the overflow slots: no hand-over buffer)
        tq_caps[k] = tier_queue_cap(R, tiers[k + 1], b.n_total);
        ENSURE(ctx, ctx->tq[k], ((size_t)tq_caps[k] + 64) * (3 * (size_t)tiers[k + 1] + 2));
        ENSURE(ctx, ctx->tq_sc[k], (size_t)tq_caps[k]);
    }
    // Regions of the first pass = slices of its dict queue: the segments, or plain chunks of 8 blocks in linear order.
    a.q_chunk = (int32_t)q_chunk;
    {
        // 32-bit words per slot: range, azimuth (in the row dtype), one word per flake (sg_queue.h)
        const size_t slot_words = (size_t)sg_dq_slot_words(tiers[0], sg_dq_hdr(b.dtype == 0 ? 4 : 8));
        if (n * slot_words * sizeof(uint32_t) > ((size_t)64 << 30))
            return fail(ctx, SNOWGPU_E_INVALID, "batch too large for the dict queue of this table density: split it");
        if (b.n_frames >= (1 << 22)) return fail(ctx, SNOWGPU_E_INVALID, "too many frames in one batch");
        ENSURE(ctx, ctx->dq, (n + 64) * slot_words);      // blocked SoA: groups of 64 slots
        ENSURE(ctx, ctx->dq_g, n);
        ENSURE(ctx, ctx->dq_sc, n);
        if (!seg_small) HIPCHK(ctx, hipMemsetAsync(ctx->qn.p, 0, sizeof(unsigned long long) * zero_words, st));     // (else k_seg_small cleared it)
        a.tn = (int32_t *)(ctx->qn.p + regions); a.tbase = ctx->tbase.p;
        a.diff2 = ctx->qn.p + 3 * regions;
        int32_t *small = (int32_t *)(ctx->qn.p + 3 * regions + (size_t)b.n_frames);      // 16 ints; behind them the compaction's per-frame tile counters
        a.tier_info = small; a.pw_count = small + 8; a.redo_cnt = small + 12;
        a.dq = ctx->dq.p; a.dq_g = ctx->dq_g.p; a.dq_sc = ctx->dq_sc.p; a.qn = ctx->qn.p; a.dq_n = b.n_total;
        const int lanes = first_block < 64 ? first_block : 64;
        a.n_regions_ub = use_seg ? (int64_t)b.n_frames * 256 : (b.n_total + a.q_chunk - 1) / a.q_chunk;
        a.blk_rows = first_block;
        a.kp_lds_quarters = 2;     // k_power's persistent blocks take half of each CU: the later tiers and the prepass run beside it (3 and 4 quarters, with the kernel at 168 VGPRs: C2 + 1 %, C2far + 8 %, C1 + 2 %)
        const size_t items_cap = n / (size_t)lanes + 2 * (size_t)a.n_regions_ub + 64;
        ENSURE(ctx, ctx->pw_items, 2 * items_cap);
        a.pw_items = ctx->pw_items.p;
        // beams with up to `few` flakes take their own kernel (k_power_few: registers only) -- unless the occlusion tap wants their dicts
        a.pw_items1 = (R->few > 0 && !b.dbg_count && lanes == 64) ? ctx->pw_items.p + items_cap : nullptr;
        a.front_max = a.pw_items1 ? std::min(R->few, std::min(3, tiers[0])) : 1;
    }
    if (use_ov) {
        ENSURE(ctx, ctx->ov, (n + 256) * SG_OV_STRIDE);
        ENSURE(ctx, ctx->ov_sc, n + 256);
        a.ov = ctx->ov.p; a.ov_sc = ctx->ov_sc.p; a.ov_cap = SG_OV_CAP;
    }
    if (use_seg) {
        a.seg_blk = ctx->seg_blk.p; a.seg_start = ctx->seg_start.p; a.seg_cnt = ctx->seg_cnt.p; a.seg_frame = ctx->seg_frame.p;
        a.seg_n = ctx->seg_n.p; a.seg_of_blk = ctx->seg_of_blk.p; a.chunk_blk = ctx->chunk_blk.p;
    }
    const bool few_first = a.pw_items1 && !serial && b.n_total > ((int64_t)1 << 19);
    // Where k_power<4> goes when the rare tiers are not rare.  The 63-entry and the global-list tier run behind k_power on its stream; with
    // 71 000 beams in them (C1: 40 k flakes per line) that chain -- 3.8 ms -- is the last thing to finish, and it only starts when k_power is
    // through.  The device leaves every batch's tier counts in page-locked memory (k_tier_gather); if the most recent ones that have landed
    // say that chain outlasts the 16-entry tier (per beam it costs ~22x as much: 53 - 129 ns against 2.4), k_power goes to the caller's
    // stream, ahead of the 8-entry tier, and the chain starts right behind k_power_few: C1 8.16 -> 7.93 ms.  Where the 16-entry tier is the
    // last to finish that order LOSES (C2far 8.49 -> 8.85 ms, C2 4.13 -> 4.23: the chain then takes CUs from the kernel everything waits for).
    // Whatever the words say, both orders give the same bytes (tests/test_gpu_fullsize.py).
    bool heavy_tail = false;
    if (few_first && n_cls >= 3 && ctx->tier_hint_d) {
        const volatile int32_t *hint = ctx->tier_hint_h;
        long tail = 0;
        for (int k = 2; k < n_cls && k < SG_MAX_CLASSES; ++k) tail += hint[k];
        heavy_tail = R->heavy_tail < 0 ? (tail >= 4096 && tail * 22 > (long)hint[1]) : R->heavy_tail == 1;
        a.tier_hint = ctx->tier_hint_d;
    }
    if (!seg_small) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
    // measurement hooks: one event pair around the whole per-beam region
    const bool timed = ctx->prof && ctx->ev_used < (int)ctx->ev_start.size();
    if (timed) { HIPCHK(ctx, hipEventRecord(ctx->ev_start[(size_t)ctx->ev_used], st)); ctx->prof_stream = st; }
    int e = 0;
    {
        const int64_t lin_blocks = (b.n_total + first_block - 1) / first_block;
        if (use_seg) {
            a.chunk = 0;                                 // every non-empty (frame, channel) pair wastes less than one block
            a.grid_blocks = total_blocks_ub + b.max_frame / first_block + 2;
        } else {
            a.blk_lo = 0; a.blk_hi = lin_blocks;
            a.grid_blocks = lin_blocks;
        }
        e = sg_launch_beams(&a, b.dtype, tiers[0], 1, st);
        // The plan of what the pass queued (work items of k_power_few / k_power; where each region's slice of the tier lists goes)
        // runs behind it on the same stream -- the tiers then start with one short kernel (k_tier_gather) and no hop between streams --
        // and the received-power kernels it feeds on a side stream, next to the later capacity tiers.
        if (!e) e = sg_launch_power(&a, b.dtype, tiers[0], st, 1, nullptr, 3);
        if (!e) {
            HIPCHK(ctx, hipEventRecord(ctx->ev_fp, st));
            HIPCHK(ctx, hipStreamWaitEvent(s_aux, ctx->ev_fp, 0));
            e = sg_launch_power(&a, b.dtype, tiers[0], s_aux, 0, few_first ? ctx->ev_few : nullptr, heavy_tail ? 1 : 3);
        }
        if (!e) {
            // Large batches: k_power_few has the chip to itself for its turn -- four waves per SIMD of it fill the register file, and
            // the tiers, the prepass and k_power do better behind it than beside it (measured: 4.37 against 4.69 ms per 256 sweeps when
            // they all start together; the other way round for a single sweep, where nothing fills anything).
            // k_tier_gather stays BEHIND this wait although it needs nothing of k_power_few: with it ahead the tiers and the prepass start
            // the moment k_power_few ends, together with k_power<4>, and take the CUs its persistent blocks would have taken -- 4.43 - 4.49
            // against 4.22 - 4.24 ms per step on one box (round 5); the 30 us it costs give k_power<4> its head start.
            // Long-tail batches (heavy_tail: the 63-entry chain outlasts everything) start the prepass beside k_power_few instead of behind
            // it: with the chain and three persistent kernels on the chip its small kernels wait for CUs (C1: k_pre_mean32 1.1 ms, k_lean_gather
            // 0.11 ms) and stand in the chain's way -- C1 7.39 -> 7.14 ms; where the tail is short the prepass is better off behind
            // k_power_few (C2 3.91 -> 3.95 the other way, C2far the same).  SNOWGPU_PREPASS_WITH_FEW=0 / 1 overrides.
            const bool pre_with_few = R->prepass_with_few < 0 ? heavy_tail : R->prepass_with_few == 1;
            if (pre_with_few && few_first && !b.thr_poly && !b.defer_thr && !pre_forked) { int prc = launch_prepass(); if (prc) return prc; }
            if (few_first) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_few, 0));
            e = sg_launch_tier_gather(&a, st);
        }
    }
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("beam launch: ") + hipGetErrorString((hipError_t)e));
    // The noise-threshold prepass streams the rows (bandwidth-bound, no LDS): it runs beside the received-power phase and
    // the later tiers (latency-bound, LDS-bound) rather than beside the sort and the scan, which it would slow down.
    if (!b.thr_poly && !b.defer_thr && !pre_forked) { int prc = launch_prepass(); if (prc) return prc; }
    // The scan put every over-full beam on the list of its tier (it counted on past a full list, so the beam knows which): the tiers
    // start as soon as it has ended, side by side -- class 0 on the caller's stream, class 1 on a side stream, and the classes from
    // the third on (the 63-entry and the global-list tier: few beams, long dependent chains) behind k_power on ITS stream, which is
    // free long before the 8- and 16-entry tiers are through (C2 4.41 -> 4.30 ms, C2far 9.20 -> 8.64 ms against "behind class 1").
    const bool side3 = n_cls >= 2;
    // (a small batch -- no k_power_few-first schedule -- is bound by the longest chain of dependent launches: there the rare tiers go behind
    // the 8-entry tier on the caller's stream, the shortest of the three chains in a single sweep's trace)
    const bool tail_main = n_cls >= 3 && !serial && !few_first;
    const bool tail_aux = n_cls >= 3 && !serial && !tail_main;
    if (side3) { HIPCHK(ctx, hipEventRecord(ctx->ev_lists, st)); HIPCHK(ctx, hipStreamWaitEvent(s_aux3, ctx->ev_lists, 0)); }
    if (tail_aux) HIPCHK(ctx, hipStreamWaitEvent(s_aux, ctx->ev_lists, 0));
    if (heavy_tail) {                                    // (behind the event the other tiers' streams wait for: they start with it, not after it)
        e = sg_launch_power(&a, b.dtype, tiers[0], st, 0, nullptr, 2);
    }
    // what the classes held in a recent batch (page-locked words the device leaves behind, scaled to this batch's size): grids of the rare tiers
    int32_t cls_hint[SG_MAX_CLASSES] = {0, 0, 0, 0};
    if (a.tier_hint && ctx->tier_hint_h) {
        const volatile int32_t *hint = ctx->tier_hint_h;
        const int64_t then_k = hint[SG_MAX_CLASSES];
        if (then_k > 0)
            for (int k = 0; k < SG_MAX_CLASSES; ++k)
                cls_hint[k] = (int32_t)std::min<int64_t>(INT32_MAX / 8, ((int64_t)hint[k] * ((b.n_total >> 10) + 1)) / then_k + 64);
    }
    for (int k = 0; k < n_cls && !e; ++k) {
        a.work_hint = k >= 2 ? cls_hint[k] : 0;
        hipStream_t sk = (k == 0 || (tail_main && k >= 2)) ? st : ((tail_aux && k >= 2) ? s_aux : s_aux3);
        a.seg_blk = nullptr;
        a.cls = k;
        if (k == n_cls - 1) {                            // the global-list tier
            e = sg_launch_huge(&a, b.dtype, sk);
            break;
        }
        const int lmax = tiers[k + 1];
        if (use_ov && lmax <= SG_OV_CAP) {               // its lists are in the overflow slots: received power only, no second scan
            a.tq = nullptr; a.tq_sc = nullptr; a.tq_cap = 0; a.ov_list = 1;
            a.work_lo = 0; a.work_hi = (int32_t)std::min<int64_t>(b.n_total, INT32_MAX);
            e = sg_launch_power_list(&a, b.dtype, lmax, sk);
            a.ov_list = 0;
            continue;
        }
        if (tier_rows) {
            a.work_lo = 0; a.work_hi = (int32_t)std::min<int64_t>(b.n_total, INT32_MAX);
            e = sg_launch_rows(&a, b.dtype, lmax, sk);
            continue;
        }
        a.tq = ctx->tq[k].p; a.tq_sc = ctx->tq_sc[k].p; a.tq_cap = (int32_t)tq_caps[k];
        a.work_lo = 0; a.work_hi = (int32_t)tq_caps[k];
        e = sg_launch_tier_scan(&a, b.dtype, lmax, sk);                  // one beam per lane, no LDS: k_power sorts as it loads
        if (!e) e = sg_launch_power_list(&a, b.dtype, lmax, sk);
        if (!e && tq_caps[k] < b.n_total) {              // entries beyond the hand-over buffer: received power in place
            a.work_lo = (int32_t)tq_caps[k]; a.work_hi = (int32_t)std::min<int64_t>(b.n_total, INT32_MAX);
            e = sg_launch_beams(&a, b.dtype, lmax, 0, sk);
        }
    }
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("tier launch: ") + hipGetErrorString((hipError_t)e));
    if (side3) { HIPCHK(ctx, hipEventRecord(ctx->ev_join3, s_aux3)); HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_join3, 0)); }
    HIPCHK(ctx, hipEventRecord(ctx->ev_join2, s_aux));
    HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_join2, 0));
    if (timed) { HIPCHK(ctx, hipEventRecord(ctx->ev_stop[(size_t)ctx->ev_used], st)); ctx->ev_used++; }
    // 4. output rows from (sorted) rows + records, round, noise-floor filter, camera crop, compaction, stats
    // (simulation.py:516-540)
    if (pre_forked) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_join0, 0));
    if (b.defer_thr && !b.thr_poly) return SNOWGPU_OK;           // the caller's polynomial is still being fitted: run_compaction finishes the batch
    return launch_compaction(ctx, b, perm, thr, regions, max_tiles);
}

// The batch's last step: output rows from (sorted) rows + records, np.round, noise-floor filter, camera crop, stable compaction,
// statistics (simulation.py:516-540).  Everything it reads was left by run_batch in the context's scratch.
static int launch_compaction(snowgpu_ctx *ctx, BatchDev &b, const int32_t *perm, const double *thr, size_t regions, int64_t max_tiles)
{
    snowgpu_ctx *R = ctx->root ? ctx->root : ctx;
    hipStream_t st = b.stream;
    // small batches: the per-frame scan inside the count kernel / the aligned finish
    unsigned long long *tiles_done = b.n_total <= ((int64_t)1 << 19) ? ctx->qn.p + 3 * regions + (size_t)b.n_frames + 8 : nullptr;
    if (b.out_keep && b.mask_map) {
        // Masked aligned finish (k_finish_aligned_masked): it reads scratch only -- the compacted rows, their sorted copy, the records -- and
        // writes the present rows of the caller's arrays; the front end, the one reader of the caller's rows, ran on `st` ahead of run_batch.
        int e = sg_launch_finish_aligned_masked(b.rows, ctx->srows.p, ctx->frame_unsorted.p, b.dtype, ctx->rec.p, ctx->rec_q.p, ctx->rng.p, thr, perm, b.frame_off,
                                                b.mask_in_off, b.mask_map, b.n_frames, ctx->ctile_cnt.p, ctx->ctile_base.p, b.out_rows, b.out_keep, b.out_counts,
                                                b.out_stats, ctx->qn.p + 3 * regions, b.no_fov ? nullptr : &R->fov, max_tiles, tiles_done, st);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("masked aligned finish launch: ") + hipGetErrorString((hipError_t)e));
        return SNOWGPU_OK;
    }
    if (b.out_keep) {
        // Aligned finish (k_finish_aligned).  b.out_rows may be b.rows: this is the first WRITE to the caller's rows, and every reader of them
        // is ordered ahead of it on `st` -- the sort (or the gather through a caller's permutation), the plane estimate of fuse_stats, the pass
        // over all rows, the tier gather, the first later tier and (small batches) the rare tiers run on `st` itself; the segment builder,
        // k_power_few / k_power and (large batches) the rare tiers on aux (ev_join, ev_join2); the other later tiers, among them
        // k_tier_scan_direct, on aux3 (ev_join3); the histogram fill, k_lean_stats / k_lean_hist, the plane kernels and the prepass on aux2,
        // whose last record is ev_join0 (launch_prepass runs whenever aux2 was forked), waited for by run_batch just ahead of this step.
        int e = sg_launch_finish_aligned(b.rows, ctx->srows.p, ctx->frame_unsorted.p, b.dtype, ctx->rec.p, ctx->rec_q.p, ctx->rng.p, thr, perm, b.frame_off, b.n_frames,
                                         ctx->ctile_cnt.p, ctx->ctile_base.p, b.out_rows, b.out_keep, b.out_counts, b.out_stats, ctx->qn.p + 3 * regions,
                                         b.no_fov ? nullptr : &R->fov, max_tiles, tiles_done, st);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("aligned finish launch: ") + hipGetErrorString((hipError_t)e));
        return SNOWGPU_OK;
    }
    if (b.pack) {
        ENSURE(ctx, ctx->pk_tile_mv, (size_t)b.n_frames * (size_t)max_tiles + 1);
        ENSURE(ctx, ctx->pk_tile_mv_base, (size_t)b.n_frames * (size_t)max_tiles + 1);
        b.pack->tile_mv = ctx->pk_tile_mv.p; b.pack->tile_mv_base = ctx->pk_tile_mv_base.p;
    }
    int e = sg_launch_compact(b.rows, ctx->srows.p, ctx->frame_unsorted.p, b.dtype, ctx->rec.p, ctx->rec_q.p, ctx->rng.p, thr, ctx->keep.p, perm, b.frame_off, b.n_frames, b.n_total,
                              ctx->ctile_cnt.p, ctx->ctile_base.p, b.out_rows, b.out_src, b.out_counts, b.out_stats,
                              ctx->qn.p + 3 * regions, b.no_fov ? nullptr : &R->fov, max_tiles, b.pack,
                              tiles_done, st);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("compaction launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// ... for a batch whose run_batch stopped ahead of it (defer_thr): b.thr_poly now holds the caller's polynomials (device memory).  The
// sizes run_batch derived are derived again -- from the same context state: tables, lasers and settings do not change inside a call.
int run_compaction(snowgpu_ctx *ctx, BatchDev &b)
{
    snowgpu_ctx *R = ctx->root ? ctx->root : ctx;
    if (!b.thr_poly) return fail(ctx, SNOWGPU_E_INVALID, "run_compaction without threshold polynomials");
    if (b.n_total == 0) return SNOWGPU_OK;                        // (run_batch filled counts and statistics)
    const int64_t max_tiles = sg_tiles(b.max_frame);
    int tiers[4], n_tiers = 0;
    choose_tiers(R, b.beam_div_deg, tiers, &n_tiers);
    const size_t q_chunk = 8 * (size_t)sg_beams_block(tiers[0]);
    const size_t regions = std::max<size_t>((size_t)b.n_frames * 256, (size_t)b.n_total / q_chunk + 2);
    if (b.out_thr_poly)
        HIPCHK(ctx, hipMemcpyAsync(b.out_thr_poly, b.thr_poly, sizeof(double) * 3 * (size_t)b.n_frames, hipMemcpyDeviceToDevice, b.stream));
    return launch_compaction(ctx, b, b.perm ? b.perm : ctx->perm.p, b.thr_poly, regions, max_tiles);
}

int status_to_error(snowgpu_ctx *ctx, const int32_t st[8])
{
    char buf[200];
    switch (st[0]) {
    case 0: return SNOWGPU_OK;
    case SNOWGPU_E_RANGE:
        snprintf(buf, sizeof buf, "index out of bounds for the %d-bin range grid: a simulated point lies at >= ~120 m (sorted row %d)", SG_RBINS, st[1]);
        return fail(ctx, SNOWGPU_E_RANGE, buf);
    case SNOWGPU_E_CHANNELS:
        return fail(ctx, SNOWGPU_E_CHANNELS, "channel column holds values other than integers in [0, 255]; pass an explicit permutation");
    case SNOWGPU_E_OVERFLOW:
        snprintf(buf, sizeof buf, "more than %d flakes intersect one beam (sorted row %d): beyond the global-list tier "
                 "(capacity = the largest uploaded table, at most SNOWGPU_MAX_FLAKES_GLOBAL)",
                 (int)std::min<uint32_t>(std::max<uint32_t>(ctx->max_flakes, 64u), 8192u), st[1]);
        return fail(ctx, SNOWGPU_E_OVERFLOW, buf);
    case SNOWGPU_E_GROUND:
        return fail(ctx, SNOWGPU_E_GROUND, "fewer than 3 ground points in a frame");
    case SNOWGPU_E_INVALID:
        return fail(ctx, SNOWGPU_E_INVALID, "a table id in table_ids was never uploaded");
    default:
        snprintf(buf, sizeof buf, "device status %d", st[0]);
        return fail(ctx, SNOWGPU_E_INVALID, buf);
    }
}
