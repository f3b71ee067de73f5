// snowgpu_api.cpp -- the C ABI of libsnowgpu.so (include/snowgpu.h) as far as it takes no rows: context, streams, settings, lasers,
// table filing, the sampler and the profile hooks.  Host-side C++; the launch sequence of a batch is snowgpu_batch.cpp, the
// device-pointer entries snowgpu_device.cpp (batches) and snowgpu_stages.cpp (stages), the host-pointer entries snowgpu_host.cpp, every
// kernel lives in a .hip file.
#include <dlfcn.h>

#include "sg_host.h"
#include "sg_table_host.h"
#include "sg_range_index.h"  // SG_QS_FITS, SG_QS_WORDS
#include <cmath>

// simulation.py:106-116: R = np.round(np.linspace(0, 120 + c*tau_h, 1230), 2).
// linspace: k * step (+ 0.0), last element = stop; round(., 2): rint(v * 100) / 100.
static void range_grid(double *out)
{
    const double stop = 120 + 299792458.0 * 1e-8;
    const int num = SG_RBINS;
    const double step = stop / (num - 1);
    for (int k = 0; k < num; ++k) {
        double v = (double)k * step + 0.0;
        if (k == num - 1) v = stop;
        out[k] = std::rint(v * 100.0) / 100.0;
    }
}

extern "C" const char *snowgpu_version(void) { return "snowgpu 0.1.0 gfx950 (MI355X) hip"; }

extern "C" int snowgpu_range_grid(double *out)
{
    if (!out) return SNOWGPU_E_INVALID;
    range_grid(out);
    return SNOWGPU_OK;
}

extern "C" const char *snowgpu_last_error(const snowgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// streams and events of one launch sequence (a user-visible context, or a lane of its host pipeline)
static int init_streams(snowgpu_ctx *ctx)
{
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    {   // The prepass stream (aux2) sits in the HIGH-priority pool.  Rounds 1-3 needed that for scheduling (its scratch-array passes
        // were starved by the long-lived LDS-heavy blocks beside them: 5.04 vs 4.93 ms per step); for the lean prepass it no longer
        // matters on the device entry (4.62 vs 4.68 ms the other way round) -- but the runtime hands out hardware queues per priority
        // pool, and with aux2 in the normal pool the host pipeline's streams share queues: 1.47 instead of 1.85 G points/s through the
        // host entry (measured).
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->aux, hipStreamNonBlocking, 0));
        HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->aux2, hipStreamNonBlocking, greatest));
        HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->aux3, hipStreamNonBlocking, 0));
    }
    for (hipEvent_t *ep : lane_events(ctx)) HIPCHK(ctx, hipEventCreateWithFlags(ep, hipEventDisableTiming));
    if (hipHostMalloc((void **)&ctx->tier_hint_h, 64, hipHostMallocMapped) == hipSuccess) {
        std::memset(ctx->tier_hint_h, 0, 64);
        if (hipHostGetDevicePointer((void **)&ctx->tier_hint_d, ctx->tier_hint_h, 0) != hipSuccess) ctx->tier_hint_d = nullptr;
    } else { (void)hipGetLastError(); ctx->tier_hint_h = nullptr; }
    return SNOWGPU_OK;
}

extern "C" int snowgpu_create(int device, snowgpu_ctx **out)
{
    if (!out) return SNOWGPU_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SNOWGPU_E_NO_DEVICE;
    snowgpu_ctx *ctx = new snowgpu_ctx();
    ctx->device = device;
    *out = ctx;   // hand the context back even on failure so that last_error is readable
    HIPCHK(ctx, hipSetDevice(device));
    { const char *v = std::getenv("SNOWGPU_TIER_CAP"); ctx->tier_cap_override = v ? std::atoll(v) : 0; }
    { const char *v = std::getenv("SNOWGPU_FIRST_TIER"); ctx->first_tier_override = v ? std::atoi(v) : 0; }
    { const char *v = std::getenv("SNOWGPU_FEW"); ctx->few = v ? std::max(0, std::min(3, std::atoi(v))) : 2; }
    { const char *v = std::getenv("SNOWGPU_HEAVY_TAIL"); ctx->heavy_tail = v ? (v[0] == '1' ? 1 : 0) : -1; }
    { const char *v = std::getenv("SNOWGPU_SERIAL"); ctx->serial = v && v[0] == '1'; }
    { const char *v = std::getenv("SNOWGPU_STATS_EARLY"); ctx->stats_early = v ? (v[0] == '1' ? 1 : 0) : -1; }
    { const char *v = std::getenv("SNOWGPU_PREPASS_WITH_FEW"); ctx->prepass_with_few = v ? (v[0] == '1' ? 1 : 0) : -1; }
    { const char *v = std::getenv("SNOWGPU_TIER_ROWS"); ctx->tier_rows = v ? (v[0] == '1' ? 1 : 0) : -1; }
    // In a process that has loaded PyTorch's HIP runtime layer the runtime moves device-to-host copies with a full-grid blit
    // kernel, which stalls whatever computes beside it: one lane and larger chunks lose least there (1.8 instead of 1.3 G
    // points/s in-process).  SNOWGPU_PIPE_LANES / snowgpu_set_pipeline override either way.
    if (void *h = dlopen("libc10_hip.so", RTLD_NOLOAD | RTLD_LAZY)) {
        dlclose(h);
        ctx->pipe_lanes = 1;
        ctx->pipe_rows = (int64_t)3 << 20;
    }
    { const char *v = std::getenv("SNOWGPU_PIPE_LANES"); if (v) ctx->pipe_lanes = std::min(std::max(std::atoi(v), 1), 4); }
    int rc = init_streams(ctx);
    if (rc) return rc;
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_las, sizeof(SgLasers)));
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_rgrid, sizeof(double) * SG_RBINS));
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_status, sizeof(int32_t) * 8));
    double grid[SG_RBINS];
    range_grid(grid);
    HIPCHK(ctx, hipMemcpy(ctx->d_rgrid, grid, sizeof(grid), hipMemcpyHostToDevice));
    ctx->h_las.n = 0;
    return SNOWGPU_OK;
}

extern "C" void snowgpu_destroy(snowgpu_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (snowgpu_ctx *ln : ctx->lanes) snowgpu_destroy(ln);      // a lane owns a stream, events and scratch only
    ctx->lanes.clear();
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipStream_t w : {ctx->s_h2d, ctx->s_d2h, ctx->lane_stream[0], ctx->lane_stream[1], ctx->lane_stream[2]}) if (w) { (void)hipStreamSynchronize(w); (void)hipStreamDestroy(w); }
    if (ctx->tier_hint_h) (void)hipHostFree(ctx->tier_hint_h);
    if (ctx->thr_stage) (void)hipHostFree(ctx->thr_stage);
    for (hipEvent_t e : ctx->thr_ev) (void)hipEventDestroy(e);
    if (ctx->mail_up_h) (void)hipHostFree(ctx->mail_up_h);
    if (ctx->mail_dn_h) (void)hipHostFree(ctx->mail_dn_h);
    ctx->mail_up_d.release(); ctx->mail_dn_d.release(); ctx->d_wet_lines.release(); ctx->wet_fit.release();
    delete ctx->pool; ctx->pool = nullptr;
    if (ctx->st_pk) (void)hipHostFree(ctx->st_pk);
    for (hipEvent_t e : ctx->pk_ev) (void)hipEventDestroy(e);
    ctx->pk_meta.release(); ctx->pk_int.release(); ctx->pk_mv.release(); ctx->pk_mvcnt.release(); ctx->pk_tile_mv.release(); ctx->pk_tile_mv_base.release();
    for (hipEvent_t e : ctx->pipe_ev) (void)hipEventDestroy(e);
    ctx->pipe_off.release(); ctx->pipe_status.release();
    for (auto &t : ctx->tables) {
        if (t.entries) (void)hipFree(t.entries);
        if (t.bin_start) (void)hipFree(t.bin_start);
        if (t.bin_q) (void)hipFree(t.bin_q);
        if (t.bin_qs) (void)hipFree(t.bin_qs);
    }
    if (ctx->d_tables) (void)hipFree(ctx->d_tables);
    if (ctx->d_las) (void)hipFree(ctx->d_las);
    if (ctx->d_rgrid) (void)hipFree(ctx->d_rgrid);
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    ctx->tile_hist.release(); ctx->tile_base.release(); ctx->perm.release(); ctx->srows.release(); ctx->tile_unsorted.release(); ctx->frame_unsorted.release();
    ctx->seg_tbl_cnt.release(); ctx->seg_tbl_base.release(); ctx->seg_blk.release(); ctx->seg_cnt.release(); ctx->seg_frame.release();
    ctx->seg_n.release(); ctx->seg_start.release(); ctx->seg_of_blk.release(); ctx->chunk_blk.release();
    ctx->rec.release(); ctx->rec_q.release(); ctx->rng.release(); ctx->dq.release(); ctx->dq_g.release(); ctx->dq_sc.release(); ctx->qn.release(); ctx->pw_items.release(); ctx->ov.release(); ctx->ov_sc.release();
    ctx->redo_list.release(); ctx->rows_c4.release(); ctx->rows_ch.release();
    ctx->tier_list.release(); ctx->tier_sparse.release(); ctx->tbase.release(); ctx->h_lists.release();
    for (int k = 0; k < SG_MAX_CLASSES; ++k) { ctx->tq[k].release(); ctx->tq_sc[k].release(); }
    ctx->ctile_cnt.release(); ctx->ctile_base.release(); ctx->table_ids.release(); ctx->out_src.release();
    ctx->rank.release(); ctx->keep.release(); ctx->rows_in.release(); ctx->rows_out.release();
    ctx->frame_off.release(); ctx->out_counts.release(); ctx->out_stats.release();
    ctx->thr_poly.release(); ctx->plane.release(); ctx->dbg_rj.release(); ctx->dbg_ratio.release();
    ctx->dbg_count.release(); ctx->frame_tables.release(); ctx->user_thr.release(); ctx->out_thr.release(); ctx->user_perm.release();
    ctx->snow_rows.release(); ctx->snow_src.release(); ctx->wet_flags.release(); ctx->snow_counts.release();
    ctx->wet_counts.release(); ctx->wet_rows.release(); ctx->wet_plane.release();
    ctx->rows_crop.release(); ctx->crop_src.release(); ctx->crop_out_src.release(); ctx->crop_counts.release(); ctx->crop_off.release(); ctx->crop_stats.release();
    ctx->dror_entry.release(); ctx->dror_cell.release(); ctx->dror_sorted.release();
    ctx->vox_table.release(); ctx->vox_slot.release(); ctx->vox_order.release(); ctx->vox_span.release(); ctx->vox_first.release();
    ctx->vox_tile_cnt.release(); ctx->vox_tile_base.release(); ctx->vox_fbase.release(); ctx->vox_m.release();
    ctx->fps_x.release(); ctx->fps_y.release(); ctx->fps_z.release(); ctx->fps_t.release(); ctx->fps_src.release();
    ctx->fpss_sec.release(); ctx->fpss_roi.release(); ctx->fpss_tile.release(); ctx->fpss_seg.release();
    ctx->ball_entry.release(); ctx->ball_cell.release(); ctx->ball_x.release(); ctx->ball_y.release(); ctx->ball_z.release(); ctx->ball_src.release();
    ctx->range_key.release();
    ctx->nn_entry.release(); ctx->nn_box.release(); ctx->nn_rec.release();
    ctx->box_rec.release(); ctx->box_table.release();
    ctx->roi_rec.release(); ctx->roi_table.release(); ctx->roi_runs.release();
    ctx->rv_rec.release(); ctx->rv_table.release(); ctx->rv_runs.release(); ctx->rv_list.release(); ctx->rv_sorted.release(); ctx->rv_offset.release();
    ctx->iou_rec.release(); ctx->nms_order.release(); ctx->nms_cand.release();
    ctx->anchor_rec.release(); ctx->anchor_top.release(); ctx->anchor_blk.release();
    ctx->paste_runs.release(); ctx->paste_frames.release(); ctx->paste_grid.release();
    ctx->scene_rowrec.release(); ctx->scene_tries.release(); ctx->scene_box_rec.release(); ctx->scene_box_table.release(); ctx->scene_box_of.release();
    sg_prepass_release(&ctx->prepass);
    sg_plane_release(&ctx->plane_scr);
    ctx->plane_est.release(); ctx->wet_plane_est.release(); ctx->plane_info.release(); ctx->stats_hist.release(); ctx->stats_rec.release();
    for (auto e : ctx->ev_start) (void)hipEventDestroy(e);
    for (auto e : ctx->ev_stop) (void)hipEventDestroy(e);
    for (hipEvent_t *ep : lane_events(ctx)) if (*ep) (void)hipEventDestroy(*ep);
    for (hipStream_t st : {ctx->aux3, ctx->aux2, ctx->aux, ctx->stream})
        if (st) (void)hipStreamDestroy(st);
    delete ctx;
}

extern "C" int snowgpu_set_lasers(snowgpu_ctx *ctx, int n, const double *focal_slope, const double *focal_offset,
                                  const int32_t *min_intensity, const int32_t *max_intensity)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n <= 0 || n > SG_MAX_LASERS || !focal_slope || !focal_offset || !min_intensity || !max_intensity)
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_lasers: need 1..256 lasers and four arrays");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < n; ++i) {
        ctx->h_las.focal_slope[i] = focal_slope[i];
        ctx->h_las.focal_offset[i] = focal_offset[i];
        ctx->h_las.min_i[i] = min_intensity[i];
        ctx->h_las.max_i[i] = max_intensity[i];
    }
    ctx->h_las.n = n;
    HIPCHK(ctx, hipMemcpy(ctx->d_las, &ctx->h_las, sizeof(SgLasers), hipMemcpyHostToDevice));
    return SNOWGPU_OK;
}

// ---- table filing --------------------------------------------------------------------------------

// hand a filed table (device arrays, owned by the context from here on) to the table list under table_id
static int register_table(snowgpu_ctx *ctx, int table_id, SgEntry *entries, uint32_t *bin_start, uint32_t n_entries, uint32_t k,
                          uint32_t max_bin)
{
    if ((size_t)table_id >= ctx->tables.size()) ctx->tables.resize((size_t)table_id + 1);
    DeviceTable &dt = ctx->tables[(size_t)table_id];
    if (dt.entries || dt.bin_start) (void)hipStreamSynchronize(ctx->stream);     // no batch may still read the old table
    if (dt.entries) (void)hipFree(dt.entries);
    if (dt.bin_start) (void)hipFree(dt.bin_start);
    if (dt.bin_q) (void)hipFree(dt.bin_q);
    if (dt.bin_qs) (void)hipFree(dt.bin_qs);
    dt.entries = entries; dt.bin_start = bin_start; dt.bin_q = nullptr; dt.bin_qs = nullptr;
    dt.desc = SgTable{};
    ctx->tables_dirty = true;
    uint32_t *q = nullptr, *qs = nullptr;
    int e = (int)hipMalloc((void **)&q, (size_t)SG_NBINS * SG_QSTEPS * sizeof(uint32_t));
    // the step-major index packs two counts into a word: only for tables whose longest bin fits 16 bits (the scan then reads bin_q).
    // Its shape is the library's choice (sg_range_index.h: SG_QS_FILE_STEPS steps of SG_QS_FILE_STEP_M metres) and travels in the descriptor.
    static_assert(SG_QS_FILE_STEPS >= 1 && SG_QS_FILE_STEPS <= 64, "k_table_index files one step per lane of a wave");
    static_assert((float)(1.0 / SG_QS_FILE_STEP_M) * SG_QS_FILE_STEP_M == 1.0, "the step length is a power of two");
    if (!e && SG_QS_FITS(max_bin)) e = (int)hipMalloc((void **)&qs, SG_QS_WORDS_OF(SG_QS_FILE_STEPS, SG_NBINS) * sizeof(uint32_t));
    if (!e) e = sg_table_index(entries, bin_start, q, qs, SG_QS_FILE_STEPS, SG_QS_FILE_STEP_M, ctx->stream);
    if (!e) e = (int)hipStreamSynchronize(ctx->stream);
    if (e) {
        if (q) (void)hipFree(q);
        if (qs) (void)hipFree(qs);
        (void)hipFree(entries); (void)hipFree(bin_start);
        dt.entries = nullptr; dt.bin_start = nullptr;
        return fail(ctx, SNOWGPU_E_HIP, std::string("table index: ") + hipGetErrorString((hipError_t)e));
    }
    dt.bin_q = q; dt.bin_qs = qs;
    dt.desc.entries = entries;
    dt.desc.bin_start = bin_start;
    dt.desc.bin_q = q;
    dt.desc.bin_qs = qs;
    dt.desc.qs_steps = qs ? (uint32_t)SG_QS_FILE_STEPS : 0u;
    dt.desc.qs_per_m = (float)(1.0 / SG_QS_FILE_STEP_M);
    // must stay SG_NBINS: bin_q and bin_qs above are sized, and filed by k_table_index, with that constant, and the scan takes the row
    // stride of bin_qs from n_bins (SG_QS_ROW(n_bins)) -- a descriptor with another n_bins would read past the arrays
    dt.desc.n_bins = (uint32_t)SG_NBINS;
    dt.desc.n_entries = n_entries;
    dt.desc.inv_bin_w = SG_NBINS / SG_TWO_PI;
    dt.desc.n_flakes = k;
    dt.desc.max_bin = max_bin;
    ctx->tables_dirty = true;
    ctx->max_flakes = std::max(ctx->max_flakes, k);
    return SNOWGPU_OK;
}

// File a table whose rows are in DEVICE memory (a table sampled there): derive, bin, sort on the device; only the record
// count comes back to size the allocation.
static int file_table_device(snowgpu_ctx *ctx, int table_id, const double *d_xyr, int64_t k)
{
    hipStream_t st = ctx->stream;
    const size_t nb = SG_NBINS;
    DevBuf<SgEntry> fl, tmp;
    DevBuf<int32_t> b0, span, misc;
    DevBuf<uint32_t> count, start, fill;
    auto cleanup = [&]() { fl.release(); tmp.release(); b0.release(); span.release(); misc.release(); count.release(); start.release(); fill.release(); };
    if (fl.ensure((size_t)std::max<int64_t>(k, 1)) || b0.ensure((size_t)std::max<int64_t>(k, 1)) || span.ensure((size_t)std::max<int64_t>(k, 1)) ||
        misc.ensure(2) || count.ensure(nb + 1) || start.ensure(nb + 1) || fill.ensure(nb + 1)) {
        cleanup();
        return fail(ctx, SNOWGPU_E_HIP, "hipMalloc failed while filing a table");
    }
    int e = sg_file_table_stage_a(d_xyr, k, fl.p, b0.p, span.p, count.p, start.p, fill.p, misc.p, st);
    uint32_t n_entries = 0;
    int32_t h_misc[2] = {0, 0};
    if (!e) e = (int)hipMemcpyAsync(&n_entries, start.p + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (!e) e = (int)hipMemcpyAsync(h_misc, misc.p, sizeof h_misc, hipMemcpyDeviceToHost, st);
    if (!e) e = (int)hipStreamSynchronize(st);
    if (e) { cleanup(); return fail(ctx, SNOWGPU_E_HIP, std::string("table filing: ") + hipGetErrorString((hipError_t)e)); }
    if (h_misc[0] > 0) {
        cleanup();
        char buf[128];
        snprintf(buf, sizeof buf, "table row %d is not a disk clear of the origin", 0x7fffffff - h_misc[0]);
        return fail(ctx, SNOWGPU_E_TABLE, buf);
    }
    if ((size_t)n_entries > (size_t)64 * (size_t)std::max<int64_t>(k, 1) + 4096) {
        cleanup();
        return fail(ctx, SNOWGPU_E_TABLE, "flakes so close to the sensor that they cover most azimuths");
    }
    SgEntry *d_entries = nullptr;
    uint32_t *d_start = nullptr;
    if (tmp.ensure((size_t)n_entries + 1) || hipMalloc((void **)&d_entries, ((size_t)n_entries + 1) * sizeof(SgEntry)) != hipSuccess ||
        hipMalloc((void **)&d_start, (nb + 1) * sizeof(uint32_t)) != hipSuccess) {
        if (d_entries) (void)hipFree(d_entries);
        cleanup();
        return fail(ctx, SNOWGPU_E_HIP, "hipMalloc failed while filing a table");
    }
    e = sg_file_table_stage_b(k, fl.p, b0.p, span.p, start.p, fill.p, tmp.p, d_entries, st);
    if (!e) e = (int)hipMemcpyAsync(d_start, start.p, (nb + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (!e) e = (int)hipStreamSynchronize(st);
    cleanup();
    if (e) { (void)hipFree(d_entries); (void)hipFree(d_start); return fail(ctx, SNOWGPU_E_HIP, std::string("table filing: ") + hipGetErrorString((hipError_t)e)); }
    return register_table(ctx, table_id, d_entries, d_start, n_entries, (uint32_t)k, (uint32_t)h_misc[1]);
}

// snowgpu_upload_table for rows that already live in DEVICE memory (K x 3 float64): filed by kernels, no host copy.
extern "C" int snowgpu_file_table_device(snowgpu_ctx *ctx, int table_id, const double *d_xyr, int64_t n_flakes)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (table_id < 0 || table_id > (1 << 20) || n_flakes < 0 || (n_flakes > 0 && !d_xyr))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_file_table_device: bad table id or size");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return file_table_device(ctx, table_id, d_xyr, n_flakes);
}

// Debug / parity tap: the per-flake quantities of a filed table by table row -- range (simulation.py:332), azimuth
// (:351-352) and the two tangent angles ordered (right, left) (geometry.py:138-190, :32-80).  out: K x 4 doubles (host).
extern "C" int snowgpu_debug_table(snowgpu_ctx *ctx, int table_id, double *out, int64_t cap_rows)
{
    if (!ctx || !out) return SNOWGPU_E_INVALID;
    if (table_id < 0 || (size_t)table_id >= ctx->tables.size() || !ctx->tables[(size_t)table_id].entries)
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_debug_table: unknown table id");
    const DeviceTable &dt = ctx->tables[(size_t)table_id];
    const size_t k = dt.desc.n_flakes;
    if ((int64_t)k > cap_rows) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_debug_table: buffer too small");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<double> d;
    if (d.ensure(std::max<size_t>(k * 4, 1))) return fail(ctx, SNOWGPU_E_HIP, "hipMalloc failed");
    int e = sg_table_dump(dt.entries, dt.desc.n_entries, d.p, ctx->stream);
    if (!e && k) e = (int)hipMemcpyAsync(out, d.p, sizeof(double) * 4 * k, hipMemcpyDeviceToHost, ctx->stream);
    if (!e) e = (int)hipStreamSynchronize(ctx->stream);
    d.release();
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("table dump: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Debug tap: the whole filed table -- bin offsets, every record of every bin and the spare one, both range indexes, and the descriptor's
// counts (include/snowgpu.h).  Copies only: what the scan would read is what comes back.
extern "C" int snowgpu_debug_table_bins(snowgpu_ctx *ctx, int table_id, uint32_t *bin_start, int64_t cap_start, void *entries, int64_t cap_entries,
                                        uint32_t *bin_q, int64_t cap_q, uint32_t *bin_qs, int64_t cap_qs, int64_t *info, double *qs_per_m)
{
    if (!ctx || !bin_start || !entries || !bin_q || !bin_qs || !info || !qs_per_m) return SNOWGPU_E_INVALID;
    if (table_id < 0 || (size_t)table_id >= ctx->tables.size() || !ctx->tables[(size_t)table_id].entries)
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_debug_table_bins: unknown table id");
    const DeviceTable &dt = ctx->tables[(size_t)table_id];
    const size_t n_start = (size_t)SG_NBINS + 1, n_rec = (size_t)dt.desc.n_entries + 1, n_q = (size_t)SG_NBINS * SG_QSTEPS;
    const size_t n_qs = dt.bin_qs ? SG_QS_WORDS_OF(dt.desc.qs_steps, SG_NBINS) : 0;
    info[0] = dt.desc.n_flakes; info[1] = dt.desc.n_entries; info[2] = dt.desc.max_bin; info[3] = dt.desc.qs_steps; info[4] = dt.bin_qs ? 1 : 0;
    *qs_per_m = (double)dt.desc.qs_per_m;
    if (cap_start < (int64_t)n_start || cap_entries < (int64_t)n_rec || cap_q < (int64_t)n_q || cap_qs < (int64_t)n_qs)
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_debug_table_bins: buffer too small (see info)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int e = (int)hipMemcpyAsync(bin_start, dt.bin_start, sizeof(uint32_t) * n_start, hipMemcpyDeviceToHost, ctx->stream);
    if (!e) e = (int)hipMemcpyAsync(entries, dt.entries, sizeof(SgEntry) * n_rec, hipMemcpyDeviceToHost, ctx->stream);
    if (!e) e = (int)hipMemcpyAsync(bin_q, dt.bin_q, sizeof(uint32_t) * n_q, hipMemcpyDeviceToHost, ctx->stream);
    if (!e && n_qs) e = (int)hipMemcpyAsync(bin_qs, dt.bin_qs, sizeof(uint32_t) * n_qs, hipMemcpyDeviceToHost, ctx->stream);
    const int es = (int)hipStreamSynchronize(ctx->stream);       // also after a failed copy: nothing may still write the caller's buffers
    if (!e) e = es;
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("table bins: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

extern "C" int snowgpu_upload_table(snowgpu_ctx *ctx, int table_id, const double *xyr, int64_t k)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (table_id < 0 || table_id > (1 << 20) || k < 0 || (k > 0 && !xyr))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_upload_table: bad table id or size");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nb = SG_NBINS;
    std::vector<SgEntry> entries;
    std::vector<uint32_t> start;
    uint32_t max_bin = 0;
    int64_t bad_row = -1;
    const int frc = sg_file_table_host(xyr, k, entries, start, max_bin, &bad_row);
    if (frc == 1) {
        char buf[160];
        snprintf(buf, sizeof buf, "snowgpu_upload_table: row %lld (%g, %g, %g) is not a disk clear of the origin",
                 (long long)bad_row, xyr[3 * bad_row], xyr[3 * bad_row + 1], xyr[3 * bad_row + 2]);
        return fail(ctx, SNOWGPU_E_TABLE, buf);
    }
    if (frc == 2) return fail(ctx, SNOWGPU_E_TABLE, "snowgpu_upload_table: flakes so close to the sensor that they cover most azimuths");
    const size_t n_entries = start[(size_t)nb];
    SgEntry *d_entries = nullptr;
    uint32_t *d_start = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d_entries, (n_entries + 1) * sizeof(SgEntry)));
    if (hipMalloc((void **)&d_start, ((size_t)nb + 1) * sizeof(uint32_t)) != hipSuccess) { (void)hipFree(d_entries); return fail(ctx, SNOWGPU_E_HIP, "hipMalloc failed for bin offsets"); }
    HIPCHK(ctx, hipMemcpy(d_entries, entries.data(), (n_entries + 1) * sizeof(SgEntry), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_start, start.data(), ((size_t)nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
    return register_table(ctx, table_id, d_entries, d_start, (uint32_t)n_entries, (uint32_t)k, max_bin);
}

extern "C" int snowgpu_free_table(snowgpu_ctx *ctx, int table_id)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (table_id < 0 || (size_t)table_id >= ctx->tables.size()) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_free_table: unknown table id");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DeviceTable &dt = ctx->tables[(size_t)table_id];
    if (dt.entries || dt.bin_start) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (dt.entries) { (void)hipFree(dt.entries); dt.entries = nullptr; }
    if (dt.bin_start) { (void)hipFree(dt.bin_start); dt.bin_start = nullptr; }
    if (dt.bin_q) { (void)hipFree(dt.bin_q); dt.bin_q = nullptr; }
    if (dt.bin_qs) { (void)hipFree(dt.bin_qs); dt.bin_qs = nullptr; }
    dt.desc = SgTable{};
    ctx->tables_dirty = true;
    return SNOWGPU_OK;
}

extern "C" int snowgpu_table_count(const snowgpu_ctx *ctx)
{
    if (!ctx) return 0;
    int n = 0;
    for (auto &t : ctx->tables) n += t.entries != nullptr;
    return n;
}

extern "C" int snowgpu_status_error(snowgpu_ctx *ctx, const int32_t *status8)
{
    if (!ctx || !status8) return SNOWGPU_E_INVALID;
    return status_to_error(ctx, status8);
}

extern "C" int snowgpu_sample_table(snowgpu_ctx *ctx, int table_id, double occupancy_ratio, double diameter_scale_mm, double r_0,
                                    uint64_t seed, double *xyr_out, int64_t cap, int64_t *n_out)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (!(occupancy_ratio > 0) || !(occupancy_ratio < 0.05) || !(diameter_scale_mm > 0) || !(r_0 > 0.05) || !(r_0 <= 500.0) || !n_out)
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_sample_table: need 0 < occupancy < 0.05, scale > 0, 0.05 < R0 <= 500 m");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const double target = occupancy_ratio * SG_PI * r_0 * r_0;
    const double s_m = diameter_scale_mm / 1000.0;
    const double mean_area = SG_PI * s_m * s_m / 3.0;         // E[pi r^2], r^2 = d^2/4 - h^2, h ~ U(-d/2, d/2), d ~ Exp(s)
    int64_t n_cand = (int64_t)(1.3 * target / mean_area) + 4096;
    int64_t rows = 0;
    DevBuf<double> d_xyr;
    for (int attempt = 0;; ++attempt) {
        if (n_cand > ((int64_t)1 << 27)) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_sample_table: table would exceed 2^27 candidates");
        if (d_xyr.ensure((size_t)n_cand * 3)) return fail(ctx, SNOWGPU_E_HIP, "hipMalloc failed for the sampled table");
        int rc = sg_sample_table(occupancy_ratio, diameter_scale_mm, r_0, seed, n_cand, d_xyr.p, n_cand, &rows, ctx->stream);
        if (rc == -2 && attempt < 4) { d_xyr.release(); n_cand *= 2; continue; }     // not enough darts: throw more
        if (rc != 0) {
            d_xyr.release();
            if (rc > 0) return fail(ctx, SNOWGPU_E_HIP, std::string("sampler: ") + hipGetErrorString((hipError_t)rc));
            return fail(ctx, SNOWGPU_E_TABLE, rc == -3 ? "sampler: a dart overlaps more than 4 earlier darts (occupancy too high for this sampler)"
                                                       : "sampler: acceptance did not settle / target area not reached");
        }
        break;
    }
    *n_out = rows;
    int rc = SNOWGPU_OK;
    if (xyr_out) {
        if (cap < rows) rc = fail(ctx, SNOWGPU_E_INVALID, "snowgpu_sample_table: output buffer too small (see *n_out)");
        else if (rows && hipMemcpy(xyr_out, d_xyr.p, sizeof(double) * 3 * (size_t)rows, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(ctx, SNOWGPU_E_HIP, "sampler copy failed");
    }
    // the table is filed where it was made: derive / bin / sort kernels on the sampler's output, no host round trip
    if (rc == SNOWGPU_OK && table_id >= 0) rc = file_table_device(ctx, table_id, d_xyr.p, rows);
    d_xyr.release();
    return rc;
}

// The status words of the last batch that went through a host-pointer entry of this context (layout: see
// snowgpu_augment_batch_device): how many beams each later capacity tier took.
extern "C" int snowgpu_last_status(snowgpu_ctx *ctx, int32_t *out8)
{
    if (!ctx || !out8) return SNOWGPU_E_INVALID;
    std::memcpy(out8, ctx->h_status, sizeof(int32_t) * 8);
    return SNOWGPU_OK;
}

// NUMA node the HIP device hangs on (sysfs, by its PCI bus id), or -1: for launchers that place one process per GPU next to it.
extern "C" int snowgpu_device_numa_node(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return -1;
    return node_of_device(device);
}

// How the results of a pipelined host-pointer batch cross the link.  mode 0 (default): the output rows and their source indices, 24 bytes
// per point.  mode 1 ("packed"): per kept row its source row | label and its intensity (8 bytes; 12 for float64 rows), the moved
// coordinates of scattered rows apart; `threads` host threads of the library (0: the CPUs this process may use minus two, at most 8) put
// the caller's out_rows / out_src together from those and from the caller's INPUT rows -- same bytes in the caller's buffers, a third of
// the download, and host cores busy copying.  For callers bound by the link who have the cores to spare.
extern "C" int snowgpu_set_result_transfer(snowgpu_ctx *ctx, int mode, int threads)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if ((mode != 0 && mode != 1) || threads < 0 || threads > 256) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_result_transfer: mode 0 or 1, 0 <= threads <= 256");
    if (mode == 1) {
        if (ctx->pool && threads != ctx->asm_threads) { delete ctx->pool; ctx->pool = nullptr; }     // (made again, with `threads`, by the next packed call)
        ctx->asm_threads = threads;
    }
    ctx->result_mode = mode;
    return SNOWGPU_OK;
}

// Timeline of the last packed call of this context, milliseconds since its start: [0] everything enqueued, [1] every download landed,
// [2] every row assembled; [3] host threads used.
extern "C" int snowgpu_debug_transfer_times(snowgpu_ctx *ctx, double *out4)
{
    if (!ctx || !out4) return SNOWGPU_E_INVALID;
    for (int i = 0; i < 3; ++i) out4[i] = ctx->pk_times[i];
    out4[3] = ctx->pool ? (double)ctx->pool->threads.size() : 0.0;
    return SNOWGPU_OK;
}

// Chunk size of the upload / compute / download pipeline of the host-pointer entry; 0 switches the pipeline off.
extern "C" int snowgpu_set_pipeline(snowgpu_ctx *ctx, int64_t chunk_rows)
{
    if (!ctx || chunk_rows < 0) return SNOWGPU_E_INVALID;
    ctx->pipe_rows = chunk_rows;
    return SNOWGPU_OK;
}

// The two fitted lines of estimate_laser_parameters (wet_ground/augmentation.py:216-219, :248-251) for the NEXT
// snowgpu_wet_ground_batch of this context, from a caller who fits them itself -- e.g. with its own NumPy, whose argpartition
// decides quirk Q8 -- instead of the device's fit: n_frames x 4 (p slope, p intercept, noise-line slope, noise-line intercept).
// Everything else (ground rows, incident angles, the < 1000-ground-rows rule, Fresnel chain, noise drop) stays on the device.
extern "C" int snowgpu_set_wet_lines(snowgpu_ctx *ctx, int n_frames, const double *lines)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || !lines) { ctx->wet_lines.clear(); return SNOWGPU_OK; }
    ctx->wet_lines.assign(lines, lines + (size_t)n_frames * 4);
    return SNOWGPU_OK;
}

// estimation_method of ground_water_augmentation (wet_ground/augmentation.py:25, :215-229, :243-253) for the wet-ground calls of this
// context: 0 = 'linear' (two regression lines), 1 = 'poly' (np.polyfit of degree 2 for the laser power, ransac_polyfit for the noise
// level -- the reference draws its RANSAC samples from NumPy's unseeded global generator; here they come from Philox keyed by `seed`).
extern "C" int snowgpu_set_wet_estimation(snowgpu_ctx *ctx, int method, uint64_t seed)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (method != 0 && method != 1) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_wet_estimation: method 0 (linear) or 1 (poly)");
    ctx->wet_estimation = method;
    ctx->wet_seed = seed;
    return SNOWGPU_OK;
}

// The curves the last wet-ground call of this context fitted, per frame: laser power c2, c1, c0 (relative_output_intensity =
// power_factor * polyval), noise level c2, c1, c0 (adaptive_noise_threshold = noise_floor * polyval), ground rows, and the RANSAC
// trial whose consensus refit was kept (-1: the fit over all points; 'linear': always -1 and c2 = 0).  out: n_frames x 8 doubles.
extern "C" int snowgpu_wet_last_fit(snowgpu_ctx *ctx, int n_frames, double *out)
{
    if (!ctx || !out || n_frames <= 0) return SNOWGPU_E_INVALID;
    if (n_frames != ctx->wet_fit_frames) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_wet_last_fit: the last wet-ground call had another number of frames");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, ctx->wet_fit.p, sizeof(double) * 8 * (size_t)n_frames, hipMemcpyDeviceToHost));
    return SNOWGPU_OK;
}

// Parity tap of the 'poly' noise fit: the device's ransac_polyfit(x, y, order=2) on m (3 .. 50) caller-supplied points with the draws of
// (seed; frame) -- out[0..2] = the quadratic's coefficients (highest power first), out[3] = the trial whose consensus refit was kept (-1: none).
extern "C" int snowgpu_debug_ransac_polyfit(snowgpu_ctx *ctx, int m, const double *x, const double *y, uint64_t seed, uint64_t frame, double *out4)
{
    if (!ctx || !x || !y || !out4) return SNOWGPU_E_INVALID;
    if (m < 3 || m > 50) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_debug_ransac_polyfit: 3 <= m <= 50");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf<double> d;
    if (d.ensure(2 * 50 + 4)) return fail(ctx, SNOWGPU_E_HIP, "hipMalloc failed");
    int rc = SNOWGPU_OK;
    hipStream_t st = ctx->stream;
    hipError_t e = hipMemcpyAsync(d.p, x, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d.p + 50, y, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = (hipError_t)sg_debug_ransac_quad(d.p, d.p + 50, m, seed, frame, d.p + 100, st);
    if (e == hipSuccess) e = hipMemcpyAsync(out4, d.p + 100, sizeof(double) * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = fail(ctx, SNOWGPU_E_HIP, std::string("ransac tap: ") + hipGetErrorString(e));
    d.release();
    return rc;
}

extern "C" int snowgpu_set_exact_math(snowgpu_ctx *ctx, int on)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    ctx->exact_math = on ? 1 : 0;
    return SNOWGPU_OK;
}

extern "C" int snowgpu_set_serial(snowgpu_ctx *ctx, int on)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    ctx->serial = on != 0;
    return SNOWGPU_OK;
}

extern "C" int snowgpu_lane_stream(snowgpu_ctx *ctx, int level, void **stream)
{
    if (!ctx || !stream || level < 0 || level > 2) return SNOWGPU_E_INVALID;
    *stream = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->lane_stream[level]) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const int prio = level == 0 ? greatest : level == 2 ? least : (least + greatest) / 2;      // (HIP: 1 low, 0 normal, -1 high)
        HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->lane_stream[level], hipStreamNonBlocking, prio));
    }
    *stream = (void *)ctx->lane_stream[level];
    return SNOWGPU_OK;
}

extern "C" int snowgpu_host_alloc(snowgpu_ctx *ctx, size_t bytes, void **ptr)
{
    if (!ctx || !ptr) return SNOWGPU_E_INVALID;
    *ptr = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostMalloc(ptr, std::max<size_t>(bytes, 8), hipHostMallocPortable));
    return SNOWGPU_OK;
}

// ctx may be NULL (or already destroyed by the caller): page-locked memory is not tied to a context, and a buffer handed
// to a caller may outlive the context that allocated it.
extern "C" int snowgpu_host_free(snowgpu_ctx *ctx, void *ptr)
{
    (void)ctx;
    if (!ptr) return SNOWGPU_OK;
    return hipHostFree(ptr) == hipSuccess ? SNOWGPU_OK : SNOWGPU_E_HIP;
}

extern "C" int snowgpu_profile_begin(snowgpu_ctx *ctx, int max_launches)
{
    if (!ctx || max_launches <= 0) return SNOWGPU_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    while ((int)ctx->ev_start.size() < max_launches) {
        hipEvent_t a, b;
        HIPCHK(ctx, hipEventCreate(&a));
        HIPCHK(ctx, hipEventCreate(&b));
        ctx->ev_start.push_back(a);
        ctx->ev_stop.push_back(b);
    }
    ctx->ev_used = 0;
    ctx->prof = true;
    return SNOWGPU_OK;
}

extern "C" int snowgpu_profile_end(snowgpu_ctx *ctx, double *beam_kernel_ms, int *n_launches)
{
    if (!ctx || !beam_kernel_ms || !n_launches) return SNOWGPU_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->prof = false;
    double sum = 0.0;
    if (ctx->ev_used > 0) HIPCHK(ctx, hipEventSynchronize(ctx->ev_stop[(size_t)ctx->ev_used - 1]));
    for (int i = 0; i < ctx->ev_used; ++i) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev_start[(size_t)i], ctx->ev_stop[(size_t)i]));
        sum += ms;
    }
    *beam_kernel_ms = sum;
    *n_launches = ctx->ev_used;
    ctx->ev_used = 0;
    return SNOWGPU_OK;
}

// Camera-FOV crop of augment(only_camera_fov=True) (simulation.py:39-47, :532-540): lidar_to_rect with
// Tr_velo_to_cam (3 x 4) and R0_rect (3 x 3), rect_to_img with P2 (3 x 4), image img_h x img_w ((1024, 1920) in the
// reference).  The crop is applied by the compaction of every later batch of this context (and num_removed counts it,
// :538) until it is switched off again.  The reference's own projection code is un-vendored: textbook KITTI, float64.
// precompute.py:96-99 crops every frame to the camera's view BEFORE augment() sees it.  With this switch on (and a crop set
// by snowgpu_set_fov) the host-pointer entry snowgpu_augment_batch does the same on the device, right after the upload;
// statistics and out_src then refer to what augment() would have been given / to rows of the original frame.
extern "C" int snowgpu_set_fov_precrop(snowgpu_ctx *ctx, int on)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    ctx->fov_pre = on ? 1 : 0;
    return SNOWGPU_OK;
}

// the crop's matrices as the kernels take them (snowgpu_set_fov, snowgpu_fov_mask_device)
SgFov make_fov(const double *v2c, const double *r0, const double *p2, int img_h, int img_w)
{
    SgFov f{};
    f.enabled = 1;
    for (int i = 0; i < 4; ++i)                      // M = V2C^T . R0^T  (4 x 3)
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc = acc + v2c[4 * k + i] * r0[3 * j + k];
            f.m[3 * i + j] = acc;
        }
    for (int i = 0; i < 12; ++i) f.p[i] = p2[i];
    f.img_h = img_h; f.img_w = img_w;
    return f;
}

extern "C" int snowgpu_set_fov(snowgpu_ctx *ctx, int enabled, const double *v2c, const double *r0, const double *p2, int img_h, int img_w)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (!enabled) { ctx->fov.enabled = 0; return SNOWGPU_OK; }
    if (!v2c || !r0 || !p2 || img_h <= 0 || img_w <= 0) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_fov: need V2C, R0, P2 and an image size");
    ctx->fov = make_fov(v2c, r0, p2, img_h, img_w);
    return SNOWGPU_OK;
}

// ---- ground plane (tools/wet_ground/planes.py:12-50) -------------------------------------------------------------------
extern "C" int snowgpu_set_plane_method(snowgpu_ctx *ctx, int method, uint64_t seed, int max_trials, int min_rows, double standard_height)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (method < SG_PLANE_REFERENCE || method > SG_PLANE_RANSAC || max_trials < 0 || max_trials > (1 << 16) || min_rows < 0)
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_plane_method: method 0 (reference), 1 (least squares) or 2 (ransac); 0 <= trials <= 65536");
    ctx->plane_par.method = method;
    ctx->plane_par.seed = seed;
    ctx->plane_par.trials = max_trials > 0 ? max_trials : 1024;
    ctx->plane_par.min_rows = min_rows;
    ctx->plane_par.std_height = standard_height;
    return SNOWGPU_OK;
}

extern "C" int snowgpu_set_threshold_callback(snowgpu_ctx *ctx, snowgpu_threshold_fn fn, void *user)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    ctx->thr_fn = fn; ctx->thr_user = fn ? user : nullptr;
    return SNOWGPU_OK;
}
