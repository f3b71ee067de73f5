// snowgpu_device.cpp -- the entries of the C ABI (include/snowgpu.h) that take DEVICE pointers and enqueue on the caller's stream: every
// *_batch_device* entry, the plane estimate, the FOV mask and the weather draw.  Each batch entry fills an SgDeviceArgs, has it checked
// (sg_device_args.h: every refusal, in one order), sets the device and runs batch_from_args() and the stages it needs.  The launch
// sequence of a batch is snowgpu_batch.cpp, the stage entries (outlier filter, voxels, keypoints, ... anchor targets) are
// snowgpu_stages.cpp; no host copy, no synchronisation, no allocation after the first call of a given size.
#include "sg_host.h"
#include "sg_launch.h"      // sg_tiles
#include "sg_weather.h"     // SgWeatherDraw and the limits of the draw

static_assert(SG_ARGS_INVALID == SNOWGPU_E_INVALID && SG_PLANE_REFERENCE == 0, "sg_device_args.h restates these two");

static int check_args(snowgpu_ctx *ctx, const SgDeviceArgs &a, const SgEntryShape &s)
{
    const snowgpu_ctx *R = ctx->root ? ctx->root : ctx;
    std::string msg;
    const int rc = sg_check_device_args(a, SgCtxView{ctx->thr_fn != nullptr, ctx->result_mode, ctx->plane_par.method, R->tables.size()}, s, &msg);
    return rc ? fail(ctx, rc, msg) : SNOWGPU_OK;
}

// what the entries with a snowfall stage take alike, in the order they take it
static SgDeviceArgs snow_args(const char *who, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets, const void *d_rows,
                              int dtype, const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly, const double *d_plane,
                              double noise_floor, const int32_t *d_perm, void *d_out_rows, int64_t *d_out_counts, int64_t *d_out_stats,
                              double *d_out_thr_poly, int32_t *d_status, void *stream)
{
    SgDeviceArgs a{};
    a.who = who; a.n_frames = n_frames; a.n_total = n_total; a.max_frame_rows = max_frame_rows; a.dtype = dtype;
    a.frame_off = d_frame_offsets; a.rows = d_rows; a.table_ids = d_table_ids; a.beam_div_deg = beam_divergence_deg;
    a.thr_poly = d_thr_poly; a.plane = d_plane; a.noise_floor = noise_floor; a.perm = d_perm; a.out_rows = d_out_rows;
    a.out_counts = d_out_counts; a.out_stats = d_out_stats; a.out_thr_poly = d_out_thr_poly; a.status = d_status; a.stream = stream;
    return a;
}

static void wet_args(SgDeviceArgs &a, const double *d_wet_plane, double water_height, double pavement_depth, double noise_floor, double power_factor,
                     int flat_earth, double delta, int replace, int32_t *d_out_flags)
{
    a.wet_plane = d_wet_plane; a.wet = SgWetScalars{water_height, pavement_depth, noise_floor, power_factor, delta, flat_earth, replace};
    a.out_flags = d_out_flags;
}

// a masked batch runs without the frame-uniform shortcut: n_total and max_frame are upper bounds to what the front end leaves
static BatchDev batch_from_args(snowgpu_ctx *ctx, const SgDeviceArgs &a, const SgEntryShape &s)
{
    BatchDev b{};
    b.n_frames = a.n_frames; b.n_total = a.n_total; b.max_frame = sg_max_frame(a.max_frame_rows, a.n_total);
    b.uniform_rows = s.masked ? 0 : sg_uniform_rows(a.max_frame_rows, a.n_frames, a.n_total);
    b.frame_off = a.frame_off; b.rows = a.rows; b.dtype = a.dtype; b.table_ids = a.table_ids; b.beam_div_deg = a.beam_div_deg;
    b.thr_poly = a.thr_poly; b.plane = a.plane; b.noise_floor = a.noise_floor; b.perm = a.perm;
    b.out_rows = a.out_rows; b.out_src = a.out_src; b.out_keep = a.out_keep;
    b.out_counts = a.out_counts; b.out_stats = a.out_stats; b.out_thr_poly = a.out_thr_poly; b.status = a.status;
    b.stream = a.stream ? (hipStream_t)a.stream : ctx->stream;
    return b;
}

// The wet settings of one call: the scalars, the context's estimation method and seed, the fit's export -- and, with take_lines, the
// caller's lines (snowgpu_set_wet_lines: one use; the upload is waited for on `st`: they leave the context here).
int wet_settings(snowgpu_ctx *ctx, const SgWetScalars &w, int n_frames, bool take_lines, hipStream_t st, SgWetParams *wp)
{
    *wp = SgWetParams{};
    wp->water_height = w.water_height; wp->pavement_depth = w.pavement_depth; wp->noise_floor = w.noise_floor;
    wp->power_factor = w.power_factor; wp->flat_earth = w.flat_earth; wp->delta = w.delta; wp->replace = w.replace;
    wp->estimation = ctx->wet_estimation; wp->seed = ctx->wet_seed;
    ENSURE(ctx, ctx->wet_fit, (size_t)n_frames * 8);
    wp->fit_out = ctx->wet_fit.p; ctx->wet_fit_frames = n_frames;
    if (!take_lines || ctx->wet_lines.empty()) return SNOWGPU_OK;
    if (ctx->wet_estimation != 0) { ctx->wet_lines.clear(); return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_wet_lines supplies LINES: not with estimation method 'poly'"); }
    if (ctx->wet_lines.size() != (size_t)n_frames * 4) { ctx->wet_lines.clear(); return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_wet_lines was given another number of frames"); }
    ENSURE(ctx, ctx->d_wet_lines, ctx->wet_lines.size());
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_wet_lines.p, ctx->wet_lines.data(), sizeof(double) * ctx->wet_lines.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    wp->lines = ctx->d_wet_lines.p;
    ctx->wet_lines.clear();
    return SNOWGPU_OK;
}

static int wet_error(snowgpu_ctx *ctx, const char *what, int e)
{
    return fail(ctx, SNOWGPU_E_HIP, std::string(what) + (e > 0 ? hipGetErrorString((hipError_t)e) : "allocation"));
}

// The snowfall stage of a masked batch, on b.stream.  Front end: the present rows of every frame are compacted, stably, into context
// scratch (rows_crop, crop_src) at offsets made on the device (crop_off); the absent rows' keep bytes -- and, out of place, their rows --
// are written on the way.  Then run_batch on that scratch: every kernel of the unmasked call, untouched, on the batch the caller would have
// had to compact.  Its last step is the masked aligned finish.
// d_weather (optional): the snow gate of every frame is part of the mask (d_keep_in may then be NULL); see sg_launch_mask_front.
static int masked_snow_stage(snowgpu_ctx *ctx, BatchDev &b, const uint8_t *d_keep_in, const double *d_weather)
{
    const size_t n = (size_t)b.n_total, esz = b.dtype == 0 ? 4 : 8;
    const int64_t max_tiles = sg_tiles(b.max_frame);
    ENSURE(ctx, ctx->ctile_cnt, (size_t)b.n_frames * (size_t)max_tiles + 1);
    ENSURE(ctx, ctx->ctile_base, (size_t)b.n_frames * (size_t)max_tiles + 1);
    ENSURE(ctx, ctx->crop_counts, (size_t)b.n_frames);
    ENSURE(ctx, ctx->crop_off, (size_t)b.n_frames + 1);
    ENSURE(ctx, ctx->rows_crop, n * 5 * esz);
    ENSURE(ctx, ctx->crop_src, n);
    int e = sg_launch_mask_front(b.rows, b.dtype, d_keep_in, d_weather, b.frame_off, b.n_frames, b.out_rows == b.rows ? nullptr : b.out_rows, b.out_keep,
                                 ctx->ctile_cnt.p, ctx->ctile_base.p, ctx->crop_counts.p, ctx->crop_off.p, ctx->rows_crop.p, ctx->crop_src.p, max_tiles, b.stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("mask front end launch: ") + hipGetErrorString((hipError_t)e));
    b.mask_in_off = b.frame_off; b.mask_map = ctx->crop_src.p; b.weather = d_weather;
    b.rows = ctx->rows_crop.p; b.frame_off = ctx->crop_off.p;
    return run_batch(ctx, b);
}

// The aligned wet stage of `a` on `st`, reading d_rows / d_keep_in (the caller's, or the snowfall stage's result: then in place): the
// context's wet settings, the plane (the caller's, or the constant one of the plane method `reference`) and sg_wet_run_aligned.
static int aligned_wet_stage(snowgpu_ctx *ctx, const SgDeviceArgs &a, const void *d_rows, const uint8_t *d_keep_in, int64_t max_frame, hipStream_t st)
{
    SgWetParams wp;
    if (int rc = wet_settings(ctx, a.wet, a.n_frames, true, st, &wp)) return rc;
    wp.weather = a.weather;
    const double *d_plane = a.wet_plane;
    if (!d_plane) {
        std::string msg;
        if (int rc = sg_check_wet_plane(a.who, d_plane, ctx->plane_par.method, &msg)) return fail(ctx, rc, msg);
        ENSURE(ctx, ctx->wet_plane_est, (size_t)a.n_frames * 4);
        int e = sg_plane_run(&ctx->plane_scr, &ctx->plane_par, d_rows, a.dtype, a.frame_off, nullptr, a.n_frames, a.n_total, max_frame, ctx->wet_plane_est.p, nullptr, st);
        if (e) return wet_error(ctx, "plane estimate: ", e);
        d_plane = ctx->wet_plane_est.p;
    }
    int e = sg_wet_run_aligned(&ctx->prepass, d_rows, a.dtype, a.frame_off, d_keep_in, a.n_frames, a.n_total, max_frame, d_plane, &wp, a.out_rows,
                               a.out_keep, a.out_counts, a.out_flags, a.status, st);
    return e ? wet_error(ctx, "wet ground: ", e) : SNOWGPU_OK;
}

// a batch without rows: nothing kept, every frame "returned as it came" (what an empty frame inside a batch reports)
static int aligned_wet_empty(snowgpu_ctx *ctx, const SgDeviceArgs &a, hipStream_t st)
{
    HIPCHK(ctx, hipMemsetAsync(a.out_counts, 0, sizeof(int64_t) * (size_t)a.n_frames, st));
    HIPCHK(ctx, hipMemsetD32Async((hipDeviceptr_t)a.out_flags, 1, (size_t)a.n_frames, st));
    return SNOWGPU_OK;
}

// Every aligned entry behind its argument fill: the check, the device, the snowfall stage (masked or not), the wet stage in place on its
// result (d_out_counts: the snowfall stage's counts are overwritten by the wet stage's, which count what is left of them).
static int run_aligned(snowgpu_ctx *ctx, const SgDeviceArgs &a, const SgEntryShape &s)
{
    if (int rc = check_args(ctx, a, s)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    BatchDev b = batch_from_args(ctx, a, s);
    const bool masked = s.masked && a.n_total > 0;        // (no row at all: the unmasked chain's answer)
    if (int rc = masked ? masked_snow_stage(ctx, b, a.keep_in, a.weather) : run_batch(ctx, b)) return rc;
    if (!s.wet) return SNOWGPU_OK;
    if (a.n_total > 0) return aligned_wet_stage(ctx, a, a.out_rows, a.out_keep, b.max_frame, b.stream);
    if (int rc = aligned_wet_empty(ctx, a, b.stream)) return rc;
    if (!a.weather) return SNOWGPU_OK;                    // with "not asked" where the wet gate is off
    int e = sg_launch_weather_flags(a.weather, a.n_frames, a.out_flags, b.stream);
    return e ? fail(ctx, SNOWGPU_E_HIP, std::string("weather flags launch: ") + hipGetErrorString((hipError_t)e)) : SNOWGPU_OK;
}

extern "C" int snowgpu_augment_batch_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                            const int64_t *d_frame_offsets,
                                            const void *d_rows, int dtype, const int32_t *d_table_ids,
                                            double beam_divergence_deg, const double *d_thr_poly, const double *d_plane,
                                            double noise_floor, const int32_t *d_perm, void *d_out_rows, int32_t *d_out_src,
                                            int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly,
                                            int32_t *d_status, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    SgDeviceArgs a = snow_args("snowgpu_augment_batch_device", n_frames, n_total, max_frame_rows, d_frame_offsets, d_rows, dtype, d_table_ids, beam_divergence_deg,
                               d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows, d_out_counts, d_out_stats, d_out_thr_poly, d_status, stream);
    a.out_src = d_out_src;
    if (int rc = check_args(ctx, a, SG_SHAPE_COMPACT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    BatchDev b = batch_from_args(ctx, a, SG_SHAPE_COMPACT);
    return run_batch(ctx, b);
}

// snowgpu_augment_batch_device with the ALIGNED result layout: every row of the input comes back at its own index (d_out_rows, which may be
// d_rows itself), d_out_keep says which of them the reference would have returned.  Same launch sequence up to the last step, which is one
// kernel (k_finish_aligned) instead of the three of the compaction.
extern "C" int snowgpu_augment_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                    const int64_t *d_frame_offsets, const void *d_rows, int dtype, const int32_t *d_table_ids,
                                                    double beam_divergence_deg, const double *d_thr_poly, const double *d_plane,
                                                    double noise_floor, const int32_t *d_perm, void *d_out_rows, uint8_t *d_out_keep,
                                                    int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly,
                                                    int32_t *d_status, void *stream)
{
    return snowgpu_augment_batch_device_aligned_masked(ctx, n_frames, n_total, max_frame_rows, d_frame_offsets, d_rows, dtype, d_table_ids, beam_divergence_deg,
                                                       d_thr_poly, d_plane, noise_floor, d_perm, nullptr, d_out_rows, d_out_keep, d_out_counts, d_out_stats,
                                                       d_out_thr_poly, d_status, stream);      // (all present)
}

// augment() followed by ground_water_augmentation() on its output (pointcloud_viewer.py:2807-2821) as ONE launch
// sequence on the caller's stream: the snowfall rows are compacted into context scratch, the wet-ground kernels read
// them there (rows of frame f: [off[f], off[f] + snowfall count[f])), and the wet scatter composes the source indices
// (final row -> snowfall row -> input row) as it writes them.  Lines left by snowgpu_set_wet_lines are not looked at.
extern "C" int snowgpu_augment_wet_batch_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                                const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                                const double *d_plane, double noise_floor, const int32_t *d_perm,
                                                const double *d_wet_plane, double water_height, double pavement_depth,
                                                double wet_noise_floor, double power_factor, int flat_earth, double delta, int replace,
                                                double *d_out_rows, int32_t *d_out_src, int64_t *d_out_counts, int64_t *d_out_stats,
                                                int32_t *d_out_flags, int32_t *d_status, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    SgDeviceArgs a = snow_args("snowgpu_augment_wet_batch_device", n_frames, n_total, max_frame_rows, d_frame_offsets, d_rows, dtype, d_table_ids,
                               beam_divergence_deg, d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows, d_out_counts, d_out_stats, nullptr, d_status, stream);
    a.out_src = d_out_src;
    wet_args(a, d_wet_plane, water_height, pavement_depth, wet_noise_floor, power_factor, flat_earth, delta, replace, d_out_flags);
    if (int rc = check_args(ctx, a, SG_SHAPE_COMPACT_WET)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t esz = dtype == 0 ? 4 : 8, n = (size_t)n_total;
    ENSURE(ctx, ctx->snow_rows, std::max<size_t>(n * 5 * esz, 8));
    ENSURE(ctx, ctx->snow_src, std::max<size_t>(n, 1));
    ENSURE(ctx, ctx->snow_counts, (size_t)n_frames);
    BatchDev b = batch_from_args(ctx, a, SG_SHAPE_COMPACT_WET);
    b.out_rows = ctx->snow_rows.p; b.out_src = ctx->snow_src.p; b.out_counts = ctx->snow_counts.p;      // the snowfall result stays in the context
    if (int rc = run_batch(ctx, b)) return rc;
    if (n == 0) {
        HIPCHK(ctx, hipMemsetAsync(d_out_counts, 0, sizeof(int64_t) * (size_t)n_frames, b.stream));
        HIPCHK(ctx, hipMemsetAsync(d_out_flags, 0, sizeof(int32_t) * (size_t)n_frames, b.stream));
        return SNOWGPU_OK;
    }
    SgWetParams wp;
    if (int rc = wet_settings(ctx, a.wet, n_frames, false, b.stream, &wp)) return rc;
    wp.src_first = ctx->snow_src.p;
    int e = 0;
    if (!d_wet_plane) {      // wet_ground/augmentation.py:41 calculate_plane(pointcloud) -- here the snowfall result -- on the device
        ENSURE(ctx, ctx->wet_plane_est, (size_t)n_frames * 4);
        e = sg_plane_run(&ctx->plane_scr, &ctx->plane_par, ctx->snow_rows.p, dtype, d_frame_offsets, ctx->snow_counts.p, n_frames, n_total, b.max_frame,
                         ctx->wet_plane_est.p, nullptr, b.stream);
        d_wet_plane = ctx->wet_plane_est.p;
    }
    if (!e) e = sg_wet_run(&ctx->prepass, ctx->snow_rows.p, dtype, d_frame_offsets, ctx->snow_counts.p, n_frames, n_total, b.max_frame,
                       d_wet_plane, &wp, d_out_rows, d_out_src, d_out_counts, d_out_flags, d_status, b.stream);
    return e ? wet_error(ctx, "wet ground: ", e) : SNOWGPU_OK;
}

// ground_water_augmentation() on frames in DEVICE memory with the aligned result: the wet model on its own, which is also the second half
// of the fused aligned entries below.
extern "C" int snowgpu_wet_ground_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                       const int64_t *d_frame_offsets, const void *d_rows, int dtype, const uint8_t *d_keep_in,
                                                       const double *d_plane, double water_height, double pavement_depth, double noise_floor,
                                                       double power_factor, int flat_earth, double delta, int replace, void *d_out_rows,
                                                       uint8_t *d_out_keep, int64_t *d_out_counts, int32_t *d_out_flags, int32_t *d_status,
                                                       void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    SgDeviceArgs a = snow_args("snowgpu_wet_ground_batch_device_aligned", n_frames, n_total, max_frame_rows, d_frame_offsets, d_rows, dtype, nullptr, 0.0,
                               nullptr, nullptr, 0.0, nullptr, d_out_rows, d_out_counts, nullptr, nullptr, d_status, stream);
    a.keep_in = d_keep_in; a.out_keep = d_out_keep;
    wet_args(a, d_plane, water_height, pavement_depth, noise_floor, power_factor, flat_earth, delta, replace, d_out_flags);
    if (int rc = check_args(ctx, a, SG_SHAPE_WET_ONLY)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(d_status, 0, sizeof(int32_t) * 8, st));
    if (n_total == 0) return aligned_wet_empty(ctx, a, st);
    return aligned_wet_stage(ctx, a, d_rows, d_keep_in, sg_max_frame(max_frame_rows, n_total), st);
}

// augment() followed by ground_water_augmentation() (pointcloud_viewer.py:2807-2821) with the aligned result, as ONE launch sequence on the
// caller's stream: run_batch with the aligned finish into d_out_rows / d_out_keep, then the wet stage IN PLACE on those two arrays.  No
// compaction, no snow_rows / snow_src / snow_counts scratch, no source indices to compose.
extern "C" int snowgpu_augment_wet_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                        const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                                        const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                                        const double *d_plane, double noise_floor, const int32_t *d_perm, void *d_out_rows,
                                                        uint8_t *d_out_keep, int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly,
                                                        int32_t *d_status, void *stream, const double *d_wet_plane, double water_height,
                                                        double pavement_depth, double wet_noise_floor, double power_factor, int flat_earth,
                                                        double delta, int replace, int32_t *d_out_flags)
{
    return snowgpu_augment_wet_batch_device_aligned_masked(ctx, n_frames, n_total, max_frame_rows, d_frame_offsets, d_rows, dtype, d_table_ids, beam_divergence_deg,
                                                           d_thr_poly, d_plane, noise_floor, d_perm, nullptr, d_out_rows, d_out_keep, d_out_counts, d_out_stats,
                                                           d_out_thr_poly, d_status, stream, d_wet_plane, water_height, pavement_depth, wet_noise_floor,
                                                           power_factor, flat_earth, delta, replace, d_out_flags);      // (all present)
}

// snowgpu_augment_batch_device_aligned with an input keep mask (snowgpu_mask.hip): a row whose d_keep_in byte is 0 is not there.  See
// include/snowgpu.h.  Without a mask, or without rows, all are present: that IS the unmasked call, checked and refused under its name.
extern "C" int snowgpu_augment_batch_device_aligned_masked(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                           const int64_t *d_frame_offsets, const void *d_rows, int dtype, const int32_t *d_table_ids,
                                                           double beam_divergence_deg, const double *d_thr_poly, const double *d_plane,
                                                           double noise_floor, const int32_t *d_perm, const uint8_t *d_keep_in, void *d_out_rows,
                                                           uint8_t *d_out_keep, int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly,
                                                           int32_t *d_status, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const bool masked = d_keep_in && n_total != 0;
    SgDeviceArgs a = snow_args(masked ? "snowgpu_augment_batch_device_aligned_masked" : "snowgpu_augment_batch_device_aligned", n_frames, n_total, max_frame_rows,
                               d_frame_offsets, d_rows, dtype, d_table_ids, beam_divergence_deg, d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows, d_out_counts,
                               d_out_stats, d_out_thr_poly, d_status, stream);
    a.keep_in = masked ? d_keep_in : nullptr; a.out_keep = d_out_keep;
    return run_aligned(ctx, a, masked ? SG_SHAPE_MASKED : SG_SHAPE_ALIGNED);
}

// snowgpu_augment_wet_batch_device_aligned whose snowfall stage is the masked one; the wet stage runs in place on d_out_rows / d_out_keep
// as in the unmasked chain (absent rows carry keep 0 there: the wet stage treats them as not there, too).
extern "C" int snowgpu_augment_wet_batch_device_aligned_masked(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                               const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                                               const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                                               const double *d_plane, double noise_floor, const int32_t *d_perm,
                                                               const uint8_t *d_keep_in, void *d_out_rows, uint8_t *d_out_keep,
                                                               int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly, int32_t *d_status,
                                                               void *stream, const double *d_wet_plane, double water_height, double pavement_depth,
                                                               double wet_noise_floor, double power_factor, int flat_earth, double delta, int replace,
                                                               int32_t *d_out_flags)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const bool masked = d_keep_in && n_total != 0;
    SgDeviceArgs a = snow_args(masked ? "snowgpu_augment_wet_batch_device_aligned_masked" : "snowgpu_augment_wet_batch_device_aligned", n_frames, n_total,
                               max_frame_rows, d_frame_offsets, d_rows, dtype, d_table_ids, beam_divergence_deg, d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows,
                               d_out_counts, d_out_stats, d_out_thr_poly, d_status, stream);
    a.keep_in = masked ? d_keep_in : nullptr; a.out_keep = d_out_keep;
    wet_args(a, d_wet_plane, water_height, pavement_depth, wet_noise_floor, power_factor, flat_earth, delta, replace, d_out_flags);
    return run_aligned(ctx, a, masked ? SG_SHAPE_MASKED_WET : SG_SHAPE_ALIGNED_WET);
}

// ---- per-frame weather: gates and wet settings in device memory (include/snowgpu.h) ---------------------------------------------------
// The masked fused chain with d_weather in place of its five wet scalars.  The snow gate joins the input mask in the front end (a frame
// left out reaches run_batch empty and keeps its keep bytes), the wet gate and the wet settings are read per frame by the wet kernels.
// Because the gates are device data the masked front end always runs, with or without d_keep_in.
extern "C" int snowgpu_augment_weather_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                            const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                                            const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                                            const double *d_plane, double noise_floor, const int32_t *d_perm,
                                                            const uint8_t *d_keep_in, void *d_out_rows, uint8_t *d_out_keep,
                                                            int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly, int32_t *d_status,
                                                            void *stream, const double *d_wet_plane, const double *d_weather, int flat_earth,
                                                            int replace, int32_t *d_out_flags)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    SgDeviceArgs a = snow_args("snowgpu_augment_weather_batch_device_aligned", n_frames, n_total, max_frame_rows, d_frame_offsets, d_rows, dtype, d_table_ids,
                               beam_divergence_deg, d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows, d_out_counts, d_out_stats, d_out_thr_poly, d_status, stream);
    a.keep_in = d_keep_in; a.out_keep = d_out_keep; a.weather = d_weather;
    wet_args(a, d_wet_plane, 0.0, 1.0, 0.0, 0.0, flat_earth, 0.0, replace, d_out_flags);
    return run_aligned(ctx, a, SG_SHAPE_WEATHER);
}

extern "C" int snowgpu_estimate_planes_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                              const int64_t *d_frame_offsets, const void *d_rows, int dtype, double *d_out_planes,
                                              int32_t *d_out_info, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || n_total < 0 || !d_frame_offsets || (n_total > 0 && !d_rows) || !d_out_planes || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_estimate_planes_device: null pointer or bad dtype");
    if (n_total >= ((int64_t)1 << 31)) return fail(ctx, SNOWGPU_E_INVALID, "batch too large: split it below 2^31 rows");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int e = sg_plane_run(&ctx->plane_scr, &ctx->plane_par, d_rows, dtype, d_frame_offsets, nullptr, n_frames, n_total, sg_max_frame(max_frame_rows, n_total),
                         d_out_planes, d_out_info, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("plane estimate: ") + (e > 0 ? hipGetErrorString((hipError_t)e) : "allocation"));
    return SNOWGPU_OK;
}

// The camera-FOV test as a producer of a keep mask: d_out_keep[i] = (d_keep_in ? d_keep_in[i] : 1) && get_fov_flag(row i), matrices and
// image size as snowgpu_set_fov takes them (the context's own crop setting is neither read nor changed).  See include/snowgpu.h.
extern "C" int snowgpu_fov_mask_device(snowgpu_ctx *ctx, int64_t n_total, const void *d_rows, int dtype, const double *v2c, const double *r0,
                                       const double *p2, int img_h, int img_w, const uint8_t *d_keep_in, uint8_t *d_out_keep, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_total < 0 || (n_total > 0 && (!d_rows || !d_out_keep)) || !v2c || !r0 || !p2 || img_h <= 0 || img_w <= 0 || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_fov_mask_device: need rows, V2C, R0, P2, an image size and an output mask");
    {
        const uint8_t *k = d_keep_in, *ok = d_out_keep;
        if (k && ok != k && ok < k + (size_t)n_total && k < ok + (size_t)n_total)
            return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_fov_mask_device: d_out_keep overlaps d_keep_in; pass d_keep_in itself or a buffer apart from it");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SgFov f = make_fov(v2c, r0, p2, img_h, img_w);
    int e = sg_launch_fov_mask(d_rows, dtype, n_total, d_keep_in, d_out_keep, &f, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("fov mask launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Which weather each frame gets, drawn on the device (snowgpu_weather.hip, sg_weather.h).  See include/snowgpu.h.
extern "C" int snowgpu_draw_weather_device(snowgpu_ctx *ctx, int n_frames, int n_lasers, int n_sets, const int32_t *d_set_ids,
                                           const snowgpu_weather_plan *plan, uint64_t seed, const uint64_t *d_step, int32_t *d_table_ids,
                                           double *d_weather, void *stream)
{
    static const char *who = "snowgpu_draw_weather_device";
    if (!ctx) return SNOWGPU_E_INVALID;
    if (!plan || !d_set_ids || !d_step || !d_table_ids || !d_weather) return fail(ctx, SNOWGPU_E_INVALID, std::string(who) + ": null pointer");
    if (n_frames <= 0 || n_frames > (1 << 22) || n_lasers <= 0 || n_lasers > SG_WEATHER_MAX_LASERS || n_sets <= 0 || n_sets > SG_WEATHER_MAX_SETS ||
        plan->n_water <= 0 || plan->n_water > SG_WEATHER_MAX_CHOICES || plan->n_pave <= 0 || plan->n_pave > SG_WEATHER_MAX_CHOICES)
        return fail(ctx, SNOWGPU_E_INVALID, std::string(who) + ": needs 1 .. 2^22 frames, 1 .. 128 lasers, 1 .. 64 table sets, 1 .. 16 water heights and pavement depths");
    if (!(plan->p_snow >= 0.0 && plan->p_snow <= 1.0) || !(plan->p_wet >= 0.0 && plan->p_wet <= 1.0))
        return fail(ctx, SNOWGPU_E_INVALID, std::string(who) + ": p_snow and p_wet are probabilities");
    auto threshold = [](double p) { const double t = std::floor(p * 4294967296.0); return t >= 4294967296.0 ? (uint64_t)1 << 32 : (uint64_t)t; };
    SgWeatherDraw d{};
    d.t_snow = threshold(plan->p_snow); d.t_wet = threshold(plan->p_wet);
    d.n_sets = n_sets; d.n_lasers = n_lasers; d.n_water = plan->n_water; d.n_pave = plan->n_pave; d.shuffle = plan->shuffle ? 1 : 0;
    for (int i = 0; i < plan->n_water; ++i) d.water[i] = plan->water_heights[i];
    for (int i = 0; i < plan->n_pave; ++i) d.pave[i] = plan->pavement_depths[i];
    d.wet_noise_floor = plan->wet_noise_floor; d.power_factor = plan->power_factor; d.delta = plan->delta;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int e = sg_launch_draw_weather(&d, n_frames, seed, d_step, d_set_ids, d_table_ids, d_weather, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("weather draw launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}
