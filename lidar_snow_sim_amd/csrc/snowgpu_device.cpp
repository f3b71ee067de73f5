// snowgpu_device.cpp -- the entries of the C ABI (include/snowgpu.h) that take DEVICE pointers and enqueue on the caller's stream: every
// *_batch_device* entry, the plane estimate, the FOV mask, the outlier filter, the voxel stage, the keypoint stage and its sectorized form, the ball query, the range image, the nearest centres, the points in boxes, the RoI point pooling, the RoI-aware voxel pooling, the box IoU and NMS, the proposal target sampling, the anchor target assignment and the weather draw.  Each batch entry fills an SgDeviceArgs, has it checked
// (sg_device_args.h: every refusal, in one order), sets the device and runs batch_from_args() and the stages it needs.  The launch
// sequence of a batch is snowgpu_batch.cpp; no host copy, no synchronisation, no allocation after the first call of a given size.
#include "sg_host.h"
#include "sg_launch.h"      // sg_tiles
#include "sg_weather.h"     // SgWeatherDraw and the limits of the draw
#include "sg_dror.h"        // the grid of the outlier filter and its domain
#include "sg_voxel.h"       // the grid of the voxel stage and the capacity of its tables
#include "sg_fps.h"         // the range of the keypoint stage and the size of its scratch
#include "sg_fps_sectors.h" // the scratch of the sectorized keypoint stage
#include "sg_ball.h"        // the grid of the ball query and the sizes of its scratch
#include "sg_nn.h"          // the grid of the nearest-centres stage and the sizes of its scratch
#include "sg_box.h"         // the record of a box and the sizes of the box stage's scratch
#include "sg_roipool.h"     // the enlarged roi and the size of the pooling stage's run table
#include "sg_roiaware.h"    // the limits of the RoI-aware voxel pooling and the sizes of its lists
#include "sg_iou.h"         // the record of the IoU and NMS stages and the size of their scratch
#include "sg_range.h"       // the geometry of the range image and the limits in the rows' dtype
#include "sg_targets.h"     // SgTargetCfg of the proposal target sampling
#include "sg_anchors.h"     // SgAnchorCfg and the record of the anchor target assignment

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

// Dynamic radius outlier removal as a producer of a keep mask (snowgpu_dror.hip; definition and grid: sg_dror.h).  See include/snowgpu.h.
extern "C" int snowgpu_dror_mask_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                        const void *d_rows, int dtype, double alpha_deg, double beta, double sr_min, int64_t k_min,
                                        const uint8_t *d_keep_in, uint8_t *d_out_keep, int32_t *d_out_neighbours, void *stream)
{
    static const char *who = "snowgpu_dror_mask_device";
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || n_total < 0 || !d_frame_offsets || (n_total > 0 && (!d_rows || !d_out_keep)) || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, std::string(who) + ": null pointer or bad dtype");
    if (n_total >= ((int64_t)1 << 31)) return fail(ctx, SNOWGPU_E_INVALID, "batch too large: split it below 2^31 rows");
    SgDrorGrid g{};
    if (sg_dror_make_grid(alpha_deg, beta, sr_min, k_min, sg_dror_cell_budget(sg_max_frame(max_frame_rows, n_total)), &g))
        return fail(ctx, SNOWGPU_E_INVALID, std::string(who) + ": needs 0 < beta alpha pi / 180 <= 0.25, a finite sr_min >= 0 and 0 <= k_min <= 65535");
    if (d_keep_in && (const uint8_t *)d_out_keep < d_keep_in + (size_t)n_total && d_keep_in < d_out_keep + (size_t)n_total)
        return fail(ctx, SNOWGPU_E_INVALID, std::string(who) + ": d_out_keep overlaps d_keep_in (or is it); the query of one row reads the keep-in bytes "
                                            "of other rows while out bytes are written: pass a buffer apart from it");
    if (n_total == 0) return SNOWGPU_OK;
    const size_t entries = (size_t)n_frames * (size_t)(g.cells + 1);
    if (entries >= ((size_t)1 << 31)) return fail(ctx, SNOWGPU_E_INVALID, std::string(who) + ": too many frames for the cell lists; split the batch");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)n_total;
    ENSURE(ctx, ctx->dror_entry, entries);
    ENSURE(ctx, ctx->dror_cell, n);
    ENSURE(ctx, ctx->dror_sorted, n * 3 * (dtype == 0 ? 4 : 8));
    int e = sg_launch_dror(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &g, ctx->dror_entry.p, ctx->dror_cell.p, ctx->dror_sorted.p,
                           d_out_keep, d_out_neighbours, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("dror launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Point-to-voxel grouping of an aligned batch (snowgpu_voxel.hip; the cell and the tables: sg_voxel.h).  See include/snowgpu.h.
extern "C" int snowgpu_voxelize_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                       const void *d_rows, int dtype, const double *range6, const double *size3, int max_points, int max_voxels,
                                       int n_features, const uint8_t *d_keep_in, void *d_out_voxels, int32_t *d_out_coords, int32_t *d_out_num_points,
                                       int32_t *d_out_voxel_offsets, int32_t *d_out_voxel_of, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgVoxelArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, range6, size3, max_points, max_voxels, n_features, d_keep_in,
                        d_out_voxels, d_out_coords, d_out_num_points, d_out_voxel_offsets, d_out_voxel_of};
    SgVoxelGrid g{};
    {
        std::string msg;
        if (int rc = sg_check_voxel_args(a, g.n, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (n_total == 0) {                                // no row: no voxel, and nothing else is launched
        HIPCHK(ctx, hipMemsetAsync(d_out_voxel_offsets, 0, sizeof(int32_t) * ((size_t)n_frames + 1), st));
        return SNOWGPU_OK;
    }
    for (int j = 0; j < 3; ++j) { g.lo[j] = range6[j]; g.size[j] = size3[j]; }
    g.max_points = max_points; g.max_voxels = max_voxels; g.n_features = n_features;
    g.cap = sg_voxel_capacity(sg_max_frame(max_frame_rows, n_total));
    g.shift = sg_voxel_shift(g.cap);
    const size_t n = (size_t)n_total, tiles = (n + 1023) / 1024;
    ENSURE(ctx, ctx->vox_table, (size_t)n_frames * (size_t)g.cap);
    ENSURE(ctx, ctx->vox_slot, n);
    ENSURE(ctx, ctx->vox_order, n);
    ENSURE(ctx, ctx->vox_first, n);
    ENSURE(ctx, ctx->vox_tile_cnt, tiles);
    ENSURE(ctx, ctx->vox_tile_base, tiles + 1);
    ENSURE(ctx, ctx->vox_fbase, (size_t)n_frames);
    ENSURE(ctx, ctx->vox_m, (size_t)n_frames);
    ENSURE(ctx, ctx->vox_span, (size_t)n_frames * (size_t)max_voxels);
    int e = sg_launch_voxelize(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &g, ctx->vox_table.p, ctx->vox_slot.p, ctx->vox_first.p,
                               ctx->vox_order.p, ctx->vox_tile_cnt.p, ctx->vox_tile_base.p, ctx->vox_fbase.p, ctx->vox_m.p, ctx->vox_span.p, d_out_voxels,
                               d_out_coords, d_out_num_points, d_out_voxel_offsets, d_out_voxel_of, st);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("voxelize launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Farthest-point keypoints of an aligned batch (snowgpu_fps.hip; the usable test, the distance and the candidate key: sg_fps.h).  See
// include/snowgpu.h.
extern "C" int snowgpu_fps_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets, const void *d_rows,
                                  int dtype, const double *range6, int n_samples, int n_features, const uint8_t *d_keep_in, int32_t *d_out_index,
                                  void *d_out_points, void *d_out_dist, int32_t *d_out_usable, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgFpsArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, range6, n_samples, n_features, d_keep_in,
                      d_out_index, d_out_points, d_out_dist, d_out_usable};
    {
        std::string msg;
        if (int rc = sg_check_fps_args(a, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SgFpsRange r;
    for (int j = 0; j < 3; ++j) { r.lo[j] = range6 ? range6[j] : -INFINITY; r.hi[j] = range6 ? range6[3 + j] : INFINITY; }
    if (n_total > 0) {
        const size_t elems = sg_fps_scratch(n_total, n_frames), bytes = elems * (dtype == 0 ? 4 : 8);
        ENSURE(ctx, ctx->fps_x, bytes);
        ENSURE(ctx, ctx->fps_y, bytes);
        ENSURE(ctx, ctx->fps_z, bytes);
        ENSURE(ctx, ctx->fps_t, bytes);
        ENSURE(ctx, ctx->fps_src, elems);
    }
    int e = sg_launch_fps(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &r, n_samples, n_features, ctx->fps_x.p, ctx->fps_y.p, ctx->fps_z.p,
                          ctx->fps_t.p, ctx->fps_src.p, d_out_index, d_out_points, d_out_dist, d_out_usable, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("fps launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Sectorized, proposal-centric keypoints of an aligned batch (snowgpu_fps.hip; the reach, the sector, the quota and the layout of the
// scratch: sg_fps_sectors.h).  See include/snowgpu.h.
extern "C" int snowgpu_fps_sectors_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                          const void *d_rows, int dtype, const double *range6, int n_samples, int n_features, const uint8_t *d_keep_in,
                                          int n_sectors, const void *d_rois, int n_rois, int roi_features, double roi_margin, int32_t *d_out_index,
                                          void *d_out_points, void *d_out_dist, int32_t *d_out_usable, int32_t *d_out_sector_offsets,
                                          int32_t *d_out_sector_count, int8_t *d_out_sector_of, double *d_out_reach2, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgFpsSectorsArgs a{{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, range6, n_samples, n_features, d_keep_in, d_out_index,
                              d_out_points, d_out_dist, d_out_usable},
                             n_sectors, d_rois, n_rois, roi_features, roi_margin, d_out_sector_offsets, d_out_sector_count, d_out_sector_of, d_out_reach2};
    {
        std::string msg;
        if (int rc = sg_check_fps_sectors_args(a, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SgFpsRange r;
    for (int j = 0; j < 3; ++j) { r.lo[j] = range6 ? range6[j] : -INFINITY; r.hi[j] = range6 ? range6[3 + j] : INFINITY; }
    const int64_t max_frame = sg_max_frame(max_frame_rows, n_total);
    if (d_rois) ENSURE(ctx, ctx->fpss_roi, (size_t)n_frames * (size_t)n_rois * 4);
    if (n_total > 0) {
        const size_t elems = sg_fpss_scratch(n_total, n_frames), bytes = elems * (dtype == 0 ? 4 : 8);
        ENSURE(ctx, ctx->fps_x, bytes);
        ENSURE(ctx, ctx->fps_y, bytes);
        ENSURE(ctx, ctx->fps_z, bytes);
        ENSURE(ctx, ctx->fps_t, bytes);
        ENSURE(ctx, ctx->fps_src, elems);
        if (!d_out_sector_of) ENSURE(ctx, ctx->fpss_sec, (size_t)n_total);
        ENSURE(ctx, ctx->fpss_tile, (size_t)n_frames * (size_t)sg_tiles(max_frame) * (size_t)n_sectors);
        ENSURE(ctx, ctx->fpss_seg, (size_t)n_frames * (size_t)n_sectors);
    }
    int e = sg_launch_fps_sectors(d_rows, dtype, n_total, max_frame, d_frame_offsets, n_frames, d_keep_in, &r, n_samples, n_features, n_sectors, d_rois, n_rois,
                                  roi_features, roi_margin, ctx->fps_x.p, ctx->fps_y.p, ctx->fps_z.p, ctx->fps_t.p, ctx->fps_src.p, ctx->fpss_sec.p,
                                  ctx->fpss_roi.p, ctx->fpss_tile.p, ctx->fpss_seg.p, d_out_index, d_out_points, d_out_dist, d_out_usable, d_out_sector_offsets,
                                  d_out_sector_count, d_out_sector_of, d_out_reach2, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("sectorized fps launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Ball-query neighbour groups around centres (snowgpu_ball.hip; the grid, the window and the selection: sg_ball.h).  See include/snowgpu.h.
extern "C" int snowgpu_ball_query_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                         const void *d_rows, int dtype, const double *range6, int n_centres, const void *d_centres, int centre_features,
                                         int n_radii, const double *radii, const int *n_samples, int n_features, const uint8_t *d_keep_in,
                                         int32_t *d_out_index, int32_t *d_out_count, void *d_out_points, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const int32_t budget = sg_ball_cell_budget(sg_max_frame(max_frame_rows, n_total));
    const SgBallArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, range6, n_centres, d_centres, centre_features, n_radii, radii,
                       n_samples, n_features, d_keep_in, d_out_index, d_out_count, d_out_points, budget};
    {
        std::string msg;
        if (int rc = sg_check_ball_args(a, nullptr, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SgFpsRange r;
    for (int j = 0; j < 3; ++j) { r.lo[j] = range6 ? range6[j] : -INFINITY; r.hi[j] = range6 ? range6[3 + j] : INFINITY; }
    SgBallGrid g{};
    sg_ball_make_grid(range6, n_radii, radii, budget, &g);
    if (n_total > 0) {
        const size_t elems = sg_ball_scratch(n_total), bytes = elems * (dtype == 0 ? 4 : 8);
        ENSURE(ctx, ctx->ball_entry, sg_ball_entries(n_frames, budget));      // (by the budget, not the grid: the radii change no allocation)
        ENSURE(ctx, ctx->ball_cell, elems);
        ENSURE(ctx, ctx->ball_x, bytes);
        ENSURE(ctx, ctx->ball_y, bytes);
        ENSURE(ctx, ctx->ball_z, bytes);
        ENSURE(ctx, ctx->ball_src, elems);
    }
    int e = sg_launch_ball(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &r, &g, n_centres, d_centres, centre_features, n_radii, radii, n_samples,
                           n_features, ctx->ball_entry.p, ctx->ball_cell.p, ctx->ball_x.p, ctx->ball_y.p, ctx->ball_z.p, ctx->ball_src.p, d_out_index, d_out_count,
                           d_out_points, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("ball query launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Range-image projection of an aligned batch (snowgpu_range.hip; the pixel functions and the key: sg_range.h).  See include/snowgpu.h.
extern "C" int snowgpu_range_image_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                          const void *d_rows, int dtype, int height, int width, const double *fov2, const int32_t *d_ring,
                                          const double *limits2, int n_features, const uint8_t *d_keep_in, void *d_out_image, int32_t *d_out_index,
                                          int32_t *d_out_pixel_of, int32_t *d_out_count, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgRangeArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, height, width, fov2, d_ring, limits2, n_features, d_keep_in,
                        d_out_image, d_out_index, d_out_pixel_of, d_out_count};
    {
        std::string msg;
        if (int rc = sg_check_range_args(a, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SgRangeGeom g{};
    g.H = height; g.W = width; g.by_ring = d_ring ? 1 : 0;
    if (!d_ring) { g.fov_up = fov2[0]; g.fov_down = fov2[1]; }
    sg_range_limits(dtype, limits2, &g.lo, &g.hi);
    if (n_total > 0) ENSURE(ctx, ctx->range_key, (size_t)n_frames * (size_t)height * (size_t)width);
    int e = sg_launch_range(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, d_ring, &g, n_features, ctx->range_key.p, d_out_image, d_out_index,
                            d_out_pixel_of, d_out_count, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("range image launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Nearest centres of every row (snowgpu_nn.hip; the grid, the walk and its stopping bound: sg_nn.h).  See include/snowgpu.h.
extern "C" int snowgpu_nearest_centres_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                              const void *d_rows, int dtype, const double *range6, int n_centres, const void *d_centres, int centre_features,
                                              int k, const uint8_t *d_keep_in, int32_t *d_out_index, void *d_out_dist2, void *d_out_weight, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgNnArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, range6, n_centres, d_centres, centre_features, k, d_keep_in,
                     d_out_index, d_out_dist2, d_out_weight, SG_NN_MAX_CELLS};
    {
        std::string msg;
        if (int rc = sg_check_nn_args(a, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SgFpsRange r;
    for (int j = 0; j < 3; ++j) { r.lo[j] = range6 ? range6[j] : -INFINITY; r.hi[j] = range6 ? range6[3 + j] : INFINITY; }
    SgNnGrid g{};
    sg_nn_make_grid(range6, n_centres, &g);
    if (n_total > 0) {
        ENSURE(ctx, ctx->nn_entry, sg_nn_entries(n_frames, sg_nn_cell_budget(n_centres)));      // (by the budget, not the grid: the range changes no allocation)
        ENSURE(ctx, ctx->nn_box, sg_nn_boxes(n_frames));
        ENSURE(ctx, ctx->nn_rec, sg_nn_records(n_frames, n_centres) * (dtype == 0 ? sizeof(SgNnRec<float>) : sizeof(SgNnRec<double>)));
    }
    int e = sg_launch_nn(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &r, &g, n_centres, d_centres, centre_features, k, ctx->nn_entry.p,
                         ctx->nn_box.p, ctx->nn_rec.p, d_out_index, d_out_dist2, d_out_weight, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("nearest centres launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Points in 3D boxes (snowgpu_box.hip; presence, the record, the membership test, the grid and its footprint: sg_box.h).  See include/snowgpu.h.
extern "C" int snowgpu_points_in_boxes_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                              const void *d_rows, int dtype, int n_boxes, const void *d_boxes, int box_features, const double *d_pose_in,
                                              const uint8_t *d_keep_in, int32_t *d_out_box_of, int32_t *d_out_count, void *d_out_local, double *d_out_pose,
                                              void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgBoxArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, n_boxes, d_boxes, box_features, d_pose_in, d_keep_in,
                      d_out_box_of, d_out_count, d_out_local, d_out_pose};
    {
        std::string msg;
        if (int rc = sg_check_box_args(a, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->box_rec, sg_box_records(n_frames, n_boxes) * (sizeof(SgBoxRec) / sizeof(double)));
    ENSURE(ctx, ctx->box_table, sg_box_table(n_frames, n_boxes));
    int e = sg_launch_box(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, n_boxes, d_boxes, box_features, d_pose_in, (SgBoxRec *)ctx->box_rec.p,
                          ctx->box_table.p, d_out_box_of, d_out_count, d_out_local, d_out_pose, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("points in boxes launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// RoI point pooling (snowgpu_roipool.hip; the enlarged roi, the runs and the scratch: sg_roipool.h).  See include/snowgpu.h.
extern "C" int snowgpu_roi_point_pool_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                             const void *d_rows, int dtype, int n_rois, const void *d_rois, int roi_features, const double *extra_width3,
                                             int n_samples, int num_features, const double *d_pose_in, const uint8_t *d_keep_in, int32_t *d_out_index,
                                             int32_t *d_out_count, void *d_out_points, void *d_out_local, double *d_out_pose, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgRoiPoolArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, n_rois, d_rois, roi_features, extra_width3, n_samples, num_features,
                          d_pose_in, d_keep_in, d_out_index, d_out_count, d_out_points, d_out_local, d_out_pose};
    {
        std::string msg;
        if (int rc = sg_check_roipool_args(a, &msg)) return fail(ctx, rc, msg);
    }
    const double ew[3] = {extra_width3 ? extra_width3[0] : 0.0, extra_width3 ? extra_width3[1] : 0.0, extra_width3 ? extra_width3[2] : 0.0};
    const int64_t longest = sg_max_frame(max_frame_rows, n_total);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->roi_rec, sg_box_records(n_frames, n_rois) * (sizeof(SgBoxRec) / sizeof(double)));
    ENSURE(ctx, ctx->roi_table, sg_box_table(n_frames, n_rois));
    if (n_total > 0) ENSURE(ctx, ctx->roi_runs, sg_roi_table(n_frames, longest, n_rois));
    int e = sg_launch_roipool(d_rows, dtype, n_total, longest, d_frame_offsets, n_frames, d_keep_in, n_rois, d_rois, roi_features, ew, n_samples, num_features,
                              d_pose_in, (SgBoxRec *)ctx->roi_rec.p, ctx->roi_table.p, ctx->roi_runs.p, d_out_index, d_out_count, d_out_points, d_out_local,
                              d_out_pose, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("roi point pool launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// RoI-aware voxel pooling (snowgpu_roiaware.hip; the sub-voxel of a member and the scratch: sg_roiaware.h).  See include/snowgpu.h.
extern "C" int snowgpu_roi_voxel_pool_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                             const void *d_rows, int dtype, int n_rois, const void *d_rois, int roi_features, const double *extra_width3,
                                             const int32_t *out_size3, int max_points, int roi_capacity, const float *d_features, int feature_channels,
                                             const double *d_pose_in, const uint8_t *d_keep_in, int32_t *d_out_roi_count, int32_t *d_out_count,
                                             int32_t *d_out_index, float *d_out_max, int32_t *d_out_argmax, float *d_out_avg, double *d_out_pose, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgRoiAwareArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, n_rois, d_rois, roi_features, extra_width3, out_size3, max_points,
                           roi_capacity, d_features, feature_channels, d_pose_in, d_keep_in, d_out_roi_count, d_out_count, d_out_index, d_out_max, d_out_argmax,
                           d_out_avg, d_out_pose};
    {
        std::string msg;
        if (int rc = sg_check_roiaware_args(a, &msg)) return fail(ctx, rc, msg);
    }
    const double ew[3] = {extra_width3 ? extra_width3[0] : 0.0, extra_width3 ? extra_width3[1] : 0.0, extra_width3 ? extra_width3[2] : 0.0};
    const int32_t grid[3] = {out_size3[0], out_size3[1], out_size3[2]};
    const int64_t longest = sg_max_frame(max_frame_rows, n_total);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->rv_rec, sg_box_records(n_frames, n_rois) * (sizeof(SgBoxRec) / sizeof(double)));
    ENSURE(ctx, ctx->rv_table, sg_box_table(n_frames, n_rois));
    if (n_total > 0) {
        ENSURE(ctx, ctx->rv_runs, sg_roi_table(n_frames, longest, n_rois));
        ENSURE(ctx, ctx->rv_list, sg_roiaware_list(n_frames, n_rois, roi_capacity));
        ENSURE(ctx, ctx->rv_sorted, sg_roiaware_list(n_frames, n_rois, roi_capacity));
        ENSURE(ctx, ctx->rv_offset, sg_roiaware_offsets(n_frames, n_rois, grid[0] * grid[1] * grid[2]));
    }
    int e = sg_launch_roiaware(d_rows, dtype, n_total, longest, d_frame_offsets, n_frames, d_keep_in, n_rois, d_rois, roi_features, ew, grid, max_points, roi_capacity,
                               d_features, (d_features || d_out_max || d_out_argmax || d_out_avg) ? feature_channels : 1, d_pose_in, (SgBoxRec *)ctx->rv_rec.p, ctx->rv_table.p, ctx->rv_runs.p, ctx->rv_list.p,
                               ctx->rv_sorted.p, ctx->rv_offset.p, d_out_roi_count, d_out_count, d_out_index, d_out_max, d_out_argmax, d_out_avg, d_out_pose,
                               stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("roi voxel pool launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Rotated box IoU (snowgpu_iou.hip; presence, the record, the clip and the two IoUs: sg_iou.h).  See include/snowgpu.h.
extern "C" int snowgpu_boxes_iou_device(snowgpu_ctx *ctx, int n_frames, int n_a, const void *d_boxes_a, int a_features, int n_b, const void *d_boxes_b,
                                        int b_features, int dtype, int mode, const double *d_pose_a, const double *d_pose_b, void *d_out_iou,
                                        int32_t *d_out_best, void *d_out_best_iou, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgIouArgs a{n_frames, n_a, d_boxes_a, a_features, n_b, d_boxes_b, b_features, dtype, mode, d_pose_a, d_pose_b, d_out_iou, d_out_best, d_out_best_iou};
    {
        std::string msg;
        if (int rc = sg_check_iou_args(a, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->iou_rec, sg_iou_records((size_t)n_frames * ((size_t)n_a + (size_t)n_b)));
    int e = sg_launch_iou(n_frames, n_a, d_boxes_a, a_features, n_b, d_boxes_b, b_features, dtype, mode, d_pose_a, d_pose_b, ctx->iou_rec.p, d_out_iou, d_out_best,
                          d_out_best_iou, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("box IoU launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Rotated NMS (snowgpu_iou.hip: the ranking by counting and the lazy sweep).  See include/snowgpu.h.
extern "C" int snowgpu_nms_device(snowgpu_ctx *ctx, int n_frames, int n_boxes, const void *d_boxes, int box_features, const void *d_scores, int dtype, int mode,
                                  double iou_thresh, double score_thresh, int post_max, const double *d_pose_in, int32_t *d_out_index, int32_t *d_out_count,
                                  void *d_out_boxes, void *d_out_scores, uint8_t *d_out_kept, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgNmsArgs a{n_frames, n_boxes, d_boxes, box_features, d_scores, dtype, mode, iou_thresh, score_thresh, post_max, d_pose_in, d_out_index, d_out_count,
                      d_out_boxes, d_out_scores, d_out_kept};
    {
        std::string msg;
        if (int rc = sg_check_nms_args(a, &msg)) return fail(ctx, rc, msg);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->iou_rec, sg_iou_records((size_t)n_frames * (size_t)n_boxes));
    ENSURE(ctx, ctx->nms_order, (size_t)n_frames * (size_t)n_boxes);
    ENSURE(ctx, ctx->nms_cand, (size_t)n_frames);
    int e = sg_launch_nms(n_frames, n_boxes, d_boxes, box_features, d_scores, dtype, mode, iou_thresh, score_thresh, post_max, d_pose_in, ctx->iou_rec.p,
                          ctx->nms_order.p, ctx->nms_cand.p, d_out_index, d_out_count, d_out_boxes, d_out_scores, d_out_kept,
                          stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("NMS launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Proposal target sampling (snowgpu_targets.hip; the classes, the draws and what a slot stores: sg_targets.h).  See include/snowgpu.h.
extern "C" int snowgpu_sample_rois_device(snowgpu_ctx *ctx, int n_frames, int n_rois, const void *d_rois, int roi_features, const void *d_overlap,
                                          const int32_t *d_assignment, int n_gt, const void *d_gt_boxes, int gt_features, int dtype,
                                          const snowgpu_roi_sampler *cfg, uint64_t seed, const uint64_t *d_step, const double *d_pose, int32_t *d_out_index,
                                          void *d_out_rois, void *d_out_roi_iou, int32_t *d_out_gt_index, void *d_out_gt_of_rois, uint8_t *d_out_reg_valid,
                                          void *d_out_cls_label, int32_t *d_out_segments, int32_t *d_out_class_count, double *d_out_pose,
                                          void *d_out_gt_local, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    SgSamplerCfg c{};
    if (cfg) c = SgSamplerCfg{cfg->roi_per_image, cfg->fg_per_image, cfg->reg_fg_thresh, cfg->cls_fg_thresh, cfg->cls_bg_thresh, cfg->cls_bg_thresh_lo,
                              cfg->hard_bg_ratio, cfg->cls_mode};
    const SgTargetsArgs a{n_frames, n_rois, d_rois, roi_features, d_overlap, d_assignment, n_gt, d_gt_boxes, gt_features, dtype, cfg ? &c : nullptr, d_step, d_pose,
                          d_out_index, d_out_rois, d_out_roi_iou, d_out_gt_index, d_out_gt_of_rois, d_out_reg_valid, d_out_cls_label, d_out_segments,
                          d_out_class_count, d_out_pose, d_out_gt_local};
    {
        std::string msg;
        if (int rc = sg_check_targets_args(a, &msg)) return fail(ctx, rc, msg);
    }
    const SgTargetCfg k{c.roi_per_image, c.fg_per_image, c.reg_fg_thresh, c.cls_fg_thresh, c.cls_bg_thresh, c.cls_bg_thresh_lo, c.hard_bg_ratio, c.cls_mode};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int e = sg_launch_sample_rois(&k, n_frames, n_rois, d_rois, roi_features, d_overlap, d_assignment, n_gt, d_gt_boxes, gt_features, dtype, seed, d_step, d_pose,
                                  d_out_index, d_out_rois, d_out_roi_iou, d_out_gt_index, d_out_gt_of_rois, d_out_reg_valid, d_out_cls_label, d_out_segments,
                                  d_out_class_count, d_out_pose, d_out_gt_local, stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("target sampling launch: ") + hipGetErrorString((hipError_t)e));
    return SNOWGPU_OK;
}

// Anchor target assignment (snowgpu_anchors.hip; presence, the BEV box, the overlap, the walk and the label rule: sg_anchors.h).  See include/snowgpu.h.
extern "C" int snowgpu_assign_anchors_device(snowgpu_ctx *ctx, int n_frames, int n_anchors, const void *d_anchors, int anchor_features,
                                             const int32_t *d_anchor_class, int n_gt, const void *d_gt_boxes, int gt_features, int dtype, int n_classes,
                                             const double *matched, const double *unmatched, int32_t *d_out_label, int32_t *d_out_gt_index,
                                             int32_t *d_out_count, int32_t *d_out_gt_count, void *d_out_iou, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgAnchorsArgs a{n_frames, n_anchors, d_anchors, anchor_features, d_anchor_class, n_gt, d_gt_boxes, gt_features, dtype, n_classes, matched, unmatched,
                          d_out_label, d_out_gt_index, d_out_count, d_out_gt_count, d_out_iou};
    {
        std::string msg;
        if (int rc = sg_check_anchors_args(a, &msg)) return fail(ctx, rc, msg);
    }
    SgAnchorCfg k{};
    k.n_classes = n_classes;
    for (int c = 0; c < n_classes; ++c) { k.matched[c] = matched[c]; k.unmatched[c] = unmatched[c]; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->anchor_rec, (size_t)n_frames * (size_t)n_gt * (sizeof(SgAnchorRec) / sizeof(double)));
    ENSURE(ctx, ctx->anchor_top, (size_t)n_frames * (size_t)n_gt);
    ENSURE(ctx, ctx->anchor_blk, (size_t)n_frames * (size_t)sg_anchors_groups(n_anchors) * 3);
    int e = sg_launch_assign_anchors(&k, n_frames, n_anchors, d_anchors, anchor_features, d_anchor_class, n_gt, d_gt_boxes, gt_features, dtype, ctx->anchor_rec.p,
                                     ctx->anchor_top.p, ctx->anchor_blk.p, d_out_label, d_out_gt_index, d_out_count, d_out_gt_count, d_out_iou,
                                     stream ? (hipStream_t)stream : ctx->stream);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("anchor assignment launch: ") + hipGetErrorString((hipError_t)e));
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
