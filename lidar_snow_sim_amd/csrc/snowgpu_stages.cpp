// snowgpu_stages.cpp -- the stage entries of the C ABI (include/snowgpu.h): static-shape stages that take DEVICE pointers to an aligned batch,
// or to boxes, and enqueue on the caller's stream.  Each fills the argument struct of its stage, has it checked (sg_device_args.h: every
// refusal, in one order), sets the device, sizes the context's scratch and calls the launcher of its .hip file.  The *_batch_device*
// entries are snowgpu_device.cpp.  No host copy, no synchronisation, no allocation after the first call of a given size.
#include <utility>

#include "sg_host.h"
#include "sg_launch.h"      // sg_tiles
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
#include "sg_centers.h"     // SgCenterCfg and the record of the centre heatmap targets
#include "sg_paste.h"       // SgPasteGroups and the scratch of the object paste
#include "sg_scene.h"       // SgSceneCfg and the scratch of the scene transforms

// one of the sg_check_*_args on its arguments: SNOWGPU_OK, or the refusal with its message in the context
template <class... Params, class... Args>
static int checked(snowgpu_ctx *ctx, int (*check)(Params...), Args &&...args)
{
    std::string msg;
    const int rc = check(std::forward<Args>(args)..., &msg);
    return rc ? fail(ctx, rc, msg) : SNOWGPU_OK;
}

static hipStream_t stream_of(snowgpu_ctx *ctx, void *stream)
{
    return stream ? (hipStream_t)stream : ctx->stream;
}

// `e`: what a launcher returned
static int launched(snowgpu_ctx *ctx, const char *name, int e)
{
    return e ? fail(ctx, SNOWGPU_E_HIP, std::string(name) + " launch: " + hipGetErrorString((hipError_t)e)) : SNOWGPU_OK;
}

// NULL: no range test
static SgFpsRange range_of(const double *range6)
{
    SgFpsRange r;
    for (int j = 0; j < 3; ++j) { r.lo[j] = range6 ? range6[j] : -INFINITY; r.hi[j] = range6 ? range6[3 + j] : INFINITY; }
    return r;
}

// NULL: zeros
static void extra_width_of(const double *extra_width3, double ew[3])
{
    for (int j = 0; j < 3; ++j) ew[j] = extra_width3 ? extra_width3[j] : 0.0;
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
    return launched(ctx, "dror", sg_launch_dror(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &g, ctx->dror_entry.p, ctx->dror_cell.p,
                                                ctx->dror_sorted.p, d_out_keep, d_out_neighbours, stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_voxel_args, a, g.n)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream_of(ctx, stream);
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
    return launched(ctx, "voxelize", sg_launch_voxelize(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &g, ctx->vox_table.p, ctx->vox_slot.p,
                                                        ctx->vox_first.p, ctx->vox_order.p, ctx->vox_tile_cnt.p, ctx->vox_tile_base.p, ctx->vox_fbase.p, ctx->vox_m.p,
                                                        ctx->vox_span.p, d_out_voxels, d_out_coords, d_out_num_points, d_out_voxel_offsets, d_out_voxel_of, st));
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
    if (int rc = checked(ctx, sg_check_fps_args, a)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SgFpsRange r = range_of(range6);
    if (n_total > 0) {
        const size_t elems = sg_fps_scratch(n_total, n_frames), bytes = elems * (dtype == 0 ? 4 : 8);
        ENSURE(ctx, ctx->fps_x, bytes);
        ENSURE(ctx, ctx->fps_y, bytes);
        ENSURE(ctx, ctx->fps_z, bytes);
        ENSURE(ctx, ctx->fps_t, bytes);
        ENSURE(ctx, ctx->fps_src, elems);
    }
    return launched(ctx, "fps", sg_launch_fps(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &r, n_samples, n_features, ctx->fps_x.p, ctx->fps_y.p,
                                              ctx->fps_z.p, ctx->fps_t.p, ctx->fps_src.p, d_out_index, d_out_points, d_out_dist, d_out_usable, stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_fps_sectors_args, a)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SgFpsRange r = range_of(range6);
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
    return launched(ctx, "sectorized fps",
                    sg_launch_fps_sectors(d_rows, dtype, n_total, max_frame, d_frame_offsets, n_frames, d_keep_in, &r, n_samples, n_features, n_sectors, d_rois, n_rois,
                                          roi_features, roi_margin, ctx->fps_x.p, ctx->fps_y.p, ctx->fps_z.p, ctx->fps_t.p, ctx->fps_src.p, ctx->fpss_sec.p,
                                          ctx->fpss_roi.p, ctx->fpss_tile.p, ctx->fpss_seg.p, d_out_index, d_out_points, d_out_dist, d_out_usable, d_out_sector_offsets,
                                          d_out_sector_count, d_out_sector_of, d_out_reach2, stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_ball_args, a, nullptr)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SgFpsRange r = range_of(range6);
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
    return launched(ctx, "ball query",
                    sg_launch_ball(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &r, &g, n_centres, d_centres, centre_features, n_radii, radii, n_samples,
                                   n_features, ctx->ball_entry.p, ctx->ball_cell.p, ctx->ball_x.p, ctx->ball_y.p, ctx->ball_z.p, ctx->ball_src.p, d_out_index, d_out_count,
                                   d_out_points, stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_range_args, a)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    SgRangeGeom g{};
    g.H = height; g.W = width; g.by_ring = d_ring ? 1 : 0;
    if (!d_ring) { g.fov_up = fov2[0]; g.fov_down = fov2[1]; }
    sg_range_limits(dtype, limits2, &g.lo, &g.hi);
    if (n_total > 0) ENSURE(ctx, ctx->range_key, (size_t)n_frames * (size_t)height * (size_t)width);
    return launched(ctx, "range image", sg_launch_range(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, d_ring, &g, n_features, ctx->range_key.p, d_out_image,
                                                        d_out_index, d_out_pixel_of, d_out_count, stream_of(ctx, stream)));
}

// Nearest centres of every row (snowgpu_nn.hip; the grid, the walk and its stopping bound: sg_nn.h).  See include/snowgpu.h.
extern "C" int snowgpu_nearest_centres_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                              const void *d_rows, int dtype, const double *range6, int n_centres, const void *d_centres, int centre_features,
                                              int k, const uint8_t *d_keep_in, int32_t *d_out_index, void *d_out_dist2, void *d_out_weight, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgNnArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, range6, n_centres, d_centres, centre_features, k, d_keep_in,
                     d_out_index, d_out_dist2, d_out_weight, SG_NN_MAX_CELLS};
    if (int rc = checked(ctx, sg_check_nn_args, a)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const SgFpsRange r = range_of(range6);
    SgNnGrid g{};
    sg_nn_make_grid(range6, n_centres, &g);
    if (n_total > 0) {
        ENSURE(ctx, ctx->nn_entry, sg_nn_entries(n_frames, sg_nn_cell_budget(n_centres)));      // (by the budget, not the grid: the range changes no allocation)
        ENSURE(ctx, ctx->nn_box, sg_nn_boxes(n_frames));
        ENSURE(ctx, ctx->nn_rec, sg_nn_records(n_frames, n_centres) * (dtype == 0 ? sizeof(SgNnRec<float>) : sizeof(SgNnRec<double>)));
    }
    return launched(ctx, "nearest centres", sg_launch_nn(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, &r, &g, n_centres, d_centres, centre_features, k,
                                                         ctx->nn_entry.p, ctx->nn_box.p, ctx->nn_rec.p, d_out_index, d_out_dist2, d_out_weight, stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_box_args, a)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->box_rec, sg_box_records(n_frames, n_boxes) * (sizeof(SgBoxRec) / sizeof(double)));
    ENSURE(ctx, ctx->box_table, sg_box_table(n_frames, n_boxes));
    return launched(ctx, "points in boxes", sg_launch_box(d_rows, dtype, n_total, d_frame_offsets, n_frames, d_keep_in, n_boxes, d_boxes, box_features, d_pose_in,
                                                          (SgBoxRec *)ctx->box_rec.p, ctx->box_table.p, d_out_box_of, d_out_count, d_out_local, d_out_pose,
                                                          stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_roipool_args, a)) return rc;
    double ew[3];
    extra_width_of(extra_width3, ew);
    const int64_t longest = sg_max_frame(max_frame_rows, n_total);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->roi_rec, sg_box_records(n_frames, n_rois) * (sizeof(SgBoxRec) / sizeof(double)));
    ENSURE(ctx, ctx->roi_table, sg_box_table(n_frames, n_rois));
    if (n_total > 0) ENSURE(ctx, ctx->roi_runs, sg_roi_table(n_frames, longest, n_rois));
    return launched(ctx, "roi point pool",
                    sg_launch_roipool(d_rows, dtype, n_total, longest, d_frame_offsets, n_frames, d_keep_in, n_rois, d_rois, roi_features, ew, n_samples, num_features,
                                      d_pose_in, (SgBoxRec *)ctx->roi_rec.p, ctx->roi_table.p, ctx->roi_runs.p, d_out_index, d_out_count, d_out_points, d_out_local,
                                      d_out_pose, stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_roiaware_args, a)) return rc;
    double ew[3];
    extra_width_of(extra_width3, ew);
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
    return launched(ctx, "roi voxel pool",
                    sg_launch_roiaware(d_rows, dtype, n_total, longest, d_frame_offsets, n_frames, d_keep_in, n_rois, d_rois, roi_features, ew, grid, max_points, roi_capacity,
                                       d_features, (d_features || d_out_max || d_out_argmax || d_out_avg) ? feature_channels : 1, d_pose_in, (SgBoxRec *)ctx->rv_rec.p,
                                       ctx->rv_table.p, ctx->rv_runs.p, ctx->rv_list.p, ctx->rv_sorted.p, ctx->rv_offset.p, d_out_roi_count, d_out_count, d_out_index,
                                       d_out_max, d_out_argmax, d_out_avg, d_out_pose, stream_of(ctx, stream)));
}

// Rotated box IoU (snowgpu_iou.hip; presence, the record, the clip and the two IoUs: sg_iou.h).  See include/snowgpu.h.
extern "C" int snowgpu_boxes_iou_device(snowgpu_ctx *ctx, int n_frames, int n_a, const void *d_boxes_a, int a_features, int n_b, const void *d_boxes_b,
                                        int b_features, int dtype, int mode, const double *d_pose_a, const double *d_pose_b, void *d_out_iou,
                                        int32_t *d_out_best, void *d_out_best_iou, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgIouArgs a{n_frames, n_a, d_boxes_a, a_features, n_b, d_boxes_b, b_features, dtype, mode, d_pose_a, d_pose_b, d_out_iou, d_out_best, d_out_best_iou};
    if (int rc = checked(ctx, sg_check_iou_args, a)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->iou_rec, sg_iou_records((size_t)n_frames * ((size_t)n_a + (size_t)n_b)));
    return launched(ctx, "box IoU", sg_launch_iou(n_frames, n_a, d_boxes_a, a_features, n_b, d_boxes_b, b_features, dtype, mode, d_pose_a, d_pose_b, ctx->iou_rec.p,
                                                  d_out_iou, d_out_best, d_out_best_iou, stream_of(ctx, stream)));
}

// Rotated NMS (snowgpu_iou.hip: the ranking by counting and the lazy sweep).  See include/snowgpu.h.
extern "C" int snowgpu_nms_device(snowgpu_ctx *ctx, int n_frames, int n_boxes, const void *d_boxes, int box_features, const void *d_scores, int dtype, int mode,
                                  double iou_thresh, double score_thresh, int post_max, const double *d_pose_in, int32_t *d_out_index, int32_t *d_out_count,
                                  void *d_out_boxes, void *d_out_scores, uint8_t *d_out_kept, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgNmsArgs a{n_frames, n_boxes, d_boxes, box_features, d_scores, dtype, mode, iou_thresh, score_thresh, post_max, d_pose_in, d_out_index, d_out_count,
                      d_out_boxes, d_out_scores, d_out_kept};
    if (int rc = checked(ctx, sg_check_nms_args, a)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->iou_rec, sg_iou_records((size_t)n_frames * (size_t)n_boxes));
    ENSURE(ctx, ctx->nms_order, (size_t)n_frames * (size_t)n_boxes);
    ENSURE(ctx, ctx->nms_cand, (size_t)n_frames);
    return launched(ctx, "NMS", sg_launch_nms(n_frames, n_boxes, d_boxes, box_features, d_scores, dtype, mode, iou_thresh, score_thresh, post_max, d_pose_in,
                                              ctx->iou_rec.p, ctx->nms_order.p, ctx->nms_cand.p, d_out_index, d_out_count, d_out_boxes, d_out_scores, d_out_kept,
                                              stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_targets_args, a)) return rc;
    const SgTargetCfg k{c.roi_per_image, c.fg_per_image, c.reg_fg_thresh, c.cls_fg_thresh, c.cls_bg_thresh, c.cls_bg_thresh_lo, c.hard_bg_ratio, c.cls_mode};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return launched(ctx, "target sampling",
                    sg_launch_sample_rois(&k, n_frames, n_rois, d_rois, roi_features, d_overlap, d_assignment, n_gt, d_gt_boxes, gt_features, dtype, seed, d_step, d_pose,
                                          d_out_index, d_out_rois, d_out_roi_iou, d_out_gt_index, d_out_gt_of_rois, d_out_reg_valid, d_out_cls_label, d_out_segments,
                                          d_out_class_count, d_out_pose, d_out_gt_local, stream_of(ctx, stream)));
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
    if (int rc = checked(ctx, sg_check_anchors_args, a)) return rc;
    SgAnchorCfg k{};
    k.n_classes = n_classes;
    for (int c = 0; c < n_classes; ++c) { k.matched[c] = matched[c]; k.unmatched[c] = unmatched[c]; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->anchor_rec, (size_t)n_frames * (size_t)n_gt * (sizeof(SgAnchorRec) / sizeof(double)));
    ENSURE(ctx, ctx->anchor_top, (size_t)n_frames * (size_t)n_gt);
    ENSURE(ctx, ctx->anchor_blk, (size_t)n_frames * (size_t)sg_anchors_groups(n_anchors) * 3);
    return launched(ctx, "anchor assignment",
                    sg_launch_assign_anchors(&k, n_frames, n_anchors, d_anchors, anchor_features, d_anchor_class, n_gt, d_gt_boxes, gt_features, dtype, ctx->anchor_rec.p,
                                             ctx->anchor_top.p, ctx->anchor_blk.p, d_out_label, d_out_gt_index, d_out_count, d_out_gt_count, d_out_iou,
                                             stream_of(ctx, stream)));
}

// Centre heatmap targets (snowgpu_centers.hip; presence, the centre, the radius, the record and the value of a pixel: sg_centers.h).  See
// include/snowgpu.h.
extern "C" int snowgpu_assign_centers_device(snowgpu_ctx *ctx, int n_frames, int n_gt, const void *d_gt_boxes, int gt_features, int dtype,
                                             const snowgpu_center_cfg *cfg, float *d_out_heatmap, int32_t *d_out_gt_index, int32_t *d_out_ind,
                                             uint8_t *d_out_mask, void *d_out_offset, int32_t *d_out_radius, int32_t *d_out_count, uint8_t *d_out_state,
                                             void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    SgCentersCfg c{};
    if (cfg) {
        c = SgCentersCfg{cfg->x0, cfg->y0, cfg->vx, cfg->vy, cfg->gaussian_overlap, cfg->stride, cfg->width, cfg->height, cfg->n_classes, cfg->n_heads,
                         cfg->max_objs, cfg->min_radius, cfg->outside, {}};
        for (int k = 0; k < 16; ++k) c.class_head[k] = cfg->class_head[k];
    }
    const SgCentersArgs a{n_frames, n_gt, d_gt_boxes, gt_features, dtype, cfg ? &c : nullptr, d_out_heatmap, d_out_gt_index, d_out_ind, d_out_mask, d_out_offset,
                          d_out_radius, d_out_count, d_out_state};
    if (int rc = checked(ctx, sg_check_centers_args, a)) return rc;
    SgCenterCfg k{};
    k.x0 = c.x0; k.y0 = c.y0; k.vx = c.vx; k.vy = c.vy; k.stride = (double)c.stride; k.overlap = c.gaussian_overlap;
    k.W = c.width; k.H = c.height; k.n_classes = c.n_classes; k.n_heads = c.n_heads; k.max_objs = c.max_objs; k.min_radius = c.min_radius; k.drop = c.outside;
    for (int j = 0; j < c.n_classes; ++j) k.class_head[j] = c.class_head[j];
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->center_rec, (size_t)n_frames * (size_t)n_gt * (sizeof(SgCenterRec) / sizeof(double)));
    return launched(ctx, "centre targets",
                    sg_launch_assign_centers(&k, n_frames, n_gt, d_gt_boxes, gt_features, dtype, ctx->center_rec.p, d_out_heatmap, d_out_gt_index, d_out_ind, d_out_mask,
                                             d_out_offset, d_out_radius, d_out_count, d_out_state, stream_of(ctx, stream)));
}

// Ground-truth object paste (snowgpu_paste.hip; the slots, the draw, the sweep and the scratch: sg_paste.h).  See include/snowgpu.h.
extern "C" int snowgpu_paste_objects_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                            const void *d_rows, int dtype, int n_gt, const void *d_gt_boxes, int gt_features, const double *d_pose_in,
                                            int64_t n_bank_points, int64_t n_bank_objects, const void *d_bank_points, const int64_t *d_bank_offsets,
                                            const void *d_bank_boxes, const double *d_bank_pose, const int32_t *d_class_offsets, int n_classes,
                                            const int32_t *sample_groups, const double *extra_width3, uint64_t seed, const uint64_t *d_step,
                                            const uint8_t *d_keep_in, void *d_out_rows, uint8_t *d_out_keep, void *d_out_gt_boxes, int32_t *d_out_object,
                                            int32_t *d_out_state, int32_t *d_out_source, int32_t *d_out_count, double *d_out_pose, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgPasteArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, n_gt, d_gt_boxes, gt_features, d_pose_in, n_bank_points, n_bank_objects,
                        d_bank_points, d_bank_offsets, d_bank_boxes, d_bank_pose, d_class_offsets, n_classes, sample_groups, extra_width3, d_step, d_keep_in,
                        d_out_rows, d_out_keep, d_out_gt_boxes, d_out_object, d_out_state, d_out_source, d_out_count, d_out_pose};
    if (int rc = checked(ctx, sg_check_paste_args, a)) return rc;
    double ew[3];
    extra_width_of(extra_width3, ew);
    SgPasteGroups g{};
    g.n_classes = n_classes;
    for (int c = 0; c < n_classes; ++c) { g.n[c] = sample_groups[c]; g.Q += sample_groups[c]; }
    const int64_t longest = sg_max_frame(max_frame_rows, n_total);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->paste_runs, sg_paste_table(n_frames, longest));
    ENSURE(ctx, ctx->paste_frames, sg_paste_frames(n_frames) * sizeof(SgPasteFrame));
    ENSURE(ctx, ctx->paste_grid, sg_paste_grid(n_frames));
    return launched(ctx, "object paste",
                    sg_launch_paste(d_rows, dtype, n_total, longest, d_frame_offsets, n_frames, d_keep_in, n_gt, d_gt_boxes, gt_features, d_pose_in, d_bank_points,
                                    d_bank_offsets, d_bank_boxes, d_bank_pose, d_class_offsets, &g, ew, seed, d_step, ctx->paste_runs.p,
                                    (SgPasteFrame *)ctx->paste_frames.p, ctx->paste_grid.p, d_out_rows, d_out_keep, d_out_gt_boxes, d_out_object, d_out_state, d_out_source, d_out_count,
                                    d_out_pose, stream_of(ctx, stream)));
}

// Scene transforms (snowgpu_scene.hip; the draws, the sweep, what a row and a box become and the scratch: sg_scene.h).  See include/snowgpu.h.
extern "C" int snowgpu_transform_scene_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                              const void *d_rows, int dtype, int n_boxes, const void *d_gt_boxes, int box_features, const double *d_pose_in,
                                              int flip, const double *rotation2, const double *scaling2, int tries, const double *local_translation3,
                                              const double *local_rotation2, const double *local_scaling2, uint64_t seed, const uint64_t *d_step,
                                              const int32_t *d_box_of, const uint8_t *d_keep_in, void *d_out_rows, uint8_t *d_out_keep, void *d_out_gt_boxes,
                                              double *d_out_world, int32_t *d_out_state, int32_t *d_out_tried, double *d_out_local, double *d_out_pose,
                                              double *d_out_tries, void *stream)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    const SgSceneArgs a{n_frames, n_total, max_frame_rows, dtype, d_frame_offsets, d_rows, n_boxes, d_gt_boxes, box_features, d_pose_in, flip, rotation2, scaling2,
                        tries, local_translation3, local_rotation2, local_scaling2, d_step, d_box_of, d_keep_in, d_out_rows, d_out_keep, d_out_gt_boxes, d_out_world,
                        d_out_state, d_out_tried, d_out_local, d_out_pose, d_out_tries};
    if (int rc = checked(ctx, sg_check_scene_args, a)) return rc;
    SgSceneCfg k{};
    k.flip = flip; k.tries = tries;
    if (rotation2) { k.rot_on = 1; k.rot[0] = rotation2[0]; k.rot[1] = rotation2[1]; }
    if (scaling2) { k.scale_on = 1; k.scale[0] = scaling2[0]; k.scale[1] = scaling2[1]; }
    if (tries > 0 && local_translation3) { k.ltrans_on = 1; for (int j = 0; j < 3; ++j) k.ltrans[j] = local_translation3[j]; }
    if (tries > 0 && local_rotation2) { k.lrot_on = 1; k.lrot[0] = local_rotation2[0]; k.lrot[1] = local_rotation2[1]; }
    if (tries > 0 && local_scaling2) { k.lscale_on = 1; k.lscale[0] = local_scaling2[0]; k.lscale[1] = local_scaling2[1]; }
    const bool own_box_of = tries > 0 && !d_box_of && n_total > 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ENSURE(ctx, ctx->scene_rowrec, sg_scene_rowrecs(n_frames, n_boxes));
    if (tries > 0 && !d_out_tries) ENSURE(ctx, ctx->scene_tries, sg_scene_tries(n_frames, n_boxes, tries));
    if (own_box_of) {
        ENSURE(ctx, ctx->scene_box_rec, sg_box_records(n_frames, n_boxes) * (sizeof(SgBoxRec) / sizeof(double)));
        ENSURE(ctx, ctx->scene_box_table, sg_box_table(n_frames, n_boxes));
        ENSURE(ctx, ctx->scene_box_of, (size_t)n_total);
    }
    return launched(ctx, "scene transforms",
                    sg_launch_scene(d_rows, dtype, n_total, sg_max_frame(max_frame_rows, n_total), d_frame_offsets, n_frames, d_keep_in, n_boxes, d_gt_boxes, box_features,
                                    d_pose_in, &k, seed, d_step, tries > 0 ? d_box_of : nullptr, (SgBoxRec *)ctx->scene_box_rec.p, ctx->scene_box_table.p,
                                    ctx->scene_box_of.p, ctx->scene_tries.p, ctx->scene_rowrec.p, d_out_rows, d_out_keep, d_out_gt_boxes, d_out_world, d_out_state,
                                    d_out_tried, d_out_local, d_out_pose, d_out_tries, stream_of(ctx, stream)));
}
