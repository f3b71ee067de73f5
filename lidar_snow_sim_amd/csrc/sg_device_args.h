// sg_device_args.h -- what the entries that take device pointers take in common, and the one place that refuses a call of theirs: pure
// argument checks on plain data.  sg_check_device_args is for the *_batch_device* entries (snowgpu_device.cpp), the sg_check_*_args above it
// for the stage entries (snowgpu_stages.cpp), and what those share stands once, ahead of them.  Nothing of HIP is included, so the whole
// refusal matrix runs on a machine without a device (tests/host_harness/*_refusals.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

// the scalars of ground_water_augmentation() (wet_ground/augmentation.py:25)
struct SgWetScalars {
    double water_height, pavement_depth, noise_floor, power_factor, delta;
    int flat_earth, replace;
};

struct SgDeviceArgs {
    const char *who;                  // the entry's name, as its messages begin
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    const int32_t *table_ids;
    double beam_div_deg;
    const double *thr_poly, *plane;
    double noise_floor;
    const int32_t *perm;
    const uint8_t *keep_in;
    void *out_rows;
    int32_t *out_src;                 // compact entries
    uint8_t *out_keep;                // aligned entries
    int64_t *out_counts, *out_stats;
    double *out_thr_poly;
    int32_t *out_flags, *status;
    void *stream;
    // the wet stage
    const double *wet_plane;
    SgWetScalars wet;
    const double *weather;            // per-frame records: they replace the five wet scalars
};

// the context settings the checks read
struct SgCtxView {
    bool thr_fn;                      // a threshold callback is set
    int result_mode;
    int plane_method;                 // SG_PLANE_*: 0 is `reference`
    size_t n_tables;
};

struct SgEntryShape {
    bool tables;                      // a snowfall stage: table ids and statistics
    bool aligned;                     // rows in input order with a keep mask (else the compact layout with source indices)
    bool masked;                      // the masked front end runs
    bool wet;                         // a wet stage: per-frame flags
    bool weather;                     // per-frame weather records
    bool empty_null_ok;               // rows and outputs may be NULL for a batch without rows
};

constexpr SgEntryShape SG_SHAPE_COMPACT      = {true,  false, false, false, false, false};   // snowgpu_augment_batch_device
constexpr SgEntryShape SG_SHAPE_COMPACT_WET  = {true,  false, false, true,  false, false};   // snowgpu_augment_wet_batch_device
constexpr SgEntryShape SG_SHAPE_ALIGNED      = {true,  true,  false, false, false, false};   // snowgpu_augment_batch_device_aligned
constexpr SgEntryShape SG_SHAPE_WET_ONLY     = {false, true,  false, true,  false, true};    // snowgpu_wet_ground_batch_device_aligned
constexpr SgEntryShape SG_SHAPE_ALIGNED_WET  = {true,  true,  false, true,  false, false};   // snowgpu_augment_wet_batch_device_aligned
constexpr SgEntryShape SG_SHAPE_MASKED       = {true,  true,  true,  false, false, false};   // ..._aligned_masked with a mask and rows
constexpr SgEntryShape SG_SHAPE_MASKED_WET   = {true,  true,  true,  true,  false, false};   // ..._wet_batch_device_aligned_masked, likewise
constexpr SgEntryShape SG_SHAPE_WEATHER      = {true,  true,  true,  true,  true,  false};   // snowgpu_augment_weather_batch_device_aligned

constexpr int SG_ARGS_INVALID = 1;    // SNOWGPU_E_INVALID (include/snowgpu.h; snowgpu_device.cpp asserts that they agree)

static inline int64_t sg_max_frame(int64_t max_frame_rows, int64_t n_total)
{
    return (max_frame_rows > 0 && max_frame_rows <= n_total) ? max_frame_rows : n_total;
}

static inline int64_t sg_uniform_rows(int64_t max_frame_rows, int n_frames, int64_t n_total)
{
    return (max_frame_rows > 0 && max_frame_rows * (int64_t)n_frames == n_total) ? max_frame_rows : 0;
}

// two arrays of `bytes` bytes that share some of them without being the same array
static inline bool sg_overlap(const void *in, const void *out, size_t bytes)
{
    const uintptr_t a = (uintptr_t)in, o = (uintptr_t)out;
    return a && o != a && o < a + bytes && a < o + bytes;
}

static inline int sg_refuse(const char *who, const char *what, std::string *msg)
{
    if (msg) *msg = std::string(who) + what;
    return SG_ARGS_INVALID;
}

// `beside`: what makes the batch a masked one
static inline int sg_refuse_perm(const char *who, const char *beside, std::string *msg)
{
    if (msg) *msg = std::string(who) + ": d_perm with " + beside + "; a caller's permutation indexes the rows of the frames it was made for, not the present ones";
    return SG_ARGS_INVALID;
}

// calculate_plane (augmentation.py:41) for an aligned wet stage: the method `reference` returns a constant and reads no row.  The two
// estimators crop the cloud into a list first; under a mask that list -- and with it the RANSAC draws -- has another order.
// The fused entries ask before anything is launched; the wet stage asks again where it needs the plane, which is the first time for
// snowgpu_wet_ground_batch_device_aligned: behind its empty batch and behind the caller's lines.
static inline int sg_check_wet_plane(const char *who, const double *wet_plane, int plane_method, std::string *msg)
{
    if (wet_plane || plane_method == 0) return 0;
    return sg_refuse(who, ": a NULL wet plane needs the plane method 'reference'; 'lsq' and 'ransac' crop the rows and have no masked form: pass the plane", msg);
}

// ---- what the checks of the stage entries share -------------------------------------------------------------------------------------------
// Each is 0, or SG_ARGS_INVALID with *msg (built on this path only).  Where a stage calls them is its own business: the order of a
// stage's checks is part of the ABI, since it decides which message a doubly wrong call gets (the "_and_" cases of the harnesses).

// `missing`: the stage's own "something required is NULL"
static inline int sg_check_head(const char *who, int n_frames, int dtype, bool missing, std::string *msg)
{
    return (n_frames <= 0 || missing || (dtype != 0 && dtype != 1)) ? sg_refuse(who, ": null pointer or bad dtype", msg) : 0;
}

static inline int sg_check_rows(int64_t n_total, std::string *msg)
{
    return n_total >= ((int64_t)1 << 31) ? sg_refuse("", "batch too large: split it below 2^31 rows", msg) : 0;
}

// the head of a stage that takes the rows of a batch
template <class Args>
static inline int sg_check_batch_head(const char *who, const Args &a, bool missing, std::string *msg)
{
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, a.n_total < 0 || !a.frame_off || missing, msg)) return rc;
    return sg_check_rows(a.n_total, msg);
}

// `longest`: sg_max_frame() of the batch
static inline int sg_check_frame(const char *who, int64_t longest, std::string *msg)
{
    return longest > ((int64_t)1 << 30) ? sg_refuse(who, ": a frame of more than 2^30 rows; split it", msg) : 0;
}

// (x0, y0, z0, x1, y1, z1) or NULL: no range test
static inline int sg_check_range6(const char *who, const double *range6, std::string *msg)
{
    if (!range6) return 0;
    for (int j = 0; j < 6; ++j)
        if (range6[j] != range6[j]) return sg_refuse(who, ": a bound of the range is NaN; pass NULL for no range, or infinite bounds", msg);
    for (int j = 0; j < 3; ++j)
        if (!(range6[j] < range6[3 + j])) return sg_refuse(who, ": the range needs lo < hi on every axis", msg);
    return 0;
}

// 3 doubles or NULL: zeros
static inline int sg_check_extra_width(const char *who, const double *extra_width, std::string *msg)
{
    for (int j = 0; extra_width && j < 3; ++j)
        if (!(extra_width[j] >= 0.0 && extra_width[j] <= 100.0))                             // (false for NaN)
            return sg_refuse(who, ": every component of extra_width must be finite and lie in 0 .. 100", msg);
    return 0;
}

// two arrays, `abytes` from a and `bbytes` from b, that share a byte (false where either is NULL or empty)
static inline bool sg_ranges_meet(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p && q && abytes && bbytes && p < q + bbytes && q < p + abytes;
}

struct SgOutSpan { const void *p; size_t bytes; const char *name; };
// `read`, `apart`: "the mask is" and "it", or "the rows are" and "them" -- or one phrase for all inputs of the stage
struct SgInSpan { const void *p; size_t bytes; const char *name, *read, *apart; };

// No output may share a byte with an input nor, with `among_outputs`, with an output before it: for output i the inputs in table order, then
// the outputs 0 .. i - 1.  `written`: "the samples are", "the image is".
template <size_t N_OUT, size_t N_IN>
static inline int sg_check_overlaps(const char *who, const SgOutSpan (&outs)[N_OUT], const SgInSpan (&ins)[N_IN], const char *written, bool among_outputs,
                                    std::string *msg)
{
    for (size_t i = 0; i < N_OUT; ++i) {
        const SgOutSpan &o = outs[i];
        for (const SgInSpan &in : ins)
            if (sg_ranges_meet(o.p, o.bytes, in.p, in.bytes))
                return sg_refuse(who, (std::string(": ") + o.name + " overlaps " + in.name + "; " + in.read + " read while " + written +
                                       " written: pass a buffer apart from " + in.apart).c_str(), msg);
        for (size_t j = 0; among_outputs && j < i; ++j)
            if (sg_ranges_meet(o.p, o.bytes, outs[j].p, outs[j].bytes))
                return sg_refuse(who, (std::string(": ") + o.name + " overlaps " + outs[j].name + "; every output needs memory of its own").c_str(), msg);
    }
    return 0;
}

// ---- snowgpu_voxelize_device ------------------------------------------------------------------------------------------------------------
struct SgVoxelArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    const double *range6, *size3;     // (x0, y0, z0, x1, y1, z1) and the voxel's edges, host memory
    int max_points, max_voxels, n_features;
    const uint8_t *keep_in;
    void *out_voxels;
    int32_t *out_coords, *out_num_points, *out_voxel_offsets, *out_voxel_of;
};

constexpr int64_t SG_VOXEL_MAX_CELLS = ((int64_t)1 << 31) - 2;

// n_j = llround((hi_j - lo_j) / size_j), in double.  0, 1: a size that is not positive and finite, 2: an axis without a cell (or a range
// that is not finite), 3: more than SG_VOXEL_MAX_CELLS cells.
static inline int sg_voxel_dims(const double *range6, const double *size3, int32_t n[3])
{
    for (int j = 0; j < 3; ++j)
        if (!(size3[j] > 0.0) || !(size3[j] <= 1.7976931348623157e308)) return 1;
    int64_t cells = 1;
    bool too_many = false;
    for (int j = 0; j < 3; ++j) {
        const double q = (range6[3 + j] - range6[j]) / size3[j];
        if (!(q >= 0.5) || !(q <= 1.7976931348623157e308)) return 2;      // (llround(q) >= 1 iff q >= 0.5; false for NaN)
        if (q >= 2147483647.0) { too_many = true; continue; }
        n[j] = (int32_t)std::llround(q);
        cells = cells > SG_VOXEL_MAX_CELLS ? cells : cells * n[j];
    }
    return too_many || cells > SG_VOXEL_MAX_CELLS ? 3 : 0;
}

// 0 and the grid's n_x, n_y, n_z, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.  Of the overlaps only
// d_out_voxel_of against d_keep_in is looked for.
static inline int sg_check_voxel_args(const SgVoxelArgs &a, int32_t n_cells[3], std::string *msg)
{
    static const char *who = "snowgpu_voxelize_device";
    if (int rc = sg_check_batch_head(who, a, !a.range6 || !a.size3 || !a.out_voxel_offsets ||
                                                 (a.n_total > 0 && (!a.rows || !a.out_voxels || !a.out_coords || !a.out_num_points)), msg)) return rc;
    if (a.n_features < 3 || a.n_features > 5) return sg_refuse(who, ": n_features must be 3, 4 or 5: the columns of a row that a voxel stores", msg);
    if (a.max_points < 1 || a.max_voxels < 1) return sg_refuse(who, ": max_points and max_voxels must be at least 1", msg);
    switch (sg_voxel_dims(a.range6, a.size3, n_cells)) {
    case 1: return sg_refuse(who, ": every voxel size must be positive and finite", msg);
    case 2: return sg_refuse(who, ": the range must be finite and hold at least one voxel on every axis (llround((hi - lo) / size) >= 1)", msg);
    case 3: return sg_refuse(who, ": the grid has more than 2^31 - 2 cells; a cell's index is kept in 31 bits", msg);
    default: break;
    }
    if ((int64_t)a.n_frames * a.max_voxels > (((int64_t)1 << 31) - 1))
        return sg_refuse(who, ": n_frames * max_voxels exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    if (sg_ranges_meet(a.out_voxel_of, (size_t)a.n_total * 4, a.keep_in, (size_t)a.n_total))
        return sg_refuse(who, ": d_out_voxel_of overlaps d_keep_in; the keep-in bytes of other rows are read while it is written: pass a buffer apart from it", msg);
    return 0;
}

// ---- snowgpu_fps_device -----------------------------------------------------------------------------------------------------------------
struct SgFpsArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    const double *range6;             // (x0, y0, z0, x1, y1, z1), host memory, or NULL: no range test
    int n_samples, n_features;
    const uint8_t *keep_in;
    int32_t *out_index;
    void *out_points, *out_dist;      // or NULL
    int32_t *out_usable;
};

// what snowgpu_fps_device and snowgpu_fps_sectors_device check alike, behind their heads
static inline int sg_check_fps_domain(const char *who, const SgFpsArgs &a, std::string *msg)
{
    if (a.n_features < 3 || a.n_features > 5) return sg_refuse(who, ": n_features must be 3, 4 or 5: the columns of a row that a keypoint carries", msg);
    if (a.n_samples < 1) return sg_refuse(who, ": n_samples must be at least 1", msg);
    if ((int64_t)a.n_frames * a.n_samples > (((int64_t)1 << 31) - 1))
        return sg_refuse(who, ": n_frames * n_samples exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    return sg_check_range6(who, a.range6, msg);
}

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.  The outputs are not compared with each other.
static inline int sg_check_fps_args(const SgFpsArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_fps_device";
    if (int rc = sg_check_batch_head(who, a, !a.out_index || !a.out_usable || (a.n_total > 0 && !a.rows), msg)) return rc;
    if (int rc = sg_check_fps_domain(who, a, msg)) return rc;
    const size_t esz = a.dtype == 0 ? 4 : 8, elems = (size_t)a.n_frames * (size_t)a.n_samples, n = (size_t)a.n_total;
    const SgOutSpan outs[3] = {
        {a.out_index, elems * 4, "d_out_index"}, {a.out_points, elems * (size_t)a.n_features * esz, "d_out_points"}, {a.out_dist, elems * esz, "d_out_dist"}};
    const SgInSpan ins[2] = {{a.keep_in, n, "d_keep_in", "the mask is", "it"}, {a.rows, n * 5 * esz, "d_rows", "the rows are", "them"}};
    return sg_check_overlaps(who, outs, ins, "the samples are", false, msg);
}

// ---- snowgpu_fps_sectors_device -----------------------------------------------------------------------------------------------------------
struct SgFpsSectorsArgs {
    SgFpsArgs fps;                    // what snowgpu_fps_device takes, with the same meaning
    int n_sectors;                    // S
    const void *rois;                 // (F, B, Cb) in the rows' dtype, or NULL: no roi test (n_rois and roi_features are then not read)
    int n_rois, roi_features;         // B, Cb
    double roi_margin;
    int32_t *out_sector_offsets, *out_sector_count;
    int8_t *out_sector_of;            // or NULL
    double *out_reach2;               // or NULL; only with rois
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_fps_sectors_args(const SgFpsSectorsArgs &s, std::string *msg)
{
    static const char *who = "snowgpu_fps_sectors_device";
    const SgFpsArgs &a = s.fps;
    if (int rc = sg_check_batch_head(who, a, !a.out_index || !a.out_usable || !s.out_sector_offsets || !s.out_sector_count || (a.n_total > 0 && !a.rows), msg)) return rc;
    if (int rc = sg_check_fps_domain(who, a, msg)) return rc;
    if (s.n_sectors < 1 || s.n_sectors > 16) return sg_refuse(who, ": n_sectors must lie in 1 .. 16", msg);
    if (s.rois) {
        if (s.n_rois < 1 || s.n_rois > 256) return sg_refuse(who, ": n_rois must lie in 1 .. 256", msg);
        if (s.roi_features < 7 || s.roi_features > 10) return sg_refuse(who, ": roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
        if (!(s.roi_margin >= 0.0 && s.roi_margin <= 1.7976931348623157e308)) return sg_refuse(who, ": roi_margin must be finite and at least 0", msg);
        if ((int64_t)a.n_frames * s.n_rois > ((int64_t)1 << 31) - 1) return sg_refuse(who, ": n_frames * n_rois exceeds 2^31 - 1; split the batch", msg);
    } else if (s.out_reach2)
        return sg_refuse(who, ": d_out_reach2 without d_rois; there is no reach to write", msg);
    // (one workgroup per 1024-row tile of every frame, as many tiles per frame as the longest has)
    if ((int64_t)a.n_frames * ((sg_max_frame(a.max_frame_rows, a.n_total) + 1023) / 1024) > (((int64_t)1 << 31) - 1) / 16)
        return sg_refuse(who, ": n_frames * ceil(max_frame_rows / 1024) exceeds 2^27 - 1; split the batch", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, F = (size_t)a.n_frames, elems = F * (size_t)a.n_samples, n = (size_t)a.n_total, S = (size_t)s.n_sectors;
    const size_t q = s.rois ? F * (size_t)s.n_rois : 0;
    const SgOutSpan outs[8] = {
        {a.out_index, elems * 4, "d_out_index"}, {a.out_points, elems * (size_t)a.n_features * esz, "d_out_points"}, {a.out_dist, elems * esz, "d_out_dist"},
        {a.out_usable, F * 4, "d_out_usable"}, {s.out_sector_offsets, F * (S + 1) * 4, "d_out_sector_offsets"}, {s.out_sector_count, F * S * 4, "d_out_sector_count"},
        {s.out_sector_of, n, "d_out_sector_of"}, {s.out_reach2, q * 8, "d_out_reach2"}};
    const SgInSpan ins[3] = {{a.keep_in, n, "d_keep_in", "the mask is", "it"}, {a.rows, n * 5 * esz, "d_rows", "the rows are", "them"},
                             {s.rois, q * (size_t)s.roi_features * esz, "d_rois", "the rois are", "them"}};
    return sg_check_overlaps(who, outs, ins, "the samples are", true, msg);
}

// ---- snowgpu_ball_query_device ------------------------------------------------------------------------------------------------------------
struct SgBallArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    const double *range6;             // (x0, y0, z0, x1, y1, z1), host memory, or NULL: no range test
    int n_centres;                    // K, per frame
    const void *centres;
    int centre_features;              // Cq
    int n_radii;                      // R
    const double *radii;              // host memory
    const int *n_samples;             // host memory
    int n_features;                   // C
    const uint8_t *keep_in;
    int32_t *out_index, *out_count;
    void *out_points;                 // or NULL
    int64_t max_cells;                // cells per frame that the grid may take (the cell budget of the batch)
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.  *total = the sum of the samples where the call is accepted.
// The outputs are not compared with each other.
static inline int sg_check_ball_args(const SgBallArgs &a, int64_t *total, std::string *msg)
{
    static const char *who = "snowgpu_ball_query_device";
    if (int rc = sg_check_batch_head(who, a, !a.centres || !a.radii || !a.n_samples || !a.out_index || !a.out_count || (a.n_total > 0 && !a.rows), msg)) return rc;
    if (a.n_features < 3 || a.n_features > 5) return sg_refuse(who, ": n_features must be 3, 4 or 5: the columns of a row that a neighbour carries", msg);
    if (a.centre_features < 3 || a.centre_features > 5) return sg_refuse(who, ": centre_features must be 3, 4 or 5: x, y, z first", msg);
    if (a.n_centres < 1) return sg_refuse(who, ": n_centres must be at least 1", msg);
    if (a.n_radii < 1 || a.n_radii > 4) return sg_refuse(who, ": n_radii must lie in 1 .. 4", msg);
    int64_t S = 0;
    for (int i = 0; i < a.n_radii; ++i) {
        if (!(a.radii[i] > 0.0 && a.radii[i] <= 1e6)) return sg_refuse(who, ": a radius must be finite, above 0 and at most 1e6", msg);
        if (a.n_samples[i] < 1 || a.n_samples[i] > 64) return sg_refuse(who, ": the samples of a radius must lie in 1 .. 64", msg);
        S += a.n_samples[i];
    }
    if ((int64_t)a.n_frames * a.n_centres > (((int64_t)1 << 31) - 1) / S)      // (F K S <= 2^31 - 1, without the product of three)
        return sg_refuse(who, ": n_frames * n_centres * samples exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    if ((int64_t)a.n_frames * (a.max_cells + 1) >= ((int64_t)1 << 31)) return sg_refuse(who, ": too many frames for the cell lists; split the batch", msg);
    if (int rc = sg_check_range6(who, a.range6, msg)) return rc;
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_centres, n = (size_t)a.n_total;
    const SgOutSpan outs[3] = {
        {a.out_index, q * (size_t)S * 4, "d_out_index"}, {a.out_count, q * (size_t)a.n_radii * 4, "d_out_count"},
        {a.out_points, q * (size_t)S * (size_t)a.n_features * esz, "d_out_points"}};
    const SgInSpan ins[3] = {{a.keep_in, n, "d_keep_in", "the mask is", "it"}, {a.rows, n * 5 * esz, "d_rows", "the rows are", "them"},
                             {a.centres, q * (size_t)a.centre_features * esz, "d_centres", "the centres are", "them"}};
    if (int rc = sg_check_overlaps(who, outs, ins, "the groups are", false, msg)) return rc;
    if (total) *total = S;
    return 0;
}

// ---- snowgpu_range_image_device -----------------------------------------------------------------------------------------------------------
struct SgRangeArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    int H, W;
    const double *fov2;               // (up, down) in radians, host memory; NULL in channel mode
    const int32_t *ring;              // one channel per row, or NULL: rows by elevation
    const double *limits2;            // (lo, hi), host memory, or NULL: (0, +inf)
    int n_features;                   // C
    const uint8_t *keep_in;
    void *out_image;
    int32_t *out_index, *out_pixel_of;
    int32_t *out_count;               // or NULL
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI: here the mode is asked for between the two halves of the head.
static inline int sg_check_range_args(const SgRangeArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_range_image_device";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, a.n_total < 0 || !a.frame_off || !a.out_image || !a.out_index || (a.n_total > 0 && (!a.rows || !a.out_pixel_of)), msg))
        return rc;
    if (!a.fov2 && !a.ring) return sg_refuse(who, ": needs fov2 (image rows by elevation) or d_ring (image rows by channel)", msg);
    if (int rc = sg_check_rows(a.n_total, msg)) return rc;
    if (a.n_features < 3 || a.n_features > 5) return sg_refuse(who, ": n_features must be 3, 4 or 5: the columns of a row that a pixel stores", msg);
    if (a.H < 1 || a.W < 1) return sg_refuse(who, ": height and width must be at least 1", msg);
    if ((int64_t)a.n_frames * a.H > (((int64_t)1 << 31) - 1) / a.W)       // (F H W <= 2^31 - 1, without the product of three)
        return sg_refuse(who, ": n_frames * height * width exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    if (!a.ring) {
        const double half_pi = 1.5707963267948966;
        for (int j = 0; j < 2; ++j)
            if (!(a.fov2[j] >= -half_pi && a.fov2[j] <= half_pi)) return sg_refuse(who, ": fov_up and fov_down must lie within [-pi/2, pi/2] (radians)", msg);
        if (!(a.fov2[1] < a.fov2[0])) return sg_refuse(who, ": the field of view needs fov_down < fov_up", msg);
    }
    if (a.limits2) {
        if (a.limits2[0] != a.limits2[0] || a.limits2[1] != a.limits2[1]) return sg_refuse(who, ": a range limit is NaN; pass NULL for (0, +inf)", msg);
        if (!(a.limits2[0] >= 0.0 && a.limits2[0] < a.limits2[1])) return sg_refuse(who, ": the range limits need 0 <= lo < hi", msg);
    }
    const size_t esz = a.dtype == 0 ? 4 : 8, px = (size_t)a.n_frames * (size_t)a.H * (size_t)a.W, n = (size_t)a.n_total;
    const SgOutSpan outs[4] = {
        {a.out_image, px * (size_t)(1 + a.n_features) * esz, "d_out_image"}, {a.out_index, px * 4, "d_out_index"},
        {a.out_pixel_of, n * 4, "d_out_pixel_of"}, {a.out_count, px * 4, "d_out_count"}};
    const SgInSpan ins[3] = {{a.keep_in, n, "d_keep_in", "the mask is", "it"}, {a.rows, n * 5 * esz, "d_rows", "the rows are", "them"},
                             {a.ring, n * 4, "d_ring", "the channels are", "them"}};
    return sg_check_overlaps(who, outs, ins, "the image is", true, msg);
}

// ---- snowgpu_nearest_centres_device -------------------------------------------------------------------------------------------------------
struct SgNnArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    const double *range6;             // (x0, y0, z0, x1, y1, z1), host memory, or NULL: no range test
    int n_centres;                    // K, per frame
    const void *centres;
    int centre_features;              // Cq
    int k;                            // neighbours of a row
    const uint8_t *keep_in;
    int32_t *out_index;
    void *out_dist2;
    void *out_weight;                 // or NULL
    int64_t max_cells;                // cells per frame that the grid may take
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_nn_args(const SgNnArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_nearest_centres_device";
    if (int rc = sg_check_batch_head(who, a, !a.centres || (a.n_total > 0 && (!a.rows || !a.out_index || !a.out_dist2)), msg)) return rc;
    if (a.centre_features < 3 || a.centre_features > 5) return sg_refuse(who, ": centre_features must be 3, 4 or 5: x, y, z first", msg);
    if (a.n_centres < 1) return sg_refuse(who, ": n_centres must be at least 1", msg);
    if (a.k < 1 || a.k > 8) return sg_refuse(who, ": k must lie in 1 .. 8", msg);
    if ((int64_t)a.n_frames * a.n_centres > ((int64_t)1 << 31) - 1) return sg_refuse(who, ": n_frames * n_centres exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    if ((int64_t)a.n_frames * (a.max_cells + 1) >= ((int64_t)1 << 31)) return sg_refuse(who, ": too many frames for the cell lists; split the batch", msg);
    if (int rc = sg_check_range6(who, a.range6, msg)) return rc;
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_centres, n = (size_t)a.n_total, slots = n * (size_t)a.k;
    const SgOutSpan outs[3] = {{a.out_index, slots * 4, "d_out_index"}, {a.out_dist2, slots * esz, "d_out_dist2"}, {a.out_weight, slots * esz, "d_out_weight"}};
    const SgInSpan ins[3] = {{a.keep_in, n, "d_keep_in", "the mask is", "it"}, {a.rows, n * 5 * esz, "d_rows", "the rows are", "them"},
                             {a.centres, q * (size_t)a.centre_features * esz, "d_centres", "the centres are", "them"}};
    return sg_check_overlaps(who, outs, ins, "the neighbours are", true, msg);
}

// ---- snowgpu_points_in_boxes_device -------------------------------------------------------------------------------------------------------
struct SgBoxArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    int n_boxes;                      // B, per frame
    const void *boxes;
    int box_features;                 // Cb
    const double *pose_in;            // or NULL: cos / sin of the heading on the device
    const uint8_t *keep_in;
    int32_t *out_box_of;
    int32_t *out_count;               // or NULL
    void *out_local;                  // or NULL
    double *out_pose;                 // or NULL
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_box_args(const SgBoxArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_points_in_boxes_device";
    if (int rc = sg_check_batch_head(who, a, !a.boxes || (a.n_total > 0 && (!a.rows || !a.out_box_of)), msg)) return rc;
    if (a.n_boxes < 1 || a.n_boxes > 256) return sg_refuse(who, ": n_boxes must lie in 1 .. 256", msg);
    if (a.box_features < 7 || a.box_features > 10) return sg_refuse(who, ": box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if ((int64_t)a.n_frames * a.n_boxes > ((int64_t)1 << 31) - 1) return sg_refuse(who, ": n_frames * n_boxes exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_boxes, n = (size_t)a.n_total;
    const SgOutSpan outs[4] = {
        {a.out_box_of, n * 4, "d_out_box_of"}, {a.out_count, q * 4, "d_out_count"}, {a.out_local, n * 3 * esz, "d_out_local"}, {a.out_pose, q * 16, "d_out_pose"}};
    const SgInSpan ins[4] = {{a.keep_in, n, "d_keep_in", "the mask is", "it"}, {a.rows, n * 5 * esz, "d_rows", "the rows are", "them"},
                             {a.boxes, q * (size_t)a.box_features * esz, "d_boxes", "the boxes are", "them"}, {a.pose_in, q * 16, "d_pose_in", "the pose is", "it"}};
    return sg_check_overlaps(who, outs, ins, "the labels are", true, msg);
}

// ---- snowgpu_roi_point_pool_device --------------------------------------------------------------------------------------------------------
struct SgRoiPoolArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    int n_rois;                       // M, per frame
    const void *rois;
    int roi_features;                 // Cb
    const double *extra_width;        // host, 3 doubles, or NULL: zeros
    int n_samples;                    // S
    int num_features;                 // C
    const double *pose_in;            // or NULL: cos / sin of the heading on the device
    const uint8_t *keep_in;
    int32_t *out_index;
    int32_t *out_count;
    void *out_points;                 // or NULL
    void *out_local;                  // or NULL
    double *out_pose;                 // or NULL
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_roipool_args(const SgRoiPoolArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_roi_point_pool_device", *read = "the mask, the rows, the rois and the pose are";
    if (int rc = sg_check_batch_head(who, a, !a.rois || !a.out_index || !a.out_count || (a.n_total > 0 && !a.rows), msg)) return rc;
    if (a.n_rois < 1 || a.n_rois > 512) return sg_refuse(who, ": n_rois must lie in 1 .. 512", msg);
    if (a.roi_features < 7 || a.roi_features > 10) return sg_refuse(who, ": roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if (a.n_samples < 1 || a.n_samples > 2048) return sg_refuse(who, ": n_samples must lie in 1 .. 2048", msg);
    if (a.num_features < 3 || a.num_features > 5) return sg_refuse(who, ": num_features must be 3, 4 or 5: the columns of a row that a roi stores", msg);
    if (int rc = sg_check_extra_width(who, a.extra_width, msg)) return rc;
    if ((int64_t)a.n_frames * a.n_rois * a.n_samples * (a.num_features > 3 ? a.num_features : 3) > ((int64_t)1 << 31) - 1)
        return sg_refuse(who, ": n_frames * n_rois * n_samples * max(num_features, 3) exceeds 2^31 - 1; split the batch", msg);
    const int64_t longest = sg_max_frame(a.max_frame_rows, a.n_total);
    if (int rc = sg_check_frame(who, longest, msg)) return rc;
    if ((int64_t)a.n_frames * a.n_rois * (longest / 512 + 1) > ((int64_t)1 << 31) - 1)    // (n_frames n_rois < 2^31 by the sample check)
        return sg_refuse(who, ": n_frames * n_rois * the 512-row runs of the longest frame exceeds 2^31 - 1; split the batch", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_rois, n = (size_t)a.n_total, k = q * (size_t)a.n_samples;
    const SgOutSpan outs[5] = {
        {a.out_index, k * 4, "d_out_index"}, {a.out_count, q * 4, "d_out_count"}, {a.out_points, k * (size_t)a.num_features * esz, "d_out_points"},
        {a.out_local, k * 3 * esz, "d_out_local"}, {a.out_pose, q * 16, "d_out_pose"}};
    const SgInSpan ins[4] = {{a.keep_in, n, "d_keep_in", read, "them"}, {a.rows, n * 5 * esz, "d_rows", read, "them"},
                             {a.rois, q * (size_t)a.roi_features * esz, "d_rois", read, "them"}, {a.pose_in, q * 16, "d_pose_in", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the pool is", true, msg);
}

// ---- snowgpu_roi_voxel_pool_device --------------------------------------------------------------------------------------------------------
struct SgRoiAwareArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    int n_rois;                       // M, per frame
    const void *rois;
    int roi_features;                 // Cb
    const double *extra_width;        // host, 3 doubles, or NULL: zeros
    const int32_t *out_size;          // host, 3 ints: Gx, Gy, Gz
    int max_points;                   // T
    int roi_capacity;                 // P
    const float *features;            // (N_total, Cf) float32, or NULL: no pooled output
    int feature_channels;             // Cf (not read without features)
    const double *pose_in;            // or NULL: cos / sin of the heading on the device
    const uint8_t *keep_in;
    int32_t *out_roi_count;
    int32_t *out_count;
    int32_t *out_index;               // or NULL
    float *out_max;                   // or NULL
    int32_t *out_argmax;              // or NULL
    float *out_avg;                   // or NULL
    double *out_pose;                 // or NULL
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_roiaware_args(const SgRoiAwareArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_roi_voxel_pool_device", *read = "the mask, the rows, the rois, the pose and the features are";
    if (int rc = sg_check_batch_head(who, a, !a.rois || !a.out_size || !a.out_roi_count || !a.out_count || (a.n_total > 0 && !a.rows), msg)) return rc;
    if (a.n_rois < 1 || a.n_rois > 512) return sg_refuse(who, ": n_rois must lie in 1 .. 512", msg);
    if (a.roi_features < 7 || a.roi_features > 10) return sg_refuse(who, ": roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if (int rc = sg_check_extra_width(who, a.extra_width, msg)) return rc;
    for (int j = 0; j < 3; ++j)
        if (a.out_size[j] < 1 || a.out_size[j] > 16) return sg_refuse(who, ": every component of out_size must lie in 1 .. 16", msg);
    if (a.max_points < 1 || a.max_points > 128) return sg_refuse(who, ": max_points must lie in 1 .. 128", msg);
    if (a.roi_capacity < 64 || a.roi_capacity > 65536) return sg_refuse(who, ": roi_capacity must lie in 64 .. 65536", msg);
    const bool pooled = a.out_max || a.out_argmax || a.out_avg;
    if (pooled && !a.features && a.n_total > 0)                                              // (a batch without a row has no feature to point to)
        return sg_refuse(who, ": d_out_max, d_out_argmax and d_out_avg need d_features; there is nothing to pool", msg);
    if ((pooled || a.features) && (a.feature_channels < 1 || a.feature_channels > 256)) return sg_refuse(who, ": feature_channels must lie in 1 .. 256", msg);
    const int64_t G = (int64_t)a.out_size[0] * a.out_size[1] * a.out_size[2], Cf = (pooled || a.features) ? a.feature_channels : 1;
    if ((int64_t)a.n_frames * a.n_rois * G * (a.max_points > Cf ? (int64_t)a.max_points : Cf) > ((int64_t)1 << 31) - 1)       // (each factor is small: no overflow)
        return sg_refuse(who, ": n_frames * n_rois * the voxels of a roi * max(max_points, feature_channels) exceeds 2^31 - 1; split the batch", msg);
    if ((int64_t)a.n_frames * a.n_rois * a.roi_capacity > ((int64_t)1 << 31) - 1)
        return sg_refuse(who, ": n_frames * n_rois * roi_capacity exceeds 2^31 - 1; split the batch or lower the capacity", msg);
    const int64_t longest = sg_max_frame(a.max_frame_rows, a.n_total);
    if (int rc = sg_check_frame(who, longest, msg)) return rc;
    if ((int64_t)a.n_frames * a.n_rois * (longest / 512 + 1) > ((int64_t)1 << 31) - 1)    // (n_frames n_rois < 2^31 by the element check)
        return sg_refuse(who, ": n_frames * n_rois * the 512-row runs of the longest frame exceeds 2^31 - 1; split the batch", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_rois, n = (size_t)a.n_total, v = q * (size_t)G, k = v * (size_t)Cf;
    const SgOutSpan outs[7] = {
        {a.out_roi_count, q * 4, "d_out_roi_count"}, {a.out_count, v * 4, "d_out_count"}, {a.out_index, v * (size_t)a.max_points * 4, "d_out_index"},
        {a.out_max, k * 4, "d_out_max"}, {a.out_argmax, k * 4, "d_out_argmax"}, {a.out_avg, k * 4, "d_out_avg"}, {a.out_pose, q * 16, "d_out_pose"}};
    const SgInSpan ins[5] = {{a.keep_in, n, "d_keep_in", read, "them"}, {a.rows, n * 5 * esz, "d_rows", read, "them"},
                             {a.rois, q * (size_t)a.roi_features * esz, "d_rois", read, "them"}, {a.pose_in, q * 16, "d_pose_in", read, "them"},
                             {a.features, n * (size_t)Cf * 4, "d_features", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the voxels are", true, msg);
}

// ---- snowgpu_boxes_iou_device -------------------------------------------------------------------------------------------------------------
struct SgIouArgs {
    int n_frames;
    int n_a;                          // M, per frame
    const void *boxes_a;
    int a_features;
    int n_b;                          // B, per frame
    const void *boxes_b;
    int b_features;
    int dtype, mode;
    const double *pose_a, *pose_b;    // or NULL: cos / sin of the heading on the device
    void *out_iou;                    // or NULL
    int32_t *out_best;                // or NULL
    void *out_best_iou;               // or NULL
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_iou_args(const SgIouArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_boxes_iou_device", *read = "the boxes and poses are";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, !a.boxes_a || !a.boxes_b, msg)) return rc;
    if (a.mode != 0 && a.mode != 1) return sg_refuse(who, ": mode must be 0 (BEV) or 1 (3D)", msg);
    if (!a.out_iou && !a.out_best && !a.out_best_iou) return sg_refuse(who, ": no output: pass d_out_iou, d_out_best or d_out_best_iou", msg);
    if (a.n_a < 1 || a.n_a > 9216 || a.n_b < 1 || a.n_b > 9216) return sg_refuse(who, ": the boxes per frame must lie in 1 .. 9216 on either side", msg);
    if (a.a_features < 7 || a.a_features > 10 || a.b_features < 7 || a.b_features > 10)
        return sg_refuse(who, ": box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if ((int64_t)a.n_frames * a.n_a * a.n_b > ((int64_t)1 << 31) - 1) return sg_refuse(who, ": n_frames * M * B exceeds 2^31 - 1; split the batch", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, qa = (size_t)a.n_frames * (size_t)a.n_a, qb = (size_t)a.n_frames * (size_t)a.n_b;
    const SgOutSpan outs[3] = {{a.out_iou, qa * (size_t)a.n_b * esz, "d_out_iou"}, {a.out_best, qa * 4, "d_out_best"}, {a.out_best_iou, qa * esz, "d_out_best_iou"}};
    const SgInSpan ins[4] = {{a.boxes_a, qa * (size_t)a.a_features * esz, "d_boxes_a", read, "them"}, {a.boxes_b, qb * (size_t)a.b_features * esz, "d_boxes_b", read, "them"},
                             {a.pose_a, qa * 16, "d_pose_a", read, "them"}, {a.pose_b, qb * 16, "d_pose_b", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the overlaps are", true, msg);
}

// ---- snowgpu_nms_device -------------------------------------------------------------------------------------------------------------------
struct SgNmsArgs {
    int n_frames;
    int n_boxes;                      // B, per frame
    const void *boxes;
    int box_features;
    const void *scores;
    int dtype, mode;
    double iou_thresh, score_thresh;
    int post_max;
    const double *pose_in;            // or NULL
    int32_t *out_index, *out_count;
    void *out_boxes, *out_scores;     // or NULL
    uint8_t *out_kept;                // or NULL
};

static inline int sg_check_nms_args(const SgNmsArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_nms_device", *read = "the boxes, scores and pose are";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, !a.boxes || !a.scores || !a.out_index || !a.out_count, msg)) return rc;
    if (a.mode != 0 && a.mode != 1) return sg_refuse(who, ": mode must be 0 (BEV) or 1 (3D)", msg);
    if (a.n_boxes < 1 || a.n_boxes > 9216) return sg_refuse(who, ": n_boxes must lie in 1 .. 9216", msg);
    if (a.box_features < 7 || a.box_features > 10) return sg_refuse(who, ": box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if (a.post_max < 1 || a.post_max > a.n_boxes) return sg_refuse(who, ": post_max must lie in 1 .. n_boxes", msg);
    if (a.iou_thresh != a.iou_thresh || a.score_thresh != a.score_thresh) return sg_refuse(who, ": a threshold is NaN", msg);
    if ((int64_t)a.n_frames * a.n_boxes > ((int64_t)1 << 31) - 1) return sg_refuse(who, ": n_frames * n_boxes exceeds 2^31 - 1; split the batch", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_boxes, k = (size_t)a.n_frames * (size_t)a.post_max;
    const SgOutSpan outs[5] = {
        {a.out_index, k * 4, "d_out_index"}, {a.out_count, (size_t)a.n_frames * 4, "d_out_count"}, {a.out_boxes, k * (size_t)a.box_features * esz, "d_out_boxes"},
        {a.out_scores, k * esz, "d_out_scores"}, {a.out_kept, q, "d_out_kept"}};
    const SgInSpan ins[3] = {{a.boxes, q * (size_t)a.box_features * esz, "d_boxes", read, "them"}, {a.scores, q * esz, "d_scores", read, "them"},
                             {a.pose_in, q * 16, "d_pose_in", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the keep list is", true, msg);
}

// ---- snowgpu_sample_rois_device -----------------------------------------------------------------------------------------------------------
struct SgSamplerCfg {                 // snowgpu_roi_sampler (include/snowgpu.h), field for field
    int roi_per_image, fg_per_image;
    double reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo, hard_bg_ratio;
    int cls_mode;
};

struct SgTargetsArgs {
    int n_frames;
    int n_rois;                       // M, per frame
    const void *rois;
    int roi_features;                 // Cb
    const void *overlap;
    const int32_t *assignment;
    int n_gt;                         // B, per frame
    const void *gt_boxes;
    int gt_features;                  // Cg
    int dtype;
    const SgSamplerCfg *cfg;          // host
    const uint64_t *step;             // device
    const double *pose_in;            // or NULL: cos / sin of the heading on the device
    int32_t *out_index;
    void *out_rois, *out_roi_iou;
    int32_t *out_gt_index;
    void *out_gt_of_rois;
    uint8_t *out_reg_valid;
    void *out_cls_label;
    int32_t *out_segments, *out_class_count;
    double *out_pose;                 // or NULL
    void *out_gt_local;               // or NULL
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_targets_args(const SgTargetsArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_sample_rois_device", *read = "the rois, overlaps, assignments, gt boxes, step and pose are";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, !a.rois || !a.overlap || !a.assignment || !a.gt_boxes || !a.cfg || !a.step || !a.out_index || !a.out_rois ||
                                   !a.out_roi_iou || !a.out_gt_index || !a.out_gt_of_rois || !a.out_reg_valid || !a.out_cls_label || !a.out_segments || !a.out_class_count, msg))
        return rc;
    const SgSamplerCfg &c = *a.cfg;
    if (a.n_rois < 1 || a.n_rois > 9216 || a.n_gt < 1 || a.n_gt > 9216) return sg_refuse(who, ": n_rois and n_gt must lie in 1 .. 9216", msg);
    if (a.roi_features < 7 || a.roi_features > 10 || a.gt_features < 7 || a.gt_features > 10)
        return sg_refuse(who, ": roi_features and gt_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if (c.roi_per_image < 1 || c.roi_per_image > 1024) return sg_refuse(who, ": roi_per_image must lie in 1 .. 1024", msg);
    if (c.fg_per_image < 0 || c.fg_per_image > c.roi_per_image) return sg_refuse(who, ": fg_per_image must lie in 0 .. roi_per_image", msg);
    if (!std::isfinite(c.reg_fg_thresh) || !std::isfinite(c.cls_fg_thresh) || !std::isfinite(c.cls_bg_thresh) || !std::isfinite(c.cls_bg_thresh_lo))
        return sg_refuse(who, ": a threshold is NaN or infinite", msg);
    if (!(c.cls_fg_thresh > c.cls_bg_thresh)) return sg_refuse(who, ": cls_fg_thresh must be above cls_bg_thresh", msg);
    if (!(c.hard_bg_ratio >= 0.0 && c.hard_bg_ratio <= 1.0)) return sg_refuse(who, ": hard_bg_ratio must lie in 0 .. 1", msg);      // (false for NaN)
    if (c.cls_mode != 0 && c.cls_mode != 1) return sg_refuse(who, ": cls_mode must be 0 (roi_iou) or 1 (cls)", msg);
    const int64_t widest = a.roi_features > a.gt_features ? a.roi_features : a.gt_features;
    if ((int64_t)a.n_frames * c.roi_per_image * widest > ((int64_t)1 << 31) - 1)
        return sg_refuse(who, ": n_frames * roi_per_image * max(roi_features, gt_features) exceeds 2^31 - 1; split the batch", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_rois, g = (size_t)a.n_frames * (size_t)a.n_gt,
                 k = (size_t)a.n_frames * (size_t)c.roi_per_image;
    const SgOutSpan outs[11] = {
        {a.out_index, k * 4, "d_out_index"}, {a.out_rois, k * (size_t)a.roi_features * esz, "d_out_rois"}, {a.out_roi_iou, k * esz, "d_out_roi_iou"},
        {a.out_gt_index, k * 4, "d_out_gt_index"}, {a.out_gt_of_rois, k * (size_t)a.gt_features * esz, "d_out_gt_of_rois"}, {a.out_reg_valid, k, "d_out_reg_valid"},
        {a.out_cls_label, k * esz, "d_out_cls_label"}, {a.out_segments, (size_t)a.n_frames * 12, "d_out_segments"},
        {a.out_class_count, (size_t)a.n_frames * 12, "d_out_class_count"}, {a.out_pose, k * 16, "d_out_pose"}, {a.out_gt_local, k * 7 * esz, "d_out_gt_local"}};
    const SgInSpan ins[6] = {{a.rois, q * (size_t)a.roi_features * esz, "d_rois", read, "them"}, {a.overlap, q * esz, "d_overlap", read, "them"},
                             {a.assignment, q * 4, "d_assignment", read, "them"}, {a.gt_boxes, g * (size_t)a.gt_features * esz, "d_gt_boxes", read, "them"},
                             {a.step, 8, "d_step", read, "them"}, {a.pose_in, q * 16, "d_pose", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the targets are", true, msg);
}

// ---- snowgpu_assign_anchors_device --------------------------------------------------------------------------------------------------------
struct SgAnchorsArgs {
    int n_frames;
    int n_anchors;                    // A, shared by all frames
    const void *anchors;
    int anchor_features;              // Ca
    const int32_t *anchor_class;
    int n_gt;                         // B, per frame
    const void *gt_boxes;
    int gt_features;                  // Cg: column 7 is the class
    int dtype;
    int n_classes;                    // NC
    const double *matched, *unmatched;        // host, NC each
    int32_t *out_label, *out_gt_index, *out_count, *out_gt_count;
    void *out_iou;                    // or NULL
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_anchors_args(const SgAnchorsArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_assign_anchors_device", *read = "the anchors, their classes and the gt boxes are";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, !a.anchors || !a.anchor_class || !a.gt_boxes || !a.matched || !a.unmatched || !a.out_label || !a.out_gt_index ||
                                   !a.out_count || !a.out_gt_count, msg))
        return rc;
    if (a.n_anchors < 1) return sg_refuse(who, ": n_anchors must be at least 1", msg);
    if (a.n_gt < 1 || a.n_gt > 256) return sg_refuse(who, ": n_gt must lie in 1 .. 256", msg);
    if (a.anchor_features < 7 || a.anchor_features > 10)
        return sg_refuse(who, ": anchor_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if (a.gt_features < 8 || a.gt_features > 10)
        return sg_refuse(who, ": gt_features must lie in 8 .. 10: cx, cy, cz, dx, dy, dz, heading, class first", msg);
    if (a.n_classes < 1 || a.n_classes > 16) return sg_refuse(who, ": n_classes must lie in 1 .. 16", msg);
    for (int c = 0; c < a.n_classes; ++c)
        if (!(0.0 < a.unmatched[c] && a.unmatched[c] <= a.matched[c] && a.matched[c] <= 1.0))                                  // (false for NaN)
            return sg_refuse(who, ": every class needs 0 < unmatched <= matched <= 1", msg);
    if ((int64_t)a.n_frames * a.n_anchors > ((int64_t)1 << 31) - 1) return sg_refuse(who, ": n_frames * n_anchors exceeds 2^31 - 1; split the batch", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)a.n_anchors, g = (size_t)a.n_frames * (size_t)a.n_gt;
    const SgOutSpan outs[5] = {
        {a.out_label, q * 4, "d_out_label"}, {a.out_gt_index, q * 4, "d_out_gt_index"}, {a.out_count, (size_t)a.n_frames * 12, "d_out_count"},
        {a.out_gt_count, g * 4, "d_out_gt_count"}, {a.out_iou, q * esz, "d_out_iou"}};
    const SgInSpan ins[3] = {{a.anchors, (size_t)a.n_anchors * (size_t)a.anchor_features * esz, "d_anchors", read, "them"},
                             {a.anchor_class, (size_t)a.n_anchors * 4, "d_anchor_class", read, "them"}, {a.gt_boxes, g * (size_t)a.gt_features * esz, "d_gt_boxes", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the targets are", true, msg);
}

// ---- snowgpu_assign_centers_device --------------------------------------------------------------------------------------------------------
struct SgCentersCfg {                 // snowgpu_center_cfg (include/snowgpu.h), field for field
    double x0, y0, vx, vy, gaussian_overlap;
    int32_t stride, width, height, n_classes, n_heads, max_objs, min_radius, outside;
    int32_t class_head[16];
};

struct SgCentersArgs {
    int n_frames;
    int n_gt;                         // B, per frame
    const void *gt_boxes;
    int gt_features;                  // Cg: column 7 is the class
    int dtype;
    const SgCentersCfg *cfg;          // host
    float *out_heatmap;
    int32_t *out_gt_index, *out_ind;
    uint8_t *out_mask;
    void *out_offset;
    int32_t *out_radius, *out_count;
    uint8_t *out_state;
};

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_centers_args(const SgCentersArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_assign_centers_device", *read = "the gt boxes are";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, !a.gt_boxes || !a.cfg || !a.out_heatmap || !a.out_gt_index || !a.out_ind || !a.out_mask || !a.out_offset ||
                                   !a.out_radius || !a.out_count || !a.out_state, msg))
        return rc;
    const SgCentersCfg &c = *a.cfg;
    if (a.n_gt < 1 || a.n_gt > 256) return sg_refuse(who, ": n_gt must lie in 1 .. 256", msg);
    if (a.gt_features < 8 || a.gt_features > 10)
        return sg_refuse(who, ": gt_features must lie in 8 .. 10: cx, cy, cz, dx, dy, dz, heading, class first", msg);
    if (c.n_classes < 1 || c.n_classes > 16) return sg_refuse(who, ": n_classes must lie in 1 .. 16", msg);
    if (c.n_heads < 1 || c.n_heads > 16) return sg_refuse(who, ": n_heads must lie in 1 .. 16", msg);
    for (int k = 0; k < c.n_classes; ++k)
        if (c.class_head[k] < 0 || c.class_head[k] >= c.n_heads) return sg_refuse(who, ": every class needs a head in 0 .. n_heads - 1", msg);
    if (c.max_objs < 1 || c.max_objs > 512) return sg_refuse(who, ": max_objs must lie in 1 .. 512", msg);
    if (c.width < 1 || c.height < 1) return sg_refuse(who, ": the feature map needs at least one pixel on either axis", msg);
    if ((int64_t)c.width * c.height > ((int64_t)1 << 31) - 1 || (int64_t)a.n_frames * c.n_classes * ((int64_t)c.width * c.height) > ((int64_t)1 << 31) - 1)
        return sg_refuse(who, ": n_frames * n_classes * height * width exceeds 2^31 - 1; split the batch", msg);
    if (!std::isfinite(c.x0) || !std::isfinite(c.y0) || !(c.vx > 0.0) || !(c.vy > 0.0) || !std::isfinite(c.vx) || !std::isfinite(c.vy))          // (false for NaN)
        return sg_refuse(who, ": the origin of the range must be finite, the voxel's x and y edges positive and finite", msg);
    if (c.stride < 1) return sg_refuse(who, ": stride must be at least 1", msg);
    if (!(c.gaussian_overlap > 0.0 && c.gaussian_overlap < 1.0)) return sg_refuse(who, ": gaussian_overlap must lie strictly between 0 and 1", msg);      // (false for NaN)
    if (c.min_radius < 0 || c.min_radius > 512) return sg_refuse(who, ": min_radius must lie in 0 .. 512", msg);
    if (c.outside != 0 && c.outside != 1) return sg_refuse(who, ": outside must be 0 (clamp) or 1 (drop)", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, q = (size_t)a.n_frames * (size_t)c.n_heads * (size_t)c.max_objs, g = (size_t)a.n_frames * (size_t)a.n_gt;
    const SgOutSpan outs[8] = {
        {a.out_heatmap, (size_t)a.n_frames * (size_t)c.n_classes * (size_t)c.height * (size_t)c.width * 4, "d_out_heatmap"}, {a.out_gt_index, q * 4, "d_out_gt_index"},
        {a.out_ind, q * 4, "d_out_ind"}, {a.out_mask, q, "d_out_mask"}, {a.out_offset, q * 2 * esz, "d_out_offset"}, {a.out_radius, q * 4, "d_out_radius"},
        {a.out_count, (size_t)a.n_frames * (size_t)c.n_heads * 4, "d_out_count"}, {a.out_state, g, "d_out_state"}};
    const SgInSpan ins[1] = {{a.gt_boxes, g * (size_t)a.gt_features * esz, "d_gt_boxes", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the targets are", true, msg);
}

// ---- snowgpu_paste_objects_device ---------------------------------------------------------------------------------------------------------
struct SgPasteArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    int n_gt;                         // B, per frame
    const void *gt_boxes;
    int gt_features;                  // Cb: column 7 is the class
    const double *pose_in;            // or NULL: cos / sin of the heading on the device
    int64_t bank_points_n, bank_objects_n;        // P, O
    const void *bank_points;
    const int64_t *bank_off;
    const void *bank_boxes;
    const double *bank_pose;
    const int32_t *class_off;         // 18 int32
    int n_classes;                    // NC
    const int32_t *groups;            // host, NC counts
    const double *extra_width;        // host, 3 doubles, or NULL: zeros
    const uint64_t *step;             // device
    const uint8_t *keep_in;           // or NULL: every row is present
    void *out_rows;
    uint8_t *out_keep;
    void *out_gt_boxes;
    int32_t *out_object, *out_state;
    int32_t *out_source;              // or NULL
    int32_t *out_count;
    double *out_pose;                 // or NULL
};

// the sum of the first min(NC, 16) sample groups, 0 without any
static inline int64_t sg_paste_slots(int n_classes, const int32_t *groups)
{
    int64_t Q = 0;
    for (int c = 0; groups && c < n_classes && c < 16; ++c) Q += groups[c];
    return Q;
}

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_paste_args(const SgPasteArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_paste_objects_device", *read = "the mask, the rows, the gt boxes, the pose, the bank and the step are";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, a.n_total < 0 || !a.frame_off || !a.gt_boxes || !a.bank_off || !a.bank_boxes || !a.bank_pose || !a.class_off ||
                                   !a.groups || !a.out_gt_boxes || !a.out_object || !a.out_state || !a.out_count || a.bank_points_n < 0 || a.bank_objects_n < 0 ||
                                   (a.bank_points_n > 0 && !a.bank_points) || (a.n_total > 0 && (!a.rows || !a.out_rows || !a.out_keep)), msg))
        return rc;
    const int64_t Q = sg_paste_slots(a.n_classes, a.groups);
    if (Q < 1 || Q > 64) return sg_refuse(who, ": the sample groups must add up to 1 .. 64 slots", msg);
    if (a.n_classes < 1 || a.n_classes > 16) return sg_refuse(who, ": n_classes must lie in 1 .. 16", msg);
    if (a.n_gt < 1 || (int64_t)a.n_gt + Q > 256) return sg_refuse(who, ": n_gt must be at least 1 and n_gt plus the slots at most 256", msg);
    if (a.gt_features < 8 || a.gt_features > 10)
        return sg_refuse(who, ": gt_features must lie in 8 .. 10: cx, cy, cz, dx, dy, dz, heading, class first", msg);
    for (int c = 0; c < a.n_classes; ++c)
        if (a.groups[c] < 0) return sg_refuse(who, ": a sample group is negative", msg);
    if (int rc = sg_check_extra_width(who, a.extra_width, msg)) return rc;
    if ((int64_t)a.n_frames * (a.n_gt + Q) * a.gt_features > ((int64_t)1 << 31) - 1)
        return sg_refuse(who, ": n_frames * (n_gt + slots) * gt_features exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_rows(a.n_total, msg)) return rc;
    if (a.bank_points_n >= ((int64_t)1 << 31) || a.bank_objects_n >= ((int64_t)1 << 31)) return sg_refuse(who, ": the bank must stay below 2^31 points and objects", msg);
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    if (!a.step) return sg_refuse(who, ": d_step is NULL; one uint64 in device memory", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, n = (size_t)a.n_total, F = (size_t)a.n_frames, g = F * (size_t)a.n_gt, k = F * (size_t)(a.n_gt + Q),
                 P = (size_t)a.bank_points_n, O = (size_t)a.bank_objects_n;
    const SgOutSpan outs[8] = {
        {a.out_rows, n * 5 * esz, "d_out_rows"}, {a.out_keep, n, "d_out_keep"}, {a.out_gt_boxes, k * (size_t)a.gt_features * esz, "d_out_gt_boxes"},
        {a.out_object, F * (size_t)Q * 4, "d_out_object"}, {a.out_state, F * (size_t)Q * 4, "d_out_state"}, {a.out_source, n * 4, "d_out_source"},
        {a.out_count, F * 16, "d_out_count"}, {a.out_pose, k * 16, "d_out_pose"}};
    const SgInSpan ins[11] = {{a.keep_in, n, "d_keep_in", read, "them"}, {a.rows, n * 5 * esz, "d_rows", read, "them"}, {a.frame_off, (F + 1) * 8, "d_frame_offsets", read, "them"},
                              {a.gt_boxes, g * (size_t)a.gt_features * esz, "d_gt_boxes", read, "them"}, {a.pose_in, g * 16, "d_pose_in", read, "them"},
                              {a.bank_points, P * 5 * esz, "d_bank_points", read, "them"}, {a.bank_off, (O + 1) * 8, "d_bank_offsets", read, "them"},
                              {a.bank_boxes, O * 8 * esz, "d_bank_boxes", read, "them"}, {a.bank_pose, O * 16, "d_bank_pose", read, "them"},
                              {a.class_off, 18 * 4, "d_class_offsets", read, "them"}, {a.step, 8, "d_step", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the batch is", true, msg);
}

// ---- snowgpu_transform_scene_device -------------------------------------------------------------------------------------------------------
struct SgSceneArgs {
    int n_frames;
    int64_t n_total, max_frame_rows;
    int dtype;
    const int64_t *frame_off;
    const void *rows;
    int n_boxes;                      // B, per frame
    const void *gt_boxes;
    int box_features;                 // Cb
    const double *pose_in;            // or NULL: cos / sin of the heading on the device
    int flip;                         // bit 0: x, bit 1: y
    const double *rotation, *scaling; // host, 2 doubles (lo, hi) each, or NULL: the part is off
    int tries;                        // T; 0: no local part, and the three below are not read
    const double *local_translation;  // host, 3 doubles, or NULL
    const double *local_rotation, *local_scaling;     // host, 2 doubles each, or NULL
    const uint64_t *step;             // device
    const int32_t *box_of;            // or NULL: made in scratch when there is a local part
    const uint8_t *keep_in;           // or NULL: every row is present
    void *out_rows;                   // may BE rows: the in-place form
    uint8_t *out_keep;
    void *out_gt_boxes;
    double *out_world;
    int32_t *out_state, *out_tried;
    double *out_local;
    double *out_pose;                 // or NULL
    double *out_tries;                // or NULL
};

// lo, hi of a range, or NULL: off
static inline bool sg_scene_range_ok(const double *r) { return !r || (std::isfinite(r[0]) && std::isfinite(r[1]) && r[0] <= r[1]); }

// 0, or SG_ARGS_INVALID with *msg.  As above, the order is part of the ABI.
static inline int sg_check_scene_args(const SgSceneArgs &a, std::string *msg)
{
    static const char *who = "snowgpu_transform_scene_device", *read = "the mask, the rows, the boxes, the pose, box_of and the step are";
    if (int rc = sg_check_head(who, a.n_frames, a.dtype, a.n_total < 0 || !a.frame_off || !a.gt_boxes || !a.out_gt_boxes || !a.out_world || !a.out_state || !a.out_tried ||
                                   !a.out_local || (a.n_total > 0 && (!a.rows || !a.out_rows || !a.out_keep)), msg))
        return rc;
    if (a.n_boxes < 1 || a.n_boxes > 256) return sg_refuse(who, ": n_boxes must lie in 1 .. 256", msg);
    if (a.box_features < 7 || a.box_features > 10) return sg_refuse(who, ": box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first", msg);
    if (a.flip < 0 || a.flip > 3) return sg_refuse(who, ": flip must lie in 0 .. 3: bit 0 the x axis, bit 1 the y axis", msg);
    if (a.tries < 0 || a.tries > 16) return sg_refuse(who, ": tries must lie in 0 .. 16", msg);
    const bool local = a.tries > 0;
    if (!sg_scene_range_ok(a.rotation) || !sg_scene_range_ok(a.scaling) || (local && (!sg_scene_range_ok(a.local_rotation) || !sg_scene_range_ok(a.local_scaling))))
        return sg_refuse(who, ": a range must be finite with lo <= hi", msg);
    if ((a.scaling && !(a.scaling[0] > 0.0)) || (local && a.local_scaling && !(a.local_scaling[0] > 0.0))) return sg_refuse(who, ": a scaling range must be above 0", msg);
    for (int j = 0; local && a.local_translation && j < 3; ++j)
        if (!(a.local_translation[j] >= 0.0 && a.local_translation[j] <= 100.0))             // (false for NaN)
            return sg_refuse(who, ": every component of the local translation must be finite and lie in 0 .. 100", msg);
    if ((int64_t)a.n_frames * a.n_boxes * (a.tries > 0 ? a.tries : 1) * 10 > ((int64_t)1 << 31) - 1)
        return sg_refuse(who, ": n_frames * n_boxes * max(tries, 1) * 10 exceeds 2^31 - 1; split the batch", msg);
    if (int rc = sg_check_rows(a.n_total, msg)) return rc;
    if (int rc = sg_check_frame(who, sg_max_frame(a.max_frame_rows, a.n_total), msg)) return rc;
    if (!a.step) return sg_refuse(who, ": d_step is NULL; one uint64 in device memory", msg);
    const size_t esz = a.dtype == 0 ? 4 : 8, n = (size_t)a.n_total, F = (size_t)a.n_frames, q = F * (size_t)a.n_boxes;
    const bool in_place = a.out_rows && a.out_rows == a.rows;                                // (the row kernel reads and writes its own row only)
    const SgOutSpan outs[9] = {
        {a.out_rows, n * 5 * esz, "d_out_rows"}, {a.out_keep, n, "d_out_keep"}, {a.out_gt_boxes, q * (size_t)a.box_features * esz, "d_out_gt_boxes"},
        {a.out_world, F * 64, "d_out_world"}, {a.out_state, q * 4, "d_out_state"}, {a.out_tried, q * 4, "d_out_tried"}, {a.out_local, q * 64, "d_out_local"},
        {a.out_pose, q * 16, "d_out_pose"}, {a.out_tries, q * (size_t)a.tries * 64, "d_out_tries"}};
    const SgInSpan ins[7] = {{a.keep_in, n, "d_keep_in", read, "them"}, {in_place ? nullptr : a.rows, n * 5 * esz, "d_rows", read, "them"},
                             {a.frame_off, (F + 1) * 8, "d_frame_offsets", read, "them"}, {a.gt_boxes, q * (size_t)a.box_features * esz, "d_gt_boxes", read, "them"},
                             {a.pose_in, q * 16, "d_pose_in", read, "them"}, {local ? a.box_of : nullptr, n * 4, "d_box_of", read, "them"}, {a.step, 8, "d_step", read, "them"}};
    return sg_check_overlaps(who, outs, ins, "the scene is", true, msg);
}

// 0, or SG_ARGS_INVALID with *msg (built on this path only).  The order is part of the ABI: it decides which message a doubly wrong call gets.
static inline int sg_check_device_args(const SgDeviceArgs &a, const SgCtxView &c, const SgEntryShape &s, std::string *msg)
{
    if (s.weather && !a.weather) return sg_refuse(a.who, ": d_weather is NULL; one record of 8 doubles per frame, in device memory", msg);
    const bool buffers = s.empty_null_ok ? (a.n_total > 0 && (!a.rows || !a.out_rows || !a.out_keep))
                                         : ((a.n_total > 0 && !a.rows) || !a.out_rows || !(s.aligned ? (const void *)a.out_keep : (const void *)a.out_src));
    if (a.n_frames <= 0 || a.n_total < 0 || !a.frame_off || buffers || (s.tables && (!a.table_ids || !a.out_stats)) || !a.out_counts ||
        (s.wet && !a.out_flags) || !a.status || (a.dtype != 0 && a.dtype != 1))
        return sg_refuse(a.who, ": null pointer or bad dtype", msg);
    if (a.n_total >= ((int64_t)1 << 31)) return sg_refuse("", "batch too large: split it below 2^31 rows", msg);
    if (!s.aligned) return 0;                      // the compact entries refuse nothing else
    if (c.thr_fn) return sg_refuse(a.who, ": a threshold callback is set; it finishes batches through the compaction only", msg);
    if (c.result_mode != 0) return sg_refuse(a.who, ": the packed result transfer is set; it is a form of the compacted result", msg);
    if (sg_overlap(a.rows, a.out_rows, (size_t)a.n_total * 5 * (a.dtype == 0 ? 4 : 8)))
        return sg_refuse(a.who, ": d_out_rows overlaps d_rows; pass d_rows itself (in place) or a buffer apart from it", msg);
    if (sg_overlap(a.keep_in, a.out_keep, (size_t)a.n_total))
        return sg_refuse(a.who, ": d_out_keep overlaps d_keep_in; pass d_keep_in itself or a buffer apart from it", msg);
    if (s.tables && s.wet)                         // (before anything is launched)
        if (int rc = sg_check_wet_plane(a.who, a.wet_plane, c.plane_method, msg)) return rc;
    if (s.masked && a.perm) return sg_refuse_perm(a.who, s.weather ? "d_weather" : "d_keep_in", msg);
    // (what run_batch needs for the segment order of the pass over all rows; the linear order reads n_total as an exact count)
    if (s.masked && a.n_total > 0 && (c.n_tables > 65536 || a.n_frames > (1 << 22)))
        return sg_refuse(a.who, ": a masked batch needs at most 65536 tables and 2^22 frames", msg);
    return 0;
}
