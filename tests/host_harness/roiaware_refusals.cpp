// roiaware_refusals.cpp -- snowgpu_roi_voxel_pool_device through every refusal of sg_check_roiaware_args (csrc/sg_device_args.h), one defect
// at a time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_roiaware_reference.py compares the lines with a table.
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, M = 3 rois of 8 columns, G = 2 x 1 x 2 voxels,
// T = 2 members, Cf = 3 channels (padded: no range below leaves its array)
static float g_rows[8 * 5 + 100], g_rois[2 * 3 * 8 + 40], g_features[8 * 3 + 100], g_max[2 * 3 * 4 * 3 + 40], g_avg[2 * 3 * 4 * 3 + 40];
static double g_pose_in[2 * 3 * 2 + 64], g_pose[2 * 3 * 2 + 16];
static uint8_t g_keep[8 + 200];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_roi_count[2 * 3 + 100], g_count[2 * 3 * 4 + 100], g_index[2 * 3 * 4 * 2 + 100], g_argmax[2 * 3 * 4 * 3 + 100];
static double g_ew[3] = {0.5, 0.25, 1.0};
static int32_t g_grid[3] = {2, 1, 2};

static void clean_call(SgRoiAwareArgs &a)
{
    a = SgRoiAwareArgs{2, 8, 4, 0, g_off, g_rows, 3, g_rois, 8, g_ew, g_grid, 2, 64, g_features, 3, g_pose_in, g_keep,
                       g_roi_count, g_count, g_index, g_max, g_argmax, g_avg, g_pose};
}

// (sizes larger than the host arrays that stand for them: nothing is given to overlap)
static void bare(SgRoiAwareArgs &a)
{
    a.out_index = nullptr; a.out_max = nullptr; a.out_argmax = nullptr; a.out_avg = nullptr; a.out_pose = nullptr; a.keep_in = nullptr; a.rows = nullptr;
    a.pose_in = nullptr; a.features = nullptr; a.n_total = 0;
    a.rois = (const void *)(uintptr_t)((uint64_t)1 << 44);
    a.out_roi_count = (int32_t *)(uintptr_t)((uint64_t)1 << 45); a.out_count = (int32_t *)(uintptr_t)((uint64_t)1 << 46);
}

int main()
{
    using Edit = std::function<void(SgRoiAwareArgs &)>;
    static double ew_neg[3] = {0.0, -0.001, 0.0}, ew_big[3] = {0.0, 0.0, 100.5}, ew_nan[3] = {std::numeric_limits<double>::quiet_NaN(), 0.0, 0.0},
                  ew_inf[3] = {0.0, std::numeric_limits<double>::infinity(), 0.0}, ew_edge[3] = {0.0, 100.0, 0.0};
    static int32_t grid_0[3] = {2, 0, 2}, grid_17[3] = {2, 2, 17}, grid_neg[3] = {-1, 2, 2}, grid_1[3] = {1, 1, 1}, grid_16[3] = {16, 16, 16};
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgRoiAwareArgs &) {}},
        {"null_frame_offsets", [](SgRoiAwareArgs &a) { a.frame_off = nullptr; }},
        {"null_rows", [](SgRoiAwareArgs &a) { a.rows = nullptr; }},
        {"null_rois", [](SgRoiAwareArgs &a) { a.rois = nullptr; }},
        {"null_out_size", [](SgRoiAwareArgs &a) { a.out_size = nullptr; }},
        {"null_out_roi_count", [](SgRoiAwareArgs &a) { a.out_roi_count = nullptr; }},
        {"null_out_count", [](SgRoiAwareArgs &a) { a.out_count = nullptr; }},
        {"null_out_index", [](SgRoiAwareArgs &a) { a.out_index = nullptr; }},
        {"null_out_max", [](SgRoiAwareArgs &a) { a.out_max = nullptr; }},
        {"null_out_argmax", [](SgRoiAwareArgs &a) { a.out_argmax = nullptr; }},
        {"null_out_avg", [](SgRoiAwareArgs &a) { a.out_avg = nullptr; }},
        {"null_out_pose", [](SgRoiAwareArgs &a) { a.out_pose = nullptr; }},
        {"null_pose_in", [](SgRoiAwareArgs &a) { a.pose_in = nullptr; }},
        {"null_keep_in", [](SgRoiAwareArgs &a) { a.keep_in = nullptr; }},
        {"null_extra_width", [](SgRoiAwareArgs &a) { a.extra_width = nullptr; }},
        {"no_features_no_pool", [](SgRoiAwareArgs &a) { a.features = nullptr; a.feature_channels = 0; a.out_max = nullptr; a.out_argmax = nullptr; a.out_avg = nullptr; }},
        {"no_features_max", [](SgRoiAwareArgs &a) { a.features = nullptr; a.out_argmax = nullptr; a.out_avg = nullptr; }},
        {"no_features_argmax", [](SgRoiAwareArgs &a) { a.features = nullptr; a.out_max = nullptr; a.out_avg = nullptr; }},
        {"no_features_avg", [](SgRoiAwareArgs &a) { a.features = nullptr; a.out_max = nullptr; a.out_argmax = nullptr; }},
        {"bad_dtype", [](SgRoiAwareArgs &a) { a.dtype = 2; }},
        {"float64", [](SgRoiAwareArgs &a) { a.dtype = 1; bare(a); }},
        {"no_frames", [](SgRoiAwareArgs &a) { a.n_frames = 0; }},
        {"negative_rows", [](SgRoiAwareArgs &a) { a.n_total = -1; }},
        {"empty_null_rows", [](SgRoiAwareArgs &a) { a.n_total = 0; a.rows = nullptr; }},
        {"empty_null_features", [](SgRoiAwareArgs &a) { a.n_total = 0; a.rows = nullptr; a.features = nullptr; }},
        {"rows_2p31", [](SgRoiAwareArgs &a) { a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; a.features = nullptr; }},
        {"rois_0", [](SgRoiAwareArgs &a) { a.n_rois = 0; }},
        {"rois_1", [](SgRoiAwareArgs &a) { a.n_rois = 1; }},
        {"rois_512", [](SgRoiAwareArgs &a) { a.n_rois = 512; bare(a); }},
        {"rois_513", [](SgRoiAwareArgs &a) { a.n_rois = 513; }},
        {"rois_negative", [](SgRoiAwareArgs &a) { a.n_rois = -4; }},
        {"roi_features_6", [](SgRoiAwareArgs &a) { a.roi_features = 6; }},
        {"roi_features_7", [](SgRoiAwareArgs &a) { a.roi_features = 7; }},
        {"roi_features_10", [](SgRoiAwareArgs &a) { a.roi_features = 10; bare(a); }},
        {"roi_features_11", [](SgRoiAwareArgs &a) { a.roi_features = 11; }},
        {"extra_width_negative", [](SgRoiAwareArgs &a) { a.extra_width = ew_neg; }},
        {"extra_width_above_100", [](SgRoiAwareArgs &a) { a.extra_width = ew_big; }},
        {"extra_width_nan", [](SgRoiAwareArgs &a) { a.extra_width = ew_nan; }},
        {"extra_width_inf", [](SgRoiAwareArgs &a) { a.extra_width = ew_inf; }},
        {"extra_width_100", [](SgRoiAwareArgs &a) { a.extra_width = ew_edge; }},
        {"out_size_0", [](SgRoiAwareArgs &a) { a.out_size = grid_0; }},
        {"out_size_17", [](SgRoiAwareArgs &a) { a.out_size = grid_17; }},
        {"out_size_negative", [](SgRoiAwareArgs &a) { a.out_size = grid_neg; }},
        {"out_size_1", [](SgRoiAwareArgs &a) { a.out_size = grid_1; }},
        {"out_size_16", [](SgRoiAwareArgs &a) { a.out_size = grid_16; bare(a); }},
        {"points_0", [](SgRoiAwareArgs &a) { a.max_points = 0; }},
        {"points_1", [](SgRoiAwareArgs &a) { a.max_points = 1; }},
        {"points_128", [](SgRoiAwareArgs &a) { a.max_points = 128; bare(a); }},
        {"points_129", [](SgRoiAwareArgs &a) { a.max_points = 129; }},
        {"capacity_63", [](SgRoiAwareArgs &a) { a.roi_capacity = 63; }},
        {"capacity_65536", [](SgRoiAwareArgs &a) { a.roi_capacity = 65536; }},
        {"capacity_65537", [](SgRoiAwareArgs &a) { a.roi_capacity = 65537; }},
        {"channels_0", [](SgRoiAwareArgs &a) { a.feature_channels = 0; }},
        {"channels_1", [](SgRoiAwareArgs &a) { a.feature_channels = 1; }},
        {"channels_256", [](SgRoiAwareArgs &a) { bare(a); a.features = (const float *)(uintptr_t)((uint64_t)1 << 43); a.feature_channels = 256; }},
        {"channels_257", [](SgRoiAwareArgs &a) { a.feature_channels = 257; }},
        // F M G max(T, Cf): 1023 x 4 x 4096 x 128 = 2145386496 fits, 1024 x 4 x 4096 x 128 = 2^31 does not, by T = 128 or by Cf = 128
        {"elements_below_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 1023; a.n_rois = 4; a.out_size = grid_16; a.max_points = 128; }},
        {"elements_above_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 1024; a.n_rois = 4; a.out_size = grid_16; a.max_points = 128; }},
        {"elements_by_channels", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 1024; a.n_rois = 4; a.out_size = grid_16; a.max_points = 1;
                                                         a.features = (const float *)(uintptr_t)((uint64_t)1 << 43); a.feature_channels = 128; }},
        {"elements_overflowing", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 2147483647; a.n_rois = 512; a.out_size = grid_16; a.max_points = 128; }},
        // F M P: 63 x 512 x 65536 = 2113929216 fits, 64 x 512 x 65536 = 2^31 does not
        {"list_below_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 63; a.n_rois = 512; a.out_size = grid_1; a.roi_capacity = 65536; }},
        {"list_above_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 64; a.n_rois = 512; a.out_size = grid_1; a.roi_capacity = 65536; }},
        {"frame_2p30_rows", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 1; a.n_rois = 1; a.n_total = (int64_t)1 << 30; a.max_frame_rows = 0;
                                                    a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"frame_2p30_plus_1_rows", [](SgRoiAwareArgs &a) { a.n_frames = 1; a.n_rois = 1; a.n_total = ((int64_t)1 << 30) + 1; a.max_frame_rows = 0; }},
        // the run table: F M (longest / 512 + 1); 1 x 512 x (2^30 / 512 + 1) = 2^30 + 512 fits, 2 frames of it do not
        {"runs_below_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 1; a.n_rois = 512; a.out_size = grid_1; a.n_total = (int64_t)1 << 30; a.max_frame_rows = 0;
                                                    a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"runs_above_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 2; a.n_rois = 512; a.out_size = grid_1; a.n_total = ((int64_t)1 << 31) - 1;
                                                    a.max_frame_rows = (int64_t)1 << 30; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"roi_count_is_keep_in", [](SgRoiAwareArgs &a) { a.out_roi_count = (int32_t *)g_keep; }},
        {"count_overlaps_keep_in", [](SgRoiAwareArgs &a) { a.keep_in = (const uint8_t *)g_count + 95; }},      // its last byte
        {"keep_in_behind_count", [](SgRoiAwareArgs &a) { a.keep_in = (const uint8_t *)g_count + 96; }},
        {"index_overlaps_rows", [](SgRoiAwareArgs &a) { a.out_index = (int32_t *)g_rows + 39; }},              // the rows' last element
        {"index_behind_rows", [](SgRoiAwareArgs &a) { a.out_index = (int32_t *)g_rows + 40; }},
        {"max_is_rois", [](SgRoiAwareArgs &a) { a.out_max = g_rois; }},
        {"argmax_overlaps_pose_in", [](SgRoiAwareArgs &a) { a.out_argmax = (int32_t *)(g_pose_in + 3); }},
        {"avg_is_features", [](SgRoiAwareArgs &a) { a.out_avg = g_features; }},
        {"max_overlaps_features", [](SgRoiAwareArgs &a) { a.out_max = g_features + 23; }},                     // the features' last element
        {"max_behind_features", [](SgRoiAwareArgs &a) { a.out_max = g_features + 24; }},
        {"pose_is_pose_in", [](SgRoiAwareArgs &a) { a.out_pose = g_pose_in; }},
        {"count_is_roi_count", [](SgRoiAwareArgs &a) { a.out_count = g_roi_count; }},
        {"count_behind_roi_count", [](SgRoiAwareArgs &a) { a.out_count = g_roi_count + 6; }},
        {"index_overlaps_count", [](SgRoiAwareArgs &a) { a.out_index = g_count + 23; }},
        {"max_overlaps_index", [](SgRoiAwareArgs &a) { a.out_max = (float *)g_index + 47; }},
        {"argmax_is_max", [](SgRoiAwareArgs &a) { a.out_argmax = (int32_t *)g_max; }},
        {"avg_overlaps_argmax", [](SgRoiAwareArgs &a) { a.out_avg = (float *)g_argmax + 71; }},
        {"avg_behind_argmax", [](SgRoiAwareArgs &a) { a.out_avg = (float *)g_argmax + 72; }},
        {"pose_overlaps_avg", [](SgRoiAwareArgs &a) { a.out_pose = (double *)g_avg + 35; }},
        {"pose_overlaps_roi_count", [](SgRoiAwareArgs &a) { a.out_roi_count = (int32_t *)g_pose + 23; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](SgRoiAwareArgs &a) { a.frame_off = nullptr; a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; a.features = nullptr; }},
        {"rows_2p31_and_rois_0", [](SgRoiAwareArgs &a) { a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; a.features = nullptr; a.n_rois = 0; }},
        {"rois_0_and_roi_features_6", [](SgRoiAwareArgs &a) { a.n_rois = 0; a.roi_features = 6; }},
        {"roi_features_6_and_extra_width_nan", [](SgRoiAwareArgs &a) { a.roi_features = 6; a.extra_width = ew_nan; }},
        {"extra_width_nan_and_out_size_0", [](SgRoiAwareArgs &a) { a.extra_width = ew_nan; a.out_size = grid_0; }},
        {"out_size_0_and_points_0", [](SgRoiAwareArgs &a) { a.out_size = grid_0; a.max_points = 0; }},
        {"points_0_and_capacity_63", [](SgRoiAwareArgs &a) { a.max_points = 0; a.roi_capacity = 63; }},
        {"capacity_63_and_no_features_max", [](SgRoiAwareArgs &a) { a.roi_capacity = 63; a.features = nullptr; a.out_argmax = nullptr; a.out_avg = nullptr; }},
        {"no_features_max_and_channels_0", [](SgRoiAwareArgs &a) { a.features = nullptr; a.out_argmax = nullptr; a.out_avg = nullptr; a.feature_channels = 0; }},
        {"channels_257_and_elements_above_2p31", [](SgRoiAwareArgs &a) { bare(a); a.features = (const float *)(uintptr_t)((uint64_t)1 << 43); a.feature_channels = 257;
                                                                         a.n_frames = 1024; a.n_rois = 4; a.out_size = grid_16; a.max_points = 128; }},
        {"elements_above_2p31_and_list_above_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 64; a.n_rois = 512; a.out_size = grid_16; a.max_points = 128; a.roi_capacity = 65536; }},
        {"list_above_2p31_and_frame_2p30_plus_1_rows", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 64; a.n_rois = 512; a.out_size = grid_1; a.roi_capacity = 65536;
                                                                               a.n_total = ((int64_t)1 << 30) + 1; a.max_frame_rows = 0; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"frame_2p30_plus_1_rows_and_runs_above_2p31", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 2; a.n_rois = 512; a.out_size = grid_1; a.n_total = ((int64_t)1 << 31) - 1;
                                                                               a.max_frame_rows = ((int64_t)1 << 30) + 1; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"runs_above_2p31_and_roi_count_is_rows", [](SgRoiAwareArgs &a) { bare(a); a.n_frames = 2; a.n_rois = 512; a.out_size = grid_1; a.n_total = ((int64_t)1 << 31) - 1;
                                                                          a.max_frame_rows = (int64_t)1 << 30; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40);
                                                                          a.out_roi_count = (int32_t *)(uintptr_t)((uint64_t)1 << 40); }},
    };
    for (const auto &cs : cases) {
        SgRoiAwareArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_roiaware_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
