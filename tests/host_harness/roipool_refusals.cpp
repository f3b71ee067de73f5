// roipool_refusals.cpp -- snowgpu_roi_point_pool_device through every refusal of sg_check_roipool_args (csrc/sg_device_args.h), one defect
// at a time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_roipool_reference.py compares the lines with a table.
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, M = 3 rois of 8 columns, S = 2 samples of C = 4
// (padded: no range below leaves its array)
static float g_rows[8 * 5 + 40], g_rois[2 * 3 * 8 + 40], g_points[2 * 3 * 2 * 4 + 40], g_local[2 * 3 * 2 * 3 + 40];
static double g_pose_in[2 * 3 * 2 + 16], g_pose[2 * 3 * 2 + 16];
static uint8_t g_keep[8 + 200];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_index[2 * 3 * 2 + 100], g_count[2 * 3 + 100];
static double g_ew[3] = {0.5, 0.25, 1.0};

static void clean_call(SgRoiPoolArgs &a)
{
    a = SgRoiPoolArgs{2, 8, 4, 0, g_off, g_rows, 3, g_rois, 8, g_ew, 2, 4, g_pose_in, g_keep, g_index, g_count, g_points, g_local, g_pose};
}

// (sizes larger than the host arrays that stand for them: nothing is given to overlap)
static void bare(SgRoiPoolArgs &a)
{
    a.out_points = nullptr; a.out_local = nullptr; a.out_pose = nullptr; a.keep_in = nullptr; a.rows = nullptr; a.pose_in = nullptr; a.n_total = 0;
    a.rois = (const void *)(uintptr_t)((uint64_t)1 << 44);
    a.out_index = (int32_t *)(uintptr_t)((uint64_t)1 << 45); a.out_count = (int32_t *)(uintptr_t)((uint64_t)1 << 46);
}

int main()
{
    using Edit = std::function<void(SgRoiPoolArgs &)>;
    static double ew_neg[3] = {0.0, -0.001, 0.0}, ew_big[3] = {0.0, 0.0, 100.5}, ew_nan[3] = {std::numeric_limits<double>::quiet_NaN(), 0.0, 0.0},
                  ew_inf[3] = {0.0, std::numeric_limits<double>::infinity(), 0.0}, ew_edge[3] = {0.0, 100.0, 0.0};
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgRoiPoolArgs &) {}},
        {"null_frame_offsets", [](SgRoiPoolArgs &a) { a.frame_off = nullptr; }},
        {"null_rows", [](SgRoiPoolArgs &a) { a.rows = nullptr; }},
        {"null_rois", [](SgRoiPoolArgs &a) { a.rois = nullptr; }},
        {"null_out_index", [](SgRoiPoolArgs &a) { a.out_index = nullptr; }},
        {"null_out_count", [](SgRoiPoolArgs &a) { a.out_count = nullptr; }},
        {"null_out_points", [](SgRoiPoolArgs &a) { a.out_points = nullptr; }},
        {"null_out_local", [](SgRoiPoolArgs &a) { a.out_local = nullptr; }},
        {"null_out_pose", [](SgRoiPoolArgs &a) { a.out_pose = nullptr; }},
        {"null_pose_in", [](SgRoiPoolArgs &a) { a.pose_in = nullptr; }},
        {"null_keep_in", [](SgRoiPoolArgs &a) { a.keep_in = nullptr; }},
        {"null_extra_width", [](SgRoiPoolArgs &a) { a.extra_width = nullptr; }},
        {"bad_dtype", [](SgRoiPoolArgs &a) { a.dtype = 2; }},
        {"float64", [](SgRoiPoolArgs &a) { a.dtype = 1; bare(a); }},
        {"no_frames", [](SgRoiPoolArgs &a) { a.n_frames = 0; }},
        {"negative_rows", [](SgRoiPoolArgs &a) { a.n_total = -1; }},
        {"empty_null_rows", [](SgRoiPoolArgs &a) { a.n_total = 0; a.rows = nullptr; }},
        {"rows_2p31", [](SgRoiPoolArgs &a) { a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; }},
        {"rois_0", [](SgRoiPoolArgs &a) { a.n_rois = 0; }},
        {"rois_1", [](SgRoiPoolArgs &a) { a.n_rois = 1; }},
        {"rois_512", [](SgRoiPoolArgs &a) { a.n_rois = 512; bare(a); }},
        {"rois_513", [](SgRoiPoolArgs &a) { a.n_rois = 513; }},
        {"rois_negative", [](SgRoiPoolArgs &a) { a.n_rois = -4; }},
        {"roi_features_6", [](SgRoiPoolArgs &a) { a.roi_features = 6; }},
        {"roi_features_7", [](SgRoiPoolArgs &a) { a.roi_features = 7; }},
        {"roi_features_10", [](SgRoiPoolArgs &a) { a.roi_features = 10; bare(a); }},
        {"roi_features_11", [](SgRoiPoolArgs &a) { a.roi_features = 11; }},
        {"samples_0", [](SgRoiPoolArgs &a) { a.n_samples = 0; }},
        {"samples_1", [](SgRoiPoolArgs &a) { a.n_samples = 1; }},
        {"samples_2048", [](SgRoiPoolArgs &a) { a.n_samples = 2048; bare(a); }},
        {"samples_2049", [](SgRoiPoolArgs &a) { a.n_samples = 2049; }},
        {"features_2", [](SgRoiPoolArgs &a) { a.num_features = 2; }},
        {"features_3", [](SgRoiPoolArgs &a) { a.num_features = 3; }},
        {"features_5", [](SgRoiPoolArgs &a) { a.num_features = 5; bare(a); }},
        {"features_6", [](SgRoiPoolArgs &a) { a.num_features = 6; }},
        {"extra_width_negative", [](SgRoiPoolArgs &a) { a.extra_width = ew_neg; }},
        {"extra_width_above_100", [](SgRoiPoolArgs &a) { a.extra_width = ew_big; }},
        {"extra_width_nan", [](SgRoiPoolArgs &a) { a.extra_width = ew_nan; }},
        {"extra_width_inf", [](SgRoiPoolArgs &a) { a.extra_width = ew_inf; }},
        {"extra_width_100", [](SgRoiPoolArgs &a) { a.extra_width = ew_edge; }},
        // F M S max(C, 3): 1023 x 341 x 2048 x 3 = 2143291392 fits, 1024 x 342 x 2048 x 3 = 2151677952 does not
        {"elements_below_2p31", [](SgRoiPoolArgs &a) { a.n_frames = 1023; a.n_rois = 341; a.n_samples = 2048; a.num_features = 3; bare(a); }},
        {"elements_above_2p31", [](SgRoiPoolArgs &a) { a.n_frames = 1024; a.n_rois = 342; a.n_samples = 2048; a.num_features = 3; bare(a); }},
        {"elements_overflowing", [](SgRoiPoolArgs &a) { a.n_frames = 2147483647; a.n_rois = 512; a.n_samples = 2048; a.num_features = 5; bare(a); }},
        {"frame_2p30_rows", [](SgRoiPoolArgs &a) { a.n_frames = 1; a.n_rois = 1; a.n_total = (int64_t)1 << 30; a.max_frame_rows = 0; a.keep_in = nullptr;
                                                   a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"frame_2p30_plus_1_rows", [](SgRoiPoolArgs &a) { a.n_frames = 1; a.n_rois = 1; a.n_total = ((int64_t)1 << 30) + 1; a.max_frame_rows = 0; }},
        // the run table: F M (longest / 512 + 1); 1 x 512 x (2^30 / 512 + 1) = 2^30 + 512 fits, 2 frames of it do not
        {"runs_below_2p31", [](SgRoiPoolArgs &a) { bare(a); a.n_frames = 1; a.n_rois = 512; a.n_samples = 1; a.n_total = (int64_t)1 << 30; a.max_frame_rows = 0; a.keep_in = nullptr;
                                                   a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"runs_above_2p31", [](SgRoiPoolArgs &a) { bare(a); a.n_frames = 2; a.n_rois = 512; a.n_samples = 1; a.n_total = ((int64_t)1 << 31) - 1; a.max_frame_rows = (int64_t)1 << 30;
                                                   a.keep_in = nullptr; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"index_is_keep_in", [](SgRoiPoolArgs &a) { a.out_index = (int32_t *)g_keep; }},
        {"index_overlaps_keep_in", [](SgRoiPoolArgs &a) { a.keep_in = (const uint8_t *)g_index + 47; }},     // its last byte
        {"keep_in_behind_index", [](SgRoiPoolArgs &a) { a.keep_in = (const uint8_t *)g_index + 48; }},
        {"count_overlaps_rows", [](SgRoiPoolArgs &a) { a.out_count = (int32_t *)g_rows + 39; }},             // the rows' last element
        {"count_behind_rows", [](SgRoiPoolArgs &a) { a.out_count = (int32_t *)g_rows + 40; }},
        {"points_is_rois", [](SgRoiPoolArgs &a) { a.out_points = g_rois; }},
        {"local_overlaps_pose_in", [](SgRoiPoolArgs &a) { a.out_local = g_pose_in + 3; }},
        {"pose_is_pose_in", [](SgRoiPoolArgs &a) { a.out_pose = g_pose_in; }},
        {"pose_overlaps_rows", [](SgRoiPoolArgs &a) { a.rows = (const float *)g_pose + 4; }},
        {"count_is_index", [](SgRoiPoolArgs &a) { a.out_count = g_index; }},
        {"count_behind_index", [](SgRoiPoolArgs &a) { a.out_count = g_index + 12; }},
        {"points_overlaps_index", [](SgRoiPoolArgs &a) { a.out_points = (float *)g_index + 11; }},
        {"points_overlaps_count", [](SgRoiPoolArgs &a) { a.out_points = (float *)g_count + 5; }},
        {"local_is_points", [](SgRoiPoolArgs &a) { a.out_local = g_points; }},
        {"local_behind_points", [](SgRoiPoolArgs &a) { a.out_local = g_points + 48; }},
        {"pose_overlaps_local", [](SgRoiPoolArgs &a) { a.out_pose = (double *)g_local + 17; }},
        {"pose_overlaps_count", [](SgRoiPoolArgs &a) { a.out_count = (int32_t *)g_pose + 23; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](SgRoiPoolArgs &a) { a.frame_off = nullptr; a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; }},
        {"rows_2p31_and_rois_0", [](SgRoiPoolArgs &a) { a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; a.n_rois = 0; }},
        {"rois_0_and_roi_features_6", [](SgRoiPoolArgs &a) { a.n_rois = 0; a.roi_features = 6; }},
        {"roi_features_6_and_samples_0", [](SgRoiPoolArgs &a) { a.roi_features = 6; a.n_samples = 0; }},
        {"samples_0_and_features_2", [](SgRoiPoolArgs &a) { a.n_samples = 0; a.num_features = 2; }},
        {"features_2_and_extra_width_nan", [](SgRoiPoolArgs &a) { a.num_features = 2; a.extra_width = ew_nan; }},
        {"extra_width_nan_and_elements_above_2p31", [](SgRoiPoolArgs &a) { a.extra_width = ew_nan; a.n_frames = 1024; a.n_rois = 342; a.n_samples = 2048; a.num_features = 3; bare(a); }},
        {"elements_above_2p31_and_frame_2p30_plus_1_rows", [](SgRoiPoolArgs &a) { a.n_frames = 1024; a.n_rois = 342; a.n_samples = 2048; a.num_features = 3; bare(a);
                                                                                  a.n_total = ((int64_t)1 << 30) + 1; a.max_frame_rows = 0; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"frame_2p30_plus_1_rows_and_runs_above_2p31", [](SgRoiPoolArgs &a) { bare(a); a.n_frames = 2; a.n_rois = 512; a.n_samples = 1; a.n_total = ((int64_t)1 << 31) - 1;
                                                                              a.max_frame_rows = ((int64_t)1 << 30) + 1; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"runs_above_2p31_and_index_is_rows", [](SgRoiPoolArgs &a) { bare(a); a.n_frames = 2; a.n_rois = 512; a.n_samples = 1; a.n_total = ((int64_t)1 << 31) - 1; a.max_frame_rows = (int64_t)1 << 30;
                                                                     a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); a.out_index = (int32_t *)(uintptr_t)((uint64_t)1 << 40); }},
    };
    for (const auto &cs : cases) {
        SgRoiPoolArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_roipool_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
