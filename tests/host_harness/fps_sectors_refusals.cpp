// fps_sectors_refusals.cpp -- snowgpu_fps_sectors_device through every refusal of sg_check_fps_sectors_args (csrc/sg_device_args.h), one
// defect at a time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device:
// prints case|code|message.  tests/test_fps_sectors_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, K = 3, C = 4, S = 2, B = 2, Cb = 7
static float g_rows[8 * 5 + 8], g_points[2 * 3 * 4 + 8], g_dist[2 * 3 + 8], g_rois[2 * 2 * 7 + 8];
static uint8_t g_keep[8 + 32];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_index[2 * 3 + 8], g_usable[2 + 4], g_offsets[2 * 3 + 4], g_count[2 * 2 + 4];
static int8_t g_sector_of[8 + 8];
static double g_reach2[2 * 2 + 4];

struct Call {
    SgFpsSectorsArgs a;
    double range6[6];
};

static void clean_call(Call &k)
{
    const double r[6] = {0.0, -2.0, -1.0, 4.0, 2.0, 1.0};
    for (int i = 0; i < 6; ++i) k.range6[i] = r[i];
    k.a = SgFpsSectorsArgs{SgFpsArgs{2, 8, 4, 0, g_off, g_rows, k.range6, 3, 4, g_keep, g_index, g_points, g_dist, g_usable},
                           2, g_rois, 2, 7, 1.6, g_offsets, g_count, g_sector_of, g_reach2};
}

int main()
{
    using Edit = std::function<void(Call &)>;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](Call &) {}},
        {"null_frame_offsets", [](Call &k) { k.a.fps.frame_off = nullptr; }},
        {"null_rows", [](Call &k) { k.a.fps.rows = nullptr; }},
        {"null_out_index", [](Call &k) { k.a.fps.out_index = nullptr; }},
        {"null_out_usable", [](Call &k) { k.a.fps.out_usable = nullptr; }},
        {"null_out_sector_offsets", [](Call &k) { k.a.out_sector_offsets = nullptr; }},
        {"null_out_sector_count", [](Call &k) { k.a.out_sector_count = nullptr; }},
        {"null_out_points", [](Call &k) { k.a.fps.out_points = nullptr; }},
        {"null_out_dist", [](Call &k) { k.a.fps.out_dist = nullptr; }},
        {"null_out_sector_of", [](Call &k) { k.a.out_sector_of = nullptr; }},
        {"null_out_reach2", [](Call &k) { k.a.out_reach2 = nullptr; }},
        {"null_keep_in", [](Call &k) { k.a.fps.keep_in = nullptr; }},
        {"null_range", [](Call &k) { k.a.fps.range6 = nullptr; }},
        {"null_rois", [](Call &k) { k.a.rois = nullptr; k.a.out_reach2 = nullptr; k.a.n_rois = 0; k.a.roi_features = 0; k.a.roi_margin = -1.0; }},      // (not read)
        {"bad_dtype", [](Call &k) { k.a.fps.dtype = 2; }},
        {"float64", [](Call &k) { k.a.fps.dtype = 1; k.a.fps.rows = nullptr; k.a.fps.n_total = 0; k.a.rois = nullptr; k.a.out_reach2 = nullptr; k.a.fps.out_points = nullptr; k.a.fps.out_dist = nullptr; }},
        {"no_frames", [](Call &k) { k.a.fps.n_frames = 0; }},
        {"negative_rows", [](Call &k) { k.a.fps.n_total = -1; }},
        {"empty_null_rows", [](Call &k) { k.a.fps.n_total = 0; k.a.fps.rows = nullptr; k.a.fps.keep_in = nullptr; k.a.out_sector_of = nullptr; }},
        {"rows_2p31", [](Call &k) { k.a.fps.n_total = (int64_t)1 << 31; k.a.fps.keep_in = nullptr; }},
        {"features_2", [](Call &k) { k.a.fps.n_features = 2; }},
        {"features_6", [](Call &k) { k.a.fps.n_features = 6; }},
        {"samples_0", [](Call &k) { k.a.fps.n_samples = 0; }},
        {"samples_1", [](Call &k) { k.a.fps.n_samples = 1; }},
        {"frames_times_samples_2p31", [](Call &k) { k.a.fps.n_frames = 2; k.a.fps.n_samples = 1 << 30; }},
        {"frame_2p30_plus_1_rows", [](Call &k) { k.a.fps.n_total = ((int64_t)1 << 30) + 1; k.a.fps.max_frame_rows = 0; }},
        {"range_nan_lo", [&](Call &k) { k.range6[1] = nan; }},
        {"range_lo_is_hi", [](Call &k) { k.range6[3] = 0.0; }},
        {"range_infinite", [&](Call &k) { k.range6[0] = -inf; k.range6[3] = inf; k.range6[5] = inf; }},
        {"sectors_0", [](Call &k) { k.a.n_sectors = 0; }},
        {"sectors_1", [](Call &k) { k.a.n_sectors = 1; }},
        // (the outputs of 16 sectors are larger than the arrays that stand for them: they get addresses of their own)
        {"sectors_16", [](Call &k) { k.a.n_sectors = 16; k.a.out_sector_offsets = (int32_t *)(uintptr_t)((uint64_t)1 << 40); k.a.out_sector_count = (int32_t *)(uintptr_t)((uint64_t)1 << 41); }},
        {"sectors_17", [](Call &k) { k.a.n_sectors = 17; }},
        {"rois_0", [](Call &k) { k.a.n_rois = 0; }},
        {"rois_1", [](Call &k) { k.a.n_rois = 1; }},
        {"rois_256", [](Call &k) { k.a.n_rois = 256; k.a.rois = (const void *)(uintptr_t)((uint64_t)1 << 42); k.a.out_reach2 = nullptr; }},
        {"rois_257", [](Call &k) { k.a.n_rois = 257; }},
        {"roi_features_6", [](Call &k) { k.a.roi_features = 6; }},
        {"roi_features_10", [](Call &k) { k.a.roi_features = 10; k.a.rois = (const void *)(uintptr_t)((uint64_t)1 << 42); }},
        {"roi_features_11", [](Call &k) { k.a.roi_features = 11; }},
        {"margin_0", [](Call &k) { k.a.roi_margin = 0.0; }},
        {"margin_negative", [](Call &k) { k.a.roi_margin = -1e-300; }},
        {"margin_nan", [&](Call &k) { k.a.roi_margin = nan; }},
        {"margin_inf", [&](Call &k) { k.a.roi_margin = inf; }},
        {"reach2_without_rois", [](Call &k) { k.a.rois = nullptr; }},
        {"tiles_2p27", [](Call &k) { k.a.fps.n_frames = 1 << 17; k.a.fps.n_samples = 1; k.a.fps.n_total = (int64_t)1 << 30; k.a.fps.max_frame_rows = 1 << 20; k.a.fps.keep_in = nullptr; }},
        {"index_is_keep_in", [](Call &k) { k.a.fps.out_index = (int32_t *)g_keep; }},
        {"sector_of_overlaps_keep_in", [](Call &k) { k.a.out_sector_of = (int8_t *)g_keep + 7; }},
        {"sector_of_behind_keep_in", [](Call &k) { k.a.out_sector_of = (int8_t *)g_keep + 8; }},
        {"points_are_rows", [](Call &k) { k.a.fps.out_points = g_rows; }},
        {"count_overlaps_rows", [](Call &k) { k.a.out_sector_count = (int32_t *)g_rows + 39; }},        // the rows' last element
        {"dist_overlaps_rois", [](Call &k) { k.a.fps.out_dist = g_rois + 27; }},                        // the rois' last element
        {"dist_behind_rois", [](Call &k) { k.a.fps.out_dist = g_rois + 28; }},
        {"reach2_are_rois", [](Call &k) { k.a.out_reach2 = (double *)g_rois; }},
        {"points_overlap_index", [](Call &k) { k.a.fps.out_index = (int32_t *)g_points + 23; }},         // the points' last element
        {"usable_overlaps_dist", [](Call &k) { k.a.fps.out_usable = (int32_t *)g_dist + 5; }},
        {"offsets_are_usable", [](Call &k) { k.a.out_sector_offsets = g_usable; }},
        {"count_overlaps_offsets", [](Call &k) { k.a.out_sector_count = g_offsets + 5; }},
        {"count_behind_offsets", [](Call &k) { k.a.out_sector_count = g_offsets + 6; }},
        {"sector_of_overlaps_count", [](Call &k) { k.a.out_sector_of = (int8_t *)g_count + 15; }},
        {"reach2_overlaps_sector_of", [](Call &k) { k.a.out_sector_of = (int8_t *)g_reach2 + 31; }},
        {"frames_times_rois_2p31", [](Call &k) { k.a.fps.n_frames = 1 << 23; k.a.fps.n_samples = 1; k.a.n_rois = 256; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](Call &k) { k.a.fps.frame_off = nullptr; k.a.fps.n_total = (int64_t)1 << 31; k.a.fps.keep_in = nullptr; }},
        {"rows_2p31_and_features_2", [](Call &k) { k.a.fps.n_total = (int64_t)1 << 31; k.a.fps.keep_in = nullptr; k.a.fps.n_features = 2; }},
        {"features_2_and_samples_0", [](Call &k) { k.a.fps.n_features = 2; k.a.fps.n_samples = 0; }},
        // (no samples_0 with frames_times_samples_2p31: a product above 2^31 - 1 needs n_samples >= 1)
        {"frames_times_samples_2p31_and_frame_2p30_plus_1_rows", [](Call &k) { k.a.fps.n_frames = 2; k.a.fps.n_samples = 1 << 30; k.a.fps.n_total = ((int64_t)1 << 30) + 1; k.a.fps.max_frame_rows = 0; }},
        {"frame_2p30_plus_1_rows_and_range_nan", [&](Call &k) { k.a.fps.n_total = ((int64_t)1 << 30) + 1; k.a.fps.max_frame_rows = 0; k.range6[5] = nan; }},
        {"range_nan_and_range_lo_is_hi", [&](Call &k) { k.range6[5] = nan; k.range6[3] = 0.0; }},
        {"range_lo_is_hi_and_sectors_0", [](Call &k) { k.range6[3] = 0.0; k.a.n_sectors = 0; }},
        {"sectors_0_and_rois_0", [](Call &k) { k.a.n_sectors = 0; k.a.n_rois = 0; }},
        {"rois_0_and_roi_features_6", [](Call &k) { k.a.n_rois = 0; k.a.roi_features = 6; }},
        {"roi_features_6_and_margin_nan", [&](Call &k) { k.a.roi_features = 6; k.a.roi_margin = nan; }},
        {"margin_nan_and_frames_times_rois_2p31", [&](Call &k) { k.a.roi_margin = nan; k.a.fps.n_frames = 1 << 23; k.a.fps.n_samples = 1; k.a.n_rois = 256; }},
        // (2^23 frames of 16 tiles each)
        {"frames_times_rois_2p31_and_tiles_2p27", [](Call &k) { k.a.fps.n_frames = 1 << 23; k.a.fps.n_samples = 1; k.a.n_rois = 256; k.a.fps.n_total = (int64_t)1 << 30; k.a.fps.max_frame_rows = 16384; k.a.fps.keep_in = nullptr; }},
        // (no reach2_without_rois with the four roi checks before it: those are made with d_rois, this one without)
        {"reach2_without_rois_and_tiles_2p27", [](Call &k) { k.a.rois = nullptr; k.a.fps.n_frames = 1 << 17; k.a.fps.n_samples = 1; k.a.fps.n_total = (int64_t)1 << 30; k.a.fps.max_frame_rows = 1 << 20; k.a.fps.keep_in = nullptr; }},
        {"tiles_2p27_and_index_overlaps_rows", [](Call &k) { k.a.fps.n_frames = 1 << 17; k.a.fps.n_samples = 1; k.a.fps.n_total = (int64_t)1 << 30; k.a.fps.max_frame_rows = 1 << 20; k.a.fps.keep_in = nullptr; k.a.fps.out_index = (int32_t *)g_rows; }},
    };
    for (const auto &cs : cases) {
        Call k;
        clean_call(k);
        cs.second(k);
        std::string msg;
        const int rc = sg_check_fps_sectors_args(k.a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
