// ball_refusals.cpp -- snowgpu_ball_query_device through every refusal of sg_check_ball_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_ball_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, K = 3 centres of 3 columns, pairs (0.5, 2), (1, 3), C = 4
// (padded by what the longest output placed behind them takes: no range below leaves its array)
static float g_rows[8 * 5 + 40], g_centres[2 * 3 * 3 + 40], g_points[2 * 3 * 5 * 4 + 8];
static uint8_t g_keep[8 + 200];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_index[2 * 3 * 5 + 8], g_count[2 * 3 * 2 + 8];

struct Call {
    SgBallArgs a;
    double range6[6], radii[4];
    int samples[4];
};

static void clean_call(Call &k)
{
    const double r[6] = {0.0, -2.0, -1.0, 4.0, 2.0, 1.0};
    for (int i = 0; i < 6; ++i) k.range6[i] = r[i];
    k.radii[0] = 0.5; k.radii[1] = 1.0; k.radii[2] = 2.0; k.radii[3] = 4.0;
    k.samples[0] = 2; k.samples[1] = 3; k.samples[2] = 1; k.samples[3] = 64;
    k.a = SgBallArgs{2, 8, 4, 0, g_off, g_rows, k.range6, 3, g_centres, 3, 2, k.radii, k.samples, 4, g_keep, g_index, g_count, g_points, 1024};
}

// (outputs larger than the host arrays that stand for them: none is given to overlap)
static void bare(Call &k) { k.a.out_points = nullptr; k.a.keep_in = nullptr; k.a.rows = nullptr; k.a.n_total = 0; k.a.centres = (const void *)(uintptr_t)((uint64_t)1 << 44); }

int main()
{
    using Edit = std::function<void(Call &)>;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](Call &) {}},
        {"null_frame_offsets", [](Call &k) { k.a.frame_off = nullptr; }},
        {"null_rows", [](Call &k) { k.a.rows = nullptr; }},
        {"null_centres", [](Call &k) { k.a.centres = nullptr; }},
        {"null_radii", [](Call &k) { k.a.radii = nullptr; }},
        {"null_samples", [](Call &k) { k.a.n_samples = nullptr; }},
        {"null_out_index", [](Call &k) { k.a.out_index = nullptr; }},
        {"null_out_count", [](Call &k) { k.a.out_count = nullptr; }},
        {"null_out_points", [](Call &k) { k.a.out_points = nullptr; }},
        {"null_keep_in", [](Call &k) { k.a.keep_in = nullptr; }},
        {"null_range", [](Call &k) { k.a.range6 = nullptr; }},
        {"bad_dtype", [](Call &k) { k.a.dtype = 2; }},
        {"float64", [](Call &k) { k.a.dtype = 1; k.a.rows = nullptr; k.a.n_total = 0; k.a.out_points = nullptr; k.a.centres = (const void *)(uintptr_t)((uint64_t)1 << 44); }},
        {"no_frames", [](Call &k) { k.a.n_frames = 0; }},
        {"negative_rows", [](Call &k) { k.a.n_total = -1; }},
        {"empty_null_rows", [](Call &k) { k.a.n_total = 0; k.a.rows = nullptr; k.a.keep_in = nullptr; }},
        {"rows_2p31", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"features_2", [](Call &k) { k.a.n_features = 2; }},
        {"features_3", [](Call &k) { k.a.n_features = 3; }},
        {"features_5", [](Call &k) { k.a.n_features = 5; k.a.out_points = nullptr; }},      // (g_points stands for C = 4)
        {"features_6", [](Call &k) { k.a.n_features = 6; }},
        {"centre_features_2", [](Call &k) { k.a.centre_features = 2; }},
        {"centre_features_5", [](Call &k) { k.a.centre_features = 5; k.a.centres = (const void *)(uintptr_t)((uint64_t)1 << 44); }},
        {"centre_features_6", [](Call &k) { k.a.centre_features = 6; }},
        {"centres_0", [](Call &k) { k.a.n_centres = 0; }},
        {"centres_negative", [](Call &k) { k.a.n_centres = -2; }},
        {"radii_0", [](Call &k) { k.a.n_radii = 0; }},
        {"radii_1", [](Call &k) { k.a.n_radii = 1; }},
        {"radii_4", [](Call &k) { k.a.n_radii = 4; bare(k); }},
        {"radii_5", [](Call &k) { k.a.n_radii = 5; }},
        {"radius_0", [](Call &k) { k.radii[1] = 0.0; }},
        {"radius_negative", [](Call &k) { k.radii[0] = -0.5; }},
        {"radius_nan", [&](Call &k) { k.radii[0] = nan; }},
        {"radius_inf", [&](Call &k) { k.radii[1] = inf; }},
        {"radius_1e6", [](Call &k) { k.radii[1] = 1e6; }},
        {"radius_above_1e6", [](Call &k) { k.radii[1] = 1000000.5; }},
        {"radius_tiny", [](Call &k) { k.radii[0] = 1e-30; }},
        {"samples_0", [](Call &k) { k.samples[1] = 0; }},
        {"samples_1", [](Call &k) { k.samples[0] = 1; }},
        {"samples_64", [](Call &k) { k.samples[1] = 64; bare(k); }},
        {"samples_65", [](Call &k) { k.samples[0] = 65; }},
        {"slots_2p31_minus_1", [](Call &k) { k.a.n_frames = 1; k.a.n_centres = 2147483647; k.a.n_radii = 1; k.samples[0] = 1; bare(k); k.a.max_cells = 0; }},
        {"slots_2p31", [](Call &k) { k.a.n_frames = 1; k.a.n_centres = 1 << 30; k.a.n_radii = 1; k.samples[0] = 2; bare(k); }},
        {"slots_overflowing", [](Call &k) { k.a.n_frames = 2147483647; k.a.n_centres = 2147483647; k.a.n_radii = 4; k.samples[0] = k.samples[1] = k.samples[2] = 64; bare(k); }},
        {"frame_2p30_rows", [](Call &k) { k.a.n_total = (int64_t)1 << 30; k.a.max_frame_rows = 0; k.a.keep_in = nullptr; k.a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"frame_2p30_plus_1_rows", [](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; }},
        {"cell_lists_fit", [](Call &k) { k.a.n_frames = 26214; k.a.max_cells = 81920; k.a.n_centres = 1; bare(k); }},
        {"cell_lists_too_large", [](Call &k) { k.a.n_frames = 26215; k.a.max_cells = 81920; k.a.n_centres = 1; bare(k); }},
        {"range_nan_lo", [&](Call &k) { k.range6[1] = nan; }},
        {"range_nan_hi", [&](Call &k) { k.range6[5] = nan; }},
        {"range_reversed", [](Call &k) { k.range6[4] = -3.0; }},
        {"range_lo_is_hi", [](Call &k) { k.range6[3] = 0.0; }},
        {"range_infinite", [&](Call &k) { k.range6[0] = -inf; k.range6[3] = inf; k.range6[5] = inf; }},
        {"index_is_keep_in", [](Call &k) { k.a.out_index = (int32_t *)g_keep; }},
        {"index_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_index + 119; }},      // its last byte
        {"keep_in_behind_index", [](Call &k) { k.a.keep_in = (const uint8_t *)g_index + 120; }},
        {"count_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_count + 47; }},
        {"points_overlap_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_points + 479; }},
        {"index_overlaps_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 39; }},               // the rows' last element
        {"index_behind_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 40; }},
        {"count_overlaps_rows", [](Call &k) { k.a.out_count = (int32_t *)g_rows; }},
        {"points_are_rows", [](Call &k) { k.a.out_points = g_rows; }},
        {"index_overlaps_centres", [](Call &k) { k.a.out_index = (int32_t *)g_centres + 17; }},         // the centres' last element
        {"index_behind_centres", [](Call &k) { k.a.out_index = (int32_t *)g_centres + 18; }},
        {"count_is_centres", [](Call &k) { k.a.out_count = (int32_t *)g_centres; }},
        {"points_overlap_centres", [](Call &k) { k.a.centres = g_points + 100; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](Call &k) { k.a.frame_off = nullptr; k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"rows_2p31_and_features_2", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; k.a.n_features = 2; }},
        {"features_2_and_centre_features_2", [](Call &k) { k.a.n_features = 2; k.a.centre_features = 2; }},
        {"centre_features_2_and_centres_0", [](Call &k) { k.a.centre_features = 2; k.a.n_centres = 0; }},
        {"centres_0_and_radii_0", [](Call &k) { k.a.n_centres = 0; k.a.n_radii = 0; }},
        {"radii_5_and_radius_0", [](Call &k) { k.a.n_radii = 5; k.radii[0] = 0.0; }},
        {"radius_0_and_samples_0", [](Call &k) { k.radii[1] = 0.0; k.samples[1] = 0; }},                  // (of one pair: the radius is looked at first)
        // (no samples_0 with slots_2p31: the product check divides by the sum of the samples, which the sample check has to let through)
        {"slots_2p31_and_frame_2p30_plus_1_rows", [](Call &k) { k.a.n_frames = 1; k.a.n_centres = 1 << 30; k.a.n_radii = 1; k.samples[0] = 2; bare(k); k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.a.rows = g_rows; }},
        {"frame_2p30_plus_1_rows_and_cell_lists_too_large", [](Call &k) { k.a.n_frames = 26215; k.a.max_cells = 81920; k.a.n_centres = 1; bare(k); k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.a.rows = g_rows; }},
        {"cell_lists_too_large_and_range_nan", [&](Call &k) { k.a.n_frames = 26215; k.a.max_cells = 81920; k.a.n_centres = 1; bare(k); k.range6[5] = nan; }},
        {"range_nan_and_range_reversed", [&](Call &k) { k.range6[5] = nan; k.range6[4] = -3.0; }},
        {"range_reversed_and_index_is_keep_in", [](Call &k) { k.range6[4] = -3.0; k.a.out_index = (int32_t *)g_keep; }},
        // The current contract: the outputs are not compared with each other.  Refusing this call is a change of behaviour, not a tidying.
        {"count_is_index", [](Call &k) { k.a.out_count = k.a.out_index; }},
    };
    for (const auto &cs : cases) {
        Call k;
        clean_call(k);
        cs.second(k);
        std::string msg;
        int64_t total = -1;
        const int rc = sg_check_ball_args(k.a, &total, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
