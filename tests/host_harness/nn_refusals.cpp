// nn_refusals.cpp -- snowgpu_nearest_centres_device through every refusal of sg_check_nn_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_nn_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, K = 3 centres of 3 columns, k = 3
// (padded by what the longest output placed behind them takes: no range below leaves its array)
static float g_rows[8 * 5 + 40], g_centres[2 * 3 * 3 + 40], g_dist2[8 * 3 + 8], g_weight[8 * 3 + 8];
static uint8_t g_keep[8 + 200];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_index[8 * 3 + 8];

struct Call {
    SgNnArgs a;
    double range6[6];
};

static void clean_call(Call &k)
{
    const double r[6] = {0.0, -2.0, -1.0, 4.0, 2.0, 1.0};
    for (int i = 0; i < 6; ++i) k.range6[i] = r[i];
    k.a = SgNnArgs{2, 8, 4, 0, g_off, g_rows, k.range6, 3, g_centres, 3, 3, g_keep, g_index, g_dist2, g_weight, 2048};
}

// (sizes larger than the host arrays that stand for them: nothing is given to overlap)
static void bare(Call &k)
{
    k.a.out_weight = nullptr; k.a.out_index = nullptr; k.a.out_dist2 = nullptr; k.a.keep_in = nullptr; k.a.rows = nullptr; k.a.n_total = 0;
    k.a.centres = (const void *)(uintptr_t)((uint64_t)1 << 44);
}

int main()
{
    using Edit = std::function<void(Call &)>;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](Call &) {}},
        {"null_frame_offsets", [](Call &k) { k.a.frame_off = nullptr; }},
        {"null_rows", [](Call &k) { k.a.rows = nullptr; }},
        {"null_centres", [](Call &k) { k.a.centres = nullptr; }},
        {"null_out_index", [](Call &k) { k.a.out_index = nullptr; }},
        {"null_out_dist2", [](Call &k) { k.a.out_dist2 = nullptr; }},
        {"null_out_weight", [](Call &k) { k.a.out_weight = nullptr; }},
        {"null_keep_in", [](Call &k) { k.a.keep_in = nullptr; }},
        {"null_range", [](Call &k) { k.a.range6 = nullptr; }},
        {"bad_dtype", [](Call &k) { k.a.dtype = 2; }},
        {"float64", [](Call &k) { k.a.dtype = 1; bare(k); }},
        {"no_frames", [](Call &k) { k.a.n_frames = 0; }},
        {"negative_rows", [](Call &k) { k.a.n_total = -1; }},
        {"empty_null_rows_and_outputs", [](Call &k) { bare(k); }},
        {"rows_2p31", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"centre_features_2", [](Call &k) { k.a.centre_features = 2; }},
        {"centre_features_5", [](Call &k) { k.a.centre_features = 5; k.a.centres = (const void *)(uintptr_t)((uint64_t)1 << 44); }},
        {"centre_features_6", [](Call &k) { k.a.centre_features = 6; }},
        {"centres_0", [](Call &k) { k.a.n_centres = 0; }},
        {"centres_negative", [](Call &k) { k.a.n_centres = -2; }},
        {"k_0", [](Call &k) { k.a.k = 0; }},
        {"k_1", [](Call &k) { k.a.k = 1; }},
        {"k_8", [](Call &k) { k.a.k = 8; bare(k); }},
        {"k_9", [](Call &k) { k.a.k = 9; }},
        {"k_negative", [](Call &k) { k.a.k = -3; }},
        {"centres_2p31_minus_1", [](Call &k) { k.a.n_frames = 1; k.a.n_centres = 2147483647; bare(k); }},
        {"centres_2p31", [](Call &k) { k.a.n_frames = 2; k.a.n_centres = 1 << 30; bare(k); }},
        {"centres_overflowing", [](Call &k) { k.a.n_frames = 2147483647; k.a.n_centres = 2147483647; bare(k); }},
        {"frame_2p30_rows", [](Call &k) { k.a.n_total = (int64_t)1 << 30; k.a.max_frame_rows = 0; k.a.keep_in = nullptr; k.a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40);
                                          k.a.out_index = (int32_t *)(uintptr_t)((uint64_t)1 << 45); k.a.out_dist2 = (void *)(uintptr_t)((uint64_t)1 << 46); k.a.out_weight = nullptr; }},
        {"frame_2p30_plus_1_rows", [](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; }},
        {"cell_lists_fit", [](Call &k) { k.a.n_frames = 1048064; k.a.n_centres = 1; bare(k); }},
        {"cell_lists_too_large", [](Call &k) { k.a.n_frames = 1048065; k.a.n_centres = 1; bare(k); }},
        {"range_nan_lo", [&](Call &k) { k.range6[1] = nan; }},
        {"range_nan_hi", [&](Call &k) { k.range6[5] = nan; }},
        {"range_reversed", [](Call &k) { k.range6[4] = -3.0; }},
        {"range_lo_is_hi", [](Call &k) { k.range6[3] = 0.0; }},
        {"range_infinite", [&](Call &k) { k.range6[0] = -inf; k.range6[3] = inf; k.range6[5] = inf; }},
        {"index_is_keep_in", [](Call &k) { k.a.out_index = (int32_t *)g_keep; }},
        {"index_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_index + 95; }},      // its last byte
        {"keep_in_behind_index", [](Call &k) { k.a.keep_in = (const uint8_t *)g_index + 96; }},
        {"dist2_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_dist2 + 95; }},
        {"weight_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_weight; }},
        {"index_overlaps_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 39; }},               // the rows' last element
        {"index_behind_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 40; }},
        {"dist2_is_rows", [](Call &k) { k.a.out_dist2 = g_rows; }},
        {"weight_overlaps_rows", [](Call &k) { k.a.out_weight = g_rows + 20; }},
        {"index_overlaps_centres", [](Call &k) { k.a.out_index = (int32_t *)g_centres + 17; }},         // the centres' last element
        {"index_behind_centres", [](Call &k) { k.a.out_index = (int32_t *)g_centres + 18; }},
        {"dist2_is_centres", [](Call &k) { k.a.out_dist2 = g_centres; }},
        {"weight_overlaps_centres", [](Call &k) { k.a.centres = g_weight + 10; }},
        {"dist2_is_index", [](Call &k) { k.a.out_dist2 = g_index; }},
        {"weight_overlaps_index", [](Call &k) { k.a.out_weight = (float *)g_index + 8; }},          // inside the index array's padding
        {"weight_is_dist2", [](Call &k) { k.a.out_weight = g_dist2; }},
        {"weight_behind_dist2", [](Call &k) { k.a.out_weight = g_dist2 + 24; k.a.out_dist2 = g_dist2; k.a.k = 1; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](Call &k) { k.a.frame_off = nullptr; k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"rows_2p31_and_centre_features_2", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; k.a.centre_features = 2; }},
        {"centre_features_2_and_centres_0", [](Call &k) { k.a.centre_features = 2; k.a.n_centres = 0; }},
        {"centres_0_and_k_0", [](Call &k) { k.a.n_centres = 0; k.a.k = 0; }},
        {"k_0_and_centres_2p31", [](Call &k) { k.a.k = 0; k.a.n_frames = 2; k.a.n_centres = 1 << 30; bare(k); }},
        {"centres_2p31_and_frame_2p30_plus_1_rows", [](Call &k) { k.a.n_frames = 2; k.a.n_centres = 1 << 30; k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; }},
        {"frame_2p30_plus_1_rows_and_cell_lists_too_large", [](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.a.n_frames = 1048065; k.a.n_centres = 1; }},
        {"cell_lists_too_large_and_range_nan", [&](Call &k) { k.a.n_frames = 1048065; k.a.n_centres = 1; bare(k); k.range6[5] = nan; }},
        {"range_nan_and_range_reversed", [&](Call &k) { k.range6[5] = nan; k.range6[4] = -3.0; }},
        {"range_reversed_and_index_is_keep_in", [](Call &k) { k.range6[4] = -3.0; k.a.out_index = (int32_t *)g_keep; }},
    };
    for (const auto &cs : cases) {
        Call k;
        clean_call(k);
        cs.second(k);
        std::string msg;
        const int rc = sg_check_nn_args(k.a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
