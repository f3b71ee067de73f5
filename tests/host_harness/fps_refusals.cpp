// fps_refusals.cpp -- snowgpu_fps_device through every refusal of sg_check_fps_args (csrc/sg_device_args.h), one defect at a time, and
// through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_fps_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, K = 3, C = 4
static float g_rows[8 * 5 + 8], g_points[2 * 3 * 4 + 8], g_dist[2 * 3 + 8];
static uint8_t g_keep[8 + 32];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_index[2 * 3 + 8], g_usable[2];

struct Call {
    SgFpsArgs a;
    double range6[6];
};

static void clean_call(Call &k)
{
    const double r[6] = {0.0, -2.0, -1.0, 4.0, 2.0, 1.0};
    for (int i = 0; i < 6; ++i) k.range6[i] = r[i];
    k.a = SgFpsArgs{2, 8, 4, 0, g_off, g_rows, k.range6, 3, 4, g_keep, g_index, g_points, g_dist, g_usable};
}

int main()
{
    using Edit = std::function<void(Call &)>;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](Call &) {}},
        {"null_frame_offsets", [](Call &k) { k.a.frame_off = nullptr; }},
        {"null_rows", [](Call &k) { k.a.rows = nullptr; }},
        {"null_out_index", [](Call &k) { k.a.out_index = nullptr; }},
        {"null_out_usable", [](Call &k) { k.a.out_usable = nullptr; }},
        {"null_out_points", [](Call &k) { k.a.out_points = nullptr; }},
        {"null_out_dist", [](Call &k) { k.a.out_dist = nullptr; }},
        {"null_keep_in", [](Call &k) { k.a.keep_in = nullptr; }},
        {"null_range", [](Call &k) { k.a.range6 = nullptr; }},
        {"bad_dtype", [](Call &k) { k.a.dtype = 2; }},
        {"float64", [](Call &k) { k.a.dtype = 1; k.a.rows = nullptr; k.a.n_total = 0; }},
        {"no_frames", [](Call &k) { k.a.n_frames = 0; }},
        {"negative_rows", [](Call &k) { k.a.n_total = -1; }},
        {"empty_null_rows", [](Call &k) { k.a.n_total = 0; k.a.rows = nullptr; k.a.keep_in = nullptr; k.a.out_points = nullptr; k.a.out_dist = nullptr; }},
        {"empty_null_out_index", [](Call &k) { k.a.n_total = 0; k.a.out_index = nullptr; }},
        {"rows_2p31", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"features_2", [](Call &k) { k.a.n_features = 2; }},
        {"features_3", [](Call &k) { k.a.n_features = 3; }},
        {"features_5", [](Call &k) { k.a.n_features = 5; }},
        {"features_6", [](Call &k) { k.a.n_features = 6; }},
        {"samples_0", [](Call &k) { k.a.n_samples = 0; }},
        {"samples_1", [](Call &k) { k.a.n_samples = 1; }},
        {"samples_negative", [](Call &k) { k.a.n_samples = -3; }},
        // (the outputs of these four would be larger than the host arrays that stand for them: none is given, or nothing to overlap)
        {"frames_times_samples_2p31_minus_1", [](Call &k) { k.a.n_frames = 1; k.a.n_samples = 2147483647; k.a.out_points = nullptr; k.a.out_dist = nullptr; k.a.keep_in = nullptr; k.a.rows = nullptr; k.a.n_total = 0; }},
        {"frames_times_samples_2p31", [](Call &k) { k.a.n_frames = 2; k.a.n_samples = 1 << 30; }},
        {"frame_2p30_rows", [](Call &k) { k.a.n_total = (int64_t)1 << 30; k.a.max_frame_rows = 0; k.a.keep_in = nullptr; k.a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40); }},
        {"frame_2p30_plus_1_rows", [](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; }},
        {"range_nan_lo", [&](Call &k) { k.range6[1] = nan; }},
        {"range_nan_hi", [&](Call &k) { k.range6[5] = nan; }},
        {"range_reversed", [](Call &k) { k.range6[4] = -3.0; }},
        {"range_lo_is_hi", [](Call &k) { k.range6[3] = 0.0; }},
        {"range_infinite", [&](Call &k) { k.range6[0] = -inf; k.range6[3] = inf; k.range6[5] = inf; }},
        {"range_inf_lo_is_hi", [&](Call &k) { k.range6[0] = inf; k.range6[3] = inf; }},
        {"index_is_keep_in", [](Call &k) { k.a.out_index = (int32_t *)g_keep; }},
        {"index_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_index + 23; }},      // its last byte
        {"keep_in_behind_index", [](Call &k) { k.a.keep_in = (const uint8_t *)g_index + 24; }},
        {"index_behind_keep_in", [](Call &k) { k.a.out_index = (int32_t *)(g_keep + 8); }},
        {"points_overlap_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_points + 95; }},
        {"dist_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_dist + 23; }},
        {"index_overlaps_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 39; }},               // the rows' last element
        {"index_behind_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 40; }},
        {"points_are_rows", [](Call &k) { k.a.out_points = g_rows; }},
        {"dist_overlaps_rows", [](Call &k) { k.a.rows = g_dist + 5; k.a.n_total = 1; }},              // one row: bytes 20 .. 39 of g_dist
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](Call &k) { k.a.frame_off = nullptr; k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"rows_2p31_and_features_2", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; k.a.n_features = 2; }},
        {"features_2_and_samples_0", [](Call &k) { k.a.n_features = 2; k.a.n_samples = 0; }},
        // (no samples_0 with frames_times_samples_2p31: a product above 2^31 - 1 needs n_samples >= 1)
        {"frames_times_samples_2p31_and_frame_2p30_plus_1_rows", [](Call &k) { k.a.n_frames = 2; k.a.n_samples = 1 << 30; k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; }},
        {"frame_2p30_plus_1_rows_and_range_nan", [&](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.range6[5] = nan; }},
        {"range_nan_and_range_reversed", [&](Call &k) { k.range6[5] = nan; k.range6[4] = -3.0; }},
        {"range_reversed_and_index_is_keep_in", [](Call &k) { k.range6[4] = -3.0; k.a.out_index = (int32_t *)g_keep; }},
        // The current contract: the outputs are not compared with each other.  Refusing this call is a change of behaviour, not a tidying.
        {"dist_is_points", [](Call &k) { k.a.out_dist = k.a.out_points; }},
    };
    for (const auto &cs : cases) {
        Call k;
        clean_call(k);
        cs.second(k);
        std::string msg;
        const int rc = sg_check_fps_args(k.a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
