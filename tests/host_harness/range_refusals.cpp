// range_refusals.cpp -- snowgpu_range_image_device through every refusal of sg_check_range_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_range_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, H = 2, W = 3, C = 4 (padded: no range below leaves
// its array)
static float g_rows[8 * 5 + 64], g_image[2 * 5 * 6 + 64];
static uint8_t g_keep[8 + 256];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_ring[8 + 64], g_index[2 * 6 + 64], g_pixel_of[8 + 64], g_count[2 * 6 + 64];

struct Call {
    SgRangeArgs a;
    double fov2[2], limits2[2];
};

static void clean_call(Call &k)
{
    k.fov2[0] = 0.05; k.fov2[1] = -0.43;
    k.limits2[0] = 0.0; k.limits2[1] = 120.0;
    k.a = SgRangeArgs{2, 8, 4, 0, g_off, g_rows, 2, 3, k.fov2, nullptr, k.limits2, 4, g_keep, g_image, g_index, g_pixel_of, g_count};
}

// (outputs larger than the host arrays that stand for them: addresses far apart, none is read)
static void bare(Call &k)
{
    k.a.keep_in = nullptr; k.a.rows = nullptr; k.a.n_total = 0; k.a.out_pixel_of = nullptr; k.a.out_count = nullptr;
    k.a.out_image = (void *)(uintptr_t)((uint64_t)1 << 44); k.a.out_index = (int32_t *)(uintptr_t)((uint64_t)1 << 45);
}

int main()
{
    using Edit = std::function<void(Call &)>;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan(""), half_pi = 1.5707963267948966;
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](Call &) {}},
        {"null_frame_offsets", [](Call &k) { k.a.frame_off = nullptr; }},
        {"null_rows", [](Call &k) { k.a.rows = nullptr; }},
        {"null_out_image", [](Call &k) { k.a.out_image = nullptr; }},
        {"null_out_index", [](Call &k) { k.a.out_index = nullptr; }},
        {"null_out_pixel_of", [](Call &k) { k.a.out_pixel_of = nullptr; }},
        {"null_out_count", [](Call &k) { k.a.out_count = nullptr; }},
        {"null_keep_in", [](Call &k) { k.a.keep_in = nullptr; }},
        {"null_limits", [](Call &k) { k.a.limits2 = nullptr; }},
        {"bad_dtype", [](Call &k) { k.a.dtype = 2; }},
        {"float64", [](Call &k) { k.a.dtype = 1; bare(k); }},
        {"no_frames", [](Call &k) { k.a.n_frames = 0; }},
        {"negative_rows", [](Call &k) { k.a.n_total = -1; }},
        {"empty_null_rows", [](Call &k) { k.a.n_total = 0; k.a.rows = nullptr; k.a.keep_in = nullptr; k.a.out_pixel_of = nullptr; }},
        {"no_mode", [](Call &k) { k.a.fov2 = nullptr; }},
        {"channel_mode", [](Call &k) { k.a.fov2 = nullptr; k.a.ring = g_ring; }},
        {"channel_mode_ignores_fov", [&](Call &k) { k.fov2[0] = nan; k.fov2[1] = 9.0; k.a.ring = g_ring; }},
        {"rows_2p31", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"features_2", [](Call &k) { k.a.n_features = 2; }},
        {"features_3", [](Call &k) { k.a.n_features = 3; }},
        {"features_5", [](Call &k) { k.a.n_features = 5; }},
        {"features_6", [](Call &k) { k.a.n_features = 6; }},
        {"height_0", [](Call &k) { k.a.H = 0; }},
        {"width_0", [](Call &k) { k.a.W = 0; }},
        {"height_negative", [](Call &k) { k.a.H = -4; }},
        {"one_pixel", [](Call &k) { k.a.H = 1; k.a.W = 1; }},
        {"pixels_2p31_minus_1", [](Call &k) { k.a.n_frames = 1; k.a.H = 1; k.a.W = 2147483647; bare(k); }},
        {"pixels_2p31", [](Call &k) { k.a.n_frames = 2; k.a.H = 1 << 15; k.a.W = 1 << 15; bare(k); }},
        {"pixels_overflowing", [](Call &k) { k.a.n_frames = 2147483647; k.a.H = 2147483647; k.a.W = 2147483647; bare(k); }},
        {"frame_2p30_rows", [](Call &k) { k.a.n_total = (int64_t)1 << 30; k.a.max_frame_rows = 0; k.a.keep_in = nullptr; k.a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40);
                                          k.a.out_pixel_of = (int32_t *)(uintptr_t)((uint64_t)1 << 46); }},
        {"frame_2p30_plus_1_rows", [](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; }},
        {"fov_half_pi", [&](Call &k) { k.fov2[0] = half_pi; k.fov2[1] = -half_pi; }},
        {"fov_up_above_half_pi", [](Call &k) { k.fov2[0] = 1.5707963267948968; }},
        {"fov_down_below_half_pi", [](Call &k) { k.fov2[1] = -1.5707963267948968; }},
        {"fov_nan", [&](Call &k) { k.fov2[0] = nan; }},
        {"fov_inf", [&](Call &k) { k.fov2[1] = -inf; }},
        {"fov_degrees", [](Call &k) { k.fov2[0] = 3.0; k.fov2[1] = -25.0; }},
        {"fov_reversed", [](Call &k) { k.fov2[0] = -0.43; k.fov2[1] = 0.05; }},
        {"fov_up_is_down", [](Call &k) { k.fov2[0] = k.fov2[1]; }},
        {"limit_nan_lo", [&](Call &k) { k.limits2[0] = nan; }},
        {"limit_nan_hi", [&](Call &k) { k.limits2[1] = nan; }},
        {"limit_lo_negative", [](Call &k) { k.limits2[0] = -0.5; }},
        {"limit_lo_is_hi", [](Call &k) { k.limits2[0] = 120.0; }},
        {"limit_reversed", [](Call &k) { k.limits2[0] = 121.0; }},
        {"limit_hi_inf", [&](Call &k) { k.limits2[1] = inf; }},
        {"limit_lo_inf", [&](Call &k) { k.limits2[0] = inf; k.limits2[1] = inf; }},
        {"limit_lo_zero_hi_tiny", [](Call &k) { k.limits2[1] = 1e-300; }},
        {"image_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_image + 239; }},       // the image's last byte
        {"keep_in_behind_image", [](Call &k) { k.a.keep_in = (const uint8_t *)g_image + 240; }},
        {"index_is_keep_in", [](Call &k) { k.a.out_index = (int32_t *)g_keep; }},
        {"pixel_of_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_pixel_of + 31; }},
        {"count_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_count + 47; }},
        {"image_is_rows", [](Call &k) { k.a.out_image = g_rows; }},
        {"index_overlaps_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 39; }},                // the rows' last element
        {"index_behind_rows", [](Call &k) { k.a.out_index = (int32_t *)g_rows + 40; }},
        {"pixel_of_overlaps_rows", [](Call &k) { k.a.out_pixel_of = (int32_t *)g_rows; }},
        {"count_overlaps_rows", [](Call &k) { k.a.out_count = (int32_t *)g_rows + 20; }},
        {"image_overlaps_ring", [](Call &k) { k.a.ring = (const int32_t *)g_image + 59; }},
        {"index_is_ring", [](Call &k) { k.a.ring = g_ring; k.a.out_index = g_ring; }},
        {"pixel_of_is_ring", [](Call &k) { k.a.ring = g_ring; k.a.out_pixel_of = g_ring; }},
        {"pixel_of_behind_ring", [](Call &k) { k.a.ring = g_ring; k.a.out_pixel_of = g_ring + 8; }},
        {"count_overlaps_ring", [](Call &k) { k.a.ring = g_ring; k.a.out_count = g_ring + 7; }},
        {"index_overlaps_image", [](Call &k) { k.a.out_index = (int32_t *)g_image + 59; }},
        {"index_behind_image", [](Call &k) { k.a.out_index = (int32_t *)g_image + 60; }},
        {"pixel_of_overlaps_image", [](Call &k) { k.a.out_pixel_of = (int32_t *)g_image; }},
        {"pixel_of_overlaps_index", [](Call &k) { k.a.out_pixel_of = g_index + 11; }},
        {"count_overlaps_image", [](Call &k) { k.a.out_count = (int32_t *)g_image + 30; }},
        {"count_is_index", [](Call &k) { k.a.out_count = g_index; }},
        {"count_overlaps_pixel_of", [](Call &k) { k.a.out_count = g_pixel_of + 7; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_no_mode", [](Call &k) { k.a.frame_off = nullptr; k.a.fov2 = nullptr; }},
        {"no_mode_and_rows_2p31", [](Call &k) { k.a.fov2 = nullptr; k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"rows_2p31_and_features_2", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; k.a.n_features = 2; }},
        {"features_2_and_height_0", [](Call &k) { k.a.n_features = 2; k.a.H = 0; }},
        // (no height_0 with pixels_2p31: a product above 2^31 - 1 needs a height and a width of at least 1)
        {"pixels_2p31_and_frame_2p30_plus_1_rows", [](Call &k) { k.a.n_frames = 2; k.a.H = 1 << 15; k.a.W = 1 << 15; bare(k); k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0;
                                                                 k.a.rows = g_rows; k.a.out_pixel_of = g_pixel_of; }},
        {"frame_2p30_plus_1_rows_and_fov_nan", [&](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.fov2[0] = nan; }},
        {"fov_degrees_and_fov_reversed", [](Call &k) { k.fov2[0] = -25.0; k.fov2[1] = 3.0; }},
        {"fov_reversed_and_limit_nan_lo", [&](Call &k) { k.fov2[0] = -0.43; k.fov2[1] = 0.05; k.limits2[0] = nan; }},
        {"limit_nan_hi_and_limit_lo_negative", [&](Call &k) { k.limits2[1] = nan; k.limits2[0] = -0.5; }},
        {"limit_reversed_and_index_is_keep_in", [](Call &k) { k.limits2[0] = 121.0; k.a.out_index = (int32_t *)g_keep; }},
    };
    for (const auto &cs : cases) {
        Call k;
        clean_call(k);
        cs.second(k);
        std::string msg;
        const int rc = sg_check_range_args(k.a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
