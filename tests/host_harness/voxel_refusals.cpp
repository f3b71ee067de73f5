// voxel_refusals.cpp -- snowgpu_voxelize_device through every refusal of sg_check_voxel_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message|n_x n_y n_z.  tests/test_voxel_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four rows
static double g_rows[8 * 5], g_voxels[2 * 3 * 2 * 5];
static uint8_t g_keep[8 + 32];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_coords[2 * 3 * 4], g_num[2 * 3], g_voff[3], g_vof[8 + 8];

struct Call {
    SgVoxelArgs a;
    double range6[6], size3[3];
};

// a call in order: float32 rows, the grid 4 x 4 x 2, T = 2, V = 3, C = 4, a mask and a voxel_of apart from it
static void clean_call(Call &k)
{
    const double r[6] = {0.0, -2.0, -1.0, 4.0, 2.0, 1.0}, s[3] = {1.0, 1.0, 1.0};
    for (int i = 0; i < 6; ++i) k.range6[i] = r[i];
    for (int i = 0; i < 3; ++i) k.size3[i] = s[i];
    k.a = SgVoxelArgs{2, 8, 4, 0, g_off, g_rows, k.range6, k.size3, 2, 3, 4, g_keep, g_voxels, g_coords, g_num, g_voff, g_vof};
}

int main()
{
    using Edit = std::function<void(Call &)>;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](Call &) {}},
        {"null_frame_offsets", [](Call &k) { k.a.frame_off = nullptr; }},
        {"null_rows", [](Call &k) { k.a.rows = nullptr; }},
        {"null_range", [](Call &k) { k.a.range6 = nullptr; }},
        {"null_size", [](Call &k) { k.a.size3 = nullptr; }},
        {"null_out_voxels", [](Call &k) { k.a.out_voxels = nullptr; }},
        {"null_out_coords", [](Call &k) { k.a.out_coords = nullptr; }},
        {"null_out_num_points", [](Call &k) { k.a.out_num_points = nullptr; }},
        {"null_out_voxel_offsets", [](Call &k) { k.a.out_voxel_offsets = nullptr; }},
        {"null_out_voxel_of", [](Call &k) { k.a.out_voxel_of = nullptr; }},
        {"null_keep_in", [](Call &k) { k.a.keep_in = nullptr; }},
        {"bad_dtype", [](Call &k) { k.a.dtype = 2; }},
        {"float64", [](Call &k) { k.a.dtype = 1; }},
        {"no_frames", [](Call &k) { k.a.n_frames = 0; }},
        {"negative_rows", [](Call &k) { k.a.n_total = -1; }},
        {"empty_null_buffers", [](Call &k) { k.a.n_total = 0; k.a.rows = nullptr; k.a.out_voxels = nullptr; k.a.out_coords = nullptr; k.a.out_num_points = nullptr; k.a.out_voxel_of = nullptr; }},
        {"empty_null_voxel_offsets", [](Call &k) { k.a.n_total = 0; k.a.out_voxel_offsets = nullptr; }},
        {"rows_2p31", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"features_2", [](Call &k) { k.a.n_features = 2; }},
        {"features_3", [](Call &k) { k.a.n_features = 3; }},
        {"features_5", [](Call &k) { k.a.n_features = 5; }},
        {"features_6", [](Call &k) { k.a.n_features = 6; }},
        {"points_0", [](Call &k) { k.a.max_points = 0; }},
        {"points_1", [](Call &k) { k.a.max_points = 1; }},
        {"voxels_0", [](Call &k) { k.a.max_voxels = 0; }},
        {"voxels_1", [](Call &k) { k.a.max_voxels = 1; }},
        {"voxels_negative", [](Call &k) { k.a.max_voxels = -3; }},
        {"size_zero", [](Call &k) { k.size3[1] = 0.0; }},
        {"size_negative", [](Call &k) { k.size3[0] = -1.0; }},
        {"size_inf", [&](Call &k) { k.size3[2] = inf; }},
        {"size_nan", [&](Call &k) { k.size3[2] = nan; }},
        {"axis_without_cell", [](Call &k) { k.range6[3] = 0.25; }},              // (0.25 - 0) / 1 rounds to 0
        {"axis_half_cell", [](Call &k) { k.range6[3] = 0.5; }},                  // llround(0.5) = 1
        {"range_reversed", [](Call &k) { k.range6[4] = -3.0; }},
        {"range_inf", [&](Call &k) { k.range6[5] = inf; }},
        {"range_nan", [&](Call &k) { k.range6[0] = nan; }},
        {"cells_2p31_minus_2", [](Call &k) { k.range6[3] = 2147483646.0; k.range6[1] = 0.0; k.range6[4] = 1.0; k.range6[2] = 0.0; }},      // 2147483646 x 1 x 1
        {"cells_2p31_minus_1", [](Call &k) { k.range6[3] = 2147483647.0; k.range6[1] = 0.0; k.range6[4] = 1.0; k.range6[2] = 0.0; }},
        {"cells_2p31_minus_2_as_product", [](Call &k) { k.range6[3] = 46341.0; k.range6[1] = 0.0; k.range6[4] = 46339.0; k.range6[2] = 0.0; }},      // 46341 x 46339 x 1 = 2 147 395 599
        {"cells_product_too_large", [](Call &k) { k.range6[3] = 46341.0; k.range6[1] = 0.0; k.range6[4] = 46341.0; k.range6[2] = 0.0; }},      // 2 147 488 281
        {"cells_1e30", [](Call &k) { k.range6[3] = 1e30; }},
        {"frames_times_voxels_2p31_minus_1", [](Call &k) { k.a.n_frames = 1; k.a.max_voxels = 2147483647; }},
        {"frames_times_voxels_2p31", [](Call &k) { k.a.n_frames = 2; k.a.max_voxels = 1 << 30; }},
        {"frame_2p30_rows", [](Call &k) { k.a.n_total = (int64_t)1 << 30; k.a.max_frame_rows = 0; k.a.keep_in = nullptr; }},
        {"frame_2p30_plus_1_rows", [](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.a.keep_in = nullptr; }},
        {"voxel_of_is_keep_in", [](Call &k) { k.a.out_voxel_of = (int32_t *)g_keep; }},
        {"voxel_of_overlaps_keep_in", [](Call &k) { k.a.keep_in = (const uint8_t *)g_vof + 31; }},      // its last byte
        {"voxel_of_behind_keep_in", [](Call &k) { k.a.out_voxel_of = (int32_t *)(g_keep + 8); }},
        {"keep_in_behind_voxel_of", [](Call &k) { k.a.keep_in = (const uint8_t *)g_vof + 32; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](Call &k) { k.a.frame_off = nullptr; k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; }},
        {"rows_2p31_and_features_2", [](Call &k) { k.a.n_total = (int64_t)1 << 31; k.a.keep_in = nullptr; k.a.n_features = 2; }},
        {"features_2_and_points_0", [](Call &k) { k.a.n_features = 2; k.a.max_points = 0; }},
        {"points_0_and_size_zero", [](Call &k) { k.a.max_points = 0; k.size3[1] = 0.0; }},
        {"size_zero_and_axis_without_cell", [](Call &k) { k.size3[1] = 0.0; k.range6[3] = 0.25; }},
        {"range_reversed_and_cells_1e30", [](Call &k) { k.range6[4] = -3.0; k.range6[3] = 1e30; }},      // (the cells' axis comes first)
        {"cells_1e30_and_frames_times_voxels_2p31", [](Call &k) { k.range6[3] = 1e30; k.a.n_frames = 2; k.a.max_voxels = 1 << 30; }},
        {"frames_times_voxels_2p31_and_frame_2p30_plus_1_rows", [](Call &k) { k.a.n_frames = 2; k.a.max_voxels = 1 << 30; k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.a.keep_in = nullptr; }},
        {"frame_2p30_plus_1_rows_and_voxel_of_is_keep_in", [](Call &k) { k.a.n_total = ((int64_t)1 << 30) + 1; k.a.max_frame_rows = 0; k.a.out_voxel_of = (int32_t *)g_keep; }},
        // The current contract: d_out_voxel_of against d_keep_in is the only overlap looked for.  Refusing this call is a change of
        // behaviour, not a tidying.
        {"coords_are_num_points", [](Call &k) { k.a.out_coords = k.a.out_num_points; }},
    };
    for (const auto &cs : cases) {
        Call k;
        clean_call(k);
        cs.second(k);
        int32_t n[3] = {0, 0, 0};
        std::string msg;
        const int rc = sg_check_voxel_args(k.a, n, &msg);
        std::printf("%s|%d|%s|%d %d %d\n", cs.first, rc, rc ? msg.c_str() : "OK", rc ? 0 : n[0], rc ? 0 : n[1], rc ? 0 : n[2]);
    }
    return 0;
}
