// centers_refusals.cpp -- snowgpu_assign_centers_device through every refusal of sg_check_centers_args (csrc/sg_device_args.h), one defect at
// a time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_centers_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: F = 2 frames, B = 3 float32 gt boxes of 8 columns, NC = 3, NH = 2, M = 4, a map of 8 x 6
// (padded: no range below leaves its array)
static float g_gt[2 * 3 * 8 + 400], g_heat[2 * 3 * 6 * 8 + 100], g_offset[2 * 2 * 4 * 2 + 100];
static int32_t g_gt_index[2 * 2 * 4 + 100], g_ind[2 * 2 * 4 + 100], g_radius[2 * 2 * 4 + 100], g_count[2 * 2 + 100];
static uint8_t g_mask[2 * 2 * 4 + 400], g_state[2 * 3 + 100];
static SgCentersCfg g_cfg;

static void clean_call(SgCentersArgs &a)
{
    g_cfg = SgCentersCfg{0.0, -40.0, 0.05, 0.05, 0.1, 8, 8, 6, 3, 2, 4, 2, 0, {0, 1, 0}};
    a = SgCentersArgs{2, 3, g_gt, 8, 0, &g_cfg, g_heat, g_gt_index, g_ind, g_mask, g_offset, g_radius, g_count, g_state};
}

// (sizes larger than the host arrays that stand for them: every pointer far from every other)
static void bare(SgCentersArgs &a)
{
    auto at = [](int k) { return (void *)(uintptr_t)((uint64_t)(k + 1) << 40); };
    a.gt_boxes = at(0); a.out_heatmap = (float *)at(1); a.out_gt_index = (int32_t *)at(2); a.out_ind = (int32_t *)at(3); a.out_mask = (uint8_t *)at(4);
    a.out_offset = at(5); a.out_radius = (int32_t *)at(6); a.out_count = (int32_t *)at(7); a.out_state = (uint8_t *)at(8);
}

int main()
{
    using Edit = std::function<void(SgCentersArgs &)>;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgCentersArgs &) {}},
        {"null_gt_boxes", [](SgCentersArgs &a) { a.gt_boxes = nullptr; }},
        {"null_cfg", [](SgCentersArgs &a) { a.cfg = nullptr; }},
        {"null_out_heatmap", [](SgCentersArgs &a) { a.out_heatmap = nullptr; }},
        {"null_out_gt_index", [](SgCentersArgs &a) { a.out_gt_index = nullptr; }},
        {"null_out_ind", [](SgCentersArgs &a) { a.out_ind = nullptr; }},
        {"null_out_mask", [](SgCentersArgs &a) { a.out_mask = nullptr; }},
        {"null_out_offset", [](SgCentersArgs &a) { a.out_offset = nullptr; }},
        {"null_out_radius", [](SgCentersArgs &a) { a.out_radius = nullptr; }},
        {"null_out_count", [](SgCentersArgs &a) { a.out_count = nullptr; }},
        {"null_out_state", [](SgCentersArgs &a) { a.out_state = nullptr; }},
        {"bad_dtype", [](SgCentersArgs &a) { a.dtype = 2; }},
        {"float64", [](SgCentersArgs &a) { a.dtype = 1; bare(a); }},
        {"no_frames", [](SgCentersArgs &a) { a.n_frames = 0; }},
        {"gt_0", [](SgCentersArgs &a) { a.n_gt = 0; }},
        {"gt_1", [](SgCentersArgs &a) { a.n_gt = 1; }},
        {"gt_256", [](SgCentersArgs &a) { a.n_gt = 256; bare(a); }},
        {"gt_257", [](SgCentersArgs &a) { a.n_gt = 257; }},
        {"gt_features_7", [](SgCentersArgs &a) { a.gt_features = 7; }},
        {"gt_features_10", [](SgCentersArgs &a) { a.gt_features = 10; bare(a); }},
        {"gt_features_11", [](SgCentersArgs &a) { a.gt_features = 11; }},
        {"classes_0", [](SgCentersArgs &) { g_cfg.n_classes = 0; }},
        {"classes_1", [](SgCentersArgs &) { g_cfg.n_classes = 1; }},
        {"classes_16", [](SgCentersArgs &a) { g_cfg.n_classes = 16; bare(a); }},
        {"classes_17", [](SgCentersArgs &) { g_cfg.n_classes = 17; }},
        {"heads_0", [](SgCentersArgs &) { g_cfg.n_heads = 0; }},
        {"heads_16", [](SgCentersArgs &a) { g_cfg.n_heads = 16; g_cfg.class_head[2] = 15; bare(a); }},
        {"heads_17", [](SgCentersArgs &) { g_cfg.n_heads = 17; }},
        {"head_negative", [](SgCentersArgs &) { g_cfg.class_head[0] = -1; }},
        {"head_at_n_heads", [](SgCentersArgs &) { g_cfg.class_head[2] = 2; }},
        {"a_head_beyond_nc_is_not_read", [](SgCentersArgs &) { g_cfg.class_head[3] = -7; }},
        {"objs_0", [](SgCentersArgs &) { g_cfg.max_objs = 0; }},
        {"objs_1", [](SgCentersArgs &) { g_cfg.max_objs = 1; }},
        {"objs_512", [](SgCentersArgs &a) { g_cfg.max_objs = 512; bare(a); }},
        {"objs_513", [](SgCentersArgs &) { g_cfg.max_objs = 513; }},
        {"width_0", [](SgCentersArgs &) { g_cfg.width = 0; }},
        {"height_negative", [](SgCentersArgs &) { g_cfg.height = -6; }},
        {"map_1x1", [](SgCentersArgs &) { g_cfg.width = 1; g_cfg.height = 1; }},
        // F NC H W: 2147483647 fits, 2^31 does not
        {"elements_at_2p31_minus_1", [](SgCentersArgs &a) { a.n_frames = 1; g_cfg.n_classes = 1; g_cfg.width = 2147483647; g_cfg.height = 1; bare(a); }},
        {"elements_at_2p31", [](SgCentersArgs &a) { a.n_frames = 2; g_cfg.n_classes = 1; g_cfg.width = 32768; g_cfg.height = 32768; bare(a); }},
        {"map_overflowing", [](SgCentersArgs &a) { a.n_frames = 1; g_cfg.width = 2147483647; g_cfg.height = 2147483647; bare(a); }},
        {"vx_0", [](SgCentersArgs &) { g_cfg.vx = 0.0; }},
        {"vy_negative", [](SgCentersArgs &) { g_cfg.vy = -0.05; }},
        {"vx_nan", [nan](SgCentersArgs &) { g_cfg.vx = nan; }},
        {"vy_inf", [inf](SgCentersArgs &) { g_cfg.vy = inf; }},
        {"x0_nan", [nan](SgCentersArgs &) { g_cfg.x0 = nan; }},
        {"y0_inf", [inf](SgCentersArgs &) { g_cfg.y0 = -inf; }},
        {"stride_0", [](SgCentersArgs &) { g_cfg.stride = 0; }},
        {"stride_1", [](SgCentersArgs &) { g_cfg.stride = 1; }},
        {"overlap_0", [](SgCentersArgs &) { g_cfg.gaussian_overlap = 0.0; }},
        {"overlap_1", [](SgCentersArgs &) { g_cfg.gaussian_overlap = 1.0; }},
        {"overlap_nan", [nan](SgCentersArgs &) { g_cfg.gaussian_overlap = nan; }},
        {"overlap_just_below_1", [](SgCentersArgs &) { g_cfg.gaussian_overlap = std::nextafter(1.0, 0.0); }},
        {"min_radius_negative", [](SgCentersArgs &) { g_cfg.min_radius = -1; }},
        {"min_radius_0", [](SgCentersArgs &) { g_cfg.min_radius = 0; }},
        {"min_radius_512", [](SgCentersArgs &) { g_cfg.min_radius = 512; }},
        {"min_radius_513", [](SgCentersArgs &) { g_cfg.min_radius = 513; }},
        {"outside_drop", [](SgCentersArgs &) { g_cfg.outside = 1; }},
        {"outside_2", [](SgCentersArgs &) { g_cfg.outside = 2; }},
        {"outside_negative", [](SgCentersArgs &) { g_cfg.outside = -1; }},
        {"heatmap_is_gt_boxes", [](SgCentersArgs &a) { a.out_heatmap = g_gt; }},
        {"heatmap_overlaps_gt_boxes", [](SgCentersArgs &a) { a.out_heatmap = g_gt + 47; }},         // the gt boxes' last element
        {"heatmap_behind_gt_boxes", [](SgCentersArgs &a) { a.out_heatmap = g_gt + 48; }},
        {"gt_index_overlaps_gt_boxes", [](SgCentersArgs &a) { a.out_gt_index = (int32_t *)g_gt + 10; }},
        {"ind_is_gt_boxes", [](SgCentersArgs &a) { a.out_ind = (int32_t *)g_gt; }},
        {"mask_overlaps_gt_boxes", [](SgCentersArgs &a) { a.out_mask = (uint8_t *)g_gt + 191; }},   // the gt boxes' last byte
        {"mask_behind_gt_boxes", [](SgCentersArgs &a) { a.out_mask = (uint8_t *)g_gt + 192; }},
        {"offset_is_gt_boxes", [](SgCentersArgs &a) { a.out_offset = g_gt; }},
        {"radius_overlaps_gt_boxes", [](SgCentersArgs &a) { a.out_radius = (int32_t *)g_gt + 47; }},
        {"count_is_gt_boxes", [](SgCentersArgs &a) { a.out_count = (int32_t *)g_gt; }},
        {"state_overlaps_gt_boxes", [](SgCentersArgs &a) { a.out_state = (uint8_t *)g_gt + 100; }},
        {"gt_index_is_heatmap", [](SgCentersArgs &a) { a.out_gt_index = (int32_t *)g_heat; }},
        {"ind_overlaps_gt_index", [](SgCentersArgs &a) { a.out_ind = g_gt_index + 15; }},
        {"ind_behind_gt_index", [](SgCentersArgs &a) { a.out_ind = g_gt_index + 16; }},
        {"mask_is_ind", [](SgCentersArgs &a) { a.out_mask = (uint8_t *)g_ind; }},
        {"offset_overlaps_mask", [](SgCentersArgs &a) { a.out_offset = g_mask + 15; }},
        {"offset_behind_mask", [](SgCentersArgs &a) { a.out_offset = g_mask + 16; }},
        {"radius_is_offset", [](SgCentersArgs &a) { a.out_radius = (int32_t *)g_offset; }},
        {"count_overlaps_radius", [](SgCentersArgs &a) { a.out_count = g_radius + 15; }},
        {"state_is_count", [](SgCentersArgs &a) { a.out_state = (uint8_t *)g_count; }},
        {"state_overlaps_heatmap", [](SgCentersArgs &a) { a.out_state = (uint8_t *)(g_heat + 287) + 3; }},   // the heatmap's last byte
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_gt_boxes_and_gt_0", [](SgCentersArgs &a) { a.gt_boxes = nullptr; a.n_gt = 0; }},
        {"gt_0_and_gt_features_7", [](SgCentersArgs &a) { a.n_gt = 0; a.gt_features = 7; }},
        {"gt_features_7_and_classes_0", [](SgCentersArgs &a) { a.gt_features = 7; g_cfg.n_classes = 0; }},
        {"classes_17_and_heads_0", [](SgCentersArgs &) { g_cfg.n_classes = 17; g_cfg.n_heads = 0; }},
        {"heads_17_and_head_negative", [](SgCentersArgs &) { g_cfg.n_heads = 17; g_cfg.class_head[0] = -1; }},
        {"head_negative_and_objs_0", [](SgCentersArgs &) { g_cfg.class_head[0] = -1; g_cfg.max_objs = 0; }},
        {"objs_513_and_height_negative", [](SgCentersArgs &) { g_cfg.max_objs = 513; g_cfg.height = -6; }},
        {"height_negative_and_map_overflowing", [](SgCentersArgs &a) { g_cfg.width = -2147483647; g_cfg.height = -6; bare(a); }},
        {"elements_at_2p31_and_vx_0", [](SgCentersArgs &a) { a.n_frames = 2; g_cfg.n_classes = 1; g_cfg.width = 32768; g_cfg.height = 32768; bare(a); g_cfg.vx = 0.0; }},
        {"vx_0_and_stride_0", [](SgCentersArgs &) { g_cfg.vx = 0.0; g_cfg.stride = 0; }},
        {"stride_0_and_overlap_0", [](SgCentersArgs &) { g_cfg.stride = 0; g_cfg.gaussian_overlap = 0.0; }},
        {"overlap_0_and_min_radius_513", [](SgCentersArgs &) { g_cfg.gaussian_overlap = 0.0; g_cfg.min_radius = 513; }},
        {"min_radius_513_and_outside_2", [](SgCentersArgs &) { g_cfg.min_radius = 513; g_cfg.outside = 2; }},
        {"outside_2_and_heatmap_is_gt_boxes", [](SgCentersArgs &a) { g_cfg.outside = 2; a.out_heatmap = g_gt; }},
    };
    for (const auto &cs : cases) {
        SgCentersArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_centers_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
