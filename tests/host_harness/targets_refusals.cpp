// targets_refusals.cpp -- snowgpu_sample_rois_device through every refusal of sg_check_targets_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_targets_reference.py compares the lines with a table.
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: F = 2 frames of M = 3 float32 rois of 8 columns, B = 2 gt boxes of 9, S = 4 slots
// (padded: no range below leaves its array)
static float g_rois[2 * 3 * 8 + 100], g_overlap[2 * 3 + 100], g_gt[2 * 2 * 9 + 100];
static int32_t g_assign[2 * 3 + 100];
static uint64_t g_step[4];
static double g_pose_in[2 * 3 * 2 + 40];
static int32_t g_index[2 * 4 + 100], g_gt_index[2 * 4 + 100], g_segments[2 * 3 + 100], g_class_count[2 * 3 + 100];
static float g_out_rois[2 * 4 * 8 + 100], g_roi_iou[2 * 4 + 100], g_gt_of[2 * 4 * 9 + 100], g_cls_label[2 * 4 + 100], g_gt_local[2 * 4 * 7 + 100];
static uint8_t g_reg_valid[2 * 4 + 100];
static double g_pose[2 * 4 * 2 + 40];
static SgSamplerCfg g_cfg;

static void clean_call(SgTargetsArgs &a)
{
    g_cfg = SgSamplerCfg{4, 2, 0.55, 0.75, 0.25, 0.1, 0.8, 0};
    a = SgTargetsArgs{2, 3, g_rois, 8, g_overlap, g_assign, 2, g_gt, 9, 0, &g_cfg, g_step, g_pose_in, g_index, g_out_rois, g_roi_iou, g_gt_index, g_gt_of, g_reg_valid,
                      g_cls_label, g_segments, g_class_count, g_pose, g_gt_local};
}

// (sizes larger than the host arrays that stand for them: every pointer far from every other)
static void bare(SgTargetsArgs &a)
{
    auto at = [](int k) { return (void *)(uintptr_t)((uint64_t)(k + 1) << 40); };
    a.rois = at(0); a.overlap = at(1); a.assignment = (const int32_t *)at(2); a.gt_boxes = at(3); a.pose_in = nullptr;
    a.out_index = (int32_t *)at(4); a.out_rois = at(5); a.out_roi_iou = at(6); a.out_gt_index = (int32_t *)at(7); a.out_gt_of_rois = at(8);
    a.out_reg_valid = (uint8_t *)at(9); a.out_cls_label = at(10); a.out_segments = (int32_t *)at(11); a.out_class_count = (int32_t *)at(12);
    a.out_pose = nullptr; a.out_gt_local = nullptr;
}

int main()
{
    using Edit = std::function<void(SgTargetsArgs &)>;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgTargetsArgs &) {}},
        {"null_rois", [](SgTargetsArgs &a) { a.rois = nullptr; }},
        {"null_overlap", [](SgTargetsArgs &a) { a.overlap = nullptr; }},
        {"null_assignment", [](SgTargetsArgs &a) { a.assignment = nullptr; }},
        {"null_gt_boxes", [](SgTargetsArgs &a) { a.gt_boxes = nullptr; }},
        {"null_cfg", [](SgTargetsArgs &a) { a.cfg = nullptr; }},
        {"null_step", [](SgTargetsArgs &a) { a.step = nullptr; }},
        {"null_out_index", [](SgTargetsArgs &a) { a.out_index = nullptr; }},
        {"null_out_rois", [](SgTargetsArgs &a) { a.out_rois = nullptr; }},
        {"null_out_roi_iou", [](SgTargetsArgs &a) { a.out_roi_iou = nullptr; }},
        {"null_out_gt_index", [](SgTargetsArgs &a) { a.out_gt_index = nullptr; }},
        {"null_out_gt_of_rois", [](SgTargetsArgs &a) { a.out_gt_of_rois = nullptr; }},
        {"null_out_reg_valid", [](SgTargetsArgs &a) { a.out_reg_valid = nullptr; }},
        {"null_out_cls_label", [](SgTargetsArgs &a) { a.out_cls_label = nullptr; }},
        {"null_out_segments", [](SgTargetsArgs &a) { a.out_segments = nullptr; }},
        {"null_out_class_count", [](SgTargetsArgs &a) { a.out_class_count = nullptr; }},
        {"null_pose_in", [](SgTargetsArgs &a) { a.pose_in = nullptr; }},
        {"null_out_pose", [](SgTargetsArgs &a) { a.out_pose = nullptr; }},
        {"null_out_gt_local", [](SgTargetsArgs &a) { a.out_gt_local = nullptr; }},
        {"bad_dtype", [](SgTargetsArgs &a) { a.dtype = 2; }},
        {"float64", [](SgTargetsArgs &a) { a.dtype = 1; bare(a); }},
        {"no_frames", [](SgTargetsArgs &a) { a.n_frames = 0; }},
        {"rois_0", [](SgTargetsArgs &a) { a.n_rois = 0; }},
        {"rois_1", [](SgTargetsArgs &a) { a.n_rois = 1; }},
        {"rois_9216", [](SgTargetsArgs &a) { a.n_rois = 9216; bare(a); }},
        {"rois_9217", [](SgTargetsArgs &a) { a.n_rois = 9217; }},
        {"gt_0", [](SgTargetsArgs &a) { a.n_gt = 0; }},
        {"gt_1", [](SgTargetsArgs &a) { a.n_gt = 1; }},
        {"gt_9216", [](SgTargetsArgs &a) { a.n_gt = 9216; bare(a); }},
        {"gt_9217", [](SgTargetsArgs &a) { a.n_gt = 9217; }},
        {"gt_negative", [](SgTargetsArgs &a) { a.n_gt = -1; }},
        {"roi_features_6", [](SgTargetsArgs &a) { a.roi_features = 6; }},
        {"roi_features_7", [](SgTargetsArgs &a) { a.roi_features = 7; }},
        {"roi_features_10", [](SgTargetsArgs &a) { a.roi_features = 10; bare(a); }},
        {"roi_features_11", [](SgTargetsArgs &a) { a.roi_features = 11; }},
        {"gt_features_6", [](SgTargetsArgs &a) { a.gt_features = 6; }},
        {"gt_features_7", [](SgTargetsArgs &a) { a.gt_features = 7; }},
        {"gt_features_10", [](SgTargetsArgs &a) { a.gt_features = 10; bare(a); }},
        {"gt_features_11", [](SgTargetsArgs &a) { a.gt_features = 11; }},
        {"slots_0", [](SgTargetsArgs &) { g_cfg.roi_per_image = 0; }},
        {"slots_1", [](SgTargetsArgs &) { g_cfg.roi_per_image = 1; g_cfg.fg_per_image = 1; }},
        {"slots_1024", [](SgTargetsArgs &a) { g_cfg.roi_per_image = 1024; bare(a); }},
        {"slots_1025", [](SgTargetsArgs &) { g_cfg.roi_per_image = 1025; }},
        {"fg_negative", [](SgTargetsArgs &) { g_cfg.fg_per_image = -1; }},
        {"fg_0", [](SgTargetsArgs &) { g_cfg.fg_per_image = 0; }},
        {"fg_all", [](SgTargetsArgs &) { g_cfg.fg_per_image = 4; }},
        {"fg_above_slots", [](SgTargetsArgs &) { g_cfg.fg_per_image = 5; }},
        {"reg_fg_nan", [nan](SgTargetsArgs &) { g_cfg.reg_fg_thresh = nan; }},
        {"cls_fg_inf", [inf](SgTargetsArgs &) { g_cfg.cls_fg_thresh = inf; }},
        {"cls_bg_minus_inf", [inf](SgTargetsArgs &) { g_cfg.cls_bg_thresh = -inf; }},
        {"cls_bg_lo_nan", [nan](SgTargetsArgs &) { g_cfg.cls_bg_thresh_lo = nan; }},
        {"thresholds_negative", [](SgTargetsArgs &) { g_cfg.reg_fg_thresh = -1.0; g_cfg.cls_bg_thresh_lo = 2.0; }},
        {"cls_fg_equals_cls_bg", [](SgTargetsArgs &) { g_cfg.cls_fg_thresh = 0.25; }},
        {"cls_fg_below_cls_bg", [](SgTargetsArgs &) { g_cfg.cls_fg_thresh = 0.2; }},
        {"ratio_negative", [](SgTargetsArgs &) { g_cfg.hard_bg_ratio = -0.01; }},
        {"ratio_0", [](SgTargetsArgs &) { g_cfg.hard_bg_ratio = 0.0; }},
        {"ratio_1", [](SgTargetsArgs &) { g_cfg.hard_bg_ratio = 1.0; }},
        {"ratio_above_1", [](SgTargetsArgs &) { g_cfg.hard_bg_ratio = 1.5; }},
        {"ratio_nan", [nan](SgTargetsArgs &) { g_cfg.hard_bg_ratio = nan; }},
        {"cls_mode_negative", [](SgTargetsArgs &) { g_cfg.cls_mode = -1; }},
        {"cls_mode_1", [](SgTargetsArgs &) { g_cfg.cls_mode = 1; }},
        {"cls_mode_2", [](SgTargetsArgs &) { g_cfg.cls_mode = 2; }},
        // F S max(Cb, Cg): 209715 x 1024 x 10 = 2147481600 fits, 209716 x 1024 x 10 = 2147491840 does not
        {"elements_below_2p31", [](SgTargetsArgs &a) { a.n_frames = 209715; g_cfg.roi_per_image = 1024; a.gt_features = 10; bare(a); }},
        {"elements_above_2p31", [](SgTargetsArgs &a) { a.n_frames = 209716; g_cfg.roi_per_image = 1024; a.roi_features = 10; bare(a); }},
        {"elements_overflowing", [](SgTargetsArgs &a) { a.n_frames = 2147483647; g_cfg.roi_per_image = 1024; bare(a); }},
        {"index_is_rois", [](SgTargetsArgs &a) { a.out_index = (int32_t *)g_rois; }},
        {"index_overlaps_rois", [](SgTargetsArgs &a) { a.out_index = (int32_t *)g_rois + 47; }},             // the rois' last element
        {"index_behind_rois", [](SgTargetsArgs &a) { a.out_index = (int32_t *)g_rois + 48; }},
        {"rois_overlaps_overlap", [](SgTargetsArgs &a) { a.out_rois = g_overlap + 5; }},
        {"roi_iou_is_assignment", [](SgTargetsArgs &a) { a.out_roi_iou = g_assign; }},
        {"gt_index_overlaps_gt_boxes", [](SgTargetsArgs &a) { a.gt_boxes = (const float *)g_gt_index + 7; }},
        {"cls_label_is_step", [](SgTargetsArgs &a) { a.out_cls_label = g_step; }},
        {"step_behind_cls_label", [](SgTargetsArgs &a) { a.step = (const uint64_t *)(g_cls_label + 8); }},
        {"pose_is_pose_in", [](SgTargetsArgs &a) { a.out_pose = g_pose_in; }},
        {"gt_local_overlaps_pose_in", [](SgTargetsArgs &a) { a.out_gt_local = g_pose_in + 11; }},
        {"rois_is_index", [](SgTargetsArgs &a) { a.out_rois = g_index; }},
        {"roi_iou_overlaps_rois", [](SgTargetsArgs &a) { a.out_roi_iou = g_out_rois + 63; }},
        {"roi_iou_behind_rois", [](SgTargetsArgs &a) { a.out_roi_iou = g_out_rois + 64; }},
        {"gt_of_rois_is_gt_index", [](SgTargetsArgs &a) { a.out_gt_of_rois = g_gt_index; }},
        {"reg_valid_overlaps_gt_of_rois", [](SgTargetsArgs &a) { a.out_reg_valid = (uint8_t *)g_gt_of + 287; }},
        {"cls_label_is_reg_valid", [](SgTargetsArgs &a) { a.out_cls_label = g_reg_valid; }},
        {"segments_overlaps_index", [](SgTargetsArgs &a) { a.out_segments = g_index + 7; }},
        {"class_count_is_segments", [](SgTargetsArgs &a) { a.out_class_count = g_segments; }},
        {"class_count_behind_segments", [](SgTargetsArgs &a) { a.out_class_count = g_segments + 6; }},
        {"pose_overlaps_class_count", [](SgTargetsArgs &a) { a.out_pose = (double *)g_class_count + 2; }},
        {"gt_local_is_pose", [](SgTargetsArgs &a) { a.out_gt_local = g_pose; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_rois_and_rois_0", [](SgTargetsArgs &a) { a.rois = nullptr; a.n_rois = 0; }},
        {"rois_0_and_roi_features_6", [](SgTargetsArgs &a) { a.n_rois = 0; a.roi_features = 6; }},
        {"roi_features_6_and_slots_0", [](SgTargetsArgs &a) { a.roi_features = 6; g_cfg.roi_per_image = 0; }},
        {"slots_0_and_fg_negative", [](SgTargetsArgs &) { g_cfg.roi_per_image = 0; g_cfg.fg_per_image = -1; }},
        {"fg_negative_and_reg_fg_nan", [nan](SgTargetsArgs &) { g_cfg.fg_per_image = -1; g_cfg.reg_fg_thresh = nan; }},
        {"reg_fg_nan_and_cls_fg_below_cls_bg", [nan](SgTargetsArgs &) { g_cfg.reg_fg_thresh = nan; g_cfg.cls_fg_thresh = 0.2; }},
        {"cls_fg_below_cls_bg_and_ratio_nan", [nan](SgTargetsArgs &) { g_cfg.cls_fg_thresh = 0.2; g_cfg.hard_bg_ratio = nan; }},
        {"ratio_nan_and_cls_mode_2", [nan](SgTargetsArgs &) { g_cfg.hard_bg_ratio = nan; g_cfg.cls_mode = 2; }},
        {"cls_mode_2_and_elements_above_2p31", [](SgTargetsArgs &a) { g_cfg.cls_mode = 2; a.n_frames = 209716; g_cfg.roi_per_image = 1024; a.roi_features = 10; bare(a); }},
        {"elements_above_2p31_and_index_is_rois", [](SgTargetsArgs &a) { a.n_frames = 209716; g_cfg.roi_per_image = 1024; a.roi_features = 10; bare(a); a.out_index = (int32_t *)a.rois; }},
    };
    for (const auto &cs : cases) {
        SgTargetsArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_targets_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
