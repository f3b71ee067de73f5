// anchors_refusals.cpp -- snowgpu_assign_anchors_device through every refusal of sg_check_anchors_args (csrc/sg_device_args.h), one defect at
// a time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_anchors_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: F = 2 frames, A = 5 float32 anchors of 7 columns, B = 3 gt boxes of 8, NC = 3
// (padded: no range below leaves its array)
static float g_anchors[5 * 7 + 100], g_gt[2 * 3 * 8 + 100], g_iou[2 * 5 + 100];
static int32_t g_class[5 + 100], g_label[2 * 5 + 100], g_gt_index[2 * 5 + 100], g_count[2 * 3 + 100], g_gt_count[2 * 3 + 100];
static double g_matched[16], g_unmatched[16];

static void clean_call(SgAnchorsArgs &a)
{
    for (int c = 0; c < 16; ++c) { g_matched[c] = 0.6; g_unmatched[c] = 0.45; }
    a = SgAnchorsArgs{2, 5, g_anchors, 7, g_class, 3, g_gt, 8, 0, 3, g_matched, g_unmatched, g_label, g_gt_index, g_count, g_gt_count, g_iou};
}

// (sizes larger than the host arrays that stand for them: every pointer far from every other)
static void bare(SgAnchorsArgs &a)
{
    auto at = [](int k) { return (void *)(uintptr_t)((uint64_t)(k + 1) << 40); };
    a.anchors = at(0); a.anchor_class = (const int32_t *)at(1); a.gt_boxes = at(2); a.out_label = (int32_t *)at(3); a.out_gt_index = (int32_t *)at(4);
    a.out_count = (int32_t *)at(5); a.out_gt_count = (int32_t *)at(6); a.out_iou = at(7);
}

int main()
{
    using Edit = std::function<void(SgAnchorsArgs &)>;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgAnchorsArgs &) {}},
        {"null_anchors", [](SgAnchorsArgs &a) { a.anchors = nullptr; }},
        {"null_anchor_class", [](SgAnchorsArgs &a) { a.anchor_class = nullptr; }},
        {"null_gt_boxes", [](SgAnchorsArgs &a) { a.gt_boxes = nullptr; }},
        {"null_matched", [](SgAnchorsArgs &a) { a.matched = nullptr; }},
        {"null_unmatched", [](SgAnchorsArgs &a) { a.unmatched = nullptr; }},
        {"null_out_label", [](SgAnchorsArgs &a) { a.out_label = nullptr; }},
        {"null_out_gt_index", [](SgAnchorsArgs &a) { a.out_gt_index = nullptr; }},
        {"null_out_count", [](SgAnchorsArgs &a) { a.out_count = nullptr; }},
        {"null_out_gt_count", [](SgAnchorsArgs &a) { a.out_gt_count = nullptr; }},
        {"null_out_iou", [](SgAnchorsArgs &a) { a.out_iou = nullptr; }},
        {"bad_dtype", [](SgAnchorsArgs &a) { a.dtype = 2; }},
        {"float64", [](SgAnchorsArgs &a) { a.dtype = 1; bare(a); }},
        {"no_frames", [](SgAnchorsArgs &a) { a.n_frames = 0; }},
        {"anchors_0", [](SgAnchorsArgs &a) { a.n_anchors = 0; }},
        {"anchors_negative", [](SgAnchorsArgs &a) { a.n_anchors = -5; }},
        {"anchors_1", [](SgAnchorsArgs &a) { a.n_anchors = 1; }},
        {"gt_0", [](SgAnchorsArgs &a) { a.n_gt = 0; }},
        {"gt_1", [](SgAnchorsArgs &a) { a.n_gt = 1; }},
        {"gt_256", [](SgAnchorsArgs &a) { a.n_gt = 256; bare(a); }},
        {"gt_257", [](SgAnchorsArgs &a) { a.n_gt = 257; }},
        {"anchor_features_6", [](SgAnchorsArgs &a) { a.anchor_features = 6; }},
        {"anchor_features_10", [](SgAnchorsArgs &a) { a.anchor_features = 10; bare(a); }},
        {"anchor_features_11", [](SgAnchorsArgs &a) { a.anchor_features = 11; }},
        {"gt_features_7", [](SgAnchorsArgs &a) { a.gt_features = 7; }},
        {"gt_features_10", [](SgAnchorsArgs &a) { a.gt_features = 10; bare(a); }},
        {"gt_features_11", [](SgAnchorsArgs &a) { a.gt_features = 11; }},
        {"classes_0", [](SgAnchorsArgs &a) { a.n_classes = 0; }},
        {"classes_1", [](SgAnchorsArgs &a) { a.n_classes = 1; }},
        {"classes_16", [](SgAnchorsArgs &a) { a.n_classes = 16; }},
        {"classes_17", [](SgAnchorsArgs &a) { a.n_classes = 17; }},
        {"unmatched_0", [](SgAnchorsArgs &) { g_unmatched[1] = 0.0; }},
        {"unmatched_negative", [](SgAnchorsArgs &) { g_unmatched[0] = -0.1; }},
        {"unmatched_above_matched", [](SgAnchorsArgs &) { g_unmatched[2] = std::nextafter(0.6, 1.0); }},
        {"unmatched_equals_matched", [](SgAnchorsArgs &) { g_unmatched[2] = 0.6; }},
        {"matched_1", [](SgAnchorsArgs &) { g_matched[0] = 1.0; }},
        {"matched_above_1", [](SgAnchorsArgs &) { g_matched[0] = std::nextafter(1.0, 2.0); }},
        {"matched_nan", [nan](SgAnchorsArgs &) { g_matched[1] = nan; }},
        {"unmatched_nan", [nan](SgAnchorsArgs &) { g_unmatched[1] = nan; }},
        {"a_class_beyond_nc_is_not_read", [nan](SgAnchorsArgs &) { g_matched[3] = nan; g_unmatched[3] = -1.0; }},
        // F A: 2147483647 fits, 2^31 does not
        {"elements_at_2p31_minus_1", [](SgAnchorsArgs &a) { a.n_frames = 1; a.n_anchors = 2147483647; bare(a); }},
        {"elements_at_2p31", [](SgAnchorsArgs &a) { a.n_frames = 2; a.n_anchors = 1073741824; bare(a); }},
        {"elements_overflowing", [](SgAnchorsArgs &a) { a.n_frames = 2147483647; a.n_anchors = 2147483647; bare(a); }},
        {"label_is_anchors", [](SgAnchorsArgs &a) { a.out_label = (int32_t *)g_anchors; }},
        {"label_overlaps_anchors", [](SgAnchorsArgs &a) { a.out_label = (int32_t *)g_anchors + 34; }},      // the anchors' last element
        {"label_behind_anchors", [](SgAnchorsArgs &a) { a.out_label = (int32_t *)g_anchors + 35; }},
        {"gt_index_is_anchor_class", [](SgAnchorsArgs &a) { a.out_gt_index = g_class; }},
        {"count_overlaps_gt_boxes", [](SgAnchorsArgs &a) { a.out_count = (int32_t *)g_gt + 47; }},
        {"gt_count_is_gt_boxes", [](SgAnchorsArgs &a) { a.out_gt_count = (int32_t *)g_gt; }},
        {"iou_overlaps_anchor_class", [](SgAnchorsArgs &a) { a.out_iou = g_class + 4; }},
        {"iou_behind_anchor_class", [](SgAnchorsArgs &a) { a.out_iou = g_class + 5; }},
        {"gt_index_is_label", [](SgAnchorsArgs &a) { a.out_gt_index = g_label; }},
        {"count_overlaps_label", [](SgAnchorsArgs &a) { a.out_count = g_label + 9; }},
        {"count_behind_label", [](SgAnchorsArgs &a) { a.out_count = g_label + 10; }},
        {"gt_count_is_count", [](SgAnchorsArgs &a) { a.out_gt_count = g_count; }},
        {"iou_overlaps_gt_count", [](SgAnchorsArgs &a) { a.out_iou = g_gt_count + 5; }},
        {"iou_is_gt_index", [](SgAnchorsArgs &a) { a.out_iou = g_gt_index; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_anchors_and_anchors_0", [](SgAnchorsArgs &a) { a.anchors = nullptr; a.n_anchors = 0; }},
        {"anchors_0_and_gt_0", [](SgAnchorsArgs &a) { a.n_anchors = 0; a.n_gt = 0; }},
        {"gt_0_and_anchor_features_6", [](SgAnchorsArgs &a) { a.n_gt = 0; a.anchor_features = 6; }},
        {"anchor_features_6_and_gt_features_7", [](SgAnchorsArgs &a) { a.anchor_features = 6; a.gt_features = 7; }},
        {"gt_features_7_and_classes_0", [](SgAnchorsArgs &a) { a.gt_features = 7; a.n_classes = 0; }},
        {"classes_17_and_unmatched_0", [](SgAnchorsArgs &a) { a.n_classes = 17; g_unmatched[1] = 0.0; }},
        {"unmatched_0_and_elements_at_2p31", [](SgAnchorsArgs &a) { g_unmatched[1] = 0.0; a.n_frames = 2; a.n_anchors = 1073741824; bare(a); }},
        {"elements_at_2p31_and_label_is_anchors", [](SgAnchorsArgs &a) { a.n_frames = 2; a.n_anchors = 1073741824; bare(a); a.out_label = (int32_t *)a.anchors; }},
    };
    for (const auto &cs : cases) {
        SgAnchorsArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_anchors_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
