// paste_refusals.cpp -- snowgpu_paste_objects_device through every refusal of sg_check_paste_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_paste_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: F = 2 frames, N = 10 float32 rows, B = 3 gt boxes of 8 columns, NC = 3 classes with
// (2, 1, 1) slots, Q = 4; a bank of O = 2 objects with P = 6 points (padded: no range below leaves its array)
static float g_rows[10 * 5 + 100], g_gt[2 * 3 * 8 + 100], g_bank_points[6 * 5 + 100], g_bank_boxes[2 * 8 + 100], g_out_rows[10 * 5 + 100], g_out_gt[2 * 7 * 8 + 100];
static uint8_t g_keep[10 + 100], g_out_keep[10 + 100];
static int64_t g_off[3 + 100], g_bank_off[3 + 100];
static double g_pose[2 * 3 * 2 + 100], g_bank_pose[2 * 2 + 100], g_out_pose[2 * 7 * 2 + 100], g_ew[3];
static int32_t g_class_off[18 + 100], g_groups[16], g_object[2 * 4 + 100], g_state[2 * 4 + 100], g_source[10 + 100], g_count[2 * 4 + 100];
static uint64_t g_step[1 + 100];

static void clean_call(SgPasteArgs &a)
{
    for (int c = 0; c < 16; ++c) g_groups[c] = 0;
    g_groups[0] = 2; g_groups[1] = 1; g_groups[2] = 1;
    g_ew[0] = g_ew[1] = g_ew[2] = 0.2;
    a = SgPasteArgs{2, 10, 6, 0, g_off, g_rows, 3, g_gt, 8, g_pose, 6, 2, g_bank_points, g_bank_off, g_bank_boxes, g_bank_pose, g_class_off, 3, g_groups, g_ew, g_step,
                    g_keep, g_out_rows, g_out_keep, g_out_gt, g_object, g_state, g_source, g_count, g_out_pose};
}

// (sizes larger than the host arrays that stand for them: every pointer far from every other)
static void bare(SgPasteArgs &a)
{
    auto at = [](int k) { return (void *)(uintptr_t)((uint64_t)(k + 1) << 40); };
    a.frame_off = (const int64_t *)at(0); a.rows = at(1); a.gt_boxes = at(2); a.pose_in = (const double *)at(3); a.bank_points = at(4);
    a.bank_off = (const int64_t *)at(5); a.bank_boxes = at(6); a.bank_pose = (const double *)at(7); a.class_off = (const int32_t *)at(8);
    a.step = (const uint64_t *)at(9); a.keep_in = (const uint8_t *)at(10); a.out_rows = at(11); a.out_keep = (uint8_t *)at(12); a.out_gt_boxes = at(13);
    a.out_object = (int32_t *)at(14); a.out_state = (int32_t *)at(15); a.out_source = (int32_t *)at(16); a.out_count = (int32_t *)at(17);
    a.out_pose = (double *)at(18);
}

int main()
{
    using Edit = std::function<void(SgPasteArgs &)>;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgPasteArgs &) {}},
        {"null_frame_off", [](SgPasteArgs &a) { a.frame_off = nullptr; }},
        {"null_rows", [](SgPasteArgs &a) { a.rows = nullptr; }},
        {"null_gt_boxes", [](SgPasteArgs &a) { a.gt_boxes = nullptr; }},
        {"null_bank_points", [](SgPasteArgs &a) { a.bank_points = nullptr; }},
        {"null_bank_off", [](SgPasteArgs &a) { a.bank_off = nullptr; }},
        {"null_bank_boxes", [](SgPasteArgs &a) { a.bank_boxes = nullptr; }},
        {"null_bank_pose", [](SgPasteArgs &a) { a.bank_pose = nullptr; }},
        {"null_class_off", [](SgPasteArgs &a) { a.class_off = nullptr; }},
        {"null_groups", [](SgPasteArgs &a) { a.groups = nullptr; }},
        {"null_out_rows", [](SgPasteArgs &a) { a.out_rows = nullptr; }},
        {"null_out_keep", [](SgPasteArgs &a) { a.out_keep = nullptr; }},
        {"null_out_gt_boxes", [](SgPasteArgs &a) { a.out_gt_boxes = nullptr; }},
        {"null_out_object", [](SgPasteArgs &a) { a.out_object = nullptr; }},
        {"null_out_state", [](SgPasteArgs &a) { a.out_state = nullptr; }},
        {"null_out_count", [](SgPasteArgs &a) { a.out_count = nullptr; }},
        {"null_pose_in", [](SgPasteArgs &a) { a.pose_in = nullptr; }},
        {"null_keep_in", [](SgPasteArgs &a) { a.keep_in = nullptr; }},
        {"null_out_source", [](SgPasteArgs &a) { a.out_source = nullptr; }},
        {"null_out_pose", [](SgPasteArgs &a) { a.out_pose = nullptr; }},
        {"null_extra_width", [](SgPasteArgs &a) { a.extra_width = nullptr; }},
        {"no_rows_needs_no_row_buffers", [](SgPasteArgs &a) { a.n_total = 0; a.rows = nullptr; a.out_rows = nullptr; a.out_keep = nullptr; }},
        {"bank_without_points", [](SgPasteArgs &a) { a.bank_points_n = 0; a.bank_points = nullptr; }},
        {"bad_dtype", [](SgPasteArgs &a) { a.dtype = 2; }},
        {"float64", [](SgPasteArgs &a) { a.dtype = 1; bare(a); }},
        {"no_frames", [](SgPasteArgs &a) { a.n_frames = 0; }},
        {"rows_negative", [](SgPasteArgs &a) { a.n_total = -1; }},
        {"slots_0", [](SgPasteArgs &) { g_groups[0] = g_groups[1] = g_groups[2] = 0; }},
        {"slots_1", [](SgPasteArgs &) { g_groups[0] = 1; g_groups[1] = g_groups[2] = 0; }},
        {"slots_64", [](SgPasteArgs &a) { g_groups[0] = 62; bare(a); }},
        {"slots_65", [](SgPasteArgs &a) { g_groups[0] = 63; bare(a); }},
        {"classes_0", [](SgPasteArgs &a) { a.n_classes = 0; }},                               // (no class, no slot: the slots' message)
        {"classes_16", [](SgPasteArgs &a) { a.n_classes = 16; }},
        {"classes_17", [](SgPasteArgs &a) { a.n_classes = 17; }},
        {"classes_negative_with_slots", [](SgPasteArgs &a) { a.n_classes = -1; }},
        {"gt_0", [](SgPasteArgs &a) { a.n_gt = 0; }},
        {"gt_1", [](SgPasteArgs &a) { a.n_gt = 1; }},
        {"gt_252", [](SgPasteArgs &a) { a.n_gt = 252; bare(a); }},
        {"gt_253", [](SgPasteArgs &a) { a.n_gt = 253; bare(a); }},
        {"gt_features_7", [](SgPasteArgs &a) { a.gt_features = 7; }},
        {"gt_features_10", [](SgPasteArgs &a) { a.gt_features = 10; bare(a); }},
        {"gt_features_11", [](SgPasteArgs &a) { a.gt_features = 11; }},
        {"group_negative", [](SgPasteArgs &) { g_groups[0] = 5; g_groups[1] = -1; }},
        {"a_group_beyond_nc_is_not_read", [](SgPasteArgs &) { g_groups[3] = -7; }},
        {"extra_width_negative", [](SgPasteArgs &) { g_ew[1] = -0.1; }},
        {"extra_width_100", [](SgPasteArgs &) { g_ew[2] = 100.0; }},
        {"extra_width_above_100", [](SgPasteArgs &) { g_ew[2] = std::nextafter(100.0, 200.0); }},
        {"extra_width_nan", [nan](SgPasteArgs &) { g_ew[0] = nan; }},
        {"extra_width_inf", [inf](SgPasteArgs &) { g_ew[0] = inf; }},
        // F (B + Q) Cb: 2147483647 does not factor into this shape; 2^31 - 8 fits, 2^31 does not
        {"elements_below_2p31", [](SgPasteArgs &a) { a.n_frames = 38347921; bare(a); }},       // x 7 x 8 = 2147483576
        {"elements_at_2p31", [](SgPasteArgs &a) { a.n_frames = 38347923; bare(a); }},          // x 7 x 8 = 2147483688
        {"rows_at_2p31", [](SgPasteArgs &a) { a.n_total = (int64_t)1 << 31; bare(a); }},
        {"bank_points_at_2p31", [](SgPasteArgs &a) { a.bank_points_n = (int64_t)1 << 31; bare(a); }},
        {"bank_objects_at_2p31", [](SgPasteArgs &a) { a.bank_objects_n = (int64_t)1 << 31; bare(a); }},
        {"frame_of_2p30", [](SgPasteArgs &a) { a.n_total = ((int64_t)1 << 30) + 5; a.max_frame_rows = (int64_t)1 << 30; bare(a); }},
        {"frame_above_2p30", [](SgPasteArgs &a) { a.n_total = ((int64_t)1 << 30) + 5; a.max_frame_rows = ((int64_t)1 << 30) + 1; bare(a); }},
        {"null_step", [](SgPasteArgs &a) { a.step = nullptr; }},
        {"out_rows_is_rows", [](SgPasteArgs &a) { a.out_rows = g_rows; }},
        {"out_rows_overlaps_rows", [](SgPasteArgs &a) { a.out_rows = g_rows + 49; }},
        {"out_rows_behind_rows", [](SgPasteArgs &a) { a.out_rows = g_rows + 50; }},
        {"out_keep_is_keep_in", [](SgPasteArgs &a) { a.out_keep = g_keep; }},
        {"out_keep_behind_keep_in", [](SgPasteArgs &a) { a.out_keep = g_keep + 10; }},
        {"out_gt_boxes_is_gt_boxes", [](SgPasteArgs &a) { a.out_gt_boxes = g_gt; }},
        {"object_overlaps_frame_off", [](SgPasteArgs &a) { a.out_object = (int32_t *)g_off + 5; }},
        {"state_is_bank_off", [](SgPasteArgs &a) { a.out_state = (int32_t *)g_bank_off; }},
        {"source_overlaps_bank_points", [](SgPasteArgs &a) { a.out_source = (int32_t *)g_bank_points + 29; }},
        {"source_behind_bank_points", [](SgPasteArgs &a) { a.out_source = (int32_t *)g_bank_points + 30; }},
        {"count_is_bank_boxes", [](SgPasteArgs &a) { a.out_count = (int32_t *)g_bank_boxes; }},
        {"count_is_class_off", [](SgPasteArgs &a) { a.out_count = g_class_off + 17; }},
        {"count_is_step", [](SgPasteArgs &a) { a.out_count = (int32_t *)g_step + 1; }},
        {"pose_is_pose_in", [](SgPasteArgs &a) { a.out_pose = g_pose; }},
        {"pose_is_bank_pose", [](SgPasteArgs &a) { a.out_pose = g_bank_pose + 3; }},
        {"out_keep_is_out_rows", [](SgPasteArgs &a) { a.out_keep = (uint8_t *)g_out_rows + 199; }},
        {"out_keep_behind_out_rows", [](SgPasteArgs &a) { a.out_keep = (uint8_t *)g_out_rows + 200; }},
        {"state_is_object", [](SgPasteArgs &a) { a.out_state = g_object; }},
        {"source_overlaps_state", [](SgPasteArgs &a) { a.out_source = g_state + 7; }},
        {"count_is_out_gt_boxes", [](SgPasteArgs &a) { a.out_count = (int32_t *)g_out_gt; }},
        {"pose_is_count", [](SgPasteArgs &a) { a.out_pose = (double *)g_count; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_gt_boxes_and_slots_0", [](SgPasteArgs &a) { a.gt_boxes = nullptr; g_groups[0] = g_groups[1] = g_groups[2] = 0; }},
        {"slots_65_and_classes_17", [](SgPasteArgs &a) { g_groups[0] = 63; a.n_classes = 17; }},
        {"classes_17_and_gt_0", [](SgPasteArgs &a) { a.n_classes = 17; a.n_gt = 0; }},
        {"gt_0_and_gt_features_7", [](SgPasteArgs &a) { a.n_gt = 0; a.gt_features = 7; }},
        {"gt_features_7_and_group_negative", [](SgPasteArgs &a) { a.gt_features = 7; g_groups[0] = 5; g_groups[1] = -1; }},
        {"group_negative_and_extra_width_nan", [nan](SgPasteArgs &) { g_groups[0] = 5; g_groups[1] = -1; g_ew[0] = nan; }},
        {"extra_width_nan_and_elements_at_2p31", [nan](SgPasteArgs &a) { g_ew[0] = nan; a.n_frames = 38347923; bare(a); }},
        {"elements_at_2p31_and_rows_at_2p31", [](SgPasteArgs &a) { a.n_frames = 38347923; a.n_total = (int64_t)1 << 31; bare(a); }},
        {"rows_at_2p31_and_bank_points_at_2p31", [](SgPasteArgs &a) { a.n_total = (int64_t)1 << 31; a.bank_points_n = (int64_t)1 << 31; bare(a); }},
        {"bank_points_at_2p31_and_frame_above_2p30", [](SgPasteArgs &a) { a.bank_points_n = (int64_t)1 << 31; a.n_total = ((int64_t)1 << 30) + 5; a.max_frame_rows = ((int64_t)1 << 30) + 1; bare(a); }},
        {"frame_above_2p30_and_null_step", [](SgPasteArgs &a) { a.n_total = ((int64_t)1 << 30) + 5; a.max_frame_rows = ((int64_t)1 << 30) + 1; bare(a); a.step = nullptr; }},
        {"null_step_and_out_rows_is_rows", [](SgPasteArgs &a) { a.step = nullptr; a.out_rows = g_rows; }},
    };
    for (const auto &cs : cases) {
        SgPasteArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_paste_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
