// scene_refusals.cpp -- snowgpu_transform_scene_device through every refusal of sg_check_scene_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_scene_reference.py compares the lines with a table.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: F = 2 frames, N = 10 float32 rows, B = 3 boxes of 8 columns, T = 4 tries (padded: no
// range below leaves its array -- the try records of a call are 1536 bytes)
static float g_rows[10 * 5 + 100], g_gt[2 * 3 * 8 + 400], g_out_rows[10 * 5 + 100], g_out_gt[2 * 3 * 8 + 100];
static uint8_t g_keep[10 + 100], g_out_keep[10 + 100];
static int64_t g_off[3 + 100];
static int32_t g_box_of[10 + 100], g_state[2 * 3 + 100], g_tried[2 * 3 + 100];
static double g_pose[2 * 3 * 2 + 100], g_world[2 * 8 + 100], g_local[2 * 3 * 8 + 400], g_out_pose[2 * 3 * 2 + 100], g_tries[2 * 3 * 4 * 8 + 100];
static double g_rot[2], g_scale[2], g_ltrans[3], g_lrot[2], g_lscale[2];
static uint64_t g_step[1 + 100];

static void clean_call(SgSceneArgs &a)
{
    g_rot[0] = -0.78; g_rot[1] = 0.78; g_scale[0] = 0.95; g_scale[1] = 1.05;
    g_ltrans[0] = g_ltrans[1] = 0.25; g_ltrans[2] = 0.0; g_lrot[0] = -0.15; g_lrot[1] = 0.15; g_lscale[0] = g_lscale[1] = 1.0;
    a = SgSceneArgs{2, 10, 6, 0, g_off, g_rows, 3, g_gt, 8, g_pose, 3, g_rot, g_scale, 4, g_ltrans, g_lrot, g_lscale, g_step, g_box_of, g_keep,
                    g_out_rows, g_out_keep, g_out_gt, g_world, g_state, g_tried, g_local, g_out_pose, g_tries};
}

// (sizes larger than the host arrays that stand for them: every pointer far from every other)
static void bare(SgSceneArgs &a)
{
    auto at = [](int k) { return (void *)(uintptr_t)((uint64_t)(k + 1) << 40); };
    a.frame_off = (const int64_t *)at(0); a.rows = at(1); a.gt_boxes = at(2); a.pose_in = (const double *)at(3); a.step = (const uint64_t *)at(4);
    a.box_of = (const int32_t *)at(5); a.keep_in = (const uint8_t *)at(6); a.out_rows = at(7); a.out_keep = (uint8_t *)at(8); a.out_gt_boxes = at(9);
    a.out_world = (double *)at(10); a.out_state = (int32_t *)at(11); a.out_tried = (int32_t *)at(12); a.out_local = (double *)at(13);
    a.out_pose = (double *)at(14); a.out_tries = (double *)at(15);
}

int main()
{
    using Edit = std::function<void(SgSceneArgs &)>;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgSceneArgs &) {}},
        {"null_frame_off", [](SgSceneArgs &a) { a.frame_off = nullptr; }},
        {"null_rows", [](SgSceneArgs &a) { a.rows = nullptr; }},
        {"null_gt_boxes", [](SgSceneArgs &a) { a.gt_boxes = nullptr; }},
        {"null_out_rows", [](SgSceneArgs &a) { a.out_rows = nullptr; }},
        {"null_out_keep", [](SgSceneArgs &a) { a.out_keep = nullptr; }},
        {"null_out_gt_boxes", [](SgSceneArgs &a) { a.out_gt_boxes = nullptr; }},
        {"null_out_world", [](SgSceneArgs &a) { a.out_world = nullptr; }},
        {"null_out_state", [](SgSceneArgs &a) { a.out_state = nullptr; }},
        {"null_out_tried", [](SgSceneArgs &a) { a.out_tried = nullptr; }},
        {"null_out_local", [](SgSceneArgs &a) { a.out_local = nullptr; }},
        {"bad_dtype", [](SgSceneArgs &a) { a.dtype = 2; }},
        {"no_frames", [](SgSceneArgs &a) { a.n_frames = 0; }},
        {"rows_negative", [](SgSceneArgs &a) { a.n_total = -1; }},
        {"null_pose_in", [](SgSceneArgs &a) { a.pose_in = nullptr; }},
        {"null_keep_in", [](SgSceneArgs &a) { a.keep_in = nullptr; }},
        {"null_box_of", [](SgSceneArgs &a) { a.box_of = nullptr; }},
        {"null_out_pose", [](SgSceneArgs &a) { a.out_pose = nullptr; }},
        {"null_out_tries", [](SgSceneArgs &a) { a.out_tries = nullptr; }},
        {"every_part_off", [](SgSceneArgs &a) { a.flip = 0; a.rotation = a.scaling = a.local_translation = a.local_rotation = a.local_scaling = nullptr; }},
        {"no_rows_needs_no_row_buffers", [](SgSceneArgs &a) { a.n_total = 0; a.rows = nullptr; a.out_rows = nullptr; a.out_keep = nullptr; }},
        {"float64", [](SgSceneArgs &a) { a.dtype = 1; bare(a); }},
        {"boxes_0", [](SgSceneArgs &a) { a.n_boxes = 0; }},
        {"boxes_1", [](SgSceneArgs &a) { a.n_boxes = 1; }},
        {"boxes_256", [](SgSceneArgs &a) { a.n_boxes = 256; bare(a); }},
        {"boxes_257", [](SgSceneArgs &a) { a.n_boxes = 257; bare(a); }},
        {"box_features_6", [](SgSceneArgs &a) { a.box_features = 6; }},
        {"box_features_7", [](SgSceneArgs &a) { a.box_features = 7; }},
        {"box_features_10", [](SgSceneArgs &a) { a.box_features = 10; bare(a); }},
        {"box_features_11", [](SgSceneArgs &a) { a.box_features = 11; }},
        {"flip_negative", [](SgSceneArgs &a) { a.flip = -1; }},
        {"flip_0", [](SgSceneArgs &a) { a.flip = 0; }},
        {"flip_4", [](SgSceneArgs &a) { a.flip = 4; }},
        {"tries_negative", [](SgSceneArgs &a) { a.tries = -1; }},
        {"tries_0", [](SgSceneArgs &a) { a.tries = 0; }},
        {"tries_16", [](SgSceneArgs &a) { a.tries = 16; bare(a); }},
        {"tries_17", [](SgSceneArgs &a) { a.tries = 17; bare(a); }},
        {"rotation_nan", [nan](SgSceneArgs &) { g_rot[0] = nan; }},
        {"rotation_inf", [inf](SgSceneArgs &) { g_rot[1] = inf; }},
        {"rotation_lo_above_hi", [](SgSceneArgs &) { g_rot[0] = 1.0; g_rot[1] = 0.5; }},
        {"rotation_lo_is_hi", [](SgSceneArgs &) { g_rot[0] = g_rot[1] = 0.5; }},
        {"scaling_lo_above_hi", [](SgSceneArgs &) { g_scale[0] = 1.1; g_scale[1] = 1.0; }},
        {"local_rotation_nan", [nan](SgSceneArgs &) { g_lrot[1] = nan; }},
        {"local_scaling_lo_above_hi", [](SgSceneArgs &) { g_lscale[0] = 1.5; }},
        {"local_ranges_are_not_read_without_tries", [nan](SgSceneArgs &a) { a.tries = 0; g_lrot[0] = nan; g_lscale[0] = -1.0; g_ltrans[0] = -1.0; }},
        {"scaling_0", [](SgSceneArgs &) { g_scale[0] = 0.0; }},
        {"scaling_negative", [](SgSceneArgs &) { g_scale[0] = -0.5; }},
        {"local_scaling_0", [](SgSceneArgs &) { g_lscale[0] = 0.0; }},
        {"translation_negative", [](SgSceneArgs &) { g_ltrans[1] = -0.1; }},
        {"translation_100", [](SgSceneArgs &) { g_ltrans[2] = 100.0; }},
        {"translation_above_100", [](SgSceneArgs &) { g_ltrans[2] = std::nextafter(100.0, 200.0); }},
        {"translation_nan", [nan](SgSceneArgs &) { g_ltrans[0] = nan; }},
        // F B max(T, 1) 10: 2^31 - 1 does not factor into this shape
        {"elements_below_2p31", [](SgSceneArgs &a) { a.n_frames = 17895697; bare(a); }},        // x 3 x 4 x 10 = 2147483640
        {"elements_at_2p31", [](SgSceneArgs &a) { a.n_frames = 17895698; bare(a); }},           // x 3 x 4 x 10 = 2147483760
        {"rows_at_2p31", [](SgSceneArgs &a) { a.n_total = (int64_t)1 << 31; bare(a); }},
        {"frame_of_2p30", [](SgSceneArgs &a) { a.n_total = ((int64_t)1 << 30) + 5; a.max_frame_rows = (int64_t)1 << 30; bare(a); }},
        {"frame_above_2p30", [](SgSceneArgs &a) { a.n_total = ((int64_t)1 << 30) + 5; a.max_frame_rows = ((int64_t)1 << 30) + 1; bare(a); }},
        {"null_step", [](SgSceneArgs &a) { a.step = nullptr; }},
        {"in_place", [](SgSceneArgs &a) { a.out_rows = g_rows; }},
        {"out_rows_overlaps_rows", [](SgSceneArgs &a) { a.out_rows = g_rows + 49; }},
        {"out_rows_behind_rows", [](SgSceneArgs &a) { a.out_rows = g_rows + 50; }},
        {"out_keep_is_keep_in", [](SgSceneArgs &a) { a.out_keep = g_keep; }},
        {"out_keep_behind_keep_in", [](SgSceneArgs &a) { a.out_keep = g_keep + 10; }},
        {"out_gt_boxes_is_gt_boxes", [](SgSceneArgs &a) { a.out_gt_boxes = g_gt; }},
        {"world_overlaps_frame_off", [](SgSceneArgs &a) { a.out_world = (double *)g_off + 2; }},
        {"state_is_box_of", [](SgSceneArgs &a) { a.out_state = g_box_of + 9; }},
        {"state_behind_box_of", [](SgSceneArgs &a) { a.out_state = g_box_of + 10; }},
        {"box_of_is_not_read_without_tries", [](SgSceneArgs &a) { a.tries = 0; a.out_state = g_box_of; }},
        {"tried_is_step", [](SgSceneArgs &a) { a.out_tried = (int32_t *)g_step + 1; }},
        {"local_is_pose_in", [](SgSceneArgs &a) { a.out_local = g_pose; }},
        {"pose_is_pose_in", [](SgSceneArgs &a) { a.out_pose = g_pose + 11; }},
        {"tries_is_gt_boxes", [](SgSceneArgs &a) { a.out_tries = (double *)g_gt; }},
        {"in_place_and_keep_in_the_rows", [](SgSceneArgs &a) { a.out_rows = g_rows; a.out_keep = (uint8_t *)g_rows + 199; }},
        {"out_keep_is_out_rows", [](SgSceneArgs &a) { a.out_keep = (uint8_t *)g_out_rows + 199; }},
        {"out_keep_behind_out_rows", [](SgSceneArgs &a) { a.out_keep = (uint8_t *)g_out_rows + 200; }},
        {"tried_is_state", [](SgSceneArgs &a) { a.out_tried = g_state; }},
        {"local_is_world", [](SgSceneArgs &a) { a.out_local = g_world + 15; }},
        {"pose_is_out_gt_boxes", [](SgSceneArgs &a) { a.out_pose = (double *)g_out_gt; }},
        {"tries_is_local", [](SgSceneArgs &a) { a.out_tries = g_local + 47; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_gt_boxes_and_boxes_0", [](SgSceneArgs &a) { a.gt_boxes = nullptr; a.n_boxes = 0; }},
        {"boxes_0_and_box_features_6", [](SgSceneArgs &a) { a.n_boxes = 0; a.box_features = 6; }},
        {"box_features_6_and_flip_4", [](SgSceneArgs &a) { a.box_features = 6; a.flip = 4; }},
        {"flip_4_and_tries_17", [](SgSceneArgs &a) { a.flip = 4; a.tries = 17; }},
        {"tries_17_and_rotation_nan", [nan](SgSceneArgs &a) { a.tries = 17; g_rot[0] = nan; }},
        {"rotation_nan_and_scaling_0", [nan](SgSceneArgs &) { g_rot[0] = nan; g_scale[0] = 0.0; }},
        {"scaling_0_and_translation_nan", [nan](SgSceneArgs &) { g_scale[0] = 0.0; g_ltrans[0] = nan; }},
        {"translation_nan_and_elements_at_2p31", [nan](SgSceneArgs &a) { g_ltrans[0] = nan; a.n_frames = 17895698; bare(a); }},
        {"elements_at_2p31_and_rows_at_2p31", [](SgSceneArgs &a) { a.n_frames = 17895698; a.n_total = (int64_t)1 << 31; bare(a); }},
        {"rows_at_2p31_and_frame_above_2p30", [](SgSceneArgs &a) { a.n_total = (int64_t)1 << 31; a.max_frame_rows = ((int64_t)1 << 30) + 1; bare(a); }},
        {"frame_above_2p30_and_null_step", [](SgSceneArgs &a) { a.n_total = ((int64_t)1 << 30) + 5; a.max_frame_rows = ((int64_t)1 << 30) + 1; bare(a); a.step = nullptr; }},
        {"null_step_and_out_rows_overlaps_rows", [](SgSceneArgs &a) { a.step = nullptr; a.out_rows = g_rows + 49; }},
    };
    for (const auto &cs : cases) {
        SgSceneArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_scene_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
