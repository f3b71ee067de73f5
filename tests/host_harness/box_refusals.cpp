// box_refusals.cpp -- snowgpu_points_in_boxes_device through every refusal of sg_check_box_args (csrc/sg_device_args.h), one defect at a
// time, and through clean calls at the edges of the domain.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints
// case|code|message.  tests/test_box_reference.py compares the lines with a table.
#include <cstdio>
#include <functional>
#include <vector>

#include "sg_device_args.h"

// host arrays of the sizes the arguments stand for: two frames of four float32 rows, B = 3 boxes of 8 columns
// (padded by what the longest output placed behind them takes: no range below leaves its array)
static float g_rows[8 * 5 + 40], g_boxes[2 * 3 * 8 + 40], g_local[8 * 3 + 8];
static double g_pose_in[2 * 3 * 2 + 16], g_pose[2 * 3 * 2 + 16];
static uint8_t g_keep[8 + 200];
static int64_t g_off[3] = {0, 4, 8};
static int32_t g_box_of[8 + 40], g_count[2 * 3 + 40];

static void clean_call(SgBoxArgs &a)
{
    a = SgBoxArgs{2, 8, 4, 0, g_off, g_rows, 3, g_boxes, 8, g_pose_in, g_keep, g_box_of, g_count, g_local, g_pose};
}

// (sizes larger than the host arrays that stand for them: nothing is given to overlap)
static void bare(SgBoxArgs &a)
{
    a.out_box_of = nullptr; a.out_count = nullptr; a.out_local = nullptr; a.out_pose = nullptr; a.keep_in = nullptr; a.rows = nullptr; a.pose_in = nullptr;
    a.n_total = 0; a.boxes = (const void *)(uintptr_t)((uint64_t)1 << 44);
}

int main()
{
    using Edit = std::function<void(SgBoxArgs &)>;
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](SgBoxArgs &) {}},
        {"null_frame_offsets", [](SgBoxArgs &a) { a.frame_off = nullptr; }},
        {"null_rows", [](SgBoxArgs &a) { a.rows = nullptr; }},
        {"null_boxes", [](SgBoxArgs &a) { a.boxes = nullptr; }},
        {"null_out_box_of", [](SgBoxArgs &a) { a.out_box_of = nullptr; }},
        {"null_out_count", [](SgBoxArgs &a) { a.out_count = nullptr; }},
        {"null_out_local", [](SgBoxArgs &a) { a.out_local = nullptr; }},
        {"null_out_pose", [](SgBoxArgs &a) { a.out_pose = nullptr; }},
        {"null_pose_in", [](SgBoxArgs &a) { a.pose_in = nullptr; }},
        {"null_keep_in", [](SgBoxArgs &a) { a.keep_in = nullptr; }},
        {"bad_dtype", [](SgBoxArgs &a) { a.dtype = 2; }},
        {"float64", [](SgBoxArgs &a) { a.dtype = 1; bare(a); }},
        {"no_frames", [](SgBoxArgs &a) { a.n_frames = 0; }},
        {"negative_rows", [](SgBoxArgs &a) { a.n_total = -1; }},
        {"empty_null_rows_and_box_of", [](SgBoxArgs &a) { a.n_total = 0; a.rows = nullptr; a.out_box_of = nullptr; }},
        {"rows_2p31", [](SgBoxArgs &a) { a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; }},
        {"boxes_0", [](SgBoxArgs &a) { a.n_boxes = 0; }},
        {"boxes_1", [](SgBoxArgs &a) { a.n_boxes = 1; }},
        {"boxes_256", [](SgBoxArgs &a) { a.n_boxes = 256; bare(a); }},
        {"boxes_257", [](SgBoxArgs &a) { a.n_boxes = 257; }},
        {"boxes_negative", [](SgBoxArgs &a) { a.n_boxes = -4; }},
        {"box_features_6", [](SgBoxArgs &a) { a.box_features = 6; }},
        {"box_features_7", [](SgBoxArgs &a) { a.box_features = 7; }},
        {"box_features_10", [](SgBoxArgs &a) { a.box_features = 10; bare(a); }},
        {"box_features_11", [](SgBoxArgs &a) { a.box_features = 11; }},
        {"slots_2p31_minus_256", [](SgBoxArgs &a) { a.n_frames = 8388607; a.n_boxes = 256; bare(a); }},
        {"slots_2p31", [](SgBoxArgs &a) { a.n_frames = 8388608; a.n_boxes = 256; bare(a); }},
        {"slots_overflowing", [](SgBoxArgs &a) { a.n_frames = 2147483647; a.n_boxes = 256; bare(a); }},
        {"frame_2p30_rows", [](SgBoxArgs &a) { a.n_total = (int64_t)1 << 30; a.max_frame_rows = 0; a.keep_in = nullptr; a.rows = (const void *)(uintptr_t)((uint64_t)1 << 40);
                                               a.out_box_of = (int32_t *)(uintptr_t)((uint64_t)1 << 45); a.out_local = nullptr; }},
        {"frame_2p30_plus_1_rows", [](SgBoxArgs &a) { a.n_total = ((int64_t)1 << 30) + 1; a.max_frame_rows = 0; }},
        {"box_of_is_keep_in", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_keep; }},
        {"box_of_overlaps_keep_in", [](SgBoxArgs &a) { a.keep_in = (const uint8_t *)g_box_of + 31; }},     // its last byte
        {"keep_in_behind_box_of", [](SgBoxArgs &a) { a.keep_in = (const uint8_t *)g_box_of + 32; }},
        {"count_overlaps_keep_in", [](SgBoxArgs &a) { a.keep_in = (const uint8_t *)g_count + 23; }},
        {"local_overlaps_keep_in", [](SgBoxArgs &a) { a.keep_in = (const uint8_t *)g_local; }},
        {"pose_overlaps_keep_in", [](SgBoxArgs &a) { a.keep_in = (const uint8_t *)g_pose + 95; }},
        {"box_of_overlaps_rows", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_rows + 39; }},              // the rows' last element
        {"box_of_behind_rows", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_rows + 40; }},
        {"count_is_rows", [](SgBoxArgs &a) { a.out_count = (int32_t *)g_rows; }},
        {"local_is_rows", [](SgBoxArgs &a) { a.out_local = g_rows; }},
        {"pose_overlaps_rows", [](SgBoxArgs &a) { a.rows = (const float *)g_pose + 4; }},
        {"box_of_overlaps_boxes", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_boxes + 47; }},            // the boxes' last element
        {"box_of_behind_boxes", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_boxes + 48; }},
        {"count_is_boxes", [](SgBoxArgs &a) { a.out_count = (int32_t *)g_boxes; }},
        {"local_overlaps_boxes", [](SgBoxArgs &a) { a.out_local = g_boxes + 30; }},
        {"pose_overlaps_boxes", [](SgBoxArgs &a) { a.boxes = (const float *)g_pose + 2; }},
        {"box_of_overlaps_pose_in", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_pose_in + 23; }},        // the given pose's last half
        {"box_of_behind_pose_in", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_pose_in + 24; }},
        {"count_is_pose_in", [](SgBoxArgs &a) { a.out_count = (int32_t *)g_pose_in; }},
        {"local_overlaps_pose_in", [](SgBoxArgs &a) { a.out_local = g_pose_in + 3; }},
        {"pose_is_pose_in", [](SgBoxArgs &a) { a.out_pose = g_pose_in; }},
        {"count_is_box_of", [](SgBoxArgs &a) { a.out_count = g_box_of; }},
        {"count_behind_box_of", [](SgBoxArgs &a) { a.out_count = g_box_of + 8; }},
        {"local_overlaps_box_of", [](SgBoxArgs &a) { a.out_local = (float *)g_box_of + 7; }},
        {"local_overlaps_count", [](SgBoxArgs &a) { a.out_local = (float *)g_count + 5; }},
        {"pose_overlaps_box_of", [](SgBoxArgs &a) { a.out_box_of = (int32_t *)g_pose + 10; }},
        {"pose_overlaps_count", [](SgBoxArgs &a) { a.out_count = (int32_t *)g_pose + 23; }},
        {"pose_is_local", [](SgBoxArgs &a) { a.out_pose = (double *)g_local; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"null_and_rows_2p31", [](SgBoxArgs &a) { a.frame_off = nullptr; a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; }},
        {"rows_2p31_and_boxes_0", [](SgBoxArgs &a) { a.n_total = (int64_t)1 << 31; a.keep_in = nullptr; a.n_boxes = 0; }},
        {"boxes_0_and_box_features_6", [](SgBoxArgs &a) { a.n_boxes = 0; a.box_features = 6; }},
        {"box_features_6_and_slots_2p31", [](SgBoxArgs &a) { a.box_features = 6; a.n_frames = 8388608; a.n_boxes = 256; bare(a); }},
        {"slots_2p31_and_frame_2p30_plus_1_rows", [](SgBoxArgs &a) { a.n_frames = 8388608; a.n_boxes = 256; a.n_total = ((int64_t)1 << 30) + 1; a.max_frame_rows = 0; }},
        {"frame_2p30_plus_1_rows_and_box_of_is_keep_in", [](SgBoxArgs &a) { a.n_total = ((int64_t)1 << 30) + 1; a.max_frame_rows = 0; a.out_box_of = (int32_t *)g_keep; }},
    };
    for (const auto &cs : cases) {
        SgBoxArgs a;
        clean_call(a);
        cs.second(a);
        std::string msg;
        const int rc = sg_check_box_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
