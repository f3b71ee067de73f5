// iou_refusals.cpp -- the refusals of snowgpu_boxes_iou_device and snowgpu_nms_device on the host: sg_check_iou_args and sg_check_nms_args
// (csrc/sg_device_args.h, which needs no HIP) over the edges of both domains; one line "<case>|<rc>|<message or OK>" per case
// (tests/test_iou_reference.py holds the expected lines).  No memory is touched: the pointers are numbers.
#include <cmath>
#include <cstdio>
#include <functional>
#include <vector>

#include "sg_device_args.h"

static void *at(uintptr_t v) { return (void *)v; }

int main()
{
    // 2 frames of 100 x 50 float32 boxes of 8 columns, every array 1 MiB apart
    const SgIouArgs iou{2, 100, at(0x100000), 8, 50, at(0x200000), 8, 0, 1, (const double *)at(0x300000), (const double *)at(0x400000),
                        at(0x500000), (int32_t *)at(0x600000), at(0x700000)};
    const SgNmsArgs nms{2, 100, at(0x100000), 8, at(0x200000), 0, 0, 0.5, 0.1, 40, (const double *)at(0x300000), (int32_t *)at(0x400000),
                        (int32_t *)at(0x500000), at(0x600000), at(0x700000), (uint8_t *)at(0x800000)};
    typedef std::function<void(SgIouArgs &)> I;
    typedef std::function<void(SgNmsArgs &)> N;
    const std::vector<std::pair<const char *, I>> ic = {
        {"iou_clean", [](SgIouArgs &) {}},
        {"iou_best_only", [](SgIouArgs &a) { a.out_iou = nullptr; a.out_best_iou = nullptr; a.pose_a = nullptr; a.pose_b = nullptr; }},
        {"iou_m_9216", [](SgIouArgs &a) { a.n_a = 9216; a.n_b = 1; a.out_iou = nullptr; }},
        {"iou_same_set", [](SgIouArgs &a) { a.boxes_b = a.boxes_a; a.n_b = a.n_a; a.pose_b = a.pose_a; }},
        {"iou_slots_2p31_minus_1", [](SgIouArgs &a) { a.n_frames = 2147483647; a.n_a = 1; a.n_b = 1; a.out_iou = nullptr; a.out_best_iou = nullptr; a.pose_a = a.pose_b = nullptr; a.boxes_b = a.boxes_a; a.out_best = (int32_t *)at((uintptr_t)1 << 40); }},
        {"iou_null_a", [](SgIouArgs &a) { a.boxes_a = nullptr; }},
        {"iou_dtype_2", [](SgIouArgs &a) { a.dtype = 2; }},
        {"iou_no_frames", [](SgIouArgs &a) { a.n_frames = 0; }},
        {"iou_mode_2", [](SgIouArgs &a) { a.mode = 2; }},
        {"iou_no_output", [](SgIouArgs &a) { a.out_iou = nullptr; a.out_best = nullptr; a.out_best_iou = nullptr; }},
        {"iou_m_0", [](SgIouArgs &a) { a.n_a = 0; }},
        {"iou_b_9217", [](SgIouArgs &a) { a.n_b = 9217; }},
        {"iou_feats_6", [](SgIouArgs &a) { a.a_features = 6; }},
        {"iou_feats_11", [](SgIouArgs &a) { a.b_features = 11; }},
        {"iou_slots_2p31", [](SgIouArgs &a) { a.n_frames = 32768; a.n_a = 256; a.n_b = 256; }},
        {"iou_out_is_boxes_b", [](SgIouArgs &a) { a.out_iou = (void *)a.boxes_b; }},
        {"iou_best_is_iou", [](SgIouArgs &a) { a.out_best = (int32_t *)a.out_iou; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"iou_null_a_and_mode_2", [](SgIouArgs &a) { a.boxes_a = nullptr; a.mode = 2; }},
        {"iou_mode_2_and_no_output", [](SgIouArgs &a) { a.mode = 2; a.out_iou = nullptr; a.out_best = nullptr; a.out_best_iou = nullptr; }},
        {"iou_no_output_and_m_0", [](SgIouArgs &a) { a.out_iou = nullptr; a.out_best = nullptr; a.out_best_iou = nullptr; a.n_a = 0; }},
        {"iou_m_0_and_feats_6", [](SgIouArgs &a) { a.n_a = 0; a.a_features = 6; }},
        {"iou_feats_6_and_slots_2p31", [](SgIouArgs &a) { a.a_features = 6; a.n_frames = 32768; a.n_a = 256; a.n_b = 256; }},
        {"iou_slots_2p31_and_out_is_boxes_b", [](SgIouArgs &a) { a.n_frames = 32768; a.n_a = 256; a.n_b = 256; a.out_iou = (void *)a.boxes_b; }},
    };
    const std::vector<std::pair<const char *, N>> nc = {
        {"nms_clean", [](SgNmsArgs &) {}},
        {"nms_bare", [](SgNmsArgs &a) { a.pose_in = nullptr; a.out_boxes = nullptr; a.out_scores = nullptr; a.out_kept = nullptr; }},
        {"nms_b_9216", [](SgNmsArgs &a) { a.n_frames = 1; a.n_boxes = 9216; a.post_max = 512; }},
        {"nms_post_max_b", [](SgNmsArgs &a) { a.post_max = a.n_boxes; }},
        {"nms_minus_inf", [](SgNmsArgs &a) { a.score_thresh = -INFINITY; a.iou_thresh = -1.0; }},
        {"nms_null_scores", [](SgNmsArgs &a) { a.scores = nullptr; }},
        {"nms_null_index", [](SgNmsArgs &a) { a.out_index = nullptr; }},
        {"nms_null_count", [](SgNmsArgs &a) { a.out_count = nullptr; }},
        {"nms_mode_m1", [](SgNmsArgs &a) { a.mode = -1; }},
        {"nms_b_0", [](SgNmsArgs &a) { a.n_boxes = 0; }},
        {"nms_b_9217", [](SgNmsArgs &a) { a.n_boxes = 9217; }},
        {"nms_feats_6", [](SgNmsArgs &a) { a.box_features = 6; }},
        {"nms_feats_11", [](SgNmsArgs &a) { a.box_features = 11; }},
        {"nms_post_max_0", [](SgNmsArgs &a) { a.post_max = 0; }},
        {"nms_post_max_b_plus_1", [](SgNmsArgs &a) { a.post_max = a.n_boxes + 1; }},
        {"nms_nan_iou_thresh", [](SgNmsArgs &a) { a.iou_thresh = NAN; }},
        {"nms_nan_score_thresh", [](SgNmsArgs &a) { a.score_thresh = NAN; }},
        {"nms_slots_2p31", [](SgNmsArgs &a) { a.n_frames = 1 << 20; a.n_boxes = 2048; a.post_max = 1; }},
        {"nms_boxes_out_is_boxes", [](SgNmsArgs &a) { a.out_boxes = (void *)a.boxes; }},
        {"nms_kept_overlaps_index", [](SgNmsArgs &a) { a.out_kept = (uint8_t *)a.out_index + 8; }},
        // two defects, of checks that stand next to each other: the earlier check's message
        {"nms_null_scores_and_mode_m1", [](SgNmsArgs &a) { a.scores = nullptr; a.mode = -1; }},
        {"nms_mode_m1_and_b_0", [](SgNmsArgs &a) { a.mode = -1; a.n_boxes = 0; }},
        {"nms_b_0_and_feats_6", [](SgNmsArgs &a) { a.n_boxes = 0; a.box_features = 6; }},
        {"nms_feats_6_and_post_max_0", [](SgNmsArgs &a) { a.box_features = 6; a.post_max = 0; }},
        {"nms_post_max_0_and_nan_iou_thresh", [](SgNmsArgs &a) { a.post_max = 0; a.iou_thresh = NAN; }},
        {"nms_nan_iou_thresh_and_slots_2p31", [](SgNmsArgs &a) { a.iou_thresh = NAN; a.n_frames = 1 << 20; a.n_boxes = 2048; a.post_max = 1; }},
        {"nms_slots_2p31_and_boxes_out_is_boxes", [](SgNmsArgs &a) { a.n_frames = 1 << 20; a.n_boxes = 2048; a.post_max = 1; a.out_boxes = (void *)a.boxes; }},
    };
    for (const auto &cs : ic) {
        SgIouArgs a = iou;
        cs.second(a);
        std::string msg;
        const int rc = sg_check_iou_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    for (const auto &cs : nc) {
        SgNmsArgs a = nms;
        cs.second(a);
        std::string msg;
        const int rc = sg_check_nms_args(a, &msg);
        std::printf("%s|%d|%s\n", cs.first, rc, rc ? msg.c_str() : "OK");
    }
    return 0;
}
