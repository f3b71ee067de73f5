// Host harness: the proposal target sampling of csrc/sg_targets.h (sg_targets_frame -- the classes, the lists, the words, the split, the
// walk, the picks and what a slot stores, the functions k_sample_rois runs on the device) compiled for the host, on a case from a file,
// for tests/test_targets_reference.py to compare byte for byte with the restatement (tests/targets_reference.py).
//   usage: targets_walk dtype F M B Cb Cg S fg_per_image reg_fg cls_fg cls_bg cls_bg_lo hard_ratio cls_mode seed step in out
//   in:    rois (F, M, Cb) T | gt (F, B, Cg) T | overlap (F, M) T | assignment (F, M) int32 | pose (F, M, 2) float64, raw, in this order
//   out:   index | rois | roi_iou | gt_index | gt_of_rois | reg_valid | cls_label | segments | class_count | pose | gt_local, raw
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sg_targets.h"

template <typename T> static bool read_all(FILE *fp, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), fp) == v.size(); }
template <typename T> static bool write_all(FILE *fp, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), fp) == v.size(); }

template <typename T>
static int run(const SgTargetCfg &c, int F, int M, int B, int Cb, int Cg, uint64_t seed, uint64_t step, const char *in, const char *out)
{
    const size_t q = (size_t)F * M, k = (size_t)F * c.S;
    std::vector<T> rois(q * Cb), gt((size_t)F * B * Cg), overlap(q);
    std::vector<int32_t> assign(q);
    std::vector<double> pose(q * 2);
    FILE *fp = fopen(in, "rb");
    if (!fp || !read_all(fp, rois) || !read_all(fp, gt) || !read_all(fp, overlap) || !read_all(fp, assign) || !read_all(fp, pose)) return 3;
    fclose(fp);
    std::vector<int32_t> index(k), gt_index(k), segments((size_t)F * 3), class_count((size_t)F * 3);
    std::vector<T> o_rois(k * Cb), roi_iou(k), gt_of(k * Cg), cls_label(k), gt_local(k * 7);
    std::vector<uint8_t> reg_valid(k);
    std::vector<double> o_pose(k * 2);
    std::vector<uint16_t> fg((size_t)M), bg((size_t)M);
    std::vector<uint32_t> words(((size_t)c.S + 3) / 4 * 4);
    const SgTargetOut<T> o{index.data(), o_rois.data(), roi_iou.data(), gt_index.data(), gt_of.data(), reg_valid.data(), cls_label.data(), segments.data(),
                           class_count.data(), o_pose.data(), gt_local.data()};
    for (int f = 0; f < F; ++f)
        sg_targets_frame<T>(c, seed, step, (uint32_t)f, M, rois.data() + (size_t)f * M * Cb, Cb, overlap.data() + (size_t)f * M, assign.data() + (size_t)f * M,
                            B, gt.data() + (size_t)f * B * Cg, Cg, pose.data() + (size_t)f * M * 2, fg.data(), bg.data(), words.data(), o);
    fp = fopen(out, "wb");
    if (!fp || !write_all(fp, index) || !write_all(fp, o_rois) || !write_all(fp, roi_iou) || !write_all(fp, gt_index) || !write_all(fp, gt_of) ||
        !write_all(fp, reg_valid) || !write_all(fp, cls_label) || !write_all(fp, segments) || !write_all(fp, class_count) || !write_all(fp, o_pose) ||
        !write_all(fp, gt_local))
        return 4;
    return fclose(fp) ? 4 : 0;
}

int main(int argc, char **argv)
{
    if (argc != 19) { fprintf(stderr, "usage: targets_walk dtype F M B Cb Cg S fg_per_image reg_fg cls_fg cls_bg cls_bg_lo hard_ratio cls_mode seed step in out\n"); return 2; }
    const int dtype = atoi(argv[1]), F = atoi(argv[2]), M = atoi(argv[3]), B = atoi(argv[4]), Cb = atoi(argv[5]), Cg = atoi(argv[6]);
    const SgTargetCfg c{atoi(argv[7]), atoi(argv[8]), strtod(argv[9], nullptr), strtod(argv[10], nullptr), strtod(argv[11], nullptr), strtod(argv[12], nullptr),
                        strtod(argv[13], nullptr), atoi(argv[14])};
    const uint64_t seed = strtoull(argv[15], nullptr, 10), step = strtoull(argv[16], nullptr, 10);
    if (F < 1 || M < 1 || M > SG_TARGETS_MAX || B < 1 || Cb < 7 || Cg < 7 || c.S < 1 || c.S > SG_TARGETS_SLOTS_MAX) return 2;
    return dtype == 0 ? run<float>(c, F, M, B, Cb, Cg, seed, step, argv[17], argv[18]) : run<double>(c, F, M, B, Cb, Cg, seed, step, argv[17], argv[18]);
}
