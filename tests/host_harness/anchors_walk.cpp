// Host harness: the anchor target assignment of csrc/sg_anchors.h (sg_anchors_frame -- presence, the BEV box, the overlap, the walk and the
// label rule, the functions the kernels of snowgpu_anchors.hip run on the device) compiled for the host, on a case from a file, for
// tests/test_anchors_reference.py to compare byte for byte with the restatement (tests/anchors_reference.py).
//   usage: anchors_walk dtype F A B Ca Cg NC matched_1 .. matched_NC unmatched_1 .. unmatched_NC in out
//   in:    anchors (A, Ca) T | anchor_class (A) int32 | gt (F, B, Cg) T, raw, in this order
//   out:   label | gt_index | count | gt_count | iou, raw
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sg_anchors.h"

template <typename T> static bool read_all(FILE *fp, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), fp) == v.size(); }
template <typename T> static bool write_all(FILE *fp, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), fp) == v.size(); }

template <typename T> static int run(const SgAnchorCfg &c, int F, int A, int B, int Ca, int Cg, const char *in, const char *out)
{
    std::vector<T> anchors((size_t)A * Ca), gt((size_t)F * B * Cg);
    std::vector<int32_t> cls((size_t)A);
    FILE *fp = fopen(in, "rb");
    if (!fp || !read_all(fp, anchors) || !read_all(fp, cls) || !read_all(fp, gt)) return 3;
    fclose(fp);
    std::vector<int32_t> label((size_t)F * A), gt_index((size_t)F * A), count((size_t)F * 3), gt_count((size_t)F * B);
    std::vector<T> iou((size_t)F * A);
    std::vector<SgAnchorRec> recs((size_t)B);
    std::vector<unsigned long long> top((size_t)B);
    const SgAnchorOut<T> o{label.data(), gt_index.data(), count.data(), gt_count.data(), iou.data()};
    for (int f = 0; f < F; ++f)
        sg_anchors_frame<T>(c, (int64_t)f, A, anchors.data(), Ca, cls.data(), B, gt.data() + (size_t)f * B * Cg, Cg, recs.data(), top.data(), o);
    fp = fopen(out, "wb");
    if (!fp || !write_all(fp, label) || !write_all(fp, gt_index) || !write_all(fp, count) || !write_all(fp, gt_count) || !write_all(fp, iou)) return 4;
    return fclose(fp) ? 4 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 8) { fprintf(stderr, "usage: anchors_walk dtype F A B Ca Cg NC matched .. unmatched .. in out\n"); return 2; }
    const int dtype = atoi(argv[1]), F = atoi(argv[2]), A = atoi(argv[3]), B = atoi(argv[4]), Ca = atoi(argv[5]), Cg = atoi(argv[6]), NC = atoi(argv[7]);
    if (F < 1 || A < 1 || B < 1 || B > SG_ANCHORS_GT_MAX || Ca < 7 || Cg < 8 || NC < 1 || NC > SG_ANCHORS_CLASSES_MAX || argc != 10 + 2 * NC) return 2;
    SgAnchorCfg c{};
    c.n_classes = NC;
    for (int k = 0; k < NC; ++k) {
        c.matched[k] = strtod(argv[8 + k], nullptr);
        c.unmatched[k] = strtod(argv[8 + NC + k], nullptr);
    }
    const char *in = argv[8 + 2 * NC], *out = argv[9 + 2 * NC];
    return dtype == 0 ? run<float>(c, F, A, B, Ca, Cg, in, out) : run<double>(c, F, A, B, Ca, Cg, in, out);
}
