// Host harness: the centre heatmap targets of csrc/sg_centers.h (sg_centers_frame -- presence, the centre, the radius, the slots, the value of a
// pixel and the tiles' lists, the functions the kernels of snowgpu_centers.hip run on the device) compiled for the host, on a case from a
// file, for tests/test_centers_reference.py to compare byte for byte with the restatement (tests/centers_reference.py).
//   usage: centers_walk dtype F B Cg x0 y0 vx vy stride W H NC NH M overlap min_radius outside head_1 .. head_NC in out
//   in:    gt (F, B, Cg) T, raw
//   out:   heatmap | gt_index | ind | mask | offset | radius | count | state, raw
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sg_centers.h"

template <typename T> static bool read_all(FILE *fp, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), fp) == v.size(); }
template <typename T> static bool write_all(FILE *fp, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), fp) == v.size(); }

template <typename T> static int run(const SgCenterCfg &c, int F, int B, int Cg, const char *in, const char *out)
{
    std::vector<T> gt((size_t)F * B * Cg);
    FILE *fp = fopen(in, "rb");
    if (!fp || !read_all(fp, gt)) return 3;
    fclose(fp);
    const size_t slots = (size_t)F * c.n_heads * c.max_objs;
    std::vector<float> heat((size_t)F * c.n_classes * c.H * c.W);
    std::vector<int32_t> gt_index(slots), ind(slots), radius(slots), count((size_t)F * c.n_heads);
    std::vector<uint8_t> mask(slots), state((size_t)F * B);
    std::vector<T> offset(slots * 2);
    std::vector<SgCenterRec> recs((size_t)B);
    const SgCenterOut<T> o{heat.data(), gt_index.data(), ind.data(), mask.data(), offset.data(), radius.data(), count.data(), state.data()};
    for (int f = 0; f < F; ++f) sg_centers_frame<T>(c, (int64_t)f, B, gt.data() + (size_t)f * B * Cg, Cg, recs.data(), o);
    fp = fopen(out, "wb");
    if (!fp || !write_all(fp, heat) || !write_all(fp, gt_index) || !write_all(fp, ind) || !write_all(fp, mask) || !write_all(fp, offset) || !write_all(fp, radius) ||
        !write_all(fp, count) || !write_all(fp, state))
        return 4;
    return fclose(fp) ? 4 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 18) { fprintf(stderr, "usage: centers_walk dtype F B Cg x0 y0 vx vy stride W H NC NH M overlap min_radius outside heads .. in out\n"); return 2; }
    const int dtype = atoi(argv[1]), F = atoi(argv[2]), B = atoi(argv[3]), Cg = atoi(argv[4]);
    SgCenterCfg c{};
    c.x0 = strtod(argv[5], nullptr); c.y0 = strtod(argv[6], nullptr); c.vx = strtod(argv[7], nullptr); c.vy = strtod(argv[8], nullptr);
    c.stride = (double)atoi(argv[9]);
    c.W = atoi(argv[10]); c.H = atoi(argv[11]); c.n_classes = atoi(argv[12]); c.n_heads = atoi(argv[13]); c.max_objs = atoi(argv[14]);
    c.overlap = strtod(argv[15], nullptr);
    c.min_radius = atoi(argv[16]); c.drop = atoi(argv[17]);
    if (F < 1 || B < 1 || B > SG_CENTERS_GT_MAX || Cg < 8 || c.W < 1 || c.H < 1 || c.n_classes < 1 || c.n_classes > SG_CENTERS_CLASSES_MAX || c.n_heads < 1 ||
        c.n_heads > SG_CENTERS_HEADS_MAX || c.max_objs < 1 || c.max_objs > SG_CENTERS_OBJS_MAX || argc != 20 + c.n_classes)
        return 2;
    for (int k = 0; k < c.n_classes; ++k) {
        c.class_head[k] = atoi(argv[18 + k]);
        if (c.class_head[k] < 0 || c.class_head[k] >= c.n_heads) return 2;
    }
    const char *in = argv[18 + c.n_classes], *out = argv[19 + c.n_classes];
    return dtype == 0 ? run<float>(c, F, B, Cg, in, out) : run<double>(c, F, B, Cg, in, out);
}
