// Host harness: the object paste of csrc/sg_paste.h (the class of a gt, the slots, the draw, the records, the conflict words and
// sg_paste_frame, the sweep -- the functions k_paste_frame runs on the device) compiled for the host, on a case from a file, for
// tests/test_paste_reference.py to compare byte for byte with the restatement (tests/paste_reference.py).
//   usage: paste_sweep dtype F B Cb O seed step in out NC n_1 .. n_NC
//   in:    gt (F, B, Cb) T | pose (F, B, 2) float64 | free (F) int32 | bank offsets (O + 1) int64 | bank boxes (O, 8) T |
//          bank pose (O, 2) float64 | class offsets (18) int32, raw, in this order
//   out:   object (F, Q) | state (F, Q) | base (F, Q) | rows pasted (F), int32, raw
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sg_paste.h"

template <typename T> static bool read_all(FILE *fp, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), fp) == v.size(); }
template <typename T> static bool write_all(FILE *fp, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), fp) == v.size(); }

template <typename T> static int run(const SgPasteGroups &g, int F, int B, int Cb, int O, uint64_t seed, uint64_t step, const char *in, const char *out)
{
    const int Q = g.Q;
    std::vector<T> gt((size_t)F * B * Cb), bank_boxes((size_t)O * 8);
    std::vector<double> pose((size_t)F * B * 2), bank_pose((size_t)O * 2);
    std::vector<int32_t> free_total((size_t)F), class_off(SG_PASTE_CLASS_OFFSETS);
    std::vector<int64_t> bank_off((size_t)O + 1);
    FILE *fp = fopen(in, "rb");
    if (!fp || !read_all(fp, gt) || !read_all(fp, pose) || !read_all(fp, free_total) || !read_all(fp, bank_off) || !read_all(fp, bank_boxes) ||
        !read_all(fp, bank_pose) || !read_all(fp, class_off))
        return 3;
    fclose(fp);
    std::vector<int32_t> object((size_t)F * Q), state((size_t)F * Q), base((size_t)F * Q), pasted_rows((size_t)F);
    std::vector<SgIouRec> gt_rec((size_t)B), cand((size_t)Q);
    std::vector<uint64_t> earlier((size_t)Q);
    std::vector<int32_t> points((size_t)Q);
    for (int f = 0; f < F; ++f) {
        int32_t cnt[SG_PASTE_CLASSES_MAX] = {0};
        for (int b = 0; b < B; ++b) {
            const T *row = gt.data() + ((size_t)f * B + b) * Cb;
            if (sg_iou_make<T>(row, pose.data() + ((size_t)f * B + b) * 2, &gt_rec[b])) {
                const int32_t c = sg_paste_class<T>(row[7]);
                if (c > 0) ++cnt[c - 1];
            }
        }
        uint64_t active = 0, present = 0, gt_hit = 0;
        for (int q = 0; q < Q; ++q) {
            const int32_t o = sg_paste_draw(g, q, cnt, class_off.data(), seed, step, (uint32_t)f);
            object[(size_t)f * Q + q] = o;
            cand[q] = SgIouRec{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            points[q] = 0;
            if (o < 0) continue;
            if (o >= O) return 5;
            active |= (uint64_t)1 << q;
            if (sg_iou_make<T>(bank_boxes.data() + (size_t)o * 8, bank_pose.data() + (size_t)o * 2, &cand[q])) present |= (uint64_t)1 << q;
            points[q] = (int32_t)(bank_off[o + 1] - bank_off[o]);
        }
        sg_paste_words(Q, B, cand.data(), gt_rec.data(), &gt_hit, earlier.data());
        pasted_rows[f] = sg_paste_frame(Q, active, present, gt_hit, earlier.data(), points.data(), free_total[f], state.data() + (size_t)f * Q, base.data() + (size_t)f * Q);
    }
    fp = fopen(out, "wb");
    if (!fp || !write_all(fp, object) || !write_all(fp, state) || !write_all(fp, base) || !write_all(fp, pasted_rows)) return 4;
    return fclose(fp) ? 4 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 12) { fprintf(stderr, "usage: paste_sweep dtype F B Cb O seed step in out NC n_1 .. n_NC\n"); return 2; }
    const int dtype = atoi(argv[1]), F = atoi(argv[2]), B = atoi(argv[3]), Cb = atoi(argv[4]), O = atoi(argv[5]), NC = atoi(argv[10]);
    const uint64_t seed = strtoull(argv[6], nullptr, 10), step = strtoull(argv[7], nullptr, 10);
    if (F < 1 || B < 1 || Cb < 8 || Cb > 10 || O < 1 || NC < 1 || NC > SG_PASTE_CLASSES_MAX || argc != 11 + NC) return 2;
    SgPasteGroups g{};
    g.n_classes = NC;
    for (int c = 0; c < NC; ++c) { g.n[c] = atoi(argv[11 + c]); g.Q += g.n[c]; }
    if (g.Q < 1 || g.Q > SG_PASTE_SLOTS_MAX) return 2;
    return dtype == 0 ? run<float>(g, F, B, Cb, O, seed, step, argv[8], argv[9]) : run<double>(g, F, B, Cb, O, seed, step, argv[8], argv[9]);
}
