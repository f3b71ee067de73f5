// Host harness: the scene transforms of csrc/sg_scene.h (the draws, the candidate, sg_scene_sweep, the box and row records, what a row
// and a box become -- the functions k_scene_frame and k_scene_rows run on the device) compiled for the host, on a case from a file, for
// tests/test_scene_reference.py to compare byte for byte with the restatement (tests/scene_reference.py).  Every cos / sin is an input.
//   usage: scene_sweep dtype F N B Cb T seed step in out flip rot_on rot_lo rot_hi scale_on scale_lo scale_hi ltrans_on ax ay az lrot_on lo hi lscale_on lo hi
//   in:    offsets (F + 1) int64 | rows (N, 5) T | keep (N) bytes | box_of (N) int32 | gt (F, B, Cb) T | pose (F, B, 2) float64 |
//          world cos / sin (F, 2) float64 | tries cos / sin (F, B, T, 2) float64, raw, in this order
//   out:   rows (N, 5) T | keep (N) bytes | gt (F, B, Cb) T | world (F, 8) | state (F, B) int32 | tried (F, B) int32 | local (F, B, 8) |
//          pose (F, B, 2) | tries (F, B, T, 8), raw
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sg_scene.h"

template <typename T> static bool read_all(FILE *fp, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), fp) == v.size(); }
template <typename T> static bool write_all(FILE *fp, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), fp) == v.size(); }

template <typename T> static int run(const SgSceneCfg &k, int F, int64_t N, int B, int Cb, uint64_t seed, uint64_t step, const char *in, const char *out)
{
    const int Tn = k.tries;
    std::vector<int64_t> off((size_t)F + 1);
    std::vector<T> rows((size_t)N * 5), gt((size_t)F * B * Cb);
    std::vector<uint8_t> keep((size_t)N);
    std::vector<int32_t> box_of((size_t)N);
    std::vector<double> pose((size_t)F * B * 2), world_cs((size_t)F * 2), tries_cs((size_t)F * B * Tn * 2);
    FILE *fp = fopen(in, "rb");
    if (!fp || !read_all(fp, off) || !read_all(fp, rows) || !read_all(fp, keep) || !read_all(fp, box_of) || !read_all(fp, gt) || !read_all(fp, pose) ||
        !read_all(fp, world_cs) || !read_all(fp, tries_cs))
        return 3;
    fclose(fp);
    std::vector<T> out_rows(rows), out_gt(gt);
    std::vector<double> world((size_t)F * 8), local((size_t)F * B * 8), out_pose((size_t)F * B * 2, 0.0), tries((size_t)F * B * Tn * 8), rowrec((size_t)B * SG_SCENE_ROWREC);
    std::vector<int32_t> state((size_t)F * B), tried((size_t)F * B);
    std::vector<SgIouRec> cur((size_t)B);
    for (int f = 0; f < F; ++f) {
        double *w = world.data() + (size_t)f * 8, *tr = tries.data() + (size_t)f * B * Tn * 8;
        sg_scene_world_draw(k, seed, step, (uint32_t)f, w);
        if (k.rot_on) { w[2] = world_cs[(size_t)f * 2]; w[3] = world_cs[(size_t)f * 2 + 1]; }
        const T *g = gt.data() + (size_t)f * B * Cb;
        for (int b = 0; b < B; ++b) sg_iou_make<T>(g + (size_t)b * Cb, pose.data() + ((size_t)f * B + b) * 2, &cur[b]);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < Tn; ++t) {
                double *r = tr + ((size_t)b * Tn + t) * 8;
                sg_scene_identity(r);
                if (cur[b].ok == 0.0) continue;
                sg_scene_try_draw(k, seed, step, (uint32_t)f, b, t, r);
                if (k.lrot_on) { const double *cs = tries_cs.data() + (((size_t)f * B + b) * Tn + t) * 2; r[3] = cs[0]; r[4] = cs[1]; }
            }
        int32_t *st = state.data() + (size_t)f * B, *tk = tried.data() + (size_t)f * B;
        sg_scene_sweep(B, Tn, cur.data(), tr, st, tk);
        for (int b = 0; b < B; ++b) {
            const size_t q = (size_t)f * B + b;
            const T *row = g + (size_t)b * Cb;
            const bool present = cur[b].ok != 0.0, moved = st[b] == SG_SCENE_MOVED;
            double ident[8];
            sg_scene_identity(ident);
            const double *r = moved ? tr + ((size_t)b * Tn + tk[b]) * 8 : ident;
            sg_scene_box_records(st[b], r, present ? (double)row[0] : 0.0, present ? (double)row[1] : 0.0, present ? (double)row[2] : 0.0, local.data() + q * 8,
                                 rowrec.data() + (size_t)b * SG_SCENE_ROWREC);
            if (present) {
                double o[7];
                sg_scene_box((double)row[6], cur[b], moved, r[5], w, o, out_pose.data() + q * 2);
                for (int j = 0; j < 7; ++j) out_gt[q * Cb + j] = (T)o[j];
            }
        }
        for (int64_t i = off[f]; i < off[f + 1]; ++i) {
            if (!keep[i]) continue;
            const T tx = rows[i * 5], ty = rows[i * 5 + 1], tz = rows[i * 5 + 2];
            if (!sg_box_row_usable<T>(tx, ty, tz)) continue;
            double x = (double)tx, y = (double)ty, z = (double)tz;
            const double *rec = nullptr;
            if (Tn > 0) {
                const int32_t b = box_of[i];
                if (b >= 0 && b < B && rowrec[(size_t)b * SG_SCENE_ROWREC + 9] != 0.0) rec = rowrec.data() + (size_t)b * SG_SCENE_ROWREC;
            }
            sg_scene_row(&x, &y, &z, rec, w);
            out_rows[i * 5] = (T)x; out_rows[i * 5 + 1] = (T)y; out_rows[i * 5 + 2] = (T)z;
        }
    }
    for (auto &v : keep) v = v ? 1 : 0;
    fp = fopen(out, "wb");
    if (!fp || !write_all(fp, out_rows) || !write_all(fp, keep) || !write_all(fp, out_gt) || !write_all(fp, world) || !write_all(fp, state) || !write_all(fp, tried) ||
        !write_all(fp, local) || !write_all(fp, out_pose) || !write_all(fp, tries))
        return 4;
    return fclose(fp) ? 4 : 0;
}

int main(int argc, char **argv)
{
    if (argc != 28) { fprintf(stderr, "usage: scene_sweep dtype F N B Cb T seed step in out flip rot(3) scale(3) ltrans(4) lrot(3) lscale(3)\n"); return 2; }
    const int dtype = atoi(argv[1]), F = atoi(argv[2]), B = atoi(argv[4]), Cb = atoi(argv[5]), Tn = atoi(argv[6]);
    const int64_t N = atoll(argv[3]);
    const uint64_t seed = strtoull(argv[7], nullptr, 10), step = strtoull(argv[8], nullptr, 10);
    if (F < 1 || N < 0 || B < 1 || B > SG_BOX_MAX || Cb < 7 || Cb > 10 || Tn < 0 || Tn > SG_SCENE_TRIES_MAX) return 2;
    SgSceneCfg k{};
    char **a = argv + 11;
    k.flip = atoi(a[0]); k.tries = Tn;
    k.rot_on = atoi(a[1]); k.rot[0] = strtod(a[2], nullptr); k.rot[1] = strtod(a[3], nullptr);
    k.scale_on = atoi(a[4]); k.scale[0] = strtod(a[5], nullptr); k.scale[1] = strtod(a[6], nullptr);
    k.ltrans_on = atoi(a[7]); for (int j = 0; j < 3; ++j) k.ltrans[j] = strtod(a[8 + j], nullptr);
    k.lrot_on = atoi(a[11]); k.lrot[0] = strtod(a[12], nullptr); k.lrot[1] = strtod(a[13], nullptr);
    k.lscale_on = atoi(a[14]); k.lscale[0] = strtod(a[15], nullptr); k.lscale[1] = strtod(a[16], nullptr);
    return dtype == 0 ? run<float>(k, F, N, B, Cb, seed, step, argv[9], argv[10]) : run<double>(k, F, N, B, Cb, seed, step, argv[9], argv[10]);
}
