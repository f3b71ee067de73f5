// box_cells.cpp -- csrc/sg_box.h on the host (hipcc --cuda-host-only -x hip, as nn_walk.cpp is compiled): the footprint of a box against
// its members, and whole frames through the filing and the walk.  tests/test_box_reference.py runs it, once more under the address and
// undefined-behaviour sanitizers.
//   box_cells cover <seed> <pairs>
//       boxes of every kind -- rotated cars, tiny, huge, beyond the grid, at 9e5, centred on cell corners --, the pose computed from the
//       heading or given and perturbed up to the 1e-6 tolerance; rows drawn from box-local coordinates, faces and corners included,
//       rounded to float32 or float64; every row that the membership test confirms must lie in a cell that the footprint marks.  Runs
//       until <pairs> confirmed (row, box) pairs are held; prints "cover <pairs> <boxes>".
//   box_cells walk <dtype> <B> <given> <rows.f64 n x 3> <keep.u8> <boxes.f64 B x 7> <pose.f64 B x 2> <out>
//       one frame: the boxes filed into the bit table, every row through its cell's words, ascending.  out: box_of (int32 n), count
//       (int32 B), local (T n x 3), pose (f64 B x 2).  Prints "walk <rows in a box>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sg_box.h"

static std::vector<unsigned char> slurp(const char *path)
{
    std::vector<unsigned char> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
    unsigned char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
    std::fclose(f);
    return v;
}

// ---- cover ----------------------------------------------------------------------------------------------------------------------------------
template <typename T> static long cover_box(std::mt19937_64 &rng, int kind, long *failures)
{
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    auto pos = [&](double a, double b) { return a + (b - a) * (0.5 + 0.5 * u(rng)); };
    double b[7];
    const double edge = 2.0 * SG_BALL_SENSOR / SG_BOX_SIDE;
    switch (kind) {
    case 0: b[0] = 80 * u(rng); b[1] = 80 * u(rng); b[3] = pos(3.5, 5); b[4] = pos(1.5, 2.2); break;                     // a car
    case 1: b[0] = 100 * u(rng); b[1] = 100 * u(rng); b[3] = pos(1e-4, 1e-2); b[4] = pos(1e-4, 1e-2); break;            // tiny
    case 2: b[0] = 1e5 * u(rng); b[1] = 1e5 * u(rng); b[3] = pos(1e3, 1e6); b[4] = pos(1e3, 1e6); break;                // huge
    case 3: b[0] = 119 + 40 * u(rng); b[1] = -(119 + 40 * u(rng)); b[3] = pos(1, 30); b[4] = pos(1, 30); break;         // across and beyond the border
    case 4: b[0] = 9e5 + 1e4 * u(rng); b[1] = -9e5 + 1e4 * u(rng); b[3] = pos(2, 50); b[4] = pos(2, 50); break;          // at 9e5
    case 5: b[0] = edge * (int)(30 * u(rng)); b[1] = edge * (int)(30 * u(rng)); b[3] = 2 * edge * (1 + (int)pos(0, 3)) - 2e-5;
            b[4] = pos(0.05, 8); break;                                                                                  // on a cell corner, faces on cell edges
    default: b[0] = 60 * u(rng); b[1] = 60 * u(rng); b[3] = pos(0.02, 0.1); b[4] = pos(4, 40); break;                     // thin and long
    }
    b[2] = 2 * u(rng); b[5] = pos(0.5, 4);
    const int hk = (int)pos(0, 6);
    b[6] = hk == 0 ? 0.0 : hk == 1 ? 1.5707963267948966 : hk == 2 ? 3.141592653589793 : hk == 3 ? 0.7853981633974483 : hk == 4 ? 1e3 * u(rng) : 3.2 * u(rng);
    if (kind == 5) b[6] = hk < 3 ? b[6] : 0.0;
    T bt[7];
    for (int j = 0; j < 7; ++j) bt[j] = (T)b[j];
    double pose[2];
    const bool given = u(rng) < 0.0;
    if (given) {                                           // the caller's pose: another rounding of the angle, stretched within the tolerance
        const double k = std::sqrt(1.0 + 0.999e-6 * u(rng)), a = (double)bt[6] + 1e-9 * u(rng);
        pose[0] = std::cos(a) * k; pose[1] = std::sin(a) * k;
    }
    SgBoxRec r;
    if (!sg_box_make<T>(bt, given ? pose : nullptr, &r)) return 0;
    int32_t ix0, ix1, iy0, iy1;
    sg_box_footprint(r, &ix0, &ix1, &iy0, &iy1);
    const double n2 = r.c * r.c + r.s * r.s;
    long held = 0;
    for (int j = 0; j < 64; ++j) {
        // local coordinates: the interior, the faces from inside (down to the last ulp of the half extent) and the corners
        double l[2];
        for (int a = 0; a < 2; ++a) {
            const double h = a == 0 ? r.hx : r.hy, pick = u(rng);
            const double sign = u(rng) < 0.0 ? -1.0 : 1.0;
            l[a] = pick < -0.2 ? h * u(rng) : pick < 0.3 ? sign * std::nextafter(h, 0.0) : pick < 0.6 ? sign * h * (1.0 - 1e-15 * pos(0, 40)) : sign * (h - 1e-9 * pos(0, 20));
        }
        const double wx = r.cx + (l[0] * r.c - l[1] * r.s) / n2, wy = r.cy + (l[0] * r.s + l[1] * r.c) / n2, wz = r.cz + r.hz * u(rng);
        const T x = (T)wx, y = (T)wy, z = (T)wz;
        if (!sg_box_row_usable<T>(x, y, z)) continue;
        double lx, ly, sz;
        if (!sg_box_inside(r, (double)x, (double)y, (double)z, &lx, &ly, &sz)) continue;      // (rounded out of the box: no member)
        ++held;
        const int32_t ix = sg_box_index((double)x), iy = sg_box_index((double)y);
        if (ix < ix0 || ix > ix1 || iy < iy0 || iy > iy1) {
            if (++*failures <= 5)
                std::fprintf(stderr, "lost member: kind %d box %.17g %.17g %.17g %.17g h %.17g pose %.17g %.17g row %.17g %.17g cell %d %d span %d %d %d %d\n", kind, r.cx,
                             r.cy, r.hx, r.hy, (double)bt[6], r.c, r.s, (double)x, (double)y, ix, iy, ix0, ix1, iy0, iy1);
        }
    }
    return held;
}

static int cover(uint64_t seed, long want)
{
    std::mt19937_64 rng(seed);
    long held = 0, boxes = 0, failures = 0;
    while (held < want) {
        for (int kind = 0; kind < 7; ++kind) {
            held += cover_box<float>(rng, kind, &failures);
            held += cover_box<double>(rng, kind, &failures);
            boxes += 2;
        }
    }
    std::printf("cover %ld %ld\n", held, boxes);
    return failures ? 1 : 0;
}

// ---- walk -----------------------------------------------------------------------------------------------------------------------------------
template <typename T> static int walk(int B, bool given, const char *frows, const char *fkeep, const char *fboxes, const char *fpose, const char *fout)
{
    const auto rb = slurp(frows), kb = slurp(fkeep), bb = slurp(fboxes), pb = slurp(fpose);
    const size_t n = kb.size();
    if (rb.size() != n * 24 || bb.size() != (size_t)B * 56 || pb.size() != (size_t)B * 16) { std::fprintf(stderr, "bad sizes\n"); return 2; }
    const double *rows = (const double *)rb.data(), *boxes = (const double *)bb.data(), *pose = (const double *)pb.data();
    const int32_t W = sg_box_words(B);
    std::vector<unsigned long long> tab((size_t)(SG_BOX_CELLS + 1) * W, 0ull);
    std::vector<SgBoxRec> rec(B);
    std::vector<double> used(2 * (size_t)B);
    std::vector<int32_t> count(B, 0), box_of(n, -1);
    std::vector<T> local(3 * n, (T)0);
    for (int b = 0; b < B; ++b) {
        T bt[7];
        for (int j = 0; j < 7; ++j) bt[j] = (T)boxes[b * 7 + j];
        const bool present = sg_box_make<T>(bt, given ? pose + 2 * b : nullptr, &rec[b]);
        used[2 * b] = rec[b].c; used[2 * b + 1] = rec[b].s;
        if (!present) continue;
        tab[(size_t)SG_BOX_CELLS * W + (b >> 6)] |= 1ull << (b & 63);
        int32_t ix0, ix1, iy0, iy1;
        sg_box_footprint(rec[b], &ix0, &ix1, &iy0, &iy1);
        for (int32_t iy = iy0; iy <= iy1; ++iy)
            for (int32_t ix = ix0; ix <= ix1; ++ix) tab[(size_t)(iy * SG_BOX_SIDE + ix) * W + (b >> 6)] |= 1ull << (b & 63);
    }
    long inside = 0;
    for (size_t i = 0; i < n; ++i) {
        const T x = (T)rows[3 * i], y = (T)rows[3 * i + 1], z = (T)rows[3 * i + 2];
        if (!kb[i] || !sg_box_row_usable<T>(x, y, z)) continue;
        const unsigned long long *words = &tab[(size_t)sg_box_cell((double)x, (double)y) * W];
        for (int32_t w = 0; w < W; ++w)
            for (unsigned long long m = words[w]; m; m &= m - 1ull) {
                const int32_t b = w * 64 + __builtin_ctzll(m);
                double lx, ly, sz;
                if (!sg_box_inside(rec[b], (double)x, (double)y, (double)z, &lx, &ly, &sz)) continue;
                ++count[b];
                if (box_of[i] < 0) { box_of[i] = b; local[3 * i] = (T)lx; local[3 * i + 1] = (T)ly; local[3 * i + 2] = (T)sz; ++inside; }
            }
    }
    FILE *f = std::fopen(fout, "wb");
    if (!f) return 2;
    std::fwrite(box_of.data(), 4, n, f);
    std::fwrite(count.data(), 4, B, f);
    std::fwrite(local.data(), sizeof(T), 3 * n, f);
    std::fwrite(used.data(), 8, 2 * (size_t)B, f);
    std::fclose(f);
    std::printf("walk %ld\n", inside);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "cover" && argc == 4) return cover(std::strtoull(argv[2], nullptr, 10), std::atol(argv[3]));
    if (mode == "walk" && argc == 10) {
        const int dtype = std::atoi(argv[2]), B = std::atoi(argv[3]);
        const bool given = std::atoi(argv[4]) != 0;
        if (B < 1 || B > SG_BOX_MAX) return 2;
        return dtype == 0 ? walk<float>(B, given, argv[5], argv[6], argv[7], argv[8], argv[9]) : walk<double>(B, given, argv[5], argv[6], argv[7], argv[8], argv[9]);
    }
    std::fprintf(stderr, "usage: box_cells cover <seed> <pairs> | walk <dtype> <B> <given> <rows> <keep> <boxes> <pose> <out>\n");
    return 2;
}
