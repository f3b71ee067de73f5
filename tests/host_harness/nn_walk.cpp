// nn_walk.cpp -- csrc/sg_nn.h on the host (hipcc --cuda-host-only -x hip, as tests/test_ball_reference.py compiles ball_cells.cpp): the
// grid, the ring walk, its stopping bound, the k-best insertion and the weights are the functions the kernels of snowgpu_nn.hip run.
//   nn_walk walk <dtype> <has_range> <x0 y0 z0 x1 y1 z1> <K> <k> <rows.f64> <keep.u8> <centres.f64> <out> <seed>
//       one frame: files the usable centres as k_nn_file does -- but with the order inside every cell shuffled by <seed> (0: ascending)
//       --, walks every usable row and writes index (int32), dist2 and weight (the rows' dtype) of all rows; prints "walk nx ny".
//   nn_walk bound <seed> <millions>
//       the bound property: over random grids, rows, visited blocks and centres in cells outside the block, B^2 = sg_nn_bound(...) never
//       exceeds the distance in T; rows and centres sit on cell boundaries, a few ulps beside them, anywhere, and beyond the domain.
//       Prints "bound <triples checked>", or the first violation and exits 1.
//   nn_walk insert
//       sg_nn_insert and sg_nn_kth against a sort for KK = 1 .. 8, both dtypes, with many equal distances.
//       Prints "insert <sequences checked>".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sg_nn.h"

template <typename T> struct Filed {
    std::vector<uint32_t> entry;
    std::vector<SgNnRec<T>> rec;
    SgNnBox box;
};

// the cell lists of one frame's centres (K x 3, already of type T), the order inside a cell shuffled
template <typename T> static Filed<T> file_centres(const SgNnGrid &g, const std::vector<T> &c, int64_t K, uint32_t seed)
{
    Filed<T> f;
    std::vector<std::vector<int32_t>> in_cell(g.cells);
    f.box = SgNnBox{0x7fffffff, -1, 0x7fffffff, -1};
    for (int64_t k = 0; k < K; ++k) {
        const T x = c[k * 3], y = c[k * 3 + 1], z = c[k * 3 + 2];
        if (!sg_ball_centre_usable<T>(x, y, z)) continue;
        const int32_t ix = sg_nn_ix(g, (double)x), iy = sg_nn_iy(g, (double)y);
        in_cell[iy * g.nx + ix].push_back((int32_t)k);
        f.box.ix0 = std::min(f.box.ix0, ix); f.box.ix1 = std::max(f.box.ix1, ix);
        f.box.iy0 = std::min(f.box.iy0, iy); f.box.iy1 = std::max(f.box.iy1, iy);
    }
    std::mt19937 gen(seed);
    f.entry.assign(g.cells + 1, 0u);
    for (int32_t cell = 0; cell < g.cells; ++cell) {
        if (seed) std::shuffle(in_cell[cell].begin(), in_cell[cell].end(), gen);
        f.entry[cell] = (uint32_t)f.rec.size();
        for (int32_t k : in_cell[cell]) {
            SgNnRec<T> r;
            r.x = c[(int64_t)k * 3]; r.y = c[(int64_t)k * 3 + 1]; r.z = c[(int64_t)k * 3 + 2]; r.c = k;
            f.rec.push_back(r);
        }
    }
    f.entry[g.cells] = (uint32_t)f.rec.size();
    return f;
}

static std::vector<double> read_f64(const char *path)
{
    std::vector<double> v;
    FILE *fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fseek(fp, 0, SEEK_END);
    const long bytes = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    v.resize((size_t)bytes / 8);
    if (bytes && fread(v.data(), 8, v.size(), fp) != v.size()) exit(2);
    fclose(fp);
    return v;
}

template <typename T, int KK>
static void walk_rows(const SgNnGrid &g, const Filed<T> &f, const SgFpsRange &range, const std::vector<T> &rows, const std::vector<uint8_t> &keep,
                      std::vector<int32_t> &index, std::vector<T> &dist2, std::vector<T> &weight)
{
    const size_t n = rows.size() / 3;
    const int k = KK;
    for (size_t i = 0; i < n; ++i) {
        SgNnKey<T> best[KK];
        sg_nn_clear<T, KK>(best);
        const T x = rows[i * 3], y = rows[i * 3 + 1], z = rows[i * 3 + 2];
        if (keep[i] && sg_fps_usable<T>(range, x, y, z)) sg_nn_walk<T, KK>(g, f.box, f.entry.data(), f.rec.data(), x, y, z, best);
        T w[KK];
        sg_nn_weights<T, KK>(best, w);
        for (int j = 0; j < k; ++j) {
            index[i * k + j] = sg_nn_key_c(best[j]);
            dist2[i * k + j] = sg_nn_key_d(best[j]);
            weight[i * k + j] = w[j];
        }
    }
}

template <typename T> static int walk_mode(char **a)
{
    const bool has_range = atoi(a[0]) != 0;
    double r6[6];
    for (int j = 0; j < 6; ++j) r6[j] = atof(a[1 + j]);
    const int64_t K = atoll(a[7]);
    const int k = atoi(a[8]);
    const std::vector<double> rows64 = read_f64(a[9]), cen64 = read_f64(a[11]);
    std::vector<uint8_t> keep(rows64.size() / 3);
    {
        FILE *fp = fopen(a[10], "rb");
        if (!fp || (keep.size() && fread(keep.data(), 1, keep.size(), fp) != keep.size())) { fprintf(stderr, "cannot read %s\n", a[10]); return 2; }
        fclose(fp);
    }
    const uint32_t seed = (uint32_t)atoll(a[13]);
    if ((int64_t)cen64.size() != K * 3 || k < 1 || k > SG_NN_MAX_K) { fprintf(stderr, "bad sizes\n"); return 2; }
    std::vector<T> rows(rows64.begin(), rows64.end()), cen(cen64.begin(), cen64.end());      // (exact: the files hold values of T)
    SgFpsRange range;
    for (int j = 0; j < 3; ++j) { range.lo[j] = has_range ? r6[j] : -INFINITY; range.hi[j] = has_range ? r6[3 + j] : INFINITY; }
    SgNnGrid g{};
    sg_nn_make_grid(has_range ? r6 : nullptr, K, &g);
    const Filed<T> f = file_centres<T>(g, cen, K, seed);
    const size_t n = rows.size() / 3;
    std::vector<int32_t> index(n * k);
    std::vector<T> dist2(n * k), weight(n * k);
    switch (k) {                                                                            // (one instance per k, as the launcher's)
        case 1: walk_rows<T, 1>(g, f, range, rows, keep, index, dist2, weight); break;
        case 2: walk_rows<T, 2>(g, f, range, rows, keep, index, dist2, weight); break;
        case 3: walk_rows<T, 3>(g, f, range, rows, keep, index, dist2, weight); break;
        case 4: walk_rows<T, 4>(g, f, range, rows, keep, index, dist2, weight); break;
        case 5: walk_rows<T, 5>(g, f, range, rows, keep, index, dist2, weight); break;
        case 6: walk_rows<T, 6>(g, f, range, rows, keep, index, dist2, weight); break;
        case 7: walk_rows<T, 7>(g, f, range, rows, keep, index, dist2, weight); break;
        default: walk_rows<T, 8>(g, f, range, rows, keep, index, dist2, weight); break;
    }
    FILE *fp = fopen(a[12], "wb");
    if (!fp) return 2;
    fwrite(index.data(), 4, index.size(), fp);
    fwrite(dist2.data(), sizeof(T), dist2.size(), fp);
    fwrite(weight.data(), sizeof(T), weight.size(), fp);
    fclose(fp);
    printf("walk %d %d\n", g.nx, g.ny);
    return 0;
}

// ---- the bound --------------------------------------------------------------------------------------------------------------------------
// a coordinate in cell column j of an axis that begins at `org`: on the boundary, a few ulps of T beside it, or anywhere in the cell; in a
// border column sometimes far beyond the domain
template <typename T> static T place(std::mt19937_64 &gen, double org, double edge, int32_t j, int32_t n)
{
    const unsigned kind = (unsigned)(gen() % 8);
    const double u = (double)(gen() >> 11) * (1.0 / 9007199254740992.0);
    if (j == 0 && kind == 7) return (T)(org - u * 700.0);
    if (j == n - 1 && kind == 7) return (T)(org + n * edge + u * 700.0);
    T v = (T)(org + (j + (kind < 3 ? 0.0 : kind < 5 ? 1.0 : u)) * edge);
    const int steps = (int)(gen() % 5) - 2;
    if (kind < 5)
        for (int s = 0; s < (steps < 0 ? -steps : steps); ++s) v = std::nextafter(v, steps < 0 ? (T)-INFINITY : (T)INFINITY);
    return v;
}

template <typename T> static long long bound_mode(uint64_t seed, long long want)
{
    std::mt19937_64 gen(seed * 2 + sizeof(T));
    const double ranges[4][6] = {{0.0, -40.0, -3.0, 70.4, 40.0, 1.0}, {0.0, -8.0, -2.0, 16.0, 8.0, 2.0}, {-9e5, -9e5, -5.0, 9e5, 9e5, 5.0}, {3.3, 0.7, -1.0, 3.4, 90.0, 1.0}};
    const int64_t Ks[6] = {1, 7, 32, 300, 2048, 100000};
    long long checked = 0;
    while (checked < want) {
        SgNnGrid g{};
        const unsigned rsel = (unsigned)(gen() % 5);
        sg_nn_make_grid(rsel < 4 ? ranges[rsel] : nullptr, Ks[gen() % 6], &g);
        for (int rep = 0; rep < 2000; ++rep) {
            SgNnBox box;
            box.ix0 = (int32_t)(gen() % g.nx); box.ix1 = box.ix0 + (int32_t)(gen() % (g.nx - box.ix0));
            box.iy0 = (int32_t)(gen() % g.ny); box.iy1 = box.iy0 + (int32_t)(gen() % (g.ny - box.iy0));
            const T x = place<T>(gen, g.x0, g.edge, (int32_t)(gen() % g.nx), g.nx), y = place<T>(gen, g.y0, g.edge, (int32_t)(gen() % g.ny), g.ny);
            const int32_t ix = sg_nn_ix(g, (double)x), iy = sg_nn_iy(g, (double)y), s = (int32_t)(gen() % 4);
            const int32_t jx0 = ix - s, jx1 = ix + s, jy0 = iy - s, jy1 = iy + s;
            const double bb = sg_nn_bound(g, box, (double)x, (double)y, jx0, jx1, jy0, jy1);
            if (bb == (double)INFINITY) {
                if (jx0 > box.ix0 || jx1 < box.ix1 || jy0 > box.iy0 || jy1 < box.iy1) { printf("an open side with an infinite bound\n"); return -1; }
                continue;
            }
            for (int t = 0; t < 12; ++t) {
                const int32_t cjx = box.ix0 + (int32_t)(gen() % (box.ix1 - box.ix0 + 1)), cjy = box.iy0 + (int32_t)(gen() % (box.iy1 - box.iy0 + 1));
                const T cx = place<T>(gen, g.x0, g.edge, cjx, g.nx), cy = place<T>(gen, g.y0, g.edge, cjy, g.ny);
                const int32_t kx = sg_nn_ix(g, (double)cx), ky = sg_nn_iy(g, (double)cy);      // (a centre on a boundary may land next door)
                if (kx < box.ix0 || kx > box.ix1 || ky < box.iy0 || ky > box.iy1) continue;    // not a centre of this frame
                if (kx >= jx0 && kx <= jx1 && ky >= jy0 && ky <= jy1) continue;                // visited
                const T d = sg_fps_dist<T>(x, y, (T)0, cx, cy, (T)0);                           // (equal z: the worst case)
                if (!((double)d >= bb)) {
                    printf("violation: row (%.17g, %.17g) block [%d, %d] x [%d, %d] centre (%.17g, %.17g) d %.17g < B^2 %.17g, edge %.17g\n", (double)x, (double)y,
                           jx0, jx1, jy0, jy1, (double)cx, (double)cy, (double)d, bb, g.edge);
                    return -1;
                }
                ++checked;
            }
        }
    }
    return checked;
}

// ---- the insertion ------------------------------------------------------------------------------------------------------------------------
template <typename T, int KK> static long long insert_sequences(std::mt19937 &gen)
{
    long long done = 0;
    for (int rep = 0; rep < 400; ++rep) {
        const int n = (int)(gen() % 40);
        std::vector<std::pair<T, int32_t>> all;
        std::vector<int32_t> number(n);
        for (int i = 0; i < n; ++i) number[i] = i * 3 + (rep & 1 ? 2000000000 - 3 * n : 0);
        std::shuffle(number.begin(), number.end(), gen);
        SgNnKey<T> best[KK];
        sg_nn_clear<T, KK>(best);
        for (int i = 0; i < n; ++i) {
            const T d = (T)((gen() % 5) * 0.25) + (gen() % 7 == 0 ? (T)1e-30 : (T)0);
            all.push_back({d, number[i]});
            sg_nn_insert<T, KK>(best, sg_nn_key(d, number[i]));
        }
        std::sort(all.begin(), all.end());
        for (int j = 0; j < KK; ++j) {
            const bool filled = j < n;
            const T d = sg_nn_key_d(best[j]);
            const int32_t c = sg_nn_key_c(best[j]);
            if (filled ? !(d == all[j].first && c == all[j].second) : !(std::isinf(d) && d > 0 && c == -1)) {
                printf("insert: KK %d slot %d of %d keys: (%g, %d)\n", KK, j, n, (double)d, c);
                return -1;
            }
        }
        const double kth = sg_nn_kth<T, KK>(best), want = KK - 1 < n ? (double)all[KK - 1].first : (double)INFINITY;
        if (kth != want) { printf("kth: KK %d of %d keys: %g, not %g\n", KK, n, kth, want); return -1; }
        ++done;
    }
    return done;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "walk" && argc == 17) return atoi(argv[2]) == 0 ? walk_mode<float>(argv + 3) : walk_mode<double>(argv + 3);
    if (mode == "bound" && argc == 4) {
        const long long want = (long long)(atof(argv[3]) * 1e6);
        const long long a = bound_mode<float>((uint64_t)atoll(argv[2]), want);
        if (a < 0) return 1;
        const long long b = bound_mode<double>((uint64_t)atoll(argv[2]), want);
        if (b < 0) return 1;
        printf("bound %lld\n", a + b);
        return 0;
    }
    if (mode == "insert") {
        std::mt19937 gen(7);
        long long total = 0;
        const long long parts[16] = {insert_sequences<float, 1>(gen), insert_sequences<float, 2>(gen), insert_sequences<float, 3>(gen), insert_sequences<float, 4>(gen),
                                     insert_sequences<float, 5>(gen), insert_sequences<float, 6>(gen), insert_sequences<float, 7>(gen), insert_sequences<float, 8>(gen),
                                     insert_sequences<double, 1>(gen), insert_sequences<double, 2>(gen), insert_sequences<double, 3>(gen), insert_sequences<double, 4>(gen),
                                     insert_sequences<double, 5>(gen), insert_sequences<double, 6>(gen), insert_sequences<double, 7>(gen), insert_sequences<double, 8>(gen)};
        for (long long p : parts) {
            if (p < 0) return 1;
            total += p;
        }
        printf("insert %lld\n", total);
        return 0;
    }
    fprintf(stderr, "usage: nn_walk walk ... | bound <seed> <millions> | insert\n");
    return 2;
}
