// The grid, the window and the walk of the ball query (csrc/sg_ball.h) compiled for the host.
//   ball_cells cover
//       For every setting -- without a range and under one, radii 0.01 .. 1000 m, at three cell budgets, float32 and float64 rows --
//       more than 10^6 (centre, row) pairs with d < r2 as the kernel computes it, most of them within a few ulps of the sphere, centres
//       inside the grid's domain and up to 600 m outside it: the row's cell (sg_ball_cell) must lie in the centre's window
//       (sg_ball_window, sg_ball_in_window).  Prints "cover <settings> <pairs>"; returns 1 with the first pair that is not covered.
//   ball_cells walk <dtype 0 | 1> <range 0 | 1> <x0> <y0> <z0> <x1> <y1> <z1> <max_frame_rows> <R> <radius>*R <samples>*R
//                   <rows: n x 3 float64> <keep: n bytes> <centres: K x 3 float64> <out> <seed>
//       ONE frame through count / scan / scatter / query as the kernels do it: the usable rows filed by cell (the order inside a cell
//       scrambled by `seed`, as the arrival of atomics scrambles it), then per centre the grid rows of its window in batches of 64 lanes,
//       the ballot, the threshold, the sort and the merge.  out: int32 index[K][S] (frame-local rows), int32 count[K][R].
//       Prints "grid <nx> <ny>".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sg_ball.h"

template <typename T>
static long cover(const double *range6, double radius, int32_t budget, std::mt19937_64 &rng, long want)
{
    SgBallGrid g{};
    SgBallPairs<T> pr;
    const int one = 1;
    sg_ball_make_grid(range6, 1, &radius, budget, &g);
    sg_ball_make_pairs<T>(1, &radius, &one, &pr);
    if (g.nx < 1 || g.ny < 1 || (int64_t)g.nx * g.ny > budget || g.cells != g.nx * g.ny) return -1;
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double x0 = range6 ? range6[0] : -SG_BALL_SENSOR, x1 = range6 ? range6[3] : SG_BALL_SENSOR;
    const double y0 = range6 ? range6[1] : -SG_BALL_SENSOR, y1 = range6 ? range6[4] : SG_BALL_SENSOR;
    long pairs = 0;
    for (long tries = 0; pairs < want && tries < 40 * want; ++tries) {
        const bool beyond = tries % 4 == 0;                        // a quarter of the centres up to 600 m outside the domain
        const double pad = beyond ? 600.0 : 0.0;
        const T cx = (T)(x0 - pad + u(rng) * (x1 - x0 + 2.0 * pad)), cy = (T)(y0 - pad + u(rng) * (y1 - y0 + 2.0 * pad)), cz = (T)(u(rng) * 4.0 - 2.0);
        // a direction, and a length at the sphere (three quarters of the pairs: within 4e-7 relative of it) or anywhere inside
        double dx = u(rng) - 0.5, dy = u(rng) - 0.5, dz = (u(rng) - 0.5) * (tries % 3 == 0 ? 0.0 : 1.0);
        const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (!(len > 1e-3)) continue;
        const double reach = tries % 4 == 3 ? u(rng) * radius : radius * (1.0 + (u(rng) - 0.75) * 4e-7);
        const T px = (T)((double)cx + dx / len * reach), py = (T)((double)cy + dy / len * reach), pz = (T)((double)cz + dz / len * reach);
        if (!sg_ball_centre_usable<T>(cx, cy, cz) || !sg_ball_centre_usable<T>(px, py, pz)) continue;
        if (!(sg_fps_dist<T>(px, py, pz, cx, cy, cz) < pr.r2[0])) continue;
        SgBallWindow w;
        sg_ball_window(g, (double)cx, (double)cy, &w);
        const int32_t cell = sg_ball_cell(g, (double)px, (double)py);
        if (cell < 0 || cell >= g.cells || !sg_ball_in_window(g, w, cell)) {
            std::printf("NOT COVERED r %.17g budget %d centre %.17g %.17g row %.17g %.17g cell %d window %d %d %d %d\n", radius, budget, (double)cx, (double)cy,
                        (double)px, (double)py, cell, w.ix0, w.ix1, w.iy0, w.iy1);
            return -1;
        }
        ++pairs;
    }
    return pairs;
}

static int run_cover()
{
    const double second[6] = {0.0, -40.0, -3.0, 70.4, 40.0, 1.0};
    const double radii[7] = {0.01, 0.1, 0.4, 0.8, 4.8, 50.0, 1000.0};
    const int32_t budgets[3] = {SG_DROR_MIN_CELLS, 8192, SG_DROR_MAX_CELLS};
    std::mt19937_64 rng(3);
    long settings = 0, total = 0;
    for (int with_range = 0; with_range < 2; ++with_range)
        for (double r : radii)
            for (int32_t b : budgets) {
                const long a = cover<float>(with_range ? second : nullptr, r, b, rng, 1000100), c = cover<double>(with_range ? second : nullptr, r, b, rng, 100000);
                if (a < 1000000 || c < 100000) { std::printf("FAILED range %d r %g budget %d: %ld %ld pairs\n", with_range, r, b, a, c); return 1; }
                ++settings;
                total += a + c;
            }
    std::printf("cover %ld %ld\n", settings, total);
    return 0;
}

template <typename T>
static int walk(const double *range6, int64_t max_frame, int R, const double *radii, const int *samples, const std::vector<double> &p,
                const std::vector<uint8_t> &keep, const std::vector<double> &cen, uint64_t seed, FILE *fo)
{
    SgFpsRange r;
    for (int j = 0; j < 3; ++j) { r.lo[j] = range6 ? range6[j] : -INFINITY; r.hi[j] = range6 ? range6[3 + j] : INFINITY; }
    SgBallGrid g{};
    SgBallPairs<T> pr;
    sg_ball_make_grid(range6, R, radii, sg_ball_cell_budget(max_frame), &g);
    sg_ball_make_pairs<T>(R, radii, samples, &pr);
    const size_t n = keep.size(), K = cen.size() / 3;
    // count / scan / scatter
    std::vector<uint32_t> entry((size_t)g.cells + 1, 0), cell_of(n, SG_DROR_NO_CELL);
    for (size_t i = 0; i < n; ++i) {
        const T x = (T)p[3 * i], y = (T)p[3 * i + 1], z = (T)p[3 * i + 2];
        if (keep[i] != 0 && sg_fps_usable<T>(r, x, y, z)) {
            cell_of[i] = (uint32_t)sg_ball_cell(g, (double)x, (double)y);
            ++entry[1 + cell_of[i]];
        }
    }
    for (int32_t c = 0, sum = 0; c < g.cells; ++c) { const uint32_t v = entry[1 + c]; entry[1 + c] = (uint32_t)sum; sum += (int32_t)v; }
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = i;
    std::mt19937_64 rng(seed);
    if (seed) std::shuffle(order.begin(), order.end(), rng);
    std::vector<T> sx(n), sy(n), sz(n);
    std::vector<int32_t> ssrc(n, -1);
    for (size_t i : order) {
        if (cell_of[i] == SG_DROR_NO_CELL) continue;
        const uint32_t pos = entry[1 + cell_of[i]]++;              // (the entry becomes the cell's end)
        sx[pos] = (T)p[3 * i]; sy[pos] = (T)p[3 * i + 1]; sz[pos] = (T)p[3 * i + 2];
        ssrc[pos] = (int32_t)i;
    }
    // query
    std::vector<int32_t> index(K * (size_t)pr.total, -1), count(K * (size_t)R, 0);
    for (size_t k = 0; k < K; ++k) {
        const T cx = (T)cen[3 * k], cy = (T)cen[3 * k + 1], cz = (T)cen[3 * k + 2];
        int32_t kept[SG_BALL_MAX_RADII][64], cnt[SG_BALL_MAX_RADII] = {0, 0, 0, 0};
        for (auto &row : kept)
            for (int32_t &v : row) v = SG_BALL_EMPTY;
        if (sg_ball_centre_usable<T>(cx, cy, cz)) {
            SgBallWindow w;
            sg_ball_window(g, (double)cx, (double)cy, &w);
            for (int iy = w.iy0; iy <= w.iy1; ++iy) {
                const uint32_t b = entry[(size_t)(iy * g.nx + w.ix0)], end = entry[(size_t)(iy * g.nx + w.ix1 + 1)];
                for (uint32_t p0 = b; p0 < end; p0 += 64)
                    for (int i = 0; i < R; ++i) {
                        int32_t batch[64];
                        bool any = false;
                        for (uint32_t l = 0; l < 64; ++l) {
                            const uint32_t q = p0 + l;
                            const bool in = q < end && sg_fps_dist<T>(sx[q], sy[q], sz[q], cx, cy, cz) < pr.r2[i];
                            cnt[i] += in ? 1 : 0;
                            any = any || sg_ball_wanted(in, in ? ssrc[q] : SG_BALL_EMPTY, kept[i][pr.samples[i] - 1]);
                            batch[l] = in ? ssrc[q] : SG_BALL_EMPTY;
                        }
                        if (!any) continue;
                        sg_ball_sort_lanes(batch);
                        sg_ball_merge_lanes(kept[i], batch);
                    }
            }
        }
        for (int i = 0; i < R; ++i) {
            count[k * (size_t)R + (size_t)i] = cnt[i];
            for (int l = 0; l < pr.samples[i]; ++l)
                index[k * (size_t)pr.total + (size_t)pr.seg[i] + (size_t)l] = cnt[i] == 0 ? -1 : (l < cnt[i] ? kept[i][l] : kept[i][0]);
        }
    }
    fwrite(index.data(), sizeof(int32_t), index.size(), fo);
    fwrite(count.data(), sizeof(int32_t), count.size(), fo);
    std::printf("grid %d %d\n", g.nx, g.ny);
    return 0;
}

static bool read_all(const char *path, std::vector<uint8_t> *out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + got);
    fclose(f);
    return true;
}

static std::vector<double> as_doubles(const std::vector<uint8_t> &raw)
{
    std::vector<double> v(raw.size() / sizeof(double));
    if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(double));
    return v;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "cover")) return run_cover();
    if (argc < 12 || strcmp(argv[1], "walk")) return 2;
    const int dtype = atoi(argv[2]), with_range = atoi(argv[3]);
    double range6[6];
    for (int j = 0; j < 6; ++j) range6[j] = atof(argv[4 + j]);
    const int64_t max_frame = atoll(argv[10]);
    const int R = atoi(argv[11]);
    if (R < 1 || R > SG_BALL_MAX_RADII || argc != 12 + 2 * R + 5 || (dtype != 0 && dtype != 1)) return 2;
    double radii[SG_BALL_MAX_RADII];
    int samples[SG_BALL_MAX_RADII];
    for (int i = 0; i < R; ++i) { radii[i] = atof(argv[12 + i]); samples[i] = atoi(argv[12 + R + i]); if (samples[i] < 1 || samples[i] > 64) return 2; }
    char **rest = argv + 12 + 2 * R;
    std::vector<uint8_t> raw_rows, keep, raw_cen;
    if (!read_all(rest[0], &raw_rows) || !read_all(rest[1], &keep) || !read_all(rest[2], &raw_cen)) return 4;
    const std::vector<double> p = as_doubles(raw_rows), cen = as_doubles(raw_cen);
    if (p.size() != keep.size() * 3 || cen.size() % 3) return 4;
    FILE *fo = fopen(rest[3], "wb");
    if (!fo) return 5;
    const uint64_t seed = (uint64_t)atoll(rest[4]);
    const int rc = dtype == 0 ? walk<float>(with_range ? range6 : nullptr, max_frame, R, radii, samples, p, keep, cen, seed, fo)
                              : walk<double>(with_range ? range6 : nullptr, max_frame, R, radii, samples, p, keep, cen, seed, fo);
    fclose(fo);
    return rc;
}
