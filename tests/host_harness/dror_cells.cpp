// The binning of the outlier filter (csrc/sg_dror.h) compiled for the host.
//   dror_cells pairs <alpha> <beta> <k_min> <sr_min> <budget> <float32: 0 | 1> <pairs per source> <seed>
//       draws pairs of points, keeps those that are neighbours by the exact rule (sg_dror_s2 and the distance test of the definition) and
//       checks that the neighbour's cell (sg_dror_cell) lies inside the query's window (sg_dror_window).  One line per source:
//       "<source> <neighbour pairs checked> <pairs whose cell lies outside the window>", then "grid ..." with the grid's numbers.
//   dror_cells cloud <alpha> <beta> <k_min> <sr_min> <budget> <in: n x 3 float64> <out: n int32>
//       one frame through the kernels' steps on the host -- file every row, walk every query's window with the exact test, stop at
//       k_min -- and writes min(count, k_min) per row (-1 for an unusable row).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sg_dror.h"

struct P { double x, y, z; };

static bool g_f32 = false;
static double rnd(double v) { return g_f32 ? (double)(float)v : v; }
static P rnd(P p) { return P{rnd(p.x), rnd(p.y), rnd(p.z)}; }

static bool neighbour(const SgDrorGrid &g, const P &a, const P &b)      // b in the ball of query a
{
    const double s2 = sg_dror_s2(g, a.x * a.x + a.y * a.y);
    const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return (dx * dx + dy * dy) + dz * dz <= s2;
}

static bool covered(const SgDrorGrid &g, const P &a, const P &b)
{
    SgDrorWindow w;
    sg_dror_window(g, a.x, a.y, sg_dror_s2(g, a.x * a.x + a.y * a.y), &w);
    const int32_t cell = sg_dror_cell(g, b.x, b.y);
    return cell >= 0 && cell < g.cells && sg_dror_in_window(g, w, cell);
}

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const double alpha = atof(argv[2]), beta = atof(argv[3]), sr_min = atof(argv[5]);
    const long k_min = atol(argv[4]);
    const int budget = atoi(argv[6]);
    SgDrorGrid g{};
    if (sg_dror_make_grid(alpha, beta, sr_min, k_min, budget, &g)) { fprintf(stderr, "outside the domain\n"); return 3; }
    const double c = sqrt(g.c2), r0 = sr_min / c;
    if (!strcmp(argv[1], "pairs") && argc >= 10) {
        g_f32 = atoi(argv[7]) != 0;
        const long per = atol(argv[8]);
        std::mt19937_64 rng((uint64_t)atoll(argv[9]));
        std::uniform_real_distribution<double> U(0.0, 1.0);
        auto dir = [&](bool flat) {
            for (;;) {
                P u{2 * U(rng) - 1, 2 * U(rng) - 1, flat ? 0.0 : 2 * U(rng) - 1};
                const double n = sqrt(u.x * u.x + u.y * u.y + u.z * u.z);
                if (n > 1e-3 && n <= 1.0) return P{u.x / n, u.y / n, u.z / n};
            }
        };
        auto at = [&](double r, double phi, double z) { return P{r * cos(phi), r * sin(phi), z}; };
        auto sr_of = [&](const P &p) { const double s = c * sqrt(p.x * p.x + p.y * p.y); return s > sr_min ? s : sr_min; };
        auto offset = [&](const P &p, const P &u, double d) { return P{p.x + u.x * d, p.y + u.y * d, p.z + u.z * d}; };
        const char *names[] = {"random", "edge", "seam", "boundary", "core", "far500", "far1e5"};
        long total = 0, total_bad = 0;
        for (int src = 0; src < 7; ++src) {
            long checked = 0, bad = 0;
            for (long it = 0; it < per; ++it) {
                P a, b;
                const double phi = (2 * U(rng) - 1) * 3.141592653589793, z = 4 * U(rng) - 2;
                switch (src) {
                case 0: a = at(0.2 + 120 * U(rng) * U(rng), phi, z); b = offset(a, dir(false), sr_of(a) * 1.05 * U(rng)); break;
                case 1: a = at(0.2 + 120 * U(rng) * U(rng), phi, z); b = offset(a, dir(it & 1), sr_of(a) * (1 - 1e-12)); break;
                case 2: a = at(0.5 + 100 * U(rng), (it & 1 ? 1 : -1) * (3.141592653589793 - 0.5 * c * U(rng)), z); b = offset(a, dir(it & 2), sr_of(a) * (it & 4 ? 1 - 1e-12 : U(rng))); break;
                case 3: a = at(r0 * (1 + (2 * U(rng) - 1) * 1.5 * c), phi, z); b = offset(a, dir(it & 1), sr_of(a) * (it & 2 ? 1 - 1e-12 : U(rng))); break;
                case 4: a = (it % 8 == 0) ? P{0, 0, z} : at(1.2 * r0 * U(rng) * U(rng), phi, z); b = (it % 16 == 8) ? P{0, 0, z + sr_min * U(rng)} : offset(a, dir(it & 1), sr_of(a) * (it & 2 ? 1 - 1e-12 : U(rng))); break;
                case 5: a = at(500, phi, z); b = offset(a, dir(it & 1), sr_of(a) * (it & 2 ? 1 - 1e-12 : U(rng))); break;
                default: a = at(1e5, phi, z); b = offset(a, dir(it & 1), sr_of(a) * (it & 2 ? 1 - 1e-12 : U(rng))); break;
                }
                a = rnd(a); b = rnd(b);
                if (!sg_dror_usable(a.x, a.y, a.z) || !sg_dror_usable(b.x, b.y, b.z)) continue;
                for (int swap = 0; swap < 2; ++swap) {      // either row may be the query
                    const P &qa = swap ? b : a, &qb = swap ? a : b;
                    if (!neighbour(g, qa, qb)) continue;
                    ++checked;
                    if (!covered(g, qa, qb)) ++bad;
                }
            }
            printf("%s %ld %ld\n", names[src], checked, bad);
            total += checked; total_bad += bad;
        }
        printf("grid cart_m %d n_ring %d n_az %d cells %d rc %.17g total %ld bad %ld\n", g.cart_m, g.n_ring, g.n_az, g.cells, g.rc, total, total_bad);
        return 0;
    }
    if (!strcmp(argv[1], "cloud") && argc >= 9) {
        FILE *fi = fopen(argv[7], "rb");
        if (!fi) return 4;
        std::vector<P> p;
        P t;
        while (fread(&t, sizeof(P), 1, fi) == 1) p.push_back(t);
        fclose(fi);
        const size_t n = p.size();
        std::vector<uint32_t> entry((size_t)g.cells + 1, 0), cell_of(n, SG_DROR_NO_CELL);
        for (size_t i = 0; i < n; ++i)
            if (sg_dror_usable(p[i].x, p[i].y, p[i].z)) { cell_of[i] = 1 + (uint32_t)sg_dror_cell(g, p[i].x, p[i].y); ++entry[cell_of[i]]; }
        uint32_t run = 0;
        for (int32_t cidx = 0; cidx < g.cells; ++cidx) { const uint32_t v = entry[1 + cidx]; entry[1 + cidx] = run; run += v; }
        std::vector<P> sorted(n);
        for (size_t i = 0; i < n; ++i)
            if (cell_of[i] != SG_DROR_NO_CELL) sorted[entry[cell_of[i]]++] = p[i];
        std::vector<int32_t> nb(n, -1);
        const int need = g.k_min + 1;
        for (size_t i = 0; i < n; ++i) {
            if (cell_of[i] == SG_DROR_NO_CELL) continue;
            const double x = p[i].x, y = p[i].y, z = p[i].z, s2 = sg_dror_s2(g, x * x + y * y);
            int cnt = 0;
            auto walk = [&](uint32_t b, uint32_t e) {
                for (uint32_t k = b; k < e && cnt < need; ++k) {
                    const double dx = sorted[k].x - x, dy = sorted[k].y - y, dz = sorted[k].z - z;
                    cnt += (dx * dx + dy * dy) + dz * dz <= s2 ? 1 : 0;
                }
            };
            SgDrorWindow w;
            sg_dror_window(g, x, y, s2, &w);
            const uint32_t *e = entry.data();
            if (w.cart)
                for (int iy = w.iy0; iy <= w.iy1; ++iy) walk(e[iy * g.cart_m + w.ix0], e[iy * g.cart_m + w.ix1 + 1]);
            if (w.polar)
                for (int ring = w.ring0; ring <= w.ring1; ++ring) {
                    const uint32_t *er = e + g.cart_m * g.cart_m + ring * g.n_az;
                    const int end = w.az0 + w.n_az;
                    if (end <= g.n_az) walk(er[w.az0], er[end]);
                    else { walk(er[w.az0], er[g.n_az]); walk(er[0], er[end - g.n_az]); }
                }
            nb[i] = cnt > 0 ? cnt - 1 : 0;
        }
        FILE *fo = fopen(argv[8], "wb");
        if (!fo) return 5;
        fwrite(nb.data(), sizeof(int32_t), n, fo);
        fclose(fo);
        return 0;
    }
    return 2;
}
