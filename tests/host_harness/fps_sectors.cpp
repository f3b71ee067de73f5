// The reach, the near test, the sector, the quota and the ballot rank of the sectorized keypoint stage (csrc/sg_fps_sectors.h) compiled for
// the host.
//   fps_sectors self <points>
//       sector: sg_fpss_sector against the same expression over libm's atan2, S = 1 .. 16, on <points> points per S concentrated at the
//               sector edges (angles within a few ulps, a few 1e-7 and a few 1e-3 of an edge, at many radii, float32 and float64 values);
//               a point where the two differ is printed as "M S x y ours libm's" (hexadecimal floats) for the caller to settle: libm's
//               atan2 is not correctly rounded everywhere;
//       quota:  every (n_0 .. n_3) in 0 .. 6 and K in 1 .. 14: sum q_s = K and q_s <= n_s for m >= K, q_s = n_s below, the winners have a
//               remainder; prints every quota as a line "q n0 n1 n2 n3 K q0 q1 q2 q3" for the caller to compare;
//       ranks:  1024 random sector bytes dealt to sixteen "waves": tile rank = the waves before + sg_fpss_rank of the wave's ballot, against
//               a sequential count.
//   fps_sectors rows <dtype 0 | 1> <S> <margin> <in: n x 3 float64> <rois: B x 6 float64, or -> <out>
//       out: int8 sector[n] (-1: not near any present roi), then float64 reach2[B].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sg_fps_sectors.h"

static int libm_sector(double x, double y, int S)
{
    const double a = atan2(y, x) + SG_FPSS_PI;
    const int s = (int)floor(a / ((2 * SG_FPSS_PI) / (double)S));
    return s < S - 1 ? s : S - 1;
}

static int self_test(long points)
{
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    long bad = 0, seen = 0;
    for (int S = 1; S <= SG_FPSS_MAX_SECTORS; ++S) {
        int hit[SG_FPSS_MAX_SECTORS] = {0};
        for (long i = 0; i < points; ++i) {
            const int k = (int)(rng() % (uint64_t)(S + 1));
            const double widths[4] = {1e-15, 3e-7, 1e-3, 0.5};
            const double th = k * ((2 * SG_FPSS_PI) / S) - SG_FPSS_PI + (uni(rng) - 0.5) * widths[rng() % 4];
            const double r = std::exp((uni(rng) - 0.3) * 12.0);
            double x = r * std::cos(th), y = r * std::sin(th);
            if (rng() & 1) { x = (double)(float)x; y = (double)(float)y; }
            if (i % 1000 == 0) { x = (rng() & 1) ? 0.0 : -0.0; }
            if (i % 1000 == 1) { y = (rng() & 1) ? 0.0 : -0.0; }
            const int got = sg_fpss_sector(x, y, S), want = libm_sector(x, y, S);
            if (got < 0 || got >= S) return 10;
            ++hit[got];
            ++seen;
            if (got != want) { ++bad; std::printf("M %d %a %a %d %d\n", S, x, y, got, want); }      // (for the caller to settle)
        }
        for (int s = 0; s < S; ++s)
            if (!hit[s]) return 11;
    }
    std::printf("sector points %ld mismatches %ld\n", seen, bad);

    long swept = 0;
    for (int code = 0; code < 7 * 7 * 7 * 7; ++code)
        for (int K = 1; K <= 14; ++K) {
            int64_t n[4] = {code % 7, code / 7 % 7, code / 49 % 7, code / 343};
            int32_t q[4];
            const int64_t m = sg_fpss_quota(n, 4, K, q);
            if (m != n[0] + n[1] + n[2] + n[3]) return 20;
            int64_t sum = 0;
            for (int s = 0; s < 4; ++s) {
                sum += q[s];
                if (q[s] < 0 || q[s] > n[s]) return 21;
                if (m < K && q[s] != n[s]) return 22;
                if (m >= K && q[s] != n[s] * K / m && !(q[s] == n[s] * K / m + 1 && n[s] * K % m > 0)) return 23;      // a winner has a remainder
            }
            if (m >= K && sum != K) return 24;
            std::printf("q %d %d %d %d %d %d %d %d %d\n", (int)n[0], (int)n[1], (int)n[2], (int)n[3], K, q[0], q[1], q[2], q[3]);
            ++swept;
        }
    // a large frame: the products need 64 bits
    {
        int64_t n[3] = {(int64_t)1 << 30, 1, ((int64_t)1 << 30) - 5};
        int32_t q[3];
        sg_fpss_quota(n, 3, 2147483647 / 2, q);
        if ((int64_t)q[0] + q[1] + q[2] != 2147483647 / 2 || q[1] > 1) return 25;
    }
    std::printf("quota swept %ld\n", swept);

    for (int S = 1; S <= SG_FPSS_MAX_SECTORS; S += 5)
        for (int round = 0; round < 20; ++round) {
            int8_t sec[SG_FPS_BLOCK];
            for (int i = 0; i < SG_FPS_BLOCK; ++i) sec[i] = (int8_t)((int)(rng() % (uint64_t)(S + 1)) - 1);
            unsigned long long bal[SG_FPS_WAVES][SG_FPSS_MAX_SECTORS] = {};
            for (int i = 0; i < SG_FPS_BLOCK; ++i)
                if (sec[i] >= 0) bal[i >> 6][sec[i]] |= 1ull << (i & 63);
            int seq[SG_FPSS_MAX_SECTORS] = {0};
            for (int i = 0; i < SG_FPS_BLOCK; ++i) {
                if (sec[i] < 0) continue;
                int before = 0;
                for (int w = 0; w < (i >> 6); ++w) before += __builtin_popcountll(bal[w][sec[i]]);
                if (before + sg_fpss_rank(bal[i >> 6][sec[i]], i & 63) != seq[sec[i]]++) return 30;
            }
        }
    std::printf("ranks ok\n");
    return 0;
}

template <typename T> static int rows_mode(int S, double margin, const std::vector<double> &p, const std::vector<double> &b, FILE *fo)
{
    const size_t n = p.size() / 3, B = b.size() / 6;
    std::vector<SgFpsRoi> rec(B);
    for (size_t k = 0; k < B; ++k) {
        T box[6];
        for (int j = 0; j < 6; ++j) box[j] = (T)b[6 * k + j];
        sg_fpss_roi<T>(box, margin, &rec[k]);
    }
    std::vector<int8_t> sec(n);
    for (size_t i = 0; i < n; ++i) {
        const T x = (T)p[3 * i], y = (T)p[3 * i + 1], z = (T)p[3 * i + 2];
        bool u = B == 0;
        for (size_t k = 0; k < B && !u; ++k) u = sg_fpss_near(rec[k], (double)x, (double)y, (double)z);
        sec[i] = (int8_t)(u ? sg_fpss_sector((double)x, (double)y, S) : -1);
    }
    fwrite(sec.data(), 1, n, fo);
    for (size_t k = 0; k < B; ++k) fwrite(&rec[k].reach2, sizeof(double), 1, fo);
    return 0;
}

static bool read_doubles(const char *path, std::vector<double> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    double c;
    while (fread(&c, sizeof(double), 1, f) == 1) v.push_back(c);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "self")) return self_test(atol(argv[2]));
    if (argc < 8 || strcmp(argv[1], "rows")) return 2;
    const int dtype = atoi(argv[2]), S = atoi(argv[3]);
    if (S < 1 || S > SG_FPSS_MAX_SECTORS || (dtype != 0 && dtype != 1)) return 2;
    std::vector<double> p, b;
    if (!read_doubles(argv[5], p) || p.size() % 3) return 4;
    if (strcmp(argv[6], "-") && (!read_doubles(argv[6], b) || b.size() % 6)) return 4;
    FILE *fo = fopen(argv[7], "wb");
    if (!fo) return 5;
    const int rc = dtype == 0 ? rows_mode<float>(S, atof(argv[4]), p, b, fo) : rows_mode<double>(S, atof(argv[4]), p, b, fo);
    fclose(fo);
    return rc;
}
