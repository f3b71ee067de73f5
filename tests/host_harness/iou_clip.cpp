// iou_clip.cpp -- csrc/sg_iou.h on the host (hipcc --cuda-host-only -x hip, as box_cells.cpp is compiled): the clip of the definition on
// random and adversarial pairs, and the areas and IoUs of given pairs for the byte comparison with tests/iou_reference.py.
//   iou_clip stress <seed> <pairs>
//       pairs of nine kinds in turn: car-sized at random; equal boxes; the same centre turned by multiples of 90 degrees; headings 1 ulp
//       apart; shared faces; slivers; coordinates up to 1e6; sizes from 1 cm to 100 m;
//       boxes a few ulps of their coordinates wide (the corners collapse).  For every pair area(a, b) and area(b, a):
//       no pass emits more vertices than the capacity holds (SG_IOU_CAP = 20; the largest count is printed), area <= min(Aa, Ab) + tol, |area(a, b) - area(b, a)| <= tol with
//       tol = 4 sqrt(2) L 32 eps R + 16 eps L^2 (tests/iou_reference.py derives it; R, L of the pair).  Prints
//       "stress <pairs> <most vertices> <largest excess / tol> <largest asymmetry / tol>" and exits 1 on a violation.
//   iou_clip areas <n> <in> <out>
//       in: n x 18 float64 (a[7], pose a[2], b[7], pose b[2]); out: n x 3 float64 (area(a, b), BEV IoU, 3D IoU) through sg_iou_make with
//       the given pose, so absent boxes are handled as on the device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sg_iou.h"

static uint64_t g_state;
static uint64_t next_u64()
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(next_u64() >> 11) * (1.0 / 9007199254740992.0)); }

static void car(double *b, double reach)
{
    b[0] = uni(-reach, reach); b[1] = uni(-reach, reach); b[2] = uni(-2, 0);
    b[3] = uni(3.5, 5.0); b[4] = uni(1.6, 2.1); b[5] = uni(1.4, 2.0); b[6] = uni(-M_PI, M_PI);
}

static void make_pair(int kind, double *a, double *b)
{
    car(a, 45.0);
    std::memcpy(b, a, 7 * sizeof(double));
    switch (kind) {
    case 0: car(b, 45.0); b[0] = a[0] + uni(-4, 4); b[1] = a[1] + uni(-4, 4); break;
    case 1: break;
    case 2: a[6] = (double)((int)uni(-4, 5)) * (M_PI / 2); b[6] = a[6] + (double)((int)uni(-4, 5)) * (M_PI / 2);
            if (next_u64() & 1) { b[0] += uni(-1, 1); b[3] = uni(1, 6); } break;
    case 3: b[6] = std::nextafter(a[6], (next_u64() & 1) ? 10.0 : -10.0); if (next_u64() & 1) b[3] = a[3] * 0.5; break;
    case 4: {
        const bool axis = next_u64() & 1;
        if (next_u64() & 1) a[6] = b[6] = (double)((int)uni(-2, 3)) * (M_PI / 2);
        const double c = std::cos(a[6]), s = std::sin(a[6]), d = axis ? a[4] : a[3];
        b[0] = a[0] + (axis ? -s : c) * d; b[1] = a[1] + (axis ? c : s) * d; break;
    }
    case 5: a[3] = std::pow(10.0, uni(-6, -3)); a[4] = uni(5, 20); b[6] = a[6] + uni(-1e-3, 1e-3); if (next_u64() & 1) { b[3] = uni(1, 5); b[4] = std::pow(10.0, uni(-6, -3)); } break;
    case 6: a[0] = uni(-1e6, 1e6); a[1] = uni(-1e6, 1e6); a[3] = std::pow(10.0, uni(0, 6)); a[4] = std::pow(10.0, uni(0, 6));
            std::memcpy(b, a, 7 * sizeof(double)); b[0] = std::fmax(-1e6, std::fmin(1e6, a[0] + uni(-1, 1) * a[3])); b[6] = uni(-1e6, 1e6);
            b[3] = std::pow(10.0, uni(0, 6)); break;
    case 8: for (int k = 3; k < 5; ++k) { a[k] = std::pow(10.0, uni(-15, -12)); b[k] = (next_u64() & 1) ? a[k] : std::pow(10.0, uni(-15, -12)); }
            b[0] = a[0] + uni(-1, 1) * a[3]; b[6] = (next_u64() & 1) ? a[6] : uni(-M_PI, M_PI); break;
    default: for (int k = 3; k < 5; ++k) { a[k] = std::pow(10.0, uni(-2, 2)); b[k] = std::pow(10.0, uni(-2, 2)); }
             b[0] = a[0] + uni(-1, 1) * a[3]; b[1] = a[1] + uni(-1, 1) * a[4]; b[6] = uni(-M_PI, M_PI); break;
    }
}

static int stress(uint64_t seed, long pairs)
{
    g_state = seed * 0x2545f4914f6cdd1dull + 1;
    const double eps = std::ldexp(1.0, -53);
    long bad = 0, present = 0;
    int most = 0;
    double worst_excess = 0.0, worst_asym = 0.0;
    for (long i = 0; i < pairs; ++i) {
        double a[7], b[7];
        make_pair((int)(i % 9), a, b);
        SgIouRec ra, rb;
        if (!sg_iou_make<double>(a, nullptr, &ra) || !sg_iou_make<double>(b, nullptr, &rb)) continue;
        ++present;
        int d = 0;
        const double ab = sg_iou_area(ra, rb, &d), ba = sg_iou_area(rb, ra, &d);
        if (d > most) most = d;
        const double La = std::sqrt(a[3] * a[3] + a[4] * a[4]), Lb = std::sqrt(b[3] * b[3] + b[4] * b[4]), L = La > Lb ? La : Lb;
        const double R = std::fmax(std::fmax(std::fabs(a[0]), std::fabs(a[1])), std::fmax(std::fabs(b[0]), std::fabs(b[1]))) + L;
        const double tol = 4 * std::sqrt(2.0) * L * 32 * eps * R + 16 * eps * L * L;
        const double Aa = a[3] * a[4], Ab = b[3] * b[4], least = Aa < Ab ? Aa : Ab;
        const double excess = (std::fmax(ab, ba) - least) / tol, asym = std::fabs(ab - ba) / tol;
        if (excess > worst_excess) worst_excess = excess;
        if (asym > worst_asym) worst_asym = asym;
        if (!(ab >= 0.0) || !(ba >= 0.0) || excess > 1.0 || asym > 1.0 || d > SG_IOU_CAP) {
            if (bad++ < 5)
                std::fprintf(stderr, "kind %d: area %.17g / %.17g, least %.17g, tol %.3g, vertices %d\n  a %.17g %.17g %.17g %.17g %.17g\n  b %.17g %.17g %.17g %.17g %.17g\n",
                             (int)(i % 9), ab, ba, least, tol, d, a[0], a[1], a[3], a[4], a[6], b[0], b[1], b[3], b[4], b[6]);
        }
    }
    std::printf("stress %ld %d %.6g %.6g\n", present, most, worst_excess, worst_asym);
    return bad ? 1 : 0;
}

static int areas(long n, const char *in, const char *out)
{
    std::vector<double> buf((size_t)n * 18), res((size_t)n * 3);
    FILE *f = std::fopen(in, "rb");
    if (!f || std::fread(buf.data(), sizeof(double), buf.size(), f) != buf.size()) return 2;
    std::fclose(f);
    for (long i = 0; i < n; ++i) {
        const double *p = &buf[(size_t)i * 18];
        SgIouRec ra, rb;
        const bool oka = sg_iou_make<double>(p, p + 7, &ra), okb = sg_iou_make<double>(p + 9, p + 16, &rb);
        res[(size_t)i * 3] = (oka && okb) ? sg_iou_area(ra, rb, nullptr) : 0.0;
        res[(size_t)i * 3 + 1] = sg_iou_pair(ra, rb, SG_IOU_MODE_BEV, nullptr);
        res[(size_t)i * 3 + 2] = sg_iou_pair(ra, rb, SG_IOU_MODE_3D, nullptr);
    }
    f = std::fopen(out, "wb");
    if (!f || std::fwrite(res.data(), sizeof(double), res.size(), f) != res.size()) return 2;
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "stress")) return stress(std::strtoull(argv[2], nullptr, 10), std::atol(argv[3]));
    if (argc == 5 && !std::strcmp(argv[1], "areas")) return areas(std::atol(argv[2]), argv[3], argv[4]);
    std::fprintf(stderr, "usage: iou_clip stress <seed> <pairs> | areas <n> <in> <out>\n");
    return 2;
}
