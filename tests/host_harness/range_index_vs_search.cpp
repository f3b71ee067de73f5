// Host harness: the candidate scan of the pass over all rows (sg_beam.h: sg_wave_scan, one-word lists) with the step-major range index
// (sg_range_index.h: bin_qs, one 8-byte load per beam) against the same scan with NO index at all -- the full binary search over each
// bin.  The index only narrows where that search starts, so every beam must meet the same flakes: the same count, the same list, the
// same order, the same overflow slot.  The tables are filed by the product's host filing (sg_table_host.h) and indexed by
// sg_range_index_fill, the function k_table_index runs on the device; its counts are checked against a plain count first.
//   tables: random; sparse (most bins empty) with a bin of 40 records between two steps and records at exactly 8.0, 16.0 and 120.0 m;
//           every record beyond every target; a bin of more than 65 535 records (no step-major index is filed: the scan reads bin_q)
//   beams:  random; targets at exactly 8.0, 16.0, 120.0 m and beyond 120 m; NaN coordinates; azimuths around the 0 / 2 pi seam (first
//           bin n_bins - 1, next bin 0)
// A "wave" of one lane (SG_PAIR_WINDOW = 1), as tests/host_harness/wave_vs_lane.cpp.
// usage: range_index_vs_search [beams per case]; exit status 1 on any mismatch.  Built and run by tests/test_range_index.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <random>
#include <cmath>
#include <limits>
#include <vector>
__host__ inline int __double2hiint(double x) { unsigned long long u; memcpy(&u, &x, 8); return (int)(u >> 32); }
__host__ inline double __hiloint2double(int hi, int lo) { unsigned long long u = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo; double x; memcpy(&x, &u, 8); return x; }
__host__ inline int __float_as_int(float x) { int i; memcpy(&i, &x, 4); return i; }
__host__ inline float __int_as_float(int i) { float x; memcpy(&x, &i, 4); return x; }
__host__ inline unsigned __float_as_uint(float x) { unsigned i; memcpy(&i, &x, 4); return i; }
__host__ inline float __uint_as_float(unsigned i) { float x; memcpy(&x, &i, 4); return x; }
__host__ inline long long __double_as_longlong(double x) { long long i; memcpy(&i, &x, 8); return i; }
__host__ inline double __longlong_as_double(long long i) { double x; memcpy(&x, &i, 8); return x; }
__host__ inline int __double2loint(double x) { unsigned long long u; memcpy(&u, &x, 8); return (int)(u & 0xffffffffu); }
template <typename T> __host__ inline T __shfl(T v, int) { return v; }
template <typename T> __host__ inline T __shfl_up(T v, int) { return v; }
template <typename T> __host__ inline T __shfl_down(T v, int) { return v; }
template <typename T> __host__ inline T __shfl_xor(T v, int) { return v; }
__host__ inline unsigned long long __ballot(int p) { return p ? 1ull : 0ull; }
__host__ inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
__host__ inline int __ffsll(long long v) { return __builtin_ffsll(v); }
__host__ inline int atomicAdd(int *p, int v) { int o = *p; *p += v; return o; }
__host__ inline int atomicOr(int *p, int v) { int o = *p; *p |= v; return o; }
#undef __device__
#define __device__
#define SG_PAIR_WINDOW 1     /* a wave of one lane takes one pair per trip */
#include "sg_beam.h"
#include "sg_table_host.h"

static const double NaN = std::numeric_limits<double>::quiet_NaN();

struct Filed {
    std::vector<SgEntry> entries;
    std::vector<uint32_t> start, q, qs;
    uint32_t max_bin = 0;
    int K = 0;
    bool has_qs = false;
    SgTable desc(bool with_qs, bool with_q) const
    {
        SgTable t{};
        t.entries = entries.data(); t.bin_start = start.data();
        t.bin_q = with_q ? q.data() : nullptr;
        t.bin_qs = with_qs && has_qs ? qs.data() : nullptr;
        t.n_bins = SG_NBINS; t.n_entries = start[SG_NBINS]; t.inv_bin_w = SG_NBINS / SG_TWO_PI; t.n_flakes = (uint32_t)K; t.max_bin = max_bin;
        return t;
    }
};

// file and index a table as the library does (snowgpu_upload_table, register_table, k_table_index); returns mismatches of the index
// against a plain count
static long file_table(const std::vector<double> &xyr, Filed &f)
{
    f.K = (int)(xyr.size() / 3);
    int64_t bad = -1;
    if (sg_file_table_host(xyr.data(), f.K, f.entries, f.start, f.max_bin, &bad)) { printf("table filing failed at row %lld\n", (long long)bad); return 1; }
    f.has_qs = SG_QS_FITS(f.max_bin);
    f.q.assign((size_t)SG_NBINS * SG_QSTEPS, 0xdeadbeefu);
    if (f.has_qs) f.qs.assign(SG_QS_WORDS(SG_NBINS), 0xdeadbeefu);
    for (int b = 0; b < SG_NBINS; ++b)
        for (int k = 0; k < SG_QSTEPS; ++k)
            sg_range_index_fill(f.entries.data(), f.start.data(), SG_NBINS, b, k, f.q.data(), f.has_qs ? f.qs.data() : nullptr);
    long badn = 0;
    for (int b = 0; b < SG_NBINS; ++b) {
        uint32_t cnt[SG_QSTEPS + 1];
        for (int k = 0; k < SG_QSTEPS; ++k) {
            cnt[k] = 0;
            for (uint32_t e = f.start[b]; e < f.start[b + 1]; ++e) cnt[k] += f.entries[e].rho < SG_QSTEP_M * (double)k;
        }
        cnt[SG_QSTEPS] = f.start[b + 1] - f.start[b];
        for (int k = 0; k < SG_QSTEPS; ++k) {
            bool ok = f.q[(size_t)b * SG_QSTEPS + k] == cnt[k];
            if (f.has_qs) {
                const uint32_t w = cnt[k] | (cnt[k + 1] << 16);
                ok = ok && f.qs[(size_t)k * SG_QS_ROW(SG_NBINS) + b] == w && (b != 0 || f.qs[(size_t)k * SG_QS_ROW(SG_NBINS) + SG_NBINS] == w);
            }
            if (!ok) { if (badn < 5) printf("INDEX bin %d step %d differs from the plain count\n", b, k); ++badn; }
        }
    }
    return badn;
}

struct Scan {
    int L;
    SgBeamOut out;
    double rho[4];
    alignas(8) uint32_t rec[6];
    int key[4];
    double ov[SG_OV_STRIDE];
    unsigned char d_t[8];
    double theta_c;
};

template <typename T, bool DEFER>
static void scan(const SgTable &tab, T px, T py, T pz, double div, Scan &s)
{
    memset(&s, 0, sizeof s);
    int cnt[64], st[2];
    T d_t;
    s.L = sg_wave_scan<T, 4, 1, DEFER, true>(true, px, py, pz, tab, div, reinterpret_cast<double *>(s.rec), nullptr, s.rho, cnt, s.key, st, 0, s.out, d_t,
                                             s.theta_c, false, s.ov, SG_OV_CAP);
    memcpy(s.d_t, &d_t, sizeof(T));
    for (int i = s.L; i < 4; ++i) { s.rho[i] = 0; s.rec[i] = 0; s.key[i] = 0; }      // beyond the list: whatever the scan left
}

static bool same(const Scan &a, const Scan &b)
{
    return a.L == b.L && a.out.n_hits == b.out.n_hits && a.out.overflow == b.out.overflow && memcmp(a.rho, b.rho, sizeof a.rho) == 0 &&
           memcmp(a.rec, b.rec, 4 * sizeof(uint32_t)) == 0 && memcmp(a.key, b.key, sizeof a.key) == 0 && memcmp(a.ov, b.ov, sizeof a.ov) == 0 &&
           memcmp(a.d_t, b.d_t, 8) == 0 && memcmp(&a.theta_c, &b.theta_c, 8) == 0;
}

struct Beam { double x, y, z; };

// the beams of every case: random ones, exact ranges on the axes and a little off them, beyond the last step, NaN, and the seam
static std::vector<Beam> make_beams(long M, unsigned long long seed)
{
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<Beam> v;
    const double exact[] = {8.0, 16.0, 120.0, 24.0, 112.0, 128.0, 150.0, 1.0e6, 7.999999, 8.000001, 119.99999, 120.00001, 0.5};
    for (double d : exact) {
        v.push_back({d, 0, 0}); v.push_back({-d, 0, 0}); v.push_back({0, d, 0}); v.push_back({0, -d, 0}); v.push_back({0, 0, d});
        for (int i = 0; i < 40; ++i) {                          // the same range, azimuths within a few beam widths of an axis
            const double az = (i % 4) * (SG_PI / 2) + (U(rng) - 0.5) * 0.02;
            v.push_back({d * std::cos(az), d * std::sin(az), 0});
        }
    }
    v.push_back({NaN, 1, 0}); v.push_back({1, NaN, 0}); v.push_back({5, 5, NaN}); v.push_back({NaN, NaN, NaN});
    v.push_back({std::numeric_limits<double>::infinity(), 1, 0});
    for (long j = 0; j < M / 4; ++j) {                          // around the seam: within three beam widths of azimuth 0
        const double d = 2.0 + 140.0 * U(rng), az = (U(rng) - 0.5) * 0.018;
        v.push_back({d * std::cos(az), d * std::sin(az), (U(rng) - 0.7) * 0.3 * d});
    }
    for (long j = 0; j < M; ++j) {
        const double d = 1.0 + 139.0 * U(rng), az = U(rng) * SG_TWO_PI, el = (U(rng) - 0.7) * 0.4;
        v.push_back({d * std::cos(el) * std::cos(az), d * std::cos(el) * std::sin(az), d * std::sin(el)});
    }
    return v;
}

// one table, every beam: the scan with the index the table has (step-major, or bin-major where none was filed) and with bin_q alone,
// each against the scan without any index
template <typename T, bool DEFER>
static long run(const char *name, const Filed &f, const std::vector<Beam> &beams, double div)
{
    const SgTable t_idx = f.desc(true, true), t_q = f.desc(false, true), t_none = f.desc(false, false);
    long badn = 0, with_flakes = 0, full = 0, seam = 0, undecided = 0;
    for (size_t j = 0; j < beams.size(); ++j) {
        const T px = (T)beams[j].x, py = (T)beams[j].y, pz = (T)beams[j].z;
        static Scan a, b, c;
        scan<T, DEFER>(t_none, px, py, pz, div, a);
        scan<T, DEFER>(t_idx, px, py, pz, div, b);
        scan<T, DEFER>(t_q, px, py, pz, div, c);
        if (!same(a, b) || !same(a, c)) {
            if (badn < 10) printf("MISMATCH %s beam %zu (%g, %g, %g): flakes met %d / %d / %d, lists %d / %d / %d\n", name, j, (double)px, (double)py, (double)pz,
                                  a.out.n_hits, b.out.n_hits, c.out.n_hits, a.L, b.L, c.L);
            ++badn;
        }
        if (a.out.n_hits & SG_HITS_UNDECIDED) ++undecided;
        if (a.L > 0) ++with_flakes;
        if (a.out.overflow) ++full;
        double th_r, th_l;
        sg_beam_limits(a.theta_c, div, th_r, th_l);
        if (a.theta_c == a.theta_c && sg_bin_of(th_r - SG_BEAM_MARGIN, t_idx.inv_bin_w, SG_NBINS) == SG_NBINS - 1 &&
            sg_bin_of(th_l + SG_BEAM_MARGIN, t_idx.inv_bin_w, SG_NBINS) != SG_NBINS - 1) ++seam;
    }
    printf("index<%s, %s> %s (%s): %zu beams, %ld mismatches; %ld with flakes, %ld beyond the list, %ld across the seam, %ld undecided\n",
           sizeof(T) == 4 ? "float32" : "float64", DEFER ? "deferred" : "in place", name, f.has_qs ? "step-major index" : "no step-major index", beams.size(), badn,
           with_flakes, full, seam, undecided);
    return badn;
}

static void add_flake(std::vector<double> &xyr, double rho, double phi, double r)
{
    // on the axes the coordinates are exact, and so is the range
    const int quarter = (int)std::lround(phi / (SG_PI / 2));
    double x = rho * std::cos(phi), y = rho * std::sin(phi);
    if (phi == quarter * (SG_PI / 2)) { const double cx[] = {1, 0, -1, 0, 1}, cy[] = {0, 1, 0, -1, 0}; x = rho * cx[quarter]; y = rho * cy[quarter]; }
    xyr.push_back(x); xyr.push_back(y); xyr.push_back(r);
}

int main(int argc, char **argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 4000;
    const double bd = 0.1718873385392;
    std::mt19937_64 rng(77);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long bad = 0;
    const std::vector<Beam> beams = make_beams(n, 5);

    {   // random, as dense as a real table
        std::vector<double> xyr;
        for (int i = 0; i < 18000; ++i) add_flake(xyr, 1.0 + 129.0 * std::sqrt(U(rng)), U(rng) * SG_TWO_PI, 0.01 * (0.3 + 1.4 * U(rng)));
        Filed f;
        bad += file_table(xyr, f);
        bad += run<float, true>("random", f, beams, bd);
        bad += run<double, false>("random", f, beams, bd);
    }
    {   // sparse: flakes on and next to the four axes only (every other bin is empty); 40 records between 8 and 16 m in the bins at the seam;
        // records at exactly 8.0, 16.0 and 120.0 m on every axis, and at the neighbouring representable ranges
        std::vector<double> xyr;
        for (int a = 0; a < 4; ++a) {
            const double phi0 = a * (SG_PI / 2);
            for (double rho : {8.0, 16.0, 120.0, 24.0, 112.0}) {
                add_flake(xyr, rho, phi0, 0.02);
                add_flake(xyr, std::nextafter(rho, 0.0), phi0, 0.02);
                add_flake(xyr, std::nextafter(rho, 1e9), phi0, 0.02);
                add_flake(xyr, rho, phi0, 0.005);                                       // an equal range: the order inside the bin is by table row
            }
            for (int i = 0; i < 40; ++i) add_flake(xyr, 8.0 + 8.0 * (i + 0.5) / 40.0, phi0 + (U(rng) - 0.5) * 0.004, 0.012);
            for (int i = 0; i < 60; ++i) add_flake(xyr, 0.6 + 135.0 * U(rng), phi0 + (U(rng) - 0.5) * 0.012, 0.004 + 0.02 * U(rng));
        }
        Filed f;
        bad += file_table(xyr, f);
        long empty = 0, crowded = 0;
        for (int b = 0; b < SG_NBINS; ++b) {
            empty += f.start[b] == f.start[b + 1];
            crowded += f.q[(size_t)b * SG_QSTEPS + 2] - f.q[(size_t)b * SG_QSTEPS + 1] > 16;
        }
        if (empty < SG_NBINS / 2 || crowded == 0) { printf("sparse table: %ld empty bins, %ld with more than 16 records in a step -- not the case meant\n", empty, crowded); ++bad; }
        bad += run<float, true>("sparse", f, beams, bd);
        bad += run<double, true>("sparse", f, beams, bd);
        bad += run<float, false>("sparse", f, beams, bd);
    }
    {   // every record beyond every target: flakes from 150 m on, the random beams end below 141 m (the exact ones at 150 m and 1e6 m reach them)
        std::vector<double> xyr;
        for (int i = 0; i < 6000; ++i) add_flake(xyr, 150.0 + 50.0 * U(rng), (i % 7 == 0 ? (U(rng) - 0.5) * 0.02 : U(rng) * SG_TWO_PI), 0.03);
        Filed f;
        bad += file_table(xyr, f);
        bad += run<float, true>("far", f, beams, bd);
    }
    {   // an empty table
        Filed f;
        bad += file_table(std::vector<double>(), f);
        bad += run<float, true>("empty", f, beams, bd);
    }
    {   // a bin of more than 65 535 records: its counts do not fit 16 bits, no step-major index is filed, the scan reads bin_q
        std::vector<double> xyr;
        for (int i = 0; i < 66000; ++i) add_flake(xyr, 2.0 + 130.0 * U(rng), 0.0010 + 0.0008 * U(rng), 0.0005);
        for (int i = 0; i < 2000; ++i) add_flake(xyr, 2.0 + 130.0 * U(rng), U(rng) * SG_TWO_PI, 0.01);
        Filed f;
        bad += file_table(xyr, f);
        if (f.max_bin <= SG_QS_MAX_BIN || f.has_qs || !f.qs.empty() || f.desc(true, true).bin_qs != nullptr) {
            printf("long-bin table: longest bin %u, step-major index filed: %d -- expected none\n", f.max_bin, (int)f.has_qs);
            ++bad;
        }
        const std::vector<Beam> few = make_beams(n / 8, 6);
        bad += run<float, true>("long bin", f, few, bd);
    }
    return bad != 0;
}
