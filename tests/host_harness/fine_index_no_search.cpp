// Host harness: the candidate scan of the pass over all rows (sg_beam.h: sg_wave_scan, one-word lists) with the step-major range index the
// library files (sg_range_index.h: SG_QS_FILE_STEPS steps of SG_QS_FILE_STEP_M metres, its shape in the table descriptor) against the same
// scan with NO index at all.  With the step-major index the scan searches nothing: every record below the upper count of the target's step
// is a candidate and the pair loop drops those at or beyond the target -- so a dropped candidate must leave nothing behind: every beam the
// same count, overflow and undecided bit, the same list (ranges, words, order), the same overflow slot.  The index's words are checked
// against a plain count first; the legacy shape (a descriptor that names none: SG_QSTEPS steps of SG_QSTEP_M) runs beside it.
//   tables: random, as dense as a bench table; sparse with 110 records inside ONE step (10 - 12 m) of each of the two bins at the 0 / 2 pi
//           seam and records at exactly 2, 4, 126, 128 m (and the representable ranges beside them) on the axes; empty; a bin of more than
//           65 535 records (no step-major index is filed: the scan searches from bin_q)
//   beams:  targets at a record's exact range and one representable value either side (in both row dtypes); on every multiple of the step
//           up to 128 m and beyond; NaN, infinity; around the seam; at the start of the crowded step (more than 64 candidates in a row are
//           dropped); across the seam with five or more flakes met and dropped candidates of the first bin between them in scan order
// A "wave" of one lane (SG_PAIR_WINDOW = 1), as tests/host_harness/range_index_vs_search.cpp.
// usage: fine_index_no_search [beams per case]; exit status 1 on any mismatch.  Built and run by tests/test_fine_index.py.
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
static const int FS = SG_QS_FILE_STEPS;
static const double FM = SG_QS_FILE_STEP_M;

struct Filed {
    std::vector<SgEntry> entries;
    std::vector<uint32_t> start, q, qs_fine, qs_legacy;
    uint32_t max_bin = 0;
    int K = 0;
    bool has_qs = false;
    // which: 0 no index at all, 1 the shape the library files, 2 the legacy shape under a descriptor that names none
    SgTable desc(int which) const
    {
        SgTable t{};
        t.entries = entries.data(); t.bin_start = start.data();
        t.n_bins = SG_NBINS; t.n_entries = start[SG_NBINS]; t.inv_bin_w = SG_NBINS / SG_TWO_PI; t.n_flakes = (uint32_t)K; t.max_bin = max_bin;
        if (which == 0) return t;
        t.bin_q = q.data();
        if (!has_qs) return t;
        if (which == 1) { t.bin_qs = qs_fine.data(); t.qs_steps = (uint32_t)FS; t.qs_per_m = (float)(1.0 / FM); }
        else t.bin_qs = qs_legacy.data();
        return t;
    }
};

// file a table as the library does (snowgpu_upload_table, register_table, k_table_index); returns mismatches of the fine index against a plain count
static long file_table(const std::vector<double> &xyr, Filed &f)
{
    f.K = (int)(xyr.size() / 3);
    int64_t bad = -1;
    if (sg_file_table_host(xyr.data(), f.K, f.entries, f.start, f.max_bin, &bad)) { printf("table filing failed at row %lld\n", (long long)bad); return 1; }
    f.has_qs = SG_QS_FITS(f.max_bin);
    f.q.assign((size_t)SG_NBINS * SG_QSTEPS, 0xdeadbeefu);
    if (f.has_qs) { f.qs_fine.assign(SG_QS_WORDS_OF(FS, SG_NBINS), 0xdeadbeefu); f.qs_legacy.assign(SG_QS_WORDS(SG_NBINS), 0xdeadbeefu); }
    for (int b = 0; b < SG_NBINS; ++b) {
        for (int k = 0; k < SG_QSTEPS; ++k) sg_range_index_fill(f.entries.data(), f.start.data(), SG_NBINS, b, k, f.q.data(), f.has_qs ? f.qs_legacy.data() : nullptr);
        if (f.has_qs) for (int k = 0; k < FS; ++k) sg_range_index_fill_steps(f.entries.data(), f.start.data(), SG_NBINS, b, k, FS, FM, nullptr, f.qs_fine.data());
    }
    long badn = 0;
    if (f.has_qs)
        for (int b = 0; b < SG_NBINS; ++b) {
            std::vector<uint32_t> cnt((size_t)FS + 1, 0u);
            for (int k = 0; k < FS; ++k)
                for (uint32_t e = f.start[b]; e < f.start[b + 1]; ++e) cnt[k] += f.entries[e].rho < FM * (double)k;
            cnt[FS] = f.start[b + 1] - f.start[b];
            for (int k = 0; k < FS; ++k) {
                const uint32_t w = cnt[k] | (cnt[k + 1] << 16);
                const bool ok = f.qs_fine[(size_t)k * SG_QS_ROW(SG_NBINS) + b] == w && (b != 0 || f.qs_fine[(size_t)k * SG_QS_ROW(SG_NBINS) + SG_NBINS] == w);
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

// count, overflow, undecided bit, list length, ranges, words, the relative order of the keys, overflow slot, range and azimuth
static bool same(const Scan &a, const Scan &b)
{
    if (a.L != b.L || (a.out.n_hits & ~SG_HITS_UNDECIDED) != (b.out.n_hits & ~SG_HITS_UNDECIDED) ||
        (a.out.n_hits & SG_HITS_UNDECIDED) != (b.out.n_hits & SG_HITS_UNDECIDED) || a.out.overflow != b.out.overflow) return false;
    for (int i = 0; i < a.L; ++i)
        for (int j = 0; j < a.L; ++j)
            if ((a.key[i] < a.key[j]) != (b.key[i] < b.key[j])) return false;
    return memcmp(a.rho, b.rho, sizeof a.rho) == 0 && memcmp(a.rec, b.rec, 4 * sizeof(uint32_t)) == 0 && memcmp(a.ov, b.ov, sizeof a.ov) == 0 &&
           memcmp(a.d_t, b.d_t, 8) == 0 && memcmp(&a.theta_c, &b.theta_c, 8) == 0;
}

struct Beam { double x, y, z; };

// ranges that records of the sparse table sit at exactly (on the axes), all representable in float32
static const double EXACT[] = {2.0, 4.0, 126.0, 128.0, 10.5, 33.25};

static std::vector<Beam> make_beams(long M, unsigned long long seed)
{
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::vector<Beam> v;
    auto axes = [&](double d) { v.push_back({d, 0, 0}); v.push_back({-d, 0, 0}); v.push_back({0, d, 0}); v.push_back({0, -d, 0}); };
    // at a record's range (rho == d is NOT nearer) and one representable value either side, of float64 and of float32 rows
    for (double d : EXACT) {
        axes(d);
        axes(std::nextafter(d, 0.0)); axes(std::nextafter(d, 1e9));
        axes((double)std::nextafterf((float)d, 0.0f)); axes((double)std::nextafterf((float)d, 1e9f));
    }
    // every multiple of the step up to 128 m, beside it, and beyond
    for (int k = 1; k * FM <= 128.0; ++k) {
        const double d = FM * k;
        axes(d);
        v.push_back({(double)std::nextafterf((float)d, 0.0f), 0, 0}); v.push_back({(double)std::nextafterf((float)d, 1e9f), 0, 0});
        for (int i = 0; i < 6; ++i) {                           // the same range a few beam widths off an axis
            const double az = (i % 4) * (SG_PI / 2) + (U(rng) - 0.5) * 0.02;
            v.push_back({d * std::cos(az), d * std::sin(az), 0});
        }
    }
    for (double d : {129.0, 130.0, 150.0, 1.0e6, 0.5}) axes(d);
    // the crowded step of the seam bins: at its start, inside, at its end; wedges in the last bin, in bin 0 and across both
    for (double d : {10.0, 10.000001, 10.05, 10.1, 10.5, 11.0, 11.99, 12.0, 12.01, 9.99})
        for (double az : {0.0, 0.0002, -0.0002, 0.0009, -0.0009, 0.0004, -0.0004}) v.push_back({d * std::cos(az), d * std::sin(az), 0});
    v.push_back({NaN, 1, 0}); v.push_back({1, NaN, 0}); v.push_back({5, 5, NaN}); v.push_back({NaN, NaN, NaN});
    v.push_back({std::numeric_limits<double>::infinity(), 1, 0}); v.push_back({1, -std::numeric_limits<double>::infinity(), 0});
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

struct Seen { long dropped_run = 0, interleaved = 0; };

// one table, every beam: the scan with the fine index and with the legacy shape, each against the scan without any index
template <typename T, bool DEFER>
static long run(const char *name, const Filed &f, const std::vector<Beam> &beams, double div, Seen *seen = nullptr)
{
    const SgTable t_none = f.desc(0), t_fine = f.desc(1), t_legacy = f.desc(2);
    long badn = 0, with_flakes = 0, full = 0, seam = 0, undecided = 0;
    for (size_t j = 0; j < beams.size(); ++j) {
        const T px = (T)beams[j].x, py = (T)beams[j].y, pz = (T)beams[j].z;
        static Scan a, b, c;
        scan<T, DEFER>(t_none, px, py, pz, div, a);
        scan<T, DEFER>(t_fine, px, py, pz, div, b);
        scan<T, DEFER>(t_legacy, px, py, pz, div, c);
        if (!same(a, b) || !same(a, c)) {
            if (badn < 10) printf("MISMATCH %s beam %zu (%.17g, %.17g, %.17g): flakes met %d / %d / %d, lists %d / %d / %d\n", name, j, (double)px, (double)py, (double)pz,
                                  a.out.n_hits, b.out.n_hits, c.out.n_hits, a.L, b.L, c.L);
            ++badn;
        }
        if (a.out.n_hits & SG_HITS_UNDECIDED) ++undecided;
        if (a.L > 0) ++with_flakes;
        if (a.out.overflow) ++full;
        if (!(a.theta_c == a.theta_c)) continue;
        double th_r, th_l;
        sg_beam_limits(a.theta_c, div, th_r, th_l);
        const int b_lo = sg_bin_of(th_r - SG_BEAM_MARGIN, t_fine.inv_bin_w, SG_NBINS), b_hi = sg_bin_of(th_l + SG_BEAM_MARGIN, t_fine.inv_bin_w, SG_NBINS);
        if (b_lo == SG_NBINS - 1 && b_hi != SG_NBINS - 1) ++seam;
        if (seen && f.has_qs) {
            // what the fine scan dropped in the first bin: candidates (the upper count of the target's step) less the records nearer than the target
            T d_t; memcpy(&d_t, a.d_t, sizeof(T));
            const double d = (double)d_t;
            if (!(d == d)) continue;
            const double dq = d * (1.0 / FM);
            const int kk = dq < (double)(FS - 1) ? (int)dq : FS - 1;
            const uint32_t cand = f.qs_fine[(size_t)kk * SG_QS_ROW(SG_NBINS) + b_lo] >> 16;
            uint32_t near = 0;
            for (uint32_t e = f.start[b_lo]; e < f.start[b_lo + 1]; ++e) near += f.entries[e].rho < d;
            const long dropped = (long)cand - (long)near;
            if (dropped > seen->dropped_run) seen->dropped_run = dropped;
            // five or more flakes met, candidates of the first bin dropped, and a flake of the second bin alone in the list or in the
            // overflow slot (by its range): the dropped ones lay between them in scan order
            const int b_nx = b_lo + 1 == SG_NBINS ? 0 : b_lo + 1;
            const int hits = a.out.n_hits & ~SG_HITS_UNDECIDED;
            bool second = false;
            for (int i = 0; i < hits && i < SG_OV_CAP; ++i) {
                if (i >= a.L && i < 4) continue;
                const double r = i < 4 ? a.rho[i] : a.ov[2 + 3 * i + 2];
                for (uint32_t e = f.start[b_nx]; e < f.start[b_nx + 1]; ++e) second = second || ((f.entries[e].flags & 1u) && f.entries[e].rho == r);
            }
            if (b_hi != b_lo && hits >= 5 && dropped > 0 && second) ++seen->interleaved;
        }
    }
    printf("fine<%s, %s> %s (%s): %zu beams, %ld mismatches; %ld with flakes, %ld beyond the list, %ld across the seam, %ld undecided\n",
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
    const long n = argc > 1 ? atol(argv[1]) : 3000;
    const double bd = 0.1718873385392;
    std::mt19937_64 rng(78);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long bad = 0;
    const std::vector<Beam> beams = make_beams(n, 9);
    printf("step-major index filed: %d steps of %g m\n", FS, FM);

    {   // random, as dense as a bench table
        std::vector<double> xyr;
        for (int i = 0; i < 18000; ++i) add_flake(xyr, 1.0 + 129.0 * std::sqrt(U(rng)), U(rng) * SG_TWO_PI, 0.01 * (0.3 + 1.4 * U(rng)));
        Filed f;
        bad += file_table(xyr, f);
        bad += run<float, true>("random", f, beams, bd);
        bad += run<double, true>("random", f, beams, bd);
        bad += run<float, false>("random", f, beams, bd);
        bad += run<double, false>("random", f, beams, bd);
    }
    {   // sparse: flakes on and next to the four axes only; records at exact ranges and beside them; 110 records between 10 and 12 m in the
        // last bin and 110 in bin 0, each flake inside its bin (a beam across the seam meets them once each, bin after bin)
        std::vector<double> xyr;
        for (int a = 0; a < 4; ++a) {
            const double phi0 = a * (SG_PI / 2);
            for (double rho : EXACT) {
                add_flake(xyr, rho, phi0, 0.02);
                add_flake(xyr, std::nextafter(rho, 0.0), phi0, 0.02);
                add_flake(xyr, std::nextafter(rho, 1e9), phi0, 0.02);
                add_flake(xyr, rho, phi0, 0.005);                                       // an equal range: the order inside the bin is by table row
            }
            for (int i = 0; i < 60; ++i) add_flake(xyr, 0.6 + 135.0 * U(rng), phi0 + (U(rng) - 0.5) * 0.012, 0.004 + 0.02 * U(rng));
        }
        for (int i = 0; i < 110; ++i) {
            add_flake(xyr, 10.0 + 2.0 * (i + 0.25) / 110.0, SG_TWO_PI - 0.0004 - 0.0006 * U(rng), 0.002);
            add_flake(xyr, 10.0 + 2.0 * (i + 0.75) / 110.0, 0.0004 + 0.0006 * U(rng), 0.002);
        }
        Filed f;
        bad += file_table(xyr, f);
        long empty = 0, crowded = 0;
        for (int b = 0; b < SG_NBINS; ++b) empty += f.start[b] == f.start[b + 1];
        const int k10 = (int)(10.0 / FM);                       // the step that holds 10 m
        for (int b : {0, SG_NBINS - 1}) {
            uint32_t in_step = 0;
            for (uint32_t e = f.start[b]; e < f.start[b + 1]; ++e) in_step += f.entries[e].rho >= FM * k10 && f.entries[e].rho < FM * (k10 + 1);
            crowded += in_step >= 100;
        }
        if (empty < SG_NBINS / 2 || crowded != 2) { printf("sparse table: %ld empty bins, %ld seam bins with 100 records in a step -- not the case meant\n", empty, crowded); ++bad; }
        Seen seen;
        bad += run<float, true>("sparse", f, beams, bd, &seen);
        bad += run<double, true>("sparse", f, beams, bd, &seen);
        bad += run<float, false>("sparse", f, beams, bd);
        bad += run<double, false>("sparse", f, beams, bd);
        printf("sparse: longest run of dropped candidates %ld, beams with five flakes or more and dropped candidates between them %ld\n", seen.dropped_run, seen.interleaved);
        if (seen.dropped_run <= 64 || seen.interleaved == 0) { printf("sparse table: the dropped candidates are not the case meant\n"); ++bad; }
    }
    {   // an empty table
        Filed f;
        bad += file_table(std::vector<double>(), f);
        bad += run<float, true>("empty", f, beams, bd);
        bad += run<double, false>("empty", f, beams, bd);
    }
    {   // a bin of more than 65 535 records: its counts do not fit 16 bits, no step-major index is filed, the scan searches from bin_q
        std::vector<double> xyr;
        for (int i = 0; i < 66000; ++i) add_flake(xyr, 2.0 + 130.0 * U(rng), 0.0010 + 0.0008 * U(rng), 0.0005);
        for (int i = 0; i < 2000; ++i) add_flake(xyr, 2.0 + 130.0 * U(rng), U(rng) * SG_TWO_PI, 0.01);
        Filed f;
        bad += file_table(xyr, f);
        if (f.max_bin <= SG_QS_MAX_BIN || f.has_qs || f.desc(1).bin_qs != nullptr) {
            printf("long-bin table: longest bin %u, step-major index filed: %d -- expected none\n", f.max_bin, (int)f.has_qs);
            ++bad;
        }
        const std::vector<Beam> few = make_beams(n / 8, 6);
        bad += run<float, true>("long bin", f, few, bd);
        bad += run<double, false>("long bin", f, few, bd);
    }
    return bad != 0;
}
