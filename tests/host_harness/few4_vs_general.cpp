// Host harness: the register path of k_power_few<T, 4> (lidar_snow_sim_amd/csrc/sg_few.h with N = 4: sg_few_prep + sg_few_zone + sg_few_bin)
// against the general per-lane path (sg_beam.h: sg_beam_dict + sg_beam_amp + sg_lane_power) for beams with one to four flakes, bit for
// bit: S, every amplitude, range and bin window, the best sum, the arg-max bin, range_error and the packed record -- for float32 and
// float64 rows, on random beams from the generator of few_vs_general.cpp (wedges at azimuth 0 / 2 pi, shared endpoints, identical
// intervals, equal ranges) and on constructed lists in which ONE scatterer owns eight or nine elementary slots, where np.sum is NumPy's
// blocked pairwise sum and no longer a running sum (sg_math.h: SgNpSum).  Both paths are the kernels' own device functions compiled for
// the host (hipcc --cuda-host-only) -- no oracle, no GPU.
// Which route a sum took is judged by the harness' OWN restatement of compute_occlusion_dict (analyse(): sorted unique endpoints, owner per
// slot, NumPy's pairwise sum and a left-to-right sum of the same widths -- none of it shares code with sg_few.h or SgNpSum).  An eight-slot
// owner SHOWS the route when the two sums give amplitudes that differ in their bits; the scan over azimuths just left of azimuth 0 (angles
// of 1e-5 .. 4e-3 rad: the widths no longer share an ulp) must find such beams, and on them the register path must give the pairwise
// amplitude.  A NINE-slot owner cannot show it: ten distinct interval ends put both limit rays strictly inside its interval, its sum
// exceeds the wedge's width and the ratio is clipped to 1 whatever the order (asserted per case); for those the harness can only require
// that the branch leaves them equal to the general path.
// usage: few4_vs_general [cases per L]; prints the largest slot count per kind of owner; exit status 1 on any mismatch, if no eight-slot
// owner showed the pairwise route and matched, or if no nine-slot owner was met.  Built and run by tests/test_few4_math.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <random>
#include <cmath>
#include <vector>
#include <algorithm>
// host overloads of the device intrinsics the list cells use
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
struct { unsigned x = 0, y = 0, z = 0; } threadIdx_host;
#undef __device__
#define __device__
#include "sg_beam.h"
#include "sg_few.h"

static const double DIV = 0.1718873385392;       // beam divergence in degrees (3 mrad)
static SgLasers g_las;

struct Tally {
    long cases = 0, bad = 0, pairwise8 = 0, pairwise9 = 0, bins = 0;
    long shows8 = 0;                                            // eight-slot owners whose amplitude depends on the order of the sum, and matched the pairwise one
    long unclipped9 = 0;                                        // nine-slot owners with a ratio below 1 (never: see above)
    int max_nearest = 0, max_farther = 0, max_target = 0;       // largest slot count per kind of owner
    long s_hist[5] = {0, 0, 0, 0, 0};
};

// compute_occlusion_dict (simulation.py:252-295) restated for the slot sums alone: per flake j and for the hard target (index 4) the number
// of elementary slots, and the ratio clip(sum / delta, 0, 1) with np.sum (numpy/_core/src/umath/loops_utils.h.src: pairwise_sum) and with a
// left-to-right sum of the same widths.
struct Own { int n = 0; double pair = 0.0, run = 0.0; };
static double np_sum(const std::vector<double> &a)
{
    const size_t n = a.size();
    if (n < 8) { double res = 0.0; for (double v : a) res += v; return res; }
    double r[8];
    for (int k = 0; k < 8; ++k) r[k] = a[k];
    size_t i = 8;
    for (; i < n - (n % 8); i += 8) for (int k = 0; k < 8; ++k) r[k] += a[i + k];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}
static void analyse(double tc, int L, const double (&a1_in)[4], const double (&a2_in)[4], Own (&o)[5])
{
    double ra, la, a1[4], a2[4];
    sg_beam_limits(tc, DIV, ra, la);
    const bool wrap = ra > la;                                  // :260-263
    if (wrap) ra -= SG_TWO_PI;
    std::vector<double> e = {ra, la};
    for (int j = 0; j < L; ++j) {
        a1[j] = a1_in[j]; a2[j] = a2_in[j];
        if (wrap && a1[j] > a2[j]) a1[j] -= SG_TWO_PI;
        e.push_back(a1[j]); e.push_back(a2[j]);
    }
    std::sort(e.begin(), e.end());
    e.erase(std::unique(e.begin(), e.end()), e.end());          // :265
    std::vector<double> w[5];
    for (size_t i = 0; i + 1 < e.size(); ++i) {
        int own = 4;
        for (int j = L - 1; j >= 0; --j) if (a1[j] <= e[i] && e[i] < a2[j]) own = j;   // the nearest flake that covers the slot (:277-286)
        w[own].push_back(e[i + 1] - e[i]);
    }
    const double delta = DIV * (SG_PI / 180.0);
    auto clip = [](double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); };
    for (int t = 0; t < 5; ++t) {
        double run = 0.0;
        for (double v : w[t]) run += v;
        o[t].n = (int)w[t].size(); o[t].pair = clip(np_sum(w[t]) / delta); o[t].run = clip(run / delta);
    }
}
// a flake's amplitude from its ratio (simulation.py:137-146, :549), as both paths write it
static double amp_of(double ratio, double r, int ch)
{
    const double beta_0 = 1 * 1e-6 / SG_PI, i_snow = 0.9 * g_las.max_i[ch], ca_p0 = i_snow / beta_0;
    return (((ca_p0 * beta_0) * ratio) * sg_xsi(r)) / (r * r);
}

// One beam through both paths.  a1 / a2 / rho: L flakes near -> far (the scan's order).
template <typename T>
static bool check(T d_t, double tc, int L, const double (&a1)[4], const double (&a2)[4], const double (&rho)[4], int ch, Tally &t, const char *what)
{
    const double d = (double)d_t;
    // ---- general path, one lane
    double g_a1[8], g_a2[8], g_rho[8], g_ratio[8];
    for (int j = 0; j < L; ++j) { g_a1[j] = a1[j]; g_a2[j] = a2[j]; g_rho[j] = rho[j]; }
    SgBeamOut o1{};
    const int S1 = sg_beam_dict<4, 1>(L, tc, d, DIV, g_a1, g_a2, g_rho, g_ratio, 0, 0, nullptr, nullptr, nullptr);
    double best1 = 0.0; int k1 = 0;
    uint32_t rec1 = 0;
    if (S1 > 0) {
        sg_beam_amp<T, 4, 1>(d_t, S1, ch, &g_las, g_a1, g_a2, g_rho, g_ratio, 0, o1, 0);
        sg_lane_power<1, false, 4, 4>(S1, nullptr, g_a1, g_a2, g_rho, g_ratio, 0, best1, k1);
        sg_beam_decide(d, ch, &g_las, best1, k1, o1);
        rec1 = sg_pack_record(o1);
    }
    // ---- the register path
    SgBeamOut o2{};
    SgFew<4> P{};
    const int S2 = sg_few_prep<T, 4>(d, tc, L, a1, a2, rho, ch, &g_las, DIV, P, o2);
    double best2 = 0.0; int k2 = 0;
    uint32_t rec2 = 0;
    if (S2) {
        int ka[5], kb[5];
        sg_few_zone<4, 0>(P, 0.0, ka[0], kb[0]);
        sg_few_zone<4, 1>(P, 0.0, ka[1], kb[1]);
        sg_few_zone<4, 2>(P, 0.0, ka[2], kb[2]);
        sg_few_zone<4, 3>(P, 0.0, ka[3], kb[3]);
        sg_few_zone<4, 4>(P, 0.0, ka[4], kb[4]);
        for (int z = 0; z <= 4; ++z)
            for (int k = ka[z]; k <= kb[z]; ++k) {
                const double sm = sg_few_bin<false, 4>(P.amp, P.rho, P.k0, P.k1, P.tamp, P.d, P.tk0, P.tk1, k, nullptr);
                if (sm > best2 || (sm == best2 && k < k2)) { best2 = sm; k2 = k; }
                ++t.bins;
            }
        sg_beam_decide(P.d, ch, &g_las, best2, k2, o2);
        rec2 = sg_pack_record(o2);
    }
    bool ok = S1 == S2 && !memcmp(&best1, &best2, 8) && k1 == k2 && o1.range_error == o2.range_error && rec1 == rec2;
    if (ok && S1 > 0) {
        for (int s = 0; s <= S1 && ok; ++s) {                   // every scatterer of the dict, the hard target last
            const double amp = s < S1 ? P.amp[s] : P.tamp, r = s < S1 ? P.rho[s] : P.d;
            const int k0 = s < S1 ? P.k0[s] : P.tk0, k1w = s < S1 ? P.k1[s] : P.tk1;
            ok = !memcmp(&amp, &g_a1[s], 8) && k0 == sg_kp_k0(g_a2[s]) && k1w == sg_kp_k1(g_a2[s]);
            // (the general path keeps the hard target's range as the float64 d; so does SgFew)
            ok = ok && !memcmp(&r, &g_rho[s], 8);
        }
    }
    ++t.cases;
    ++t.s_hist[S2];
    // what the harness' own restatement says about the slots: counts, and whether the order of a sum shows
    Own own[5];
    analyse(tc, L, a1, a2, own);
    int most = 0, s_idx = 0;
    unsigned slots = 0;
    for (int j = 0; j <= 4; ++j) {
        const int c = own[j].n;
        slots |= (unsigned)c << (4 * j);
        int &m = j == 4 ? t.max_target : (j == 0 ? t.max_nearest : t.max_farther);
        if (c > m) m = c;
        if (c > most) most = c;
        if (j < 4 && c > 0) {
            if (c >= 8 && ok && S2 > s_idx) {
                const double want = amp_of(own[j].pair, rho[j], ch), other = amp_of(own[j].run, rho[j], ch);
                if (c == 9 && (own[j].pair < 1.0 || own[j].run < 1.0)) ++t.unclipped9;
                if (memcmp(&want, &other, 8)) {                 // the order of the sum shows in this flake's amplitude
                    if (!memcmp(&P.amp[s_idx], &want, 8)) { if (c == 8) ++t.shows8; }
                    else ok = false;
                }
            }
            ++s_idx;
        }
    }
    if (ok && s_idx != S2) ok = false;                          // (the restatement's dict has as many flakes as both paths')
    if (ok && most == 8) ++t.pairwise8;
    if (ok && most == 9) ++t.pairwise9;
    if (!ok) {
        if (t.bad < 10)
            printf("MISMATCH %s T=%s L=%d d=%.17g tc=%.17g slots=%05x: S %d/%d best %.17g/%.17g k %d/%d rec %08x/%08x range_error %d/%d\n", what,
                   sizeof(T) == 4 ? "f32" : "f64", L, d, tc, slots, S1, S2, best1, best2, k1, k2, rec1, rec2, o1.range_error, o2.range_error);
        ++t.bad;
    }
    return ok;
}

// the random beams of few_vs_general.cpp, with exactly L of up to four flakes
template <typename T>
static void run_random(int L, long n, unsigned long long seed, Tally &t)
{
    constexpr int N = 4;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    for (long it = 0; it < n; ++it) {
        const T d_t = (T)(3.0 + 100.0 * U(rng) * U(rng));
        const double d = (double)d_t;
        double tc = (double)(T)(U(rng) * SG_TWO_PI);
        if (it % 500 == 0) tc = (double)(T)(U(rng) * 0.002);
        if (it % 500 == 1) tc = (double)(T)(SG_TWO_PI - U(rng) * 0.002);
        double tr, tl; sg_beam_limits(tc, DIV, tr, tl);
        const double half = DIV / 2 * (SG_PI / 180.0);
        double a1[N], a2[N], rho[N];
        const double cluster = d * U(rng);
        for (int j = 0; j < N; ++j) {
            double c = tc + (U(rng) * 2.4 - 1.2) * half, w = half * (0.01 + 0.7 * U(rng) * U(rng));
            a1[j] = c - w; a2[j] = c + w;
            if (U(rng) < 0.3) a1[j] = tr;
            if (U(rng) < 0.3) a2[j] = tl;
            if (U(rng) < 0.1 && j > 0) a1[j] = a2[j - 1];       // shared endpoints
            if (U(rng) < 0.05 && j > 0) { a1[j] = a1[j - 1]; a2[j] = a2[j - 1]; }   // identical intervals
            if (a1[j] < 0) a1[j] += SG_TWO_PI;
            if (a2[j] < 0) a2[j] += SG_TWO_PI;
            if (a1[j] > SG_TWO_PI) a1[j] -= SG_TWO_PI;
            if (a2[j] > SG_TWO_PI) a2[j] -= SG_TWO_PI;
            const double u = U(rng);
            rho[j] = u < 0.4 ? d - 4.0 * U(rng) : (u < 0.7 ? cluster + 3.0 * U(rng) : d * U(rng));
            if (U(rng) < 0.05) rho[j] = d * std::sqrt(w / half) * (0.98 + 0.04 * U(rng));
            if (!(rho[j] > 0.05)) rho[j] = 0.05 + U(rng);
            if (!(rho[j] < d)) rho[j] = d * (0.999 - 0.0001 * j);
            if (U(rng) < 0.02 && j > 0) rho[j] = rho[j - 1];    // equal ranges
        }
        for (int i = 1; i < L; ++i)                              // near -> far, stable (the scan's order)
            for (int q = i; q > 0 && rho[q - 1] > rho[q]; --q) { std::swap(rho[q - 1], rho[q]); std::swap(a1[q - 1], a1[q]); std::swap(a2[q - 1], a2[q]); }
        check<T>(d_t, tc, L, a1, a2, rho, (int)(U(rng) * 64) & 63, t, "random");
    }
}

// Constructed lists.  Offsets are fractions of the wedge's width from the beam's azimuth; irregular, so that the order of a sum over
// the slot widths shows in its last bits.  An interval is taken as it is, NOT clipped to the limit rays: this is what lets one
// scatterer reach eight or nine slots with four flakes (sg_few.h), and the functions under test take any list.
template <typename T>
static void run_constructed(Tally &t)
{
    const double w = DIV * (SG_PI / 180.0);
    struct Fl { double lo, hi, rho; };
    auto beam = [&](const char *what, double az, std::vector<Fl> fl, int expect_most, int ch) {
        std::stable_sort(fl.begin(), fl.end(), [](const Fl &x, const Fl &y) { return x.rho < y.rho; });
        const T d_t = (T)60.0;
        const double tc = (double)(T)az;
        double a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0}, rho[4] = {0, 0, 0, 0};
        const int L = (int)fl.size();
        for (int j = 0; j < L; ++j) {
            a1[j] = az + fl[j].lo * w; a2[j] = az + fl[j].hi * w; rho[j] = fl[j].rho;   // (a flake lies where it lies: only the beam's azimuth is rounded to T)
            if (a1[j] < 0) a1[j] += SG_TWO_PI;                   // (geometry.py:26-27: angles in [0, 2 pi))
            if (a2[j] < 0) a2[j] += SG_TWO_PI;
            if (a1[j] >= SG_TWO_PI) a1[j] -= SG_TWO_PI;
            if (a2[j] >= SG_TWO_PI) a2[j] -= SG_TWO_PI;
        }
        Tally one;
        const bool ok = check<T>(d_t, tc, L, a1, a2, rho, ch, one, what);
        const int most = std::max(one.max_nearest, std::max(one.max_farther, one.max_target));
        if (ok && expect_most >= 0 && most != expect_most) {
            printf("CONSTRUCTION %s T=%s: the largest owner has %d slots, not %d\n", what, sizeof(T) == 4 ? "f32" : "f64", most, expect_most);
            ++one.bad;
        }
        t.cases += one.cases; t.bad += one.bad; t.pairwise8 += one.pairwise8; t.pairwise9 += one.pairwise9; t.bins += one.bins; t.shows8 += one.shows8; t.unclipped9 += one.unclipped9;
        t.max_nearest = std::max(t.max_nearest, one.max_nearest); t.max_farther = std::max(t.max_farther, one.max_farther);
        t.max_target = std::max(t.max_target, one.max_target);
        for (int s = 0; s < 5; ++s) t.s_hist[s] += one.s_hist[s];
    };
    // three small flakes inside the wedge, pairwise disjoint (endpoints -0.41 .. 0.43 w; the limit rays at -0.5 w and 0.5 w)
    const Fl in0{-0.41, -0.287, 21.3}, in1{-0.113, 0.071, 9.7}, in2{0.237, 0.43, 33.1};
    // azimuths: an ordinary one; one just left of azimuth 0 (angles of 0.16 .. 3.8 mrad: five binades); and one that puts azimuth 0 inside
    // the rightmost small flake: the wedge wraps, the spanning flake and that one straddle the 0 / 2 pi seam, the others lie left of it
    for (double az : {1.0, 2.0e-3, 0.35 * w}) {
        // the nearest flake spans the other three and both limit rays: nine slots
        beam("nearest9", az, {{-0.613, 0.587, 3.5}, in0, in1, in2}, 9, 3);
        // the second nearest does; the nearest, inside the wedge, takes one slot out of it: eight
        beam("second8", az, {{-0.613, 0.587, 12.5}, in0, in1, in2}, 8, 10);
        // the farthest does: it is left with the slots nobody nearer covers (2 gaps between the three + 2 up to the rays + 2 beyond them)
        beam("farthest6", az, {{-0.613, 0.587, 45.0}, in0, in1, in2}, 6, 17);
        // a byte-identical twin of the middle flake: the copy later in the list owns nothing
        beam("twin", az, {in0, in1, in1, in2}, -1, 24);
        beam("twin_nearest9", az, {{-0.613, 0.587, 3.5}, {-0.613, 0.587, 3.5}, in0, in2}, -1, 24);
        // a flake wholly behind a nearer one, at a middle range: owns nothing, S < L
        beam("hidden", az, {in0, in1, {-0.05, 0.03, 15.2}, in2}, -1, 31);
        // four disjoint flakes strictly inside the wedge: the hard target at its maximum of five slots
        beam("comb4", az, {in0, in1, in2, {-0.24, -0.17, 5.1}}, 5, 38);
        // three and two flakes under a nearest one that spans everything: seven and five slots (running sums)
        beam("nearest7", az, {{-0.613, 0.587, 3.5}, in0, in2}, 7, 45);
        beam("single", az, {in1}, -1, 46);
    }
    // Eight slots with a sum BELOW the wedge's width, so that its last bits reach the amplitude, at 301 azimuths just left of azimuth 0 in steps of
    // 1e-5 rad (angles from 1e-5 rad up: the widths stop being multiples of one ulp, and a running sum rounds where the pairwise sum does not):
    //   near8    the nearest flake from beyond the right limit ray to short of the left one, the other three inside it;
    //   second8  the second nearest spans both rays and the other three; the nearest takes a quarter of the wedge out of its middle, so its
    //            eight slots lie in two groups and their sum does not telescope.
    // The harness counts on how many of them the order of the sum shows in the amplitude (shows8); run_all() fails if on none.
    for (int i = 0; i <= 300; ++i) {
        const double az = 1.57e-3 + 1e-5 * i;
        beam("near8", az, {{-0.52, 0.45, 3.5}, in0, in1, in2}, 8, 3);
        beam("second8_apart", az, {{-0.52, 0.51, 12.5}, in0, {-0.15, 0.10, 9.7}, in2}, 8, 10);
    }
    // every flake inverted (right end beyond the left end, seen by a beam whose limits do not wrap: it covers nothing, simulation.py:284,
    // but its ends cut slots): all nine slots are the hard target's, which then has no flake left -- S = 0 on both paths
    beam("inverted4", 1.0, {{0.41, -0.387, 21.3}, {0.113, -0.071, 9.7}, {0.33, -0.23, 33.1}, {0.613, -0.587, 3.5}}, 9, 52);
    // ... and with one honest flake among them the target's sum of eight goes the pairwise way
    beam("inverted3", 1.0, {{0.41, -0.387, 21.3}, {0.113, -0.071, 9.7}, {0.33, -0.23, 33.1}, {-0.02, 0.05, 3.5}}, 8, 52);
}

template <typename T>
static long run_all(long n, const char *name)
{
    Tally t;
    for (int L = 1; L <= 4; ++L) {
        Tally r;
        run_random<T>(L, n, 4400 + 10 * L + sizeof(T), r);
        printf("few4<%s> L=%d: %ld cases, %ld mismatches; S histogram %ld %ld %ld %ld %ld; %.2f bins per beam; most slots: nearest %d farther %d target %d; pairwise sums that matched: %ld of eight, %ld of nine\n",
               name, L, r.cases, r.bad, r.s_hist[0], r.s_hist[1], r.s_hist[2], r.s_hist[3], r.s_hist[4], (double)r.bins / r.cases, r.max_nearest, r.max_farther,
               r.max_target, r.pairwise8, r.pairwise9);
        t.bad += r.bad;
    }
    Tally c;
    run_constructed<T>(c);
    printf("few4<%s> constructed: %ld cases, %ld mismatches; most slots: nearest %d farther %d target %d; pairwise sums that matched: %ld of eight, %ld of nine; "
           "eight-slot owners whose amplitude shows the order of the sum, all equal to the pairwise one: %ld; nine-slot owners with a ratio below 1: %ld\n", name,
           c.cases, c.bad, c.max_nearest, c.max_farther, c.max_target, c.pairwise8, c.pairwise9, c.shows8, c.unclipped9);
    long bad = t.bad + c.bad;
    if (c.shows8 == 0) { printf("few4<%s>: on no eight-slot owner does the order of the sum show: the pairwise route is not tested\n", name); ++bad; }
    if (c.pairwise9 == 0) { printf("few4<%s>: no owner with nine slots\n", name); ++bad; }
    if (c.unclipped9) { printf("few4<%s>: a nine-slot owner with a ratio below 1: the argument in the header is wrong\n", name); ++bad; }
    return bad;
}

int main(int argc, char **argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 300000;
    g_las.n = 64;
    for (int i = 0; i < 64; ++i) { g_las.max_i[i] = (i % 7 == 0) ? 230 : 255; g_las.min_i[i] = 0; g_las.focal_slope[i] = 0.001 * i; g_las.focal_offset[i] = 0.9; }
    long bad = 0;
    bad += run_all<float>(n, "f32");
    bad += run_all<double>(n, "f64");
    return bad != 0;
}
