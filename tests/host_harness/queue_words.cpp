// Host harness: the dict queue of the pass over all rows (csrc/sg_queue.h) -- one word per listed flake, resolved by the reader -- against what
// the scan handed over before: float64 planes of range, azimuth and (a1, a2, rho) per flake, the angles resolved by the writer (sg_hit_angles)
// and rho taken from the scan's list.  On a filed table, random beams (and beams aimed at azimuth 0, at record 0 of the table and at near, wide
// flakes) are scanned by sg_wave_scan_t with the one-word lists, as k_beams scans them; every beam is stored into a slot with the writer's
// functions and, once a whole run of slots is full, loaded and resolved with the readers' -- both sg_dq_resolve_all and sg_dq_resolve.
// Per beam (d, theta, L) and per flake (a1, a2, rho) must be the old hand-over's values bit for bit, for the layouts of the list capacities
// 4, 8, 16 and 63.  Also: slot addressing across a group boundary, and no two (slot, plane) cells share a word.
// usage: queue_words [beams]; exit status 1 on any mismatch or population the run failed to produce.  Built and run by tests/test_queue_words.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <random>
#include <cmath>
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
struct { unsigned x = 0, y = 0, z = 0; } threadIdx_host;
#undef __device__
#define __device__
#define SG_PAIR_WINDOW 1     /* a wave of one lane takes one pair per trip */
#include "sg_queue.h"
#include "sg_table_host.h"

constexpr int LIST = 4;          // the scan's list capacity (k_beams<T, 4, ..>)
constexpr int RUN = 192;         // slots filled before any is read: three groups, from slot 40 on -- the run crosses two group boundaries
constexpr int SLOT0 = 40;

struct Old { double plane[2 + 3 * LIST]; int L; };      // the old hand-over of one beam, in its plane order

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }

template <typename T>
static long run(long M, unsigned long long seed, int lmax, long (&pop)[12])
{
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const int K = 18000;
    const double div = 0.1718873385392;                 // 3 mrad
    std::vector<double> xyr((size_t)K * 3);
    for (int i = 0; i < K; ++i) {
        // one flake in sixty near the sensor: wider than the wedge there, so both limit rays cut them
        const double rho = i % 60 == 0 ? 1.0 + 3.0 * U(rng) : 1.0 + 79.0 * std::sqrt(U(rng)), phi = U(rng) * SG_TWO_PI;
        xyr[3 * i] = rho * std::cos(phi); xyr[3 * i + 1] = rho * std::sin(phi); xyr[3 * i + 2] = 0.01 * (0.3 + 1.4 * U(rng));
    }
    std::vector<SgEntry> entries;
    std::vector<uint32_t> start;
    uint32_t max_bin = 0;
    int64_t bad = -1;
    if (sg_file_table_host(xyr.data(), K, entries, start, max_bin, &bad)) { printf("table filing failed at row %lld\n", (long long)bad); return 1; }
    SgTable tab{};
    tab.entries = entries.data(); tab.bin_start = start.data(); tab.bin_q = nullptr;
    tab.n_bins = SG_NBINS; tab.n_entries = (uint32_t)start[SG_NBINS]; tab.inv_bin_w = SG_NBINS / SG_TWO_PI; tab.n_flakes = (uint32_t)K; tab.max_bin = max_bin;
    constexpr int H = sg_dq_hdr((int)sizeof(T));
    const int slot_words = sg_dq_slot_words(lmax, H);
    std::vector<uint64_t> qmem(((size_t)(SLOT0 + RUN + 64) * slot_words + 1) / 2);      // 8-byte aligned; (n + 64) slots' worth, as the library sizes it
    uint32_t *q = reinterpret_cast<uint32_t *>(qmem.data());
    std::vector<Old> old(RUN);
    long badn = 0;
    int filled = 0;
    auto check_run = [&]() {
        for (int i = 0; i < filled; ++i) {
            const int64_t slot = SLOT0 + i;
            const Old &o = old[i];
            double d, tc;
            sg_dq_load_header<T>(q, slot, lmax, d, tc);
            uint32_t w[LIST];
            for (int j = 0; j < LIST; ++j) w[j] = sg_dq_load_word<T>(q, slot, lmax, j);      // (beyond the list: whatever the cell holds)
            double th_r, th_l, a1[LIST], a2[LIST], rho[LIST];
            sg_beam_limits(tc, div, th_r, th_l);
            sg_dq_resolve_all<LIST>(w, o.L, tab.entries, th_r, th_l, a1, a2, rho);
            bool ok = same(d, o.plane[0]) && same(tc, o.plane[1]);
            for (int j = 0; ok && j < o.L; ++j) {
                double b1, b2, br;
                sg_dq_resolve(w[j], tab.entries, th_r, th_l, b1, b2, br);
                ok = same(a1[j], o.plane[2 + 3 * j]) && same(a2[j], o.plane[3 + 3 * j]) && same(rho[j], o.plane[4 + 3 * j]) &&
                     same(b1, a1[j]) && same(b2, a2[j]) && same(br, rho[j]) && same(sg_dq_rho(w[j], tab.entries), rho[j]);
            }
            if (!ok) { if (badn < 10) printf("MISMATCH slot %lld (list of %d)\n", (long long)slot, o.L); ++badn; }
        }
        filled = 0;
        for (size_t i = 0; i < qmem.size(); ++i) qmem[i] = 0xa5a5a5a5deadbeefull ^ (uint64_t)i * 0x9e3779b97f4a7c15ull;      // stale cells
    };
    check_run();
    for (long n = 0; n < M; ++n) {
        double d = 3.0 + 72.0 * U(rng), az = U(rng) * SG_TWO_PI, el = (U(rng) - 0.7) * 0.4;
        const int kind = (int)(n % 16);
        if (kind == 1) az = (U(rng) - 0.5) * 2.5e-3;                                         // wedges that straddle azimuth 0
        if (kind == 2) { az = entries[0].phi + (U(rng) - 0.5) * 1e-3; d = entries[0].rho + 1.0 + 40.0 * U(rng); el = 0.0; }   // record 0 of the table
        if (az < 0) az += SG_TWO_PI;
        const T px = (T)(d * std::cos(el) * std::cos(az)), py = (T)(d * std::cos(el) * std::sin(az)), pz = (T)(d * std::sin(el));
        double w_rho[LIST];
        alignas(8) uint32_t rec_store[LIST + 2];
        int w_cnt[64], w_key[LIST], w_st[2];
        SgBeamOut wo{};
        T d_t, theta_t;
        const int L = sg_wave_scan_t<T, LIST, 1, false, true, false>(true, px, py, pz, tab, div, reinterpret_cast<double *>(rec_store), nullptr, w_rho, w_cnt, w_key, w_st, 0,
                                                                     wo, d_t, theta_t, false, nullptr, 0);
        if (L == 0) { ++pop[0]; continue; }              // (an over-full list is handed over all the same here: the format does not care)
        // the old hand-over: the writer resolves
        Old &o = old[filled];
        o.L = L;
        o.plane[0] = (double)d_t; o.plane[1] = (double)theta_t;
        double th_r, th_l;
        sg_beam_limits((double)theta_t, div, th_r, th_l);
        if (th_r > th_l) ++pop[5];
        for (int j = 0; j < L; ++j) {
            sg_hit_angles(rec_store[j], tab.entries, th_r, th_l, o.plane[2 + 3 * j], o.plane[3 + 3 * j]);
            o.plane[4 + 3 * j] = w_rho[j];
            ++pop[6 + (rec_store[j] >> 30)];             // limit-ray bits: none, right, left, both
            if ((rec_store[j] & 0x3fffffffu) == 0u) ++pop[10];
        }
        ++pop[L];
        // the new one: the writer stores what its list holds
        const int64_t slot = SLOT0 + filled;
        sg_dq_store_header<T>(q, slot, lmax, d_t, theta_t);
        for (int j = 0; j < L; ++j) sg_dq_store_word<T>(q, slot, lmax, j, rec_store[j]);
        if (++filled == RUN) check_run();
    }
    check_run();
    printf("queue<%s, capacity %d, %d header word%s>: %ld beams, %ld mismatches\n", sizeof(T) == 4 ? "float32" : "float64", lmax, H, H == 1 ? "" : "s", M, badn);
    return badn;
}

// slots 63 and 64 lie in different groups; no two cells of `slots` slots share a word, none leaves the queue, and together they fill it
static long layout(int lmax, int hdr)
{
    const int slots = 256;
    const int64_t gw = 64 * (int64_t)sg_dq_slot_words(lmax, hdr), total = (slots / 64) * gw;
    long bad = 0;
    std::vector<int> owner((size_t)total, -1);
    for (int s = 0; s < slots; ++s)
        for (int p = 0; p < lmax + 2; ++p) {
            const int64_t c = sg_dq_cell(s, p, lmax, hdr);
            const int len = p < 2 ? hdr : 1;
            if (p < 2 && c % hdr != 0) ++bad;                                                  // a header cell is aligned to its length
            for (int k = 0; k < len; ++k) {
                if (c + k < 0 || c + k >= total || owner[(size_t)(c + k)] != -1) { ++bad; continue; }
                owner[(size_t)(c + k)] = s * 128 + p;
            }
        }
    for (int64_t i = 0; i < total; ++i) if (owner[(size_t)i] == -1) ++bad;
    for (int p = 0; p < lmax + 2; ++p) {
        const int len = p < 2 ? hdr : 1;
        if (sg_dq_cell(63, p, lmax, hdr) - sg_dq_cell(62, p, lmax, hdr) != len) ++bad;         // neighbours within a group
        if (sg_dq_cell(64, p, lmax, hdr) != gw + sg_dq_cell(0, p, lmax, hdr)) ++bad;           // slot 64 opens the second group
        if (sg_dq_cell(63, p, lmax, hdr) >= gw || sg_dq_cell(64, p, lmax, hdr) < gw) ++bad;
    }
    printf("layout<capacity %d, %d header word%s>: %ld faults\n", lmax, hdr, hdr == 1 ? "" : "s", bad);
    return bad;
}

int main(int argc, char **argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 100000;
    long bad = 0;
    long pop[12] = {0};
    const int caps[4] = {4, 8, 16, 63};
    for (int c = 0; c < 4; ++c) {
        bad += run<float>(c == 0 ? n : n / 4, 31 + c, caps[c], pop);
        bad += run<double>(c == 0 ? n : n / 4, 41 + c, caps[c], pop);
        bad += layout(caps[c], 1) + layout(caps[c], 2);
    }
    printf("populations: no flake %ld, lists of 1 / 2 / 3 / 4: %ld / %ld / %ld / %ld, wrapped wedges %ld, words with no / right / left / both limit-ray bits: "
           "%ld / %ld / %ld / %ld, words of record 0: %ld\n", pop[0], pop[1], pop[2], pop[3], pop[4], pop[5], pop[6], pop[7], pop[8], pop[9], pop[10]);
    for (int i = 1; i <= 10; ++i)
        if (pop[i] == 0) { printf("population %d is empty\n", i); bad += 1; }
    return bad != 0;
}
