// Host probe (no GPU): what the scan pays for taking every record below the UPPER count of the target's step of the step-major range index as a
// candidate instead of searching for the records nearer than the target (csrc/sg_range_index.h, sg_beam.h: sg_wave_scan), as a function of
// the step length -- on a bench table and the rows of a bench sweep, first two bins of every beam (the ones the wave's pair loop takes).
// Per step length: the trips of the search it replaces (per wave of 64 consecutive rows: ceil(log2(longest bracket + 1))), the pairs per
// beam with the search and without, and the trips of the pair loop per wave (ceil(pairs of the wave / 64)) with and without.
//   python: bench.make_tables(...)[0] -> table.bin (K x 3 float64), bench.make_frame(...)[:, :3] -> rows.bin (N x 3 float32)
//   hipcc --cuda-host-only -x hip -O2 -std=c++17 -I lidar_snow_sim_amd/csrc -I include scripts/probe/range_step_probe.cpp -o probe && ./probe table.bin rows.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#include <cmath>
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
#include "sg_beam.h"
#include "sg_table_host.h"

static std::vector<char> slurp(const char *p) { FILE *f = fopen(p, "rb"); std::vector<char> b; if (!f) return b; fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); b.resize((size_t)n); if (fread(b.data(), 1, (size_t)n, f) != (size_t)n) b.clear(); fclose(f); return b; }

static int ceil_log2(uint32_t v) { int t = 0; while ((1u << t) < v) ++t; return t; }      // ceil(log2(v)), v >= 1

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::vector<char> tb = slurp(argv[1]), rb = slurp(argv[2]);
    const int64_t K = (int64_t)(tb.size() / 24), N = (int64_t)(rb.size() / 12);
    const double *xyr = (const double *)tb.data();
    const float *rows = (const float *)rb.data();
    std::vector<SgEntry> entries;
    std::vector<uint32_t> start;
    uint32_t max_bin = 0;
    int64_t bad = -1;
    if (sg_file_table_host(xyr, K, entries, start, max_bin, &bad)) { printf("filing failed\n"); return 1; }
    const double div = 0.1718873385392;
    const struct { int steps; double m; } shapes[] = {{16, 8.0}, {32, 4.0}, {64, 2.0}};
    for (const auto &sh : shapes) {
        std::vector<uint32_t> qs(SG_QS_WORDS_OF(sh.steps, SG_NBINS));
        for (int b = 0; b < SG_NBINS; ++b)
            for (int k = 0; k < sh.steps; ++k) sg_range_index_fill_steps(entries.data(), start.data(), SG_NBINS, b, k, sh.steps, sh.m, nullptr, qs.data());
        double pairs = 0, cands = 0, beams = 0, waves = 0, search_trips = 0, loop_trips = 0, loop_trips_ns = 0;
        for (int64_t w0 = 0; w0 < N; w0 += 64) {
            uint32_t bracket = 0, wp = 0, wc = 0;
            for (int64_t i = w0; i < w0 + 64 && i < N; ++i) {
                float d_t;
                const SgBeamGeo g = sg_beam_geometry<float>(rows[3 * i], rows[3 * i + 1], rows[3 * i + 2], div, false, d_t);
                if (!(g.d == g.d)) continue;
                const int nb = SG_NBINS;
                const int b_lo = sg_bin_of(g.theta_r - SG_BEAM_MARGIN, SG_NBINS / SG_TWO_PI, nb), b_hi = sg_bin_of(g.theta_l + SG_BEAM_MARGIN, SG_NBINS / SG_TWO_PI, nb);
                int span = b_hi - b_lo; if (span < 0) span += nb;
                const double dq = g.d * (1.0 / sh.m);
                const int kk = dq < (double)(sh.steps - 1) ? (int)dq : sh.steps - 1;
                for (int s = 0; s <= span && s < 2; ++s) {
                    const int b = (b_lo + s) % nb;
                    const uint32_t word = qs[(size_t)kk * SG_QS_ROW(nb) + b], lo = word & 0xffffu, hi = word >> 16;
                    const uint32_t near = sg_bin_count_below(entries.data(), start[b], start[b + 1], g.d);
                    wp += near; wc += hi;
                    if (hi - lo > bracket) bracket = hi - lo;
                }
                beams += 1;
            }
            pairs += wp; cands += wc; waves += 1;
            search_trips += ceil_log2(bracket + 1);
            loop_trips += (wp + 63) / 64; loop_trips_ns += (wc + 63) / 64;
        }
        printf("%2d steps of %g m: search trips per wave %.2f; pairs per beam %.3f with the search, %.3f without (%+.1f %%); pair-loop trips per wave %.2f -> %.2f\n",
               sh.steps, sh.m, search_trips / waves, pairs / beams, cands / beams, 100.0 * (cands / pairs - 1.0), loop_trips / waves, loop_trips_ns / waves);
    }
    return 0;
}
