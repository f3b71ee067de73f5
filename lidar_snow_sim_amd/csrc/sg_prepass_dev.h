// sg_prepass_dev.h -- device types and helpers shared by the noise-threshold prepass (snowgpu_prepass.hip) and the wet-ground
// model (snowgpu_wet.hip): the per-frame record and the argument block of their kernels, fixed-order reductions, the histogram's
// binning, NumPy's float32 leaf sum, the small regression -- and the few host functions of snowgpu_prepass.hip that the wet-ground
// file calls (the scratch pool; the two kernels both chains run, which are launched from the file that defines them).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "sg_common.h"
#include "sg_prepass.h"
#include "sg_lean.h"
#include "sg_weather.h"

#define PB 256
#define HX 50     /* range rows of the histogram (augmentation.py:232) */
#define HY 2555   /* normalised-intensity bins */

struct PreFrame {          // per-frame state shared by the kernels
    double n_ground;       // ground rows
    double xmean, ymean;   // mean range / mean normalised intensity
    double xmean32;        // np.mean of the float32 range column as NumPy computes it (float32 pairwise sum)
    double ymax;           // max normalised intensity (histogram range, augmentation.py:233)
    double p0, p1;         // linregress(dist, normalised)            augmentation.py:216-219
    double pmin0, pmin1;   // noise line                              augmentation.py:248-251
    double poly[3];        // simulation.py:467
    // wet model, estimation_method = 'poly' (augmentation.py:223-229, :243-246): quadratics in range instead of the two lines
    double pq[3];          // np.polyfit(dist, normalised, 2)
    double mq[3];          // ransac_polyfit(x, min_vals, order=2)
    int32_t rows_done;     // lean chain: histogram rows whose minimum has been taken (k_lean_rowmin_solve: the block that completes the frame fits its lines)
    int32_t quad;          // 1: k_wet_apply evaluates pq / mq
    int32_t ransac_trial;  // the trial whose consensus refit was kept (-1: the fit over all points)
    int32_t unchanged;     // wet path: 1 = < 1000 ground rows (augmentation.py:51-52), 2 = the frame's wet gate is off (PreArgs::weather)
    int32_t need_mean32;   // float32 rows and the noise line falls back to p (augmentation.py:250-251)
    // lean snowfall prepass (k_lean_*): centred second moments of (range, I / cos) and the sums of the quadratic fit
    double sxx, sxy;
    double q[11];          // LQ_* below
};
// (LQ_* : the sums of the quadratic fit, LP_* : the per-tile partials -- sg_lean.h)

struct PreArgs {
    const void *rows;
    const void *srows;          // optional (snowfall prepass): the channel sort's sorted copy of the frames that came unsorted ...
    const int32_t *frame_unsorted;   // ... and which frames those are (sg_common.h: SgBeamArgs)
    const int64_t *frame_off;
    const int64_t *frame_cnt;   // optional: rows actually present in frame f (compacted input); else off[f+1] - off[f]
    int n_frames;
    int64_t max_tiles;
    const double *plane;   // n_frames x 4
    double delta;          // ground band half width (0.5 in the snowfall path)
    int flat_earth;        // wet: incident angle from -z (augmentation.py:61-63)
    int cos_only;          // snowfall prepass: only cos(incident angle) is ever used -> g_ang holds the cosine itself and
                           // cos(arccos(c)) is taken as c (a relative difference of ~1e-16, far inside the prepass tolerance);
                           // saves an acos and two cos per ground row
    int rows_as_f64;       // wet: np.hstack with the float64 height column promotes the ground rows to float64
                           // (augmentation.py:50), so range / mean are float64 whatever the input dtype
    double noise_floor, power_factor;
    const double *lines_override;   // optional n_frames x 4 (p slope, p intercept, noise-line slope, intercept): replaces the two fitted lines
    double *qpart;         // estimation_method = 'poly': per tile the 8 sums of the quadratic fit of (range, I / cos)
    uint64_t seed;         // ... and the seed of its RANSAC draws
    // per-row scratch (n_total)
    double *g_dist, *g_norm, *g_ang;   // range, I / cos(angle), incident angle (or its cosine: cos_only); g_norm = NaN for non-ground rows
    // per-tile partials: [frame][tile][k]
    double *part;          // 12 doubles per tile
    int32_t *hist;         // [frame][HX][HY]
    double *rowmin;        // [frame][HX]  yedges[argmin] or -1
    float *cdist;          // ground ranges compacted in row order (float32 rows only)
    PreFrame *fr;
    int32_t *status;
    const uint8_t *keep;   // optional (aligned wet stage), indexed like the rows: 0 = the row is not there (an earlier stage removed it) and
                           // k_pre_ground<T, true> takes it for a non-ground row; NULL: every row is present
    const double *weather; // optional n_frames x SG_WEATHER_REC (sg_weather.h): per-frame gates and wet settings in DEVICE memory.  The wet stage
                           // reads delta, noise_floor and power_factor there instead of above and skips a frame whose wet gate is 0
                           // (fr.unchanged = 2); the snowfall prepass reports no missing ground for a frame whose snow gate is 0
};

__device__ __forceinline__ int64_t pre_rows(const PreArgs &a, int f)
{
    return a.frame_cnt ? a.frame_cnt[f] : a.frame_off[f + 1] - a.frame_off[f];
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o));
    return v;
}
// block reduction of K values in a fixed order: lanes -> waves -> wave 0
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double *smem /* 4*K */)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) for (int k = 0; k < K; ++k) smem[w * K + k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < K; ++k) v[k] = ((smem[k] + smem[K + k]) + smem[2 * K + k]) + smem[3 * K + k];
}

// One wave per frame: lane l sums tiles l, l + 64, ... in order, then the 64 lane totals are combined by a fixed
// shuffle tree -- deterministic, and ~64x shorter than one thread walking every tile.
template <int K>
__device__ __forceinline__ void frame_sums(const double *part, int64_t tiles, const int (&col)[K], double (&out)[K])
{
    const int lane = threadIdx.x & 63;
    for (int k = 0; k < K; ++k) out[k] = 0.0;
    for (int64_t t = lane; t < tiles; t += 64)
        for (int k = 0; k < K; ++k) out[k] += part[t * 12 + col[k]];
    for (int k = 0; k < K; ++k) {
        for (int o = 32; o > 0; o >>= 1) out[k] += __shfl_xor(out[k], o);
    }
}

// searchsorted(edges, v, side='right') - 1 on edges = linspace(lo, hi, nb + 1), last edge inclusive
// (np.histogramdd).  Edge k is k * step + lo, the last one exactly hi.
__device__ __forceinline__ int hist_bin(double v, double lo, double hi, int nb)
{
    if (!(v >= lo) || !(v <= hi)) return -1;
    const double step = (hi - lo) / nb;
    int k = (int)floor((v - lo) / step);
    if (k < 0) k = 0;
    if (k > nb) k = nb;
    // settle against the edge values NumPy compares with
    while (k > 0 && !(((k == nb) ? hi : (double)k * step + lo) <= v)) --k;
    while (k < nb && (((k + 1 == nb) ? hi : (double)(k + 1) * step + lo) <= v)) ++k;
    if (k >= nb) k = nb - 1;                                             // v == last edge
    return k;
}

// ---- P2b/P2c (float32 rows): np.mean(range) exactly as NumPy computes it ----------------------------------------
// scipy.stats.linregress uses np.mean(x) of the float32 range column for the intercept (augmentation.py:216);
// NumPy sums float32 with its pairwise scheme (blocks of <= 128 values, 8 interleaved accumulators, halves split
// at a multiple of 8) and divides in float32.  On frames where the laser-power line nearly cancels that rounding
// is visible in the rewritten intensities, so it is reproduced operation for operation: the ground ranges are
// first compacted in row order, then one block per frame walks NumPy's recursion.
__device__ __forceinline__ float np_leaf_sum_f32(const float *v, int n)     // n <= 128
{
    if (n < 8) {
        float res = -0.0f;
        for (int i = 0; i < n; ++i) res += v[i];
        return res;
    }
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = v[j];
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += v[i + j];
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += v[i];
    return res;
}

// linregress(x, y) for a handful of points: slope = cov / var, intercept = ymean - slope * xmean
__device__ __forceinline__ void small_linregress(const double *x, const double *y, int n, double &slope, double &icpt)
{
    double xm = 0, ym = 0;
    for (int i = 0; i < n; ++i) { xm += x[i]; ym += y[i]; }
    xm /= n; ym /= n;
    double sxx = 0, sxy = 0;
    for (int i = 0; i < n; ++i) { sxx += (x[i] - xm) * (x[i] - xm); sxy += (x[i] - xm) * (y[i] - ym); }
    slope = (sxy / n) / (sxx / n);
    icpt = ym - slope * xm;
}

// ================================================================================================================
// host side: defined in snowgpu_prepass.hip, called from snowgpu_wet.hip too

// buffers of the scratch pool (SgPrepassScratch)
enum { B_GDIST = 0, B_GNORM, B_GCOS, B_PART, B_HIST, B_ROWMIN, B_FRAME, B_CLS, B_NEWI, B_TCNT, B_TBASE, B_CDIST, B_LEAF, B_QPART, B_N };
static_assert(B_N <= 16, "SgPrepassScratch holds 16 buffers");

// buffer i of the pool holds at least `bytes` afterwards (grown with a quarter to spare); 0, or -1 on allocation failure
int sg_pre_ensure(SgPrepassScratch *s, int i, size_t bytes);
// k_pre_rowmin: the row minima of every frame's histogram
int sg_pre_launch_rowmin(const PreArgs &a, hipStream_t st);
// leaves of NumPy's pairwise float32 sum over a frame's ground ranges (they hold 65..128 values): B_LEAF holds n_frames x 3 x this many ints
static inline int pre_max_leaves(int64_t max_frame) { return (int)(max_frame / 64 + 8); }
// k_pre_mean32 (after a gather of the ground ranges into a.cdist; B_LEAF reserved): NumPy's float32 mean for the frames that asked for it,
// then -- thr_poly given -- their quadratic
int sg_pre_launch_mean32(SgPrepassScratch *s, const PreArgs &a, int64_t max_frame, double *thr_poly, hipStream_t st);
