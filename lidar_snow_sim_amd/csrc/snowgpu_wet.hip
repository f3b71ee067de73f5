// snowgpu_wet.hip -- the wet-ground model on gfx950, with the full per-frame estimator it starts from.
//
//   wet-ground augmentation   wet_ground/augmentation.py:25-161 + wet_ground/phy_equations.py:35-108
//   its estimate              wet_ground/augmentation.py:195-266 (estimate_laser_parameters: 'linear' and 'poly')
//
// The estimate: ground rows by plane distance, incident angle, I / cos(angle) against range, a least-squares line, a 50 x 2555
// (range x normalised intensity) histogram whose per-range-row sparsest occupied bin gives the noise line -- or the two quadratics of
// 'poly'.  estimate() keeps range, angle and I / cos of every ground row in float64 scratch arrays, because the per-row rewrite
// (k_wet_apply, k_wet_apply_aligned) needs them again.  Only sg_wet_run and sg_wet_run_aligned run it -- the second with the keep bytes
// of an earlier stage as a mask over the rows (k_pre_ground<T, true>) --; the snowfall path's noise threshold comes from the lean chain of
// snowgpu_prepass.hip, which keeps no per-row scratch.  The two kernels both chains run (k_pre_rowmin, k_pre_mean32) and the scratch
// pool are that file's and are reached through sg_prepass_dev.h.  Reductions run in a fixed order, as there.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <cstdlib>
#include "sg_common.h"
#include "sg_prepass.h"
#include "sg_prepass_dev.h"
#include "sg_philox.h"
#include "sg_math.h"
#include "sg_launch.h"

// ---- P1: ground rows, incident angle, normalised intensity; tile partials (count, sum x, sum y, max y) ------
// MASKED (the aligned wet stage: a.keep, one byte per row): a row whose byte is 0 is not there -- it is taken for a non-ground row, gets
// g_norm = NaN and adds nothing to the tile's count, sums or maximum; everything downstream keys off g_norm != g_norm.
template <typename T, bool MASKED>
__global__ __launch_bounds__(PB) void k_pre_ground(PreArgs a)
{
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const double *wr = a.weather ? a.weather + (int64_t)f * SG_WEATHER_REC : nullptr;
    if (wr && wr[SG_W_WET] == 0.0) {
        // The frame's wet gate is off: its rows are not looked at.  It leaves here as a frame without a ground row -- the state every later
        // kernel of the estimate already meets for an empty or fully masked frame -- and k_pre_means marks it (fr.unchanged = 2).
        for (int q = 0; q < 4; ++q) {
            const int64_t r = tile0 + q * PB + threadIdx.x;
            if (r < n) a.g_norm[base + r] = NAN;
        }
        if (threadIdx.x == 0) {
            double *o = a.part + ((int64_t)f * a.max_tiles + blockIdx.x) * 12;
            o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = -INFINITY;
        }
        return;
    }
    const double delta = wr ? wr[SG_W_DELTA] : a.delta;
    const double *pl = a.plane + 4 * f;
    const double w0 = pl[0], w1 = pl[1], w2 = pl[2], h = pl[3];
    const double wn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);              // np.linalg.norm(w)
    const T *rows = (const T *)a.rows;
    double v[3] = {0.0, 0.0, 0.0};
    double ymax = -INFINITY;
    T rx[4], ry[4], rz[4], ri[4];                // all loads of the tile in flight before the first use
    uint8_t present[4] = {1, 1, 1, 1};
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        const T *p = rows + (base + (r < n ? r : 0)) * 5;
        rx[q] = p[0]; ry[q] = p[1]; rz[q] = p[2]; ri[q] = p[3];
        if (MASKED) present[q] = a.keep[base + (r < n ? r : 0)];
    }
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        if (r >= n) continue;
        const T x = rx[q], y = ry[q], z = rz[q], inten = ri[q];
        const double dot = ((double)x * w0 + (double)y * w1) + (double)z * w2;   // np.matmul(pc[:, :3], w)
        const double hog = dot + h;
        double gn = NAN, gd = 0.0, ga = 0.0;
        if (hog < delta && hog > -delta && (!MASKED || present[q])) {   // simulation.py:450-451 / augmentation.py:46-47
            double nrm;
            if (sizeof(T) == 4 && !a.rows_as_f64) nrm = (double)sqrtf((float)((x * x + y * y) + z * z));   // float32 norm (simulation.py:455)
            else { const double xd = (double)x, yd = (double)y, zd = (double)z; nrm = sqrt((xd * xd + yd * yd) + zd * zd); }
            double c;
            if (a.flat_earth) c = -((double)z / (nrm * 1.0));            // augmentation.py:61-63
            else c = dot / (nrm * wn);                                   // simulation.py:454-455
            if (a.cos_only) {
                ga = fabs(c) <= 1.0 ? c : NAN;                           // arccos outside [-1, 1] is NaN in the reference too
                gn = (double)inten / ga;
            } else {
                ga = acos(c);
                gn = (double)inten / cos(ga);                            // augmentation.py:207
            }
            gd = nrm;                                                    // augmentation.py:208
            v[0] += 1.0; v[1] += gd; v[2] += gn;
            ymax = fmax(ymax, gn);
        }
        a.g_norm[base + r] = gn;                                         // NaN marks a non-ground row: range / angle are then never read
        if (gn == gn) { a.g_dist[base + r] = gd; a.g_ang[base + r] = ga; }
    }
    __shared__ double sm[12];
    __shared__ double smax[4];
    block_sum<3>(v, sm);
    ymax = wave_max(ymax);
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = ymax;
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = a.part + ((int64_t)f * a.max_tiles + blockIdx.x) * 12;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
        o[3] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    }
}

// ---- P2: per frame: counts, means, max ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pre_means(PreArgs a, int min_ground, int err_code)
{
    const int f = blockIdx.x;
    if (f >= a.n_frames) return;
    const int lane = threadIdx.x;
    const int64_t n = pre_rows(a, f);
    const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
    double *part = a.part + (int64_t)f * a.max_tiles * 12;
    // exclusive prefix of the per-tile ground counts (exact: integers), max of the per-tile maxima
    double run = 0.0, ym = -INFINITY;
    for (int64_t t0 = 0; t0 < tiles; t0 += 64) {
        const int64_t t = t0 + lane;
        const double c = t < tiles ? part[t * 12 + 0] : 0.0;
        if (t < tiles) ym = fmax(ym, part[t * 12 + 3]);
        double inc = c;                                          // inclusive scan across the wave
        for (int o = 1; o < 64; o <<= 1) { const double v = __shfl_up(inc, o); if (lane >= o) inc += v; }
        if (t < tiles) part[t * 12 + 6] = run + inc - c;         // ground rows in earlier tiles
        run += __shfl(inc, 63);
    }
    for (int o = 32; o > 0; o >>= 1) ym = fmax(ym, __shfl_xor(ym, o));
    const int cols[2] = {1, 2};
    double sums[2];
    frame_sums<2>(part, tiles, cols, sums);
    if (lane == 0) {
        const double c = run;
        PreFrame &fr = a.fr[f];
        fr.n_ground = c;
        fr.xmean = c > 0 ? sums[0] / c : 0.0;
        fr.ymean = c > 0 ? sums[1] / c : 0.0;
        fr.xmean32 = (double)(float)fr.xmean;   // refined by k_pre_mean32 when the value is actually used
        fr.need_mean32 = 0;
        fr.ymax = fabs(ym);                                              // np.abs(np.max(...)), augmentation.py:233
        fr.unchanged = 0;
        fr.quad = 0; fr.ransac_trial = -1;
        if (c < (double)min_ground) {
            if (err_code) atomicCAS(&a.status[0], 0, err_code);          // snowfall: TypeError in the reference (Q7)
            fr.unchanged = 1;                                            // wet: frame returned unchanged
        }
        if (a.weather && a.weather[(int64_t)f * SG_WEATHER_REC + SG_W_WET] == 0.0) fr.unchanged = 2;   // wet stage not asked: returned unchanged, too
    }
}

// ---- P2b (float32 rows): the ground ranges compacted in row order, for k_pre_mean32 (snowgpu_prepass.hip) -------------
__global__ __launch_bounds__(PB) void k_pre_gather(PreArgs a)
{
    const int f = blockIdx.y;
    if (!a.fr[f].need_mean32) return;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    __shared__ int wc[4][4];
    const int tid = threadIdx.x, wv = tid >> 6;
    const unsigned long long lt = (1ull << (tid & 63)) - 1ull;
    bool g[4];
    int pre[4];
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + tid;
        const double gn = r < n ? a.g_norm[base + r] : NAN;
        g[q] = gn == gn;
        const unsigned long long m = __ballot(g[q]);
        pre[q] = __popcll(m & lt);
        if ((tid & 63) == 0) wc[q][wv] = __popcll(m);
    }
    __syncthreads();
    int run = (int)a.part[((int64_t)f * a.max_tiles + blockIdx.x) * 12 + 6];
    for (int q = 0; q < 4; ++q) {
        int off = run;
        for (int ww = 0; ww < wv; ++ww) off += wc[q][ww];
        if (g[q]) a.cdist[base + off + pre[q]] = (float)a.g_dist[base + tile0 + q * PB + tid];
        run += wc[q][0] + wc[q][1] + wc[q][2] + wc[q][3];
    }
}

// ---- P3: centred second moments (np.cov inside linregress) + the 50 x 2555 histogram ----------------------------
__global__ __launch_bounds__(PB) void k_pre_moments(PreArgs a)
{
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const PreFrame fr = a.fr[f];
    double v[2] = {0.0, 0.0};
    int32_t *hist = a.hist + (int64_t)f * HX * HY;
    int key[4] = {-1, -1, -1, -1};
    double gnv[4], gdv[4];                       // all loads of the tile in flight before the first use
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        gnv[q] = r < n ? a.g_norm[base + r] : NAN;
    }
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        gdv[q] = gnv[q] == gnv[q] ? a.g_dist[base + r] : 0.0;
    }
    for (int q = 0; q < 4; ++q) {
        const double gn = gnv[q];
        if (gn != gn) continue;
        const double gd = gdv[q];
        const double dx = gd - fr.xmean, dy = gn - fr.ymean;
        v[0] += dx * dx; v[1] += dx * dy;
        const int bx = hist_bin(gd, 10.0, 70.0, HX);                     // augmentation.py:232-233
        const int by = hist_bin(gn, 5.0, fr.ymax, HY);
        if (bx >= 0 && by >= 0) key[q] = bx * HY + by;
    }
    // Neighbouring rows are neighbouring azimuths of one laser: same range, similar intensity -- most rows of a tile hit the
    // same few bins, and same-address atomics serialise in L2.  The tile's 1024 keys are first counted in an LDS hash table
    // (open addressing, 2048 slots), then every distinct bin is added to the frame's histogram once.  (Counting per wave
    // with a ballot loop, one round per distinct key, was three quarters of this kernel's instructions.)
    __shared__ int t_key[2048], t_cnt[2048];
    for (int i = threadIdx.x; i < 2048; i += PB) { t_key[i] = -1; t_cnt[i] = 0; }
    __syncthreads();
    for (int q = 0; q < 4; ++q) {
        const int k = key[q];
        if (k < 0) continue;
        unsigned slot = ((unsigned)k * 2654435761u) >> 21;
        for (;;) {
            const int prev = atomicCAS(&t_key[slot], -1, k);
            if (prev == -1 || prev == k) { atomicAdd(&t_cnt[slot], 1); break; }
            slot = (slot + 1) & 2047u;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += PB)
        if (t_key[i] >= 0) atomicAdd(&hist[t_key[i]], t_cnt[i]);
    __shared__ double sm[8];
    block_sum<2>(v, sm);
    if (threadIdx.x == 0) {
        double *o = a.part + ((int64_t)f * a.max_tiles + blockIdx.x) * 12;
        o[4] = v[0]; o[5] = v[1];
    }
}

// ---- P5: the two lines ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pre_lines(PreArgs a, int xmean_f32)
{
    const int f = blockIdx.x;
    if (f >= a.n_frames) return;
    PreFrame &fr = a.fr[f];
    const int64_t n = pre_rows(a, f);
    const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
    const int cols[2] = {4, 5};
    double mom[2];
    frame_sums<2>(a.part + (int64_t)f * a.max_tiles * 12, tiles, cols, mom);
    // min_vals > 5 (augmentation.py:238), x = centres of the surviving range rows (:240-241): the lanes fetch the 50 row minima in one round
    // and squeeze them, in row order, into LDS by a ballot (thread 0 reading them one after the other into scratch arrays: 37 us)
    __shared__ double xs[HX], ys[HX];
    const int lane = threadIdx.x;
    const double mv = lane < HX ? a.rowmin[(int64_t)f * HX + lane] : 0.0;
    const bool keep = lane < HX && mv > 5;
    const unsigned long long mask = __ballot(keep);
    if (keep) {
        const double xstep = (70.0 - 10.0) / HX;
        const double e0 = (double)lane * xstep + 10.0;
        const double e1 = (lane + 1 == HX) ? 70.0 : (double)(lane + 1) * xstep + 10.0;
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        xs[pos] = (e0 + e1) / 2; ys[pos] = mv;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int m = __popcll(mask);
    const double sxx = mom[0], sxy = mom[1];
    const double ng = fr.n_ground;
    double slope = 0, icpt = 0;
    if (ng >= 3) {
        slope = (sxy / ng) / (sxx / ng);                                 // scipy linregress: ssxym / ssxm
        // np.mean of a float32 column is a float32; the intercept is ymean - slope * xmean (augmentation.py:216)
        const double xm = xmean_f32 ? fr.xmean32 : fr.xmean;
        icpt = fr.ymean - slope * xm;
    }
    fr.p0 = slope; fr.p1 = icpt;
    if (m > 3) small_linregress(xs, ys, m, fr.pmin0, fr.pmin1);         // augmentation.py:248-249
    else { fr.pmin0 = slope; fr.pmin1 = icpt; fr.need_mean32 = xmean_f32; }   // :250-251
}

// The caller's lines instead of the fitted ones (snowgpu_set_wet_lines: a host that fits them with its own NumPy, quirk Q8).
__global__ void k_pre_override_lines(PreArgs a)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n_frames) return;
    PreFrame &fr = a.fr[f];
    fr.p0 = a.lines_override[4 * f]; fr.p1 = a.lines_override[4 * f + 1];
    fr.pmin0 = a.lines_override[4 * f + 2]; fr.pmin1 = a.lines_override[4 * f + 3];
    fr.need_mean32 = 0;
}

// ================================================================================================================
// estimation_method = 'poly' of the wet-ground model (augmentation.py:223-229, :243-246, ransac_polyfit :171-192).
// Laser power: np.polyfit(range, I / cos, 2) over the ground rows -- least squares, here through the normal equations in the
// centred and scaled variable u = (d - 60) / 60 (ranges live in [0, 120] m: the 3 x 3 system is then well conditioned in float64;
// NumPy scales the Vandermonde columns and solves by SVD -- same minimiser, agreement ~1e-12 relative).
// Noise level: ransac_polyfit(x, min_vals, order=2) over the <= 50 range rows of the histogram whose sparsest bin lies above 5 --
// fit over all points first; then k = 100 trials: n = 15 indices drawn with replacement, a quadratic through them, its inliers
// (|residual| < t = 0.1), and if there are more than d = 15 of them and more than f = 0.8 of all points a refit on the inliers,
// kept when its summed absolute residual over the inliers undercuts the best so far (the first fit's is summed over ALL points,
// as in the reference).  The reference draws from NumPy's process-global, unseeded generator (np.random.randint, :183), so two runs
// of the reference disagree; here trial t of frame f draws from Philox4x32-10 keyed by (seed; f, t): same cloud + same seed = same
// curve, on every run and GPU.  Parity is therefore unpinned by construction (DESIGN.md section 9 says how it is tested instead).
#define PQ_C 60.0
#define PQ_S 60.0
#define PQ_COLS 8      /* sum u^4, u^3, u^2, u, 1, u^2 y, u y, y */
#define RQ_N 15
#define RQ_K 100
#define RQ_T 0.1
#define RQ_D 15
#define RQ_F 0.8

// least-squares quadratic from the 8 sums in u; returns false for a singular system (fewer than 3 distinct abscissae)
__device__ __forceinline__ bool quad_solve_u(const double *q, double &c2, double &c1, double &c0)
{
    double G[3][4] = {{q[0], q[1], q[2], q[5]}, {q[1], q[2], q[3], q[6]}, {q[2], q[3], q[4], q[7]}};
    for (int i = 0; i < 3; ++i) {                                        // Gaussian elimination, partial pivoting
        int piv = i;
        for (int r = i + 1; r < 3; ++r) if (fabs(G[r][i]) > fabs(G[piv][i])) piv = r;
        if (piv != i) for (int k = 0; k < 4; ++k) { const double t = G[i][k]; G[i][k] = G[piv][k]; G[piv][k] = t; }
        if (!(fabs(G[i][i]) > 1e-13 * (fabs(q[0]) + fabs(q[4]) + 1.0))) return false;
        for (int r = i + 1; r < 3; ++r) {
            const double m = G[r][i] / G[i][i];
            for (int k = i; k < 4; ++k) G[r][k] -= m * G[i][k];
        }
    }
    double x[3];
    for (int i = 2; i >= 0; --i) {
        double t = G[i][3];
        for (int k = i + 1; k < 3; ++k) t -= G[i][k] * x[k];
        x[i] = t / G[i][i];
    }
    c2 = x[0]; c1 = x[1]; c0 = x[2];
    return true;
}
// y = c2 u^2 + c1 u + c0 with u = (d - C) / S, as coefficients of d (highest power first, np.polyfit's order)
__device__ __forceinline__ void quad_u_to_d(double c2, double c1, double c0, double *out)
{
    const double a = c2 / (PQ_S * PQ_S), b = c1 / PQ_S;
    out[0] = a;
    out[1] = b - 2.0 * a * PQ_C;
    out[2] = (a * PQ_C * PQ_C - b * PQ_C) + c0;
}
__device__ __forceinline__ double quad_eval_u(double c2, double c1, double c0, double u) { return (c2 * u + c1) * u + c0; }

__global__ __launch_bounds__(PB) void k_pre_quad_part(PreArgs a)
{
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    double v[PQ_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        const double gn = r < n ? a.g_norm[base + r] : NAN;
        if (gn != gn) continue;
        const double u = (a.g_dist[base + r] - PQ_C) * (1.0 / PQ_S), u2 = u * u;
        v[0] += u2 * u2; v[1] += u2 * u; v[2] += u2; v[3] += u; v[4] += 1.0; v[5] += u2 * gn; v[6] += u * gn; v[7] += gn;
    }
    __shared__ double sm[4 * PQ_COLS];
    block_sum<PQ_COLS>(v, sm);
    if (threadIdx.x == 0) {
        double *o = a.qpart + ((int64_t)f * a.max_tiles + blockIdx.x) * PQ_COLS;
        for (int k = 0; k < PQ_COLS; ++k) o[k] = v[k];
    }
}

// ransac_polyfit(x, y, order=2) (augmentation.py:171-192) by one block of 128 threads: the fit over all m points (every thread, same
// arithmetic), trial `tid` per thread, the reference's "first trial that reaches the smallest error" by thread 0.  xs / ys: the m <= 50
// points in shared memory.  Returns (thread 0 only) the coefficients in u = (x - PQ_C) / PQ_S and the winning trial (-1: the first fit).
__device__ __forceinline__ void ransac_quad_block(const double *xs, const double *ys, int m, uint64_t seed, uint64_t f, double *s_err,
                                                  double (*s_fit)[3], double &b2, double &b1, double &b0, int &win)
{
    const int tid = threadIdx.x;
    auto fit = [&](auto &&weight, double &c2, double &c1, double &c0) -> bool {     // least squares over the points with weight(i) copies
        double q[PQ_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < m; ++i) {
            const double w = weight(i);
            if (w == 0.0) continue;
            const double u = (xs[i] - PQ_C) * (1.0 / PQ_S), u2 = u * u, y = ys[i];
            q[0] += w * (u2 * u2); q[1] += w * (u2 * u); q[2] += w * u2; q[3] += w * u; q[4] += w; q[5] += w * (u2 * y); q[6] += w * (u * y); q[7] += w * y;
        }
        return quad_solve_u(q, c2, c1, c0);
    };
    // the fit over all points and its summed absolute residual (:179-180)
    double best_err = 0.0;
    b2 = 0; b1 = 0; b0 = 0;
    if (!fit([](int) { return 1.0; }, b2, b1, b0)) { b2 = 0.0; b1 = 0.0; double sy = 0; for (int i = 0; i < m; ++i) sy += ys[i]; b0 = sy / m; }
    for (int i = 0; i < m; ++i) best_err += fabs(quad_eval_u(b2, b1, b0, (xs[i] - PQ_C) * (1.0 / PQ_S)) - ys[i]);
    // trial `tid` (:182-191)
    double t_err = INFINITY, t2 = 0, t1 = 0, t0 = 0;
    if (tid < RQ_K) {
        unsigned char cnt[HX];
        for (int i = 0; i < HX; ++i) cnt[i] = 0;
        for (int d4 = 0; d4 < (RQ_N + 3) / 4; ++d4) {                    // n indices in [0, m), with replacement
            uint32_t u[4];
            philox_u32x4(seed, f, (uint32_t)(tid * 4 + d4), 0x504F4C59u /* "POLY" */, u);
            for (int k = 0; k < 4 && d4 * 4 + k < RQ_N; ++k) cnt[(int)(((uint64_t)u[k] * (uint64_t)m) >> 32)]++;
        }
        double m2, m1, m0;
        if (fit([&](int i) { return (double)cnt[i]; }, m2, m1, m0)) {
            unsigned long long inl = 0;
            int n_in = 0;
            for (int i = 0; i < m; ++i)
                if (fabs(quad_eval_u(m2, m1, m0, (xs[i] - PQ_C) * (1.0 / PQ_S)) - ys[i]) < RQ_T) { inl |= 1ull << i; ++n_in; }
            if (n_in > RQ_D && (double)n_in > (double)m * RQ_F && fit([&](int i) { return ((inl >> i) & 1ull) ? 1.0 : 0.0; }, t2, t1, t0)) {
                t_err = 0.0;
                for (int i = 0; i < m; ++i)
                    if ((inl >> i) & 1ull) t_err += fabs(quad_eval_u(t2, t1, t0, (xs[i] - PQ_C) * (1.0 / PQ_S)) - ys[i]);
            }
        }
    }
    s_err[tid] = t_err; s_fit[tid][0] = t2; s_fit[tid][1] = t1; s_fit[tid][2] = t0;
    __syncthreads();
    win = -1;
    if (tid == 0) {                                                      // the reference's loop keeps the FIRST trial that reaches the smallest error
        for (int t = 0; t < RQ_K; ++t)
            if (s_err[t] < best_err) { best_err = s_err[t]; win = t; }
        if (win >= 0) { b2 = s_fit[win][0]; b1 = s_fit[win][1]; b0 = s_fit[win][2]; }
    }
}

// One block of 128 threads per frame: the power quadratic from the tile sums (wave 0), the noise quadratic by RANSAC (one trial per thread).
__global__ __launch_bounds__(128) void k_pre_quad_fit(PreArgs a, int err_code)
{
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    PreFrame &fr = a.fr[f];
    if (fr.unchanged) return;
    __shared__ double xs[HX], ys[HX], s_err[128];
    __shared__ double s_fit[128][3];
    __shared__ int s_m;
    if (tid < 64) {                                                      // np.polyfit(dist, normalised, 2): fixed-order sums over the tiles
        const int64_t n = pre_rows(a, f);
        const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
        const double *part = a.qpart + (int64_t)f * a.max_tiles * PQ_COLS;
        double q[PQ_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t t = lane; t < tiles; t += 64)
            for (int k = 0; k < PQ_COLS; ++k) q[k] += part[t * PQ_COLS + k];
        for (int k = 0; k < PQ_COLS; ++k)
            for (int o = 32; o > 0; o >>= 1) q[k] += __shfl_xor(q[k], o);
        if (tid == 0) {
            double c2, c1, c0;
            if (quad_solve_u(q, c2, c1, c0)) quad_u_to_d(c2, c1, c0, fr.pq);
            else { fr.pq[0] = 0.0; fr.pq[1] = fr.p0; fr.pq[2] = fr.p1; }   // degenerate ranges: the regression line
            int m = 0;                                                   // min_vals > 5 (augmentation.py:238), x = centres of those range rows (:240-241)
            const double xstep = (70.0 - 10.0) / HX;
            for (int r = 0; r < HX; ++r) {
                const double mv = a.rowmin[(int64_t)f * HX + r];
                if (mv > 5) {
                    const double e0 = (double)r * xstep + 10.0;
                    const double e1 = (r + 1 == HX) ? 70.0 : (double)(r + 1) * xstep + 10.0;
                    xs[m] = (e0 + e1) / 2; ys[m] = mv; ++m;
                }
            }
            s_m = m;
        }
    }
    __syncthreads();
    const int m = s_m;
    if (m == 0) {                                                        // np.polyfit on an empty vector: TypeError in the reference (augmentation.py:179)
        if (tid == 0) { if (err_code) atomicCAS(&a.status[0], 0, err_code); fr.mq[0] = 0.0; fr.mq[1] = fr.pmin0; fr.mq[2] = fr.pmin1; fr.quad = 1; }
        return;
    }
    if (m < 3) {
        // One or two usable range rows: np.polyfit(x, y, 2) (:179) answers an under-determined system with the MINIMUM-NORM solution of its
        // column-scaled Vandermonde system (lstsq on lhs / sqrt(sum lhs^2), then c / scale) and a RankWarning; no RANSAC trial can replace
        // it (a consensus set needs more than d = 15 points, :187), so ransac_polyfit returns exactly that fit.  Columns x^2, x, 1.
        if (tid == 0) {
            double sc[3] = {0, 0, 0}, A[2][3];
            for (int i = 0; i < m; ++i) { const double x = xs[i]; sc[0] += (x * x) * (x * x); sc[1] += x * x; sc[2] += 1.0; }
            for (int k = 0; k < 3; ++k) sc[k] = sqrt(sc[k]);
            for (int i = 0; i < m; ++i) { const double x = xs[i]; A[i][0] = sc[0] > 0 ? x * x / sc[0] : 0.0; A[i][1] = sc[1] > 0 ? x / sc[1] : 0.0; A[i][2] = 1.0 / sc[2]; }
            double w[2] = {0, 0};
            if (m == 1) {
                const double g = A[0][0] * A[0][0] + A[0][1] * A[0][1] + A[0][2] * A[0][2];
                w[0] = ys[0] / g;
            } else {
                const double g00 = A[0][0] * A[0][0] + A[0][1] * A[0][1] + A[0][2] * A[0][2], g11 = A[1][0] * A[1][0] + A[1][1] * A[1][1] + A[1][2] * A[1][2];
                const double g01 = A[0][0] * A[1][0] + A[0][1] * A[1][1] + A[0][2] * A[1][2], det = g00 * g11 - g01 * g01;
                if (fabs(det) > 1e-14 * g00 * g11) { w[0] = (g11 * ys[0] - g01 * ys[1]) / det; w[1] = (g00 * ys[1] - g01 * ys[0]) / det; }
                else { w[0] = w[1] = 0.5 * (ys[0] + ys[1]) / (g00 + g01); }          // the same abscissa twice: rank one
            }
            for (int k = 0; k < 3; ++k) {
                double c = 0;
                for (int i = 0; i < m; ++i) c += A[i][k] * w[i];
                fr.mq[k] = sc[k] > 0 ? c / sc[k] : 0.0;
            }
            fr.quad = 1;
        }
        return;
    }
    double b2, b1, b0;
    int win;
    ransac_quad_block(xs, ys, m, a.seed, (uint64_t)f, s_err, s_fit, b2, b1, b0, win);
    if (tid == 0) { quad_u_to_d(b2, b1, b0, fr.mq); fr.quad = 1; fr.ransac_trial = win; }
}

// debug / parity tap: ransac_polyfit on the caller's points (m <= 50), draws of (seed; frame): out = c2, c1, c0 (coefficients of x), trial kept
__global__ __launch_bounds__(128) void k_debug_ransac_quad(const double *x, const double *y, int m, uint64_t seed, uint64_t frame, double *out)
{
    __shared__ double xs[HX], ys[HX], s_err[128];
    __shared__ double s_fit[128][3];
    for (int i = threadIdx.x; i < m; i += 128) { xs[i] = x[i]; ys[i] = y[i]; }
    __syncthreads();
    double b2, b1, b0;
    int win;
    ransac_quad_block(xs, ys, m, seed, frame, s_err, s_fit, b2, b1, b0, win);
    if (threadIdx.x == 0) { quad_u_to_d(b2, b1, b0, out); out[3] = (double)win; }
}

extern "C" int sg_debug_ransac_quad(const double *d_x, const double *d_y, int m, uint64_t seed, uint64_t frame, double *d_out, void *stream)
{
    hipLaunchKernelGGL(k_debug_ransac_quad, dim3(1), dim3(128), 0, (hipStream_t)stream, d_x, d_y, m, seed, frame, d_out);
    SG_CHECK_LAUNCH();
    return 0;
}

// the fitted curves of the last estimate, per frame: (power c2, c1, c0, noise c2, c1, c0, ground rows, RANSAC trial kept or -1);
// 'linear' frames report their lines as quadratics with c2 = 0
__global__ void k_pre_export_fit(PreArgs a, double *out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n_frames) return;
    const PreFrame &fr = a.fr[f];
    double *o = out + (int64_t)f * 8;
    if (fr.quad) { for (int k = 0; k < 3; ++k) { o[k] = fr.pq[k]; o[3 + k] = fr.mq[k]; } }
    else { o[0] = 0.0; o[1] = fr.p0; o[2] = fr.p1; o[3] = 0.0; o[4] = fr.pmin0; o[5] = fr.pmin1; }
    o[6] = fr.n_ground; o[7] = (double)fr.ransac_trial;
}

// ================================================================================================================
// wet ground (augmentation.py:88-159; phy_equations.py:35-108)

// phy_equations.py:35-67 fresnel_power(ain, n_in, n_out), from the sine and cosine of the incidence angle instead of the angle: the
// refraction angle only ever enters as its sine -- n_in / n_out sin(ain), clipped (:41-43) -- and its cosine, the root of 1 - sin^2
// (cos(arcsin(s)), :44-46), and the angle the chain hands on (total_transmittance, :81-83) is used the same way, so no arcsin, sine or
// cosine is taken here at all; the two amplitude pairs share their denominators' reciprocals, and `frac` (:47) enters as its reciprocal.
// The same numbers to a few 1e-16 (the wet path's intensities are float64 values compared at 1e-9 / 1e-7: tests/test_gpu_parity.py
// ::test_L6_wet_ground, test_gpu_fullsize.py) -- the library sin / arcsin / cos and 18 divisions per row were 0.88 ms of a fused
// 256-sweep step.
struct Fresnel { double rs, ts, rp, tp, s_out, c_out; };
__device__ __forceinline__ Fresnel fresnel_power(double si, double ci, double n_in, double n_out)
{
    Fresnel r;
    double s = si * n_in / n_out;                                    // :41
    s = s < -1 ? -1 : (s > 1 ? 1 : s);                               // :42-43
    const double co = sqrt(1.0 - s * s);                             // cos(aout), aout = arcsin(s) (:44-46)
    r.s_out = s; r.c_out = co;
    const double a = n_in * ci, b = n_out * co, c = n_out * ci, d = n_in * co;
    const double i1 = 1.0 / (a + b), i2 = 1.0 / (c + d);
    const double rs = (a - b) * i1, ts = 2 * a * i1;                 // :49-50
    const double rp = (c - d) * i2, tp = 2 * a * i2;                 // :51-52
    const double inv_frac = (n_out * co) / (ci * n_in);              // 1 / (cos(ain) n_in / n_out / cos(aout)) (:47)
    r.rs = rs * rs; r.ts = ts * ts * inv_frac; r.rp = rp * rp; r.tp = tp * tp * inv_frac;   // :54-57
    return r;
}

struct WetArgs {
    PreArgs p;
    double water_height, pavement_depth;
    int replace;
    uint8_t *cls;          // per row: 1 = non-ground, 2 = kept ground, 0 = dropped
    double *new_i;         // per row: rewritten intensity
    int32_t *tile_cnt;     // [frame][tile][2]
    int32_t *tile_base;    // [frame][tile][2]
    double *out_rows;
    int32_t *out_src;
    int64_t *out_counts;
    int32_t *out_flags;
    const int32_t *src_first;   // SgWetParams::src_first
};

// The per-row chain of a ground row (augmentation.py:90-131, :146) from its range, incidence angle and intensity and the frame's fitted curves:
// ni = what new_intensities holds after :131 (0 below the noise limit); returns whether the row is kept (:146).  Written down once for
// k_wet_apply (compact result) and k_wet_apply_aligned (aligned result).
struct WetFrame { double water_height, pavement_depth, noise_floor, power_factor; };     // the call's scalars, or the frame's weather record
__device__ __forceinline__ WetFrame wet_frame(const PreArgs &a, int f, double water_height, double pavement_depth)
{
    if (!a.weather) return WetFrame{water_height, pavement_depth, a.noise_floor, a.power_factor};
    const double *wr = a.weather + (int64_t)f * SG_WEATHER_REC;
    return WetFrame{wr[SG_W_WATER], wr[SG_W_PAVE], wr[SG_W_NOISE], wr[SG_W_POWER]};
}

__device__ __forceinline__ bool wet_row_chain(const WetFrame &wf, const PreFrame &fr, double gd, double ang, double inten, double &ni)
{
    double gs, gc;
    sg_sincos_0_2pi(ang, gs, gc);                                // the incidence angle lies in [0, pi] (an arccos)
    double rel, thr;
    if (fr.quad) {                                               // estimation_method = 'poly'
        const double gd2 = gd * gd;
        rel = wf.power_factor * ((fr.pq[0] * gd2 + fr.pq[1] * gd) + fr.pq[2]);        // :228-229
        thr = wf.noise_floor * ((fr.mq[0] * gd2 + fr.mq[1] * gd) + fr.mq[2]);         // :245-246
    } else {
        rel = wf.power_factor * (fr.p0 * gd + fr.p1);             // :221
        thr = wf.noise_floor * (fr.pmin0 * gd + fr.pmin1);        // :252-253
    }
    const double refl = inten / gc / rel;                        // :90
    double rho = refl < 0.05 ? 0.05 : (refl > 1 ? 1 : refl);     // :109 np.clip(reflectivities, 0.05, 1)
    const Fresnel aw = fresnel_power(gs, gc, 1.0003, 1.33);      // phy_equations.py:81
    const Fresnel wa = fresnel_power(aw.s_out, aw.c_out, 1.33, 1.0003);   // :83 (the angle inside the water)
    const double ts = aw.ts * rho * wa.ts / (1 - rho * wa.rs);   // :86
    const double tp = aw.tp * rho * wa.tp / (1 - rho * wa.rp);   // :89
    const double t = fmax(tp, ts);                               // augmentation.py:119
    double fw = wf.water_height / wf.pavement_depth;                  // :122
    fw = fw < 0 ? 0 : (fw > 1 ? 1 : fw);
    const double tw = (1 - fw) * refl + fw * t / ang;            // :123
    double v = rel * gc * tw;                                    // :126
    v = v < 0 ? 0 : (v > inten ? inten : v);                     // np.clip(., 0, intensity)
    const double lim = thr * gc;
    if (v < lim) v = 0;                                          // :128, :131
    ni = v;
    return v > lim;                                              // :146
}

template <typename T>
__global__ __launch_bounds__(PB) void k_wet_apply(WetArgs w)
{
    const PreArgs &a = w.p;
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const PreFrame fr = a.fr[f];
    const WetFrame wf = wet_frame(a, f, w.water_height, w.pavement_depth);
    const T *rows = (const T *)a.rows;
    int cnt_a = 0, cnt_b = 0;
    double gns[4], gds[4], angs[4], ins[4];                              // the thread's four rows side by side: every load first
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        const bool in = r < n && !fr.unchanged;
        gns[q] = in ? a.g_norm[base + r] : NAN;
        const bool ground = gns[q] == gns[q];
        gds[q] = ground ? a.g_dist[base + r] : 0.0;
        angs[q] = ground ? a.g_ang[base + r] : 1.0;
        ins[q] = ground ? (double)rows[(base + r) * 5 + 3] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        if (r >= n) continue;
        uint8_t cls;
        double ni = 0.0;
        const double gn = gns[q];
        if (fr.unchanged) { cls = 1; }                                   // frame returned as is (augmentation.py:51-52)
        else if (gn != gn) { cls = 1; }
        else cls = wet_row_chain(wf, fr, gds[q], angs[q], ins[q], ni) ? 2 : 0;
        w.cls[base + r] = cls;
        if (cls == 2) w.new_i[base + r] = ni;                            // (read back for kept ground rows only: k_wet_scatter)
        cnt_a += cls == 1; cnt_b += cls == 2;
    }
    __shared__ int sa[4], sb[4];
    for (int o = 32; o > 0; o >>= 1) { cnt_a += __shfl_down(cnt_a, o); cnt_b += __shfl_down(cnt_b, o); }
    if ((threadIdx.x & 63) == 0) { sa[threadIdx.x >> 6] = cnt_a; sb[threadIdx.x >> 6] = cnt_b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t *o = w.tile_cnt + ((int64_t)f * a.max_tiles + blockIdx.x) * 2;
        o[0] = sa[0] + sa[1] + sa[2] + sa[3];
        o[1] = sb[0] + sb[1] + sb[2] + sb[3];
    }
}

// per frame: tile offsets of the two output runs ([non-ground ; kept ground], augmentation.py:147-150).  One WAVE per frame: lane l takes
// tiles l, l + 64, .. (a thread per frame walked its 128 tiles twice, load after load: 52 us of a 256-sweep step).
__global__ __launch_bounds__(64) void k_wet_scan(WetArgs w)
{
    const PreArgs &a = w.p;
    const int f = blockIdx.x, lane = threadIdx.x;
    const int64_t n = pre_rows(a, f);
    const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
    const int32_t *c = w.tile_cnt + (int64_t)f * a.max_tiles * 2;
    int32_t *b = w.tile_base + (int64_t)f * a.max_tiles * 2;
    int na = 0, nb = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += 64) {
        const int64_t t = t0 + lane;
        const int ca = t < tiles ? c[2 * t] : 0, cb = t < tiles ? c[2 * t + 1] : 0;
        int ia = ca, ib = cb;
        for (int o = 1; o < 64; o <<= 1) {
            const int x = __shfl_up(ia, o), y = __shfl_up(ib, o);
            if (lane >= o) { ia += x; ib += y; }
        }
        if (t < tiles) { b[2 * t] = na + ia - ca; b[2 * t + 1] = nb + ib - cb; }
        na += __shfl(ia, 63); nb += __shfl(ib, 63);
    }
    for (int64_t t = lane; t < tiles; t += 64) b[2 * t + 1] += na;                    // ground after non-ground (same lane wrote it)
    if (lane == 0) {
        w.out_counts[f] = na + nb;
        w.out_flags[f] = a.fr[f].unchanged;
    }
}

template <typename T>
__global__ __launch_bounds__(PB) void k_wet_scatter(WetArgs w)
{
    const PreArgs &a = w.p;
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const T *rows = (const T *)a.rows;
    const int unchanged = a.fr[f].unchanged;
    __shared__ int wc[4][4][2];
    const int tid = threadIdx.x, wv = tid >> 6;
    const unsigned long long lt = (1ull << (tid & 63)) - 1ull;
    uint8_t c[4];
    int pre[4];
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + tid;
        c[q] = r < n ? w.cls[base + r] : 0;
        const unsigned long long ma = __ballot(c[q] == 1), mb = __ballot(c[q] == 2);
        pre[q] = c[q] == 1 ? __popcll(ma & lt) : __popcll(mb & lt);
        if ((tid & 63) == 0) { wc[q][wv][0] = __popcll(ma); wc[q][wv][1] = __popcll(mb); }
    }
    __syncthreads();
    const int32_t *tb = w.tile_base + ((int64_t)f * a.max_tiles + blockIdx.x) * 2;
    int run[2] = {tb[0], tb[1]};
    // every load of the thread's four rows before the first store (the argument struct carries no `restrict`: behind a store to out_rows the
    // compiler may not start the next row's loads, and the kernel was a chain of four round trips per thread: 0.59 ms per 256 sweeps)
    T sx[4], sy[4], sz[4], si[4], sl[4];
    double nw[4];
    int32_t sf[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = base + tile0 + q * PB + tid;
        const T *s = rows + (c[q] ? r : base) * 5;
        sx[q] = s[0]; sy[q] = s[1]; sz[q] = s[2]; si[q] = s[3]; sl[q] = s[4];
        nw[q] = c[q] == 2 ? w.new_i[r] : 0.0;
        sf[q] = (c[q] && w.src_first) ? w.src_first[r] : (int32_t)(r - base);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (c[q]) {
            const int k = c[q] - 1;
            int off = run[k];
            for (int ww = 0; ww < wv; ++ww) off += wc[q][ww][k];
            const int64_t dst = base + off + pre[q];
            double *d = w.out_rows + dst * 5;
            d[0] = (double)sx[q]; d[1] = (double)sy[q]; d[2] = (double)sz[q];
            d[3] = (c[q] == 2) ? nw[q] : (double)si[q];                  // augmentation.py:151-153
            double lab = (double)sl[q];
            if (!unchanged) {
                if (w.replace) lab = 0.0;                                // :155-156
                if (c[q] == 2) lab = 1.0;                                // :159
            }
            d[4] = lab;
            w.out_src[dst] = sf[q];
        }
        for (int k = 0; k < 2; ++k) run[k] += wc[q][0][k] + wc[q][1][k] + wc[q][2][k] + wc[q][3][k];
    }
}

// ---- the aligned wet stage: every row stays where it lies ------------------------------------------------------------------------------
// The wet model never moves a point (augmentation.py:145-159): a non-ground row is copied, a ground row gets a new intensity and label 1
// or is dropped.  So the result can keep the input's size and order, one keep byte beside every row, and needs neither k_wet_scan /
// k_wet_scatter (they only build the reference's [non-ground ; kept ground] order) nor the cls / new_i scratch.
struct WetAlignedArgs {
    PreArgs p;             // p.keep: the keep bytes that came in (NULL: every row present); p.frame_cnt = NULL (tiles of the full row range)
    double water_height, pavement_depth;
    int replace;
    void *out_rows;        // rows of the input's dtype; may be p.rows itself (in place)
    uint8_t *out_keep;     // may be p.keep itself
    int32_t *tile_cnt;     // [frame][tile]: rows kept
    int64_t *out_counts;
    int32_t *out_flags;
};

// Per row (processed frame): keep-in 0 -> as it came, keep 0; not ground -> column 4 = 0 under `replace` (:155-156), keep 1; ground, kept
// (:146) -> the new intensity (:153, rounded once to T), label 1 (:159), keep 1; ground, dropped -> the value new_intensities held after
// :131, label 1, keep 0.  A frame with fewer than 1000 present ground rows (:51-52) keeps rows and keep bytes as they came.  Out of place
// every row is stored whole; in place only columns 3 and 4 of the rows that change, and the keep bytes that change.
template <typename T>
__global__ __launch_bounds__(PB) void k_wet_apply_aligned(WetAlignedArgs w)
{
    const PreArgs &a = w.p;
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = a.frame_off[f + 1] - base;
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const PreFrame fr = a.fr[f];
    const WetFrame wf = wet_frame(a, f, w.water_height, w.pavement_depth);
    const T *rows = (const T *)a.rows;
    T *out = (T *)w.out_rows;
    const bool whole = (const void *)out != a.rows, same_keep = w.out_keep == a.keep;
    // every load of the thread's four rows before the first store (the argument struct carries no `restrict`, and out_rows / out_keep may
    // BE the input: see k_wet_scatter).  A thread reads and writes its own four rows only, so in place nothing is read after it was written.
    double gns[4], gds[4], angs[4];
    T sx[4], sy[4], sz[4], si[4], sl[4];
    uint8_t kin[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        const bool in = r < n;
        kin[q] = in ? (a.keep ? a.keep[base + r] : (uint8_t)1) : (uint8_t)0;
        gns[q] = (in && !fr.unchanged) ? a.g_norm[base + r] : NAN;       // (NaN for a row that is not there, too: k_pre_ground<T, true>)
        const bool ground = gns[q] == gns[q];
        gds[q] = ground ? a.g_dist[base + r] : 0.0;
        angs[q] = ground ? a.g_ang[base + r] : 1.0;
        const T *s = rows + (base + (in ? r : 0)) * 5;
        sx[q] = sy[q] = sz[q] = si[q] = sl[q] = (T)0;
        if (whole) { sx[q] = s[0]; sy[q] = s[1]; sz[q] = s[2]; si[q] = s[3]; sl[q] = s[4]; }
        else if (ground) si[q] = s[3];
    }
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        if (r >= n) continue;
        T inten = si[q], lab = sl[q];
        uint8_t k = kin[q];
        bool new_i = false, new_l = false;                               // column 3 / column 4 is rewritten (in place: the only stores)
        if (!fr.unchanged && k) {
            const double gn = gns[q];
            if (gn != gn) {
                if (w.replace) { lab = (T)0; new_l = true; }             // :155-156
            } else {
                double ni;
                k = wet_row_chain(wf, fr, gds[q], angs[q], (double)si[q], ni) ? 1 : 0;
                inten = (T)ni; lab = (T)1; new_i = new_l = true;         // :153, :159
            }
        }
        T *d = out + (base + r) * 5;
        if (whole) { d[0] = sx[q]; d[1] = sy[q]; d[2] = sz[q]; d[3] = inten; d[4] = lab; }
        else {
            if (new_i) d[3] = inten;                                     // (a non-ground row's intensity was not even loaded)
            if (new_l) d[4] = lab;
        }
        if (!same_keep || k != kin[q]) w.out_keep[base + r] = k;
        cnt += k != 0;
    }
    __shared__ int sc[4];
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) w.tile_cnt[(int64_t)f * a.max_tiles + blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
}

// per frame: rows kept and the "returned as it came" flag.  One wave per frame, lane l taking tiles l, l + 64, .. as k_wet_scan does;
// integers in a fixed order, no atomics.
__global__ __launch_bounds__(64) void k_wet_count(WetAlignedArgs w)
{
    const PreArgs &a = w.p;
    const int f = blockIdx.x, lane = threadIdx.x;
    const int64_t n = a.frame_off[f + 1] - a.frame_off[f];
    const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
    const int32_t *c = w.tile_cnt + (int64_t)f * a.max_tiles;
    int sum = 0;                                                         // (a batch holds fewer than 2^31 rows)
    for (int64_t t = lane; t < tiles; t += 64) sum += c[t];
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) {
        w.out_counts[f] = sum;
        w.out_flags[f] = a.fr[f].unchanged;
    }
}

// Source rows of a chained result (snowfall, then wet ground): final row -> snowfall row -> input row.
__global__ __launch_bounds__(PB) void k_compose_src(const int64_t *__restrict__ frame_off, const int64_t *__restrict__ counts,
                                                   const int32_t *__restrict__ second, const int32_t *__restrict__ first,
                                                   int32_t *__restrict__ out)
{
    const int f = blockIdx.y;
    const int64_t base = frame_off[f], n = counts[f];
    for (int64_t i = (int64_t)blockIdx.x * PB + threadIdx.x; i < n; i += (int64_t)gridDim.x * PB)
        out[base + i] = first[base + second[base + i]];
}

// ================================================================================================================
// host side

static int estimate(SgPrepassScratch *s, PreArgs &a, int dtype, int64_t n_total, int64_t max_frame, int min_ground,
                    int err_code, bool exact_f32_mean, hipStream_t st)
{
    const int64_t max_tiles = sg_tiles(max_frame);
    a.max_tiles = max_tiles;
    const size_t n = (size_t)(n_total > 0 ? n_total : 1), nf = (size_t)a.n_frames;
    if (sg_pre_ensure(s, B_GDIST, n * 8) || sg_pre_ensure(s, B_GNORM, n * 8) || sg_pre_ensure(s, B_GCOS, n * 8) ||
        sg_pre_ensure(s, B_PART, nf * (size_t)max_tiles * 12 * 8) || sg_pre_ensure(s, B_HIST, nf * HX * HY * 4) ||
        sg_pre_ensure(s, B_ROWMIN, nf * HX * 8) || sg_pre_ensure(s, B_FRAME, nf * sizeof(PreFrame)) || (dtype == 0 && sg_pre_ensure(s, B_CDIST, n * 4)) ||
        (dtype == 0 && exact_f32_mean && sg_pre_ensure(s, B_LEAF, nf * 3 * (size_t)pre_max_leaves(max_frame) * 4)))
        return -1;
    a.g_dist = (double *)s->buf[B_GDIST]; a.g_norm = (double *)s->buf[B_GNORM]; a.g_ang = (double *)s->buf[B_GCOS];
    a.part = (double *)s->buf[B_PART]; a.hist = (int32_t *)s->buf[B_HIST]; a.rowmin = (double *)s->buf[B_ROWMIN];
    a.fr = (PreFrame *)s->buf[B_FRAME];
    a.cdist = (float *)s->buf[B_CDIST];
    hipError_t e = hipMemsetAsync(a.hist, 0, nf * HX * HY * 4, st);
    if (e != hipSuccess) return (int)e;
    dim3 grid((unsigned)max_tiles, (unsigned)a.n_frames);
    const int rc = sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (a.keep) hipLaunchKernelGGL((k_pre_ground<T, true>), grid, dim3(PB), 0, st, a);
        else hipLaunchKernelGGL((k_pre_ground<T, false>), grid, dim3(PB), 0, st, a);
        SG_CHECK_LAUNCH();
        return 0;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_pre_means, dim3((unsigned)a.n_frames), dim3(64), 0, st, a, min_ground, err_code);
    SG_CHECK_LAUNCH();

    hipLaunchKernelGGL(k_pre_moments, grid, dim3(PB), 0, st, a);
    SG_CHECK_LAUNCH();
    if (int rc = sg_pre_launch_rowmin(a, st)) return rc;
    hipLaunchKernelGGL(k_pre_lines, dim3((unsigned)a.n_frames), dim3(64), 0, st, a, (dtype == 0 && !a.rows_as_f64) ? 1 : 0);
    SG_CHECK_LAUNCH();
    if (a.lines_override) {
        hipLaunchKernelGGL(k_pre_override_lines, dim3((unsigned)((a.n_frames + 63) / 64)), dim3(64), 0, st, a);
        SG_CHECK_LAUNCH();
    }
    if (dtype == 0 && exact_f32_mean) {
        // only frames whose noise line fell back to p = linregress(range, I / cos) need the float32 mean; the two
        // kernels below leave at once for every other frame
        hipLaunchKernelGGL(k_pre_gather, grid, dim3(PB), 0, st, a);
        SG_CHECK_LAUNCH();
        return sg_pre_launch_mean32(s, a, max_frame, nullptr, st);
    }
    return 0;
}

// The estimate both wet entries start from: the argument block from the call's parameters, estimate(), the two quadratics of 'poly', the
// export of the fitted curves.  keep: the aligned stage's keep bytes (NULL: every row present).
static int wet_fit(SgPrepassScratch *s, PreArgs &a, const void *rows, int dtype, const int64_t *frame_off, const int64_t *frame_cnt,
                   const uint8_t *keep, int n_frames, int64_t n_total, int64_t max_frame, const double *plane, const SgWetParams *wp,
                   int32_t *status, hipStream_t st)
{
    a.lines_override = wp->lines;
    a.rows = rows; a.frame_off = frame_off; a.frame_cnt = frame_cnt; a.keep = keep; a.n_frames = n_frames; a.plane = plane; a.delta = wp->delta;
    a.flat_earth = wp->flat_earth; a.rows_as_f64 = 1; a.noise_floor = wp->noise_floor; a.power_factor = wp->power_factor; a.status = status;
    a.weather = wp->weather;
    int rc = estimate(s, a, dtype, n_total, max_frame, 1000, 0, false, st);
    if (rc) return rc;
    if (wp->estimation == 1) {                       // 'poly': the two quadratics replace the two lines
        if (sg_pre_ensure(s, B_QPART, (size_t)n_frames * (size_t)a.max_tiles * PQ_COLS * 8)) return -1;
        a.qpart = (double *)s->buf[B_QPART]; a.seed = wp->seed;
        hipLaunchKernelGGL(k_pre_quad_part, dim3((unsigned)a.max_tiles, (unsigned)n_frames), dim3(PB), 0, st, a);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_pre_quad_fit, dim3((unsigned)n_frames), dim3(128), 0, st, a, 7 /* SNOWGPU_E_GROUND */);
        SG_CHECK_LAUNCH();
    }
    if (wp->fit_out) {
        hipLaunchKernelGGL(k_pre_export_fit, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), 0, st, a, wp->fit_out);
        SG_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int sg_wet_run(SgPrepassScratch *s, const void *rows, int dtype, const int64_t *frame_off,
                          const int64_t *frame_cnt, int n_frames, int64_t n_total, int64_t max_frame, const double *plane, const SgWetParams *wp, double *out_rows, int32_t *out_src,
                          int64_t *out_counts, int32_t *out_flags, int32_t *status, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    WetArgs w{};
    PreArgs &a = w.p;
    int rc = wet_fit(s, a, rows, dtype, frame_off, frame_cnt, nullptr, n_frames, n_total, max_frame, plane, wp, status, st);
    if (rc) return rc;
    const size_t n = (size_t)(n_total > 0 ? n_total : 1), nf = (size_t)n_frames;
    if (sg_pre_ensure(s, B_CLS, n) || sg_pre_ensure(s, B_NEWI, n * 8) || sg_pre_ensure(s, B_TCNT, nf * (size_t)a.max_tiles * 2 * 4) ||
        sg_pre_ensure(s, B_TBASE, nf * (size_t)a.max_tiles * 2 * 4))
        return -1;
    w.water_height = wp->water_height; w.pavement_depth = wp->pavement_depth; w.replace = wp->replace;
    w.cls = (uint8_t *)s->buf[B_CLS]; w.new_i = (double *)s->buf[B_NEWI];
    w.tile_cnt = (int32_t *)s->buf[B_TCNT]; w.tile_base = (int32_t *)s->buf[B_TBASE];
    w.out_rows = out_rows; w.out_src = out_src; w.out_counts = out_counts; w.out_flags = out_flags; w.src_first = wp->src_first;
    dim3 grid((unsigned)a.max_tiles, (unsigned)n_frames);
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_wet_apply<T>, grid, dim3(PB), 0, st, w);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_wet_scan, dim3((unsigned)n_frames), dim3(64), 0, st, w);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_wet_scatter<T>, grid, dim3(PB), 0, st, w);
        SG_CHECK_LAUNCH();
        return 0;
    });
}

// sg_wet_run with the ALIGNED result: rows of the input's dtype at the input's own index in out_rows (which may be `rows`), one keep
// byte per row in out_keep (which may be keep_in).  keep_in: optional, 0 = the row is not there.  Frames are walked over their full row
// range; src_first of wp is unused (row i IS input row i).
extern "C" int sg_wet_run_aligned(SgPrepassScratch *s, const void *rows, int dtype, const int64_t *frame_off, const uint8_t *keep_in,
                                  int n_frames, int64_t n_total, int64_t max_frame, const double *plane, const SgWetParams *wp, void *out_rows,
                                  uint8_t *out_keep, int64_t *out_counts, int32_t *out_flags, int32_t *status, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    WetAlignedArgs w{};
    PreArgs &a = w.p;
    int rc = wet_fit(s, a, rows, dtype, frame_off, nullptr, keep_in, n_frames, n_total, max_frame, plane, wp, status, st);
    if (rc) return rc;
    if (sg_pre_ensure(s, B_TCNT, (size_t)n_frames * (size_t)a.max_tiles * 4)) return -1;
    w.water_height = wp->water_height; w.pavement_depth = wp->pavement_depth; w.replace = wp->replace;
    w.out_rows = out_rows; w.out_keep = out_keep; w.tile_cnt = (int32_t *)s->buf[B_TCNT]; w.out_counts = out_counts; w.out_flags = out_flags;
    dim3 grid((unsigned)a.max_tiles, (unsigned)n_frames);
    return sg_by_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_wet_apply_aligned<decltype(t)>, grid, dim3(PB), 0, st, w);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_wet_count, dim3((unsigned)n_frames), dim3(64), 0, st, w);
        SG_CHECK_LAUNCH();
        return 0;
    });
}

extern "C" int sg_launch_compose_src(const int64_t *frame_off, const int64_t *counts, int n_frames, int64_t max_frame,
                                     const int32_t *second, const int32_t *first, int32_t *out, void *stream)
{
    if (n_frames <= 0 || max_frame <= 0) return 0;
    const unsigned gx = (unsigned)std::min<int64_t>((max_frame + PB - 1) / PB, 64);
    hipLaunchKernelGGL(k_compose_src, dim3(gx, (unsigned)n_frames), dim3(PB), 0, (hipStream_t)stream, frame_off, counts, second, first, out);
    SG_CHECK_LAUNCH();
    return 0;
}
