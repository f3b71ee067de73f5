// snowgpu_prepass.hip -- the noise-threshold prepass of the snowfall path on gfx950 (the "lean" chain).
//
//   simulation.py:449-467 + wet_ground/augmentation.py:195-266 ('linear'): ground rows by plane distance, incident angle,
//   I / cos(angle) against range, a least-squares line, a 50 x 2555 (range x normalised intensity) histogram whose per-range-row
//   sparsest occupied bin gives the noise line, the quadratic of simulation.py:467.
//
// The reference does this with NumPy/SciPy calls on the host; here it is a chain of small kernels, one grid row per frame,
// whose floating-point reductions run in a fixed order (tile partials -> ordered final sum) so that a
// batch is reproducible run to run.  The reductions are float64; they agree with NumPy's to ~1e-12, not
// bit for bit (NumPy's own summation order depends on its build) -- see DESIGN.md "prepass tolerance".
//
// Who runs what: sg_prepass_run (every snowfall batch), sg_prepass_stats_run (snowgpu_prepass_stats: a caller that takes the row
// minima itself) and sg_prepass_stats_early run the k_lean_* chain below, which keeps no per-row scratch.  The full estimator with its
// per-row arrays (k_pre_ground / means / moments / lines / gather, k_pre_quad_*) is snowgpu_wet.hip's and runs for sg_wet_run only.  The
// two share k_pre_rowmin and k_pre_mean32, which live here (sg_prepass_dev.h: sg_pre_launch_rowmin, sg_pre_launch_mean32), and the
// scratch pool.
#include <hip/hip_runtime.h>
#include <math.h>
#include <algorithm>
#include <cstdlib>
#include "sg_common.h"
#include "sg_prepass.h"
#include "sg_prepass_dev.h"
#include "sg_lean.h"
#include "sg_math.h"
#include "sg_launch.h"

// ---- the two kernels the full estimator (snowgpu_wet.hip) runs too --------------------------------------------
// np.mean(range) of float32 rows exactly as NumPy computes it (sg_prepass_dev.h: np_leaf_sum_f32): one block per frame walks NumPy's
// recursion over the ground ranges a gather kernel compacted in row order (k_lean_gather; k_pre_gather for the full estimator)
__device__ void lean_solve_frame_fwd(const PreArgs &a, int f, double *thr_poly);

__global__ __launch_bounds__(PB) void k_pre_mean32(PreArgs a, int *leaf_buf, int max_leaves, double *thr_poly_or_null)
{
    const int f = blockIdx.x;
    const int n = (int)a.fr[f].n_ground;
    if (n <= 0 || !a.fr[f].need_mean32) {
        // A frame without a ground row waits for no mean, but its quadratic waited for this kernel (lean_lines_wave): the zeros
        // lean_solve_frame gives fewer than 3 ground rows, instead of whatever an earlier batch left in the row.
        if (n <= 0 && a.fr[f].need_mean32 && thr_poly_or_null && threadIdx.x == 0) {
            double *out = thr_poly_or_null + 3 * f;
            out[0] = out[1] = out[2] = 0.0;
        }
        return;
    }
    const float *v = a.cdist + a.frame_off[f];
    int *leaf_off = leaf_buf + (int64_t)f * 3 * max_leaves;      // per frame: offsets, lengths, sums (as float bits)
    int *leaf_len = leaf_off + max_leaves;
    float *leaf_sum = (float *)(leaf_len + max_leaves);
    const int PW_MAX_LEAVES = max_leaves;
    __shared__ int n_leaves;
    if (threadIdx.x == 0) {                     // depth-first walk of pairwise_sum's recursion: leaves in order
        int stack_off[40], stack_len[40], sp = 0, nl = 0;
        stack_off[0] = 0; stack_len[0] = n; sp = 1;
        while (sp > 0 && nl < PW_MAX_LEAVES) {
            --sp;
            const int o = stack_off[sp], l = stack_len[sp];
            if (l <= 128) { leaf_off[nl] = o; leaf_len[nl] = l; ++nl; }
            else {
                int n2 = l / 2;
                n2 -= n2 % 8;
                stack_off[sp] = o + n2; stack_len[sp] = l - n2; ++sp;        // right half: visited second
                stack_off[sp] = o; stack_len[sp] = n2; ++sp;                 // left half: visited first
            }
        }
        n_leaves = nl;
    }
    __syncthreads();                            // (global writes of this block are visible to it after the barrier)
    for (int i = threadIdx.x; i < n_leaves; i += PB) leaf_sum[i] = np_leaf_sum_f32(v + leaf_off[i], leaf_len[i]);
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {                     // sum(l) = sum(left) + sum(right): post-order over the same tree
        // explicit evaluation stack: entries are either pending sizes (>= 0) or the "add" marker (-1)
        int cmd[96], sp = 0, next_leaf = 0, vs = 0;
        float val[48];
        cmd[sp++] = n;
        while (sp > 0) {
            const int c = cmd[--sp];
            if (c == -1) { const float r = val[--vs]; const float l = val[--vs]; val[vs++] = l + r; }
            else if (c <= 128) { val[vs++] = leaf_sum[next_leaf++]; }
            else {
                int n2 = c / 2;
                n2 -= n2 % 8;
                cmd[sp++] = -1; cmd[sp++] = c - n2; cmd[sp++] = n2;          // evaluate left, then right, then add
            }
        }
        const float total = 0.0f + val[0];      // np.add.reduce: identity + pairwise sum
        PreFrame &fr = a.fr[f];
        fr.xmean32 = (double)(total / (float)n);                             // _mean: float32 true_divide
        fr.p1 = fr.ymean - fr.p0 * fr.xmean32;                               // linregress intercept (augmentation.py:216)
        fr.pmin1 = fr.p1;                                                    // pmin = p (:250-251)
        if (thr_poly_or_null) lean_solve_frame_fwd(a, f, thr_poly_or_null);  // the lean chain: the quadratic waited for this intercept
    }
}

// ---- P4: per range row, the sparsest occupied bin (first one on ties) ------------------------------------------
// hist[hist == 0] = len(ground); ymins = argpartition(hist, 2, axis=1)[:, 0]  (augmentation.py:234-236).  NumPy's
// portable selection leaves the FIRST minimum there (argmin); an all-empty row gives bin 0.
__global__ __launch_bounds__(PB) void k_pre_rowmin(PreArgs a)
{
    const int f = blockIdx.y, row = blockIdx.x;
    const int32_t *h = a.hist + ((int64_t)f * HX + row) * HY;
    const PreFrame fr = a.fr[f];
    const int ng = (int)fr.n_ground;
    int best = 0x7fffffff, bidx = 0x7fffffff;
    constexpr int TRIPS = (HY + PB - 1) / PB;
    int cs[TRIPS];
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {                                    // the row's counts in one round of loads (a load per trip of a loop waited for each)
        const int b = threadIdx.x + i * PB;
        cs[i] = b < HY ? h[b] : -1;
    }
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        int c = cs[i];
        if (c < 0) continue;
        if (c == 0) c = ng;
        if (c < best) { best = c; bidx = threadIdx.x + i * PB; }         // ascending b per thread: first minimum
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_down(best, o), oi = __shfl_down(bidx, o);
        if (ob < best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    __shared__ int sb[4], si[4];
    if ((threadIdx.x & 63) == 0) { sb[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bidx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sb[w] < best || (sb[w] == best && si[w] < bidx)) { best = sb[w]; bidx = si[w]; }
        const double step = (fr.ymax - 5.0) / HY;
        const double edge = (bidx == HY) ? fr.ymax : (double)bidx * step + 5.0;   // yedges[ymins], augmentation.py:237
        a.rowmin[(int64_t)f * HX + row] = edge;
    }
}

// ================================================================================================================
// The lean chain.  The full estimator (snowgpu_wet.hip, kept by the wet-ground model, whose per-row rewrite needs range, angle and I / cos of every
// ground row again) moves every ground row through three float64 scratch arrays -- written once, read twice: 2.8 GB per 256-sweep
// step when the snowfall path used it too (rounds 1 - 3), more than the per-beam kernels fetch.  The snowfall path needs less: k_lean_stats streams the rows ONCE and leaves, per 1024-row tile, everything that is a plain sum --
// count, sums and tile-centred second moments of (range, I / cos) for the regression line, the maximum for the histogram
// range, and the sums of the quadratic fit, which are LINEAR in the noise line (y_i = nf (pmin0 d_i + pmin1) c_i, so
// sum a y = nf (pmin0 sum a d c + pmin1 sum a c)) and can therefore be taken before the line is known; k_lean_hist streams
// the rows a second time for the 50 x 2555 histogram (its bin edges need the maximum), recomputing the three per-row values
// instead of loading them.  Tiles are combined per frame in a fixed order (Chan's pairwise update for the centred
// moments), so a batch is reproducible run to run.  No per-row scratch at all.
template <typename T>
__global__ __launch_bounds__(PB) void k_lean_stats(PreArgs a)
{
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const T *rows = (const T *)a.rows;
    T rx[4], ry[4], rz[4], ri[4];                // all loads of the tile in flight before the first use
    bool valid[4];
    // rows to threads as the channel sort's first kernel deals them (wave w: rows [256 w, 256 w + 256) of the tile in four rounds of 64): the
    // statistics taken there and here are then the same sums in the same order -- the same bits whichever kernel a call uses
    const int w = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + w * 256 + q * 64 + lane;
        valid[q] = r < n;
        const T *p = rows + (base + (valid[q] ? r : 0)) * 5;
        rx[q] = p[0]; ry[q] = p[1]; rz[q] = p[2]; ri[q] = p[3];
    }
    __shared__ double sm[58];
    SgLeanTile lt;
    lt.plane = a.plane; lt.delta = a.delta; lt.part = a.part; lt.max_tiles = a.max_tiles;
    lean_tile_stats<T>(lt, f, blockIdx.x, rx, ry, rz, ri, valid, sm);
}

// one wave per frame: exclusive prefix of the tile counts, means, maximum, centred moments and the fit's sums
__global__ __launch_bounds__(64) void k_lean_means(PreArgs a, int min_ground, int err_code)
{
    const int f = blockIdx.x;
    if (f >= a.n_frames) return;
    const int lane = threadIdx.x;
    const int64_t n = pre_rows(a, f);
    const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
    double *part = a.part + (int64_t)f * a.max_tiles * LP_COLS;
    double run = 0.0, ym = -INFINITY, sx = 0.0, sy = 0.0;
    for (int64_t t0 = 0; t0 < tiles; t0 += 64) {
        const int64_t t = t0 + lane;
        const double c = t < tiles ? part[t * LP_COLS + LP_N] : 0.0;
        if (t < tiles) { ym = fmax(ym, part[t * LP_COLS + LP_YMAX]); sx += part[t * LP_COLS + LP_SX]; sy += part[t * LP_COLS + LP_SY]; }
        double inc = c;                                          // inclusive scan across the wave (exact: integers)
        for (int o = 1; o < 64; o <<= 1) { const double v = __shfl_up(inc, o); if (lane >= o) inc += v; }
        if (t < tiles) part[t * LP_COLS + LP_PREFIX] = run + inc - c;    // ground rows in earlier tiles
        run += __shfl(inc, 63);
    }
    for (int o = 32; o > 0; o >>= 1) { ym = fmax(ym, __shfl_xor(ym, o)); sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o); }
    const double cnt = run;
    const double xm = cnt > 0 ? sx / cnt : 0.0, ymn = cnt > 0 ? sy / cnt : 0.0;
    // M2 = sum over tiles of (tile-centred M2 + n_t (tile mean - frame mean)^2): lane l takes tiles l, l + 64, .., fixed tree
    double mxx = 0.0, mxy = 0.0, q[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t t = lane; t < tiles; t += 64) {
        const double *o = part + t * LP_COLS;
        const double nt = o[LP_N];
        if (nt > 0) {
            const double dxm = o[LP_SX] / nt - xm, dym = o[LP_SY] / nt - ymn;
            mxx += o[LP_MXX] + nt * (dxm * dxm);
            mxy += o[LP_MXY] + nt * (dxm * dym);
        }
        for (int k = 0; k < 11; ++k) q[k] += o[LP_Q0 + k];
    }
    for (int o = 32; o > 0; o >>= 1) {
        mxx += __shfl_xor(mxx, o); mxy += __shfl_xor(mxy, o);
        for (int k = 0; k < 11; ++k) q[k] += __shfl_xor(q[k], o);
    }
    if (lane == 0) {
        PreFrame &fr = a.fr[f];
        fr.n_ground = cnt;
        fr.xmean = xm; fr.ymean = ymn;
        fr.xmean32 = (double)(float)xm;         // refined by k_pre_mean32 when the value is actually used
        fr.need_mean32 = 0;
        fr.ymax = fabs(ym);                                              // np.abs(np.max(...)), augmentation.py:233
        fr.unchanged = 0;
        fr.sxx = mxx; fr.sxy = mxy;
        fr.rows_done = 0;
        for (int k = 0; k < 11; ++k) fr.q[k] = q[k];
        if (cnt < (double)min_ground) {
            // TypeError in the reference (Q7) -- unless the frame was gated out of the snowfall stage: it is empty because it was not asked
            if (err_code && !(a.weather && a.weather[(int64_t)f * SG_WEATHER_REC + SG_W_SNOW] == 0.0)) atomicCAS(&a.status[0], 0, err_code);
            fr.unchanged = 1;
        }
    }
}

// the 50 x 2555 histogram from the rows themselves (second and last pass over them)
template <typename T>
__global__ __launch_bounds__(PB) void k_lean_hist(PreArgs a)
{
    const int f = blockIdx.y;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    // A frame that came unsorted (firing order) is read from the sort's sorted copy: neighbouring rows are then neighbouring azimuths
    // of one laser again and fall into the same few bins (the tile's LDS table below), where a firing-order tile holds 64 lasers'
    // rows and as many distinct bins (measured: 1.07 instead of 0.88 ms, beside the tiers).  The histogram does not depend on the
    // row order.  The per-tile ground counts describe the tiles of the ARRIVAL order, so only sorted frames can skip by them.
    const bool uns = a.frame_unsorted && a.frame_unsorted[f];
    if (!uns && a.part[((int64_t)f * a.max_tiles + blockIdx.x) * LP_COLS + LP_N] == 0.0) return;       // no ground row in this tile
    const double *pl = a.plane + 4 * f;
    const double w0 = pl[0], w1 = pl[1], w2 = pl[2], h = pl[3];
    const double wn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double ymaxv = a.fr[f].ymax;
    const T *rows = (const T *)(uns ? a.srows : a.rows);
    int32_t *hist = a.hist + (int64_t)f * HX * HY;
    T rx[4], ry[4], rz[4], ri[4];
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        const T *p = rows + (base + (r < n ? r : 0)) * 5;
        rx[q] = p[0]; ry[q] = p[1]; rz[q] = p[2]; ri[q] = p[3];
    }
    int key[4] = {-1, -1, -1, -1};
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + threadIdx.x;
        double gd, gn, gc;
        if (r < n && lean_row<T>(a.delta, w0, w1, w2, h, wn, rx[q], ry[q], rz[q], ri[q], gd, gn, gc) && gn == gn) {
            const int bx = hist_bin(gd, 10.0, 70.0, HX);                 // augmentation.py:232-233
            const int by = hist_bin(gn, 5.0, ymaxv, HY);
            if (bx >= 0 && by >= 0) key[q] = bx * HY + by;
        }
    }
    // the tile's keys are counted in an LDS hash table first, then one atomic per distinct bin (see k_pre_moments)
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
}

// the two lines from the frame's centred moments (k_lean_means) and the histogram's row minima (one thread per frame)
__device__ __forceinline__ void lean_lines_frame(const PreArgs &a, int f, int xmean_f32)
{
    PreFrame &fr = a.fr[f];
    const double ng = fr.n_ground;
    double slope = 0, icpt = 0;
    if (ng >= 3) {
        slope = (fr.sxy / ng) / (fr.sxx / ng);                           // scipy linregress: ssxym / ssxm
        const double xm = xmean_f32 ? fr.xmean32 : fr.xmean;             // np.mean of a float32 column is a float32 (augmentation.py:216)
        icpt = fr.ymean - slope * xm;
    }
    fr.p0 = slope; fr.p1 = icpt;
    double xs[HX], ys[HX];
    int m = 0;
    const double xstep = (70.0 - 10.0) / HX;
    for (int r = 0; r < HX; ++r) {
        const double mv = ((const volatile double *)a.rowmin)[(int64_t)f * HX + r];   // (written by other blocks of this launch in k_lean_rowmin_solve: past the L1)
        if (mv > 5) {                                                    // augmentation.py:238
            const double e0 = (double)r * xstep + 10.0;
            const double e1 = (r + 1 == HX) ? 70.0 : (double)(r + 1) * xstep + 10.0;
            xs[m] = (e0 + e1) / 2; ys[m] = mv; ++m;                      // :240-241
        }
    }
    if (m > 3) small_linregress(xs, ys, m, fr.pmin0, fr.pmin1);         // augmentation.py:248-249
    else { fr.pmin0 = slope; fr.pmin1 = icpt; fr.need_mean32 = xmean_f32; }   // :250-251
}

__global__ __launch_bounds__(64) void k_lean_lines(PreArgs a, int xmean_f32)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f < a.n_frames) lean_lines_frame(a, f, xmean_f32);
}

// ground ranges compacted in row order for the frames that need NumPy's float32 mean (k_pre_mean32), from the rows
template <typename T>
__global__ __launch_bounds__(PB) void k_lean_gather(PreArgs a)
{
    const int f = blockIdx.y;
    if (!a.fr[f].need_mean32) return;
    const int64_t base = a.frame_off[f], n = pre_rows(a, f);
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const double *pl = a.plane + 4 * f;
    const double w0 = pl[0], w1 = pl[1], w2 = pl[2], h = pl[3];
    const double wn = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const T *rows = (const T *)a.rows;
    __shared__ int wc[4][4];
    const int tid = threadIdx.x, wv = tid >> 6;
    const unsigned long long lt = (1ull << (tid & 63)) - 1ull;
    if (a.frame_unsorted && a.frame_unsorted[f]) {
        // The reference sorts the frame by channel before it estimates (simulation.py:447), and NumPy's float32 sum depends on the order of
        // its terms: a frame that came unsorted is gathered from the sort's sorted copy, in that order.  The tile prefixes count the tiles
        // of the arrival order, so the frame's first block walks the whole sorted frame instead, 256 rows a trip (only frames whose noise
        // line fell back come here).
        if (blockIdx.x != 0) return;
        const T *srows = (const T *)a.srows;
        int run = 0;
        for (int64_t r0 = 0; r0 < n; r0 += PB) {
            const int64_t r = r0 + tid;
            double gd = 0.0, gn, gc;
            bool gr = false;
            if (r < n) {
                const T *p = srows + (base + r) * 5;
                gr = lean_row<T>(a.delta, w0, w1, w2, h, wn, p[0], p[1], p[2], p[3], gd, gn, gc) && gn == gn;
            }
            const unsigned long long m = __ballot(gr);
            if ((tid & 63) == 0) wc[0][wv] = __popcll(m);
            __syncthreads();
            int off = run;
            for (int ww = 0; ww < wv; ++ww) off += wc[0][ww];
            if (gr) a.cdist[base + off + __popcll(m & lt)] = (float)gd;
            run += wc[0][0] + wc[0][1] + wc[0][2] + wc[0][3];
            __syncthreads();
        }
        return;
    }
    bool g[4];
    int pre[4];
    double gdv[4];
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * PB + tid;
        double gn, gc;
        g[q] = false;
        if (r < n) {
            const T *p = rows + (base + r) * 5;
            g[q] = lean_row<T>(a.delta, w0, w1, w2, h, wn, p[0], p[1], p[2], p[3], gdv[q], gn, gc) && gn == gn;
        }
        const unsigned long long m = __ballot(g[q]);
        pre[q] = __popcll(m & lt);
        if ((tid & 63) == 0) wc[q][wv] = __popcll(m);
    }
    __syncthreads();
    int run = (int)a.part[((int64_t)f * a.max_tiles + blockIdx.x) * LP_COLS + LP_PREFIX];
    for (int q = 0; q < 4; ++q) {
        int off = run;
        for (int ww = 0; ww < wv; ++ww) off += wc[q][ww];
        if (g[q]) a.cdist[base + off + pre[q]] = (float)gdv[q];
        run += wc[q][0] + wc[q][1] + wc[q][2] + wc[q][3];
    }
}

// the quadratic from the frame's sums and its noise line (columns scaled by their norms, as np.polyfit does); one thread per frame
__device__ __forceinline__ void lean_solve_frame(const PreArgs &a, int f, double *thr_poly);
__device__ void lean_solve_frame_fwd(const PreArgs &a, int f, double *thr_poly) { lean_solve_frame(a, f, thr_poly); }
__device__ __forceinline__ void lean_solve_frame(const PreArgs &a, int f, double *thr_poly)
{
    const PreFrame &fr = a.fr[f];
    double *out = thr_poly + 3 * f;
    const double nn = fr.n_ground;
    if (nn < 3) { out[0] = out[1] = out[2] = 0.0; return; }
    const double *q = fr.q;
    const double nf = a.noise_floor, m0 = fr.pmin0, m1 = fr.pmin1;
    // sum a y with y = (nf (pmin0 d + pmin1)) c  (augmentation.py:252-253, simulation.py:462): linear in the line
    const double s5 = nf * (m0 * q[LQ_A2GC] + m1 * q[LQ_A2C]);
    const double s6 = nf * (m0 * q[LQ_A1GC] + m1 * q[LQ_A1C]);
    const double s7 = nf * (m0 * q[LQ_GC] + m1 * q[LQ_C]);
    const double c2 = sqrt(q[LQ_A2A2]), c1 = sqrt(q[LQ_A1A1]), c0 = sqrt(nn);
    double G[3][4] = {{q[LQ_A2A2] / (c2 * c2), q[LQ_A2A1] / (c2 * c1), q[LQ_A2] / (c2 * c0), s5 / c2},
                      {q[LQ_A2A1] / (c1 * c2), q[LQ_A1A1] / (c1 * c1), q[LQ_A1] / (c1 * c0), s6 / c1},
                      {q[LQ_A2] / (c0 * c2), q[LQ_A1] / (c0 * c1), nn / (c0 * c0), s7 / c0}};
    for (int i = 0; i < 3; ++i) {                                        // Gaussian elimination, partial pivoting
        int piv = i;
        for (int r = i + 1; r < 3; ++r) if (fabs(G[r][i]) > fabs(G[piv][i])) piv = r;
        if (piv != i) for (int k = 0; k < 4; ++k) { const double t = G[i][k]; G[i][k] = G[piv][k]; G[piv][k] = t; }
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
    out[0] = x[0] / c2; out[1] = x[1] / c1; out[2] = x[2] / c0;
    a.fr[f].poly[0] = out[0]; a.fr[f].poly[1] = out[1]; a.fr[f].poly[2] = out[2];
}

// The two lines and (unless the frame needs NumPy's float32 mean first) the quadratic of one frame by ONE WAVE (all 64 lanes call it): the
// lanes fetch the frame's 50 row minima in one round and squeeze out the rows without one (augmentation.py:238) by a ballot, in row order,
// into LDS (xs, ys: HX doubles each); lane 0 then runs the fits on them -- lean_lines_frame's statements.  (A thread per frame read the
// minima one after the other, 50 round trips, into arrays that lived in scratch memory: 46 us at the end of the prepass chain of a
// 256-sweep step, which ends the step's side branch.)  VOL: the minima were written by other blocks of the running launch -- read past the L1.
template <bool VOL>
__device__ __forceinline__ void lean_lines_wave(const PreArgs &a, int f, int xmean_f32, double *xs, double *ys, double *thr_poly)
{
    static_assert(HX <= 64, "one lane per range row");
    const int lane = threadIdx.x & 63;
    double mv = 0.0;
    if (lane < HX) mv = VOL ? ((const volatile double *)a.rowmin)[(int64_t)f * HX + lane] : a.rowmin[(int64_t)f * HX + lane];
    const bool keep = lane < HX && mv > 5;                               // augmentation.py:238
    const unsigned long long mask = __ballot(keep);
    if (keep) {
        const double xstep = (70.0 - 10.0) / HX;
        const double e0 = (double)lane * xstep + 10.0;
        const double e1 = (lane + 1 == HX) ? 70.0 : (double)(lane + 1) * xstep + 10.0;
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        xs[pos] = (e0 + e1) / 2; ys[pos] = mv;                           // :240-241
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                   // written and read by the lanes of one wave: no barrier, but keep the order
    if (lane != 0) return;
    const int m = __popcll(mask);
    PreFrame &fr = a.fr[f];
    const double ng = fr.n_ground;
    double slope = 0, icpt = 0;
    if (ng >= 3) {
        slope = (fr.sxy / ng) / (fr.sxx / ng);                           // scipy linregress: ssxym / ssxm
        const double xm = xmean_f32 ? fr.xmean32 : fr.xmean;             // np.mean of a float32 column is a float32 (augmentation.py:216)
        icpt = fr.ymean - slope * xm;
    }
    fr.p0 = slope; fr.p1 = icpt;
    if (m > 3) small_linregress(xs, ys, m, fr.pmin0, fr.pmin1);         // augmentation.py:248-249
    else { fr.pmin0 = slope; fr.pmin1 = icpt; fr.need_mean32 = xmean_f32; }   // :250-251
    if (!fr.need_mean32) lean_solve_frame(a, f, thr_poly);
}

// ... after k_pre_rowmin (large batches): one wave per frame
__global__ __launch_bounds__(64) void k_lean_lines_solve(PreArgs a, int xmean_f32, double *thr_poly)
{
    const int f = blockIdx.x;
    if (f >= a.n_frames) return;
    __shared__ double xs[HX], ys[HX];
    lean_lines_wave<false>(a, f, xmean_f32, xs, ys, thr_poly);
}

// Small batches (up to 16 frames: bound by their chain of dependent launches): row minima of a frame's histogram (one block per range
// row: 50 per frame) and -- by whichever block completes the frame -- the two lines and, unless the frame needs NumPy's float32 mean
// first (k_lean_gather, k_pre_mean32), the quadratic, in ONE launch (a single 1024-thread block per frame did this before: 78 us of a
// single sweep's 460, the longest link of its prepass chain).  Large batches keep k_pre_rowmin + k_lean_lines_solve: "the block that
// completes the frame" costs a device-scope fence per block, and on this chip -- eight XCDs, each with its own L2 -- such a fence writes
// the XCD's L2 back: 12 800 of them made this kernel 0.74 ms long on 256 sweeps, against 0.10 ms for the two launches.
__global__ __launch_bounds__(PB) void k_lean_rowmin_solve(PreArgs a, int xmean_f32, double *thr_poly)
{
    const int f = blockIdx.y, row = blockIdx.x;
    const int32_t *h = a.hist + ((int64_t)f * HX + row) * HY;
    PreFrame &fr = a.fr[f];
    const int ng = (int)fr.n_ground;
    int best = 0x7fffffff, bidx = 0x7fffffff;
    for (int b = threadIdx.x; b < HY; b += PB) {
        int c = h[b];
        if (c == 0) c = ng;                                                  // hist[hist == 0] = len(ground) (augmentation.py:234-235)
        if (c < best) { best = c; bidx = b; }                                // ascending b per thread: first minimum
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_down(best, o), oi = __shfl_down(bidx, o);
        if (ob < best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    __shared__ int sb[4], si[4], s_last;
    __shared__ double s_xs[HX], s_ys[HX];
    if ((threadIdx.x & 63) == 0) { sb[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bidx; }
    if (threadIdx.x == 0) s_last = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (sb[w] < best || (sb[w] == best && si[w] < bidx)) { best = sb[w]; bidx = si[w]; }
        const double step = (fr.ymax - 5.0) / HY;
        a.rowmin[(int64_t)f * HX + row] = (bidx == HY) ? fr.ymax : (double)bidx * step + 5.0;   // yedges[ymins] (:237)
        __threadfence();                                                     // the row's minimum before the count that announces it
        s_last = atomicAdd(&fr.rows_done, 1) == HX - 1;                      // this block completed the frame
        if (s_last) __threadfence();
    }
    __syncthreads();
    if (s_last && threadIdx.x < 64) lean_lines_wave<true>(a, f, xmean_f32, s_xs, s_ys, thr_poly);   // (one thread did this: 50 loads in a row)
}

// ================================================================================================================
// host side

int sg_pre_ensure(SgPrepassScratch *s, int i, size_t bytes)
{
    if (bytes <= s->cap[i]) return 0;
    if (s->buf[i]) (void)hipFree(s->buf[i]);
    s->buf[i] = nullptr; s->cap[i] = 0;
    const size_t want = bytes + bytes / 4 + 256;
    if (hipMalloc(&s->buf[i], want) != hipSuccess) return -1;
    s->cap[i] = want;
    return 0;
}

extern "C" void sg_prepass_release(SgPrepassScratch *s)
{
    for (int i = 0; i < 16; ++i) { if (s->buf[i]) (void)hipFree(s->buf[i]); s->buf[i] = nullptr; s->cap[i] = 0; }
}

int sg_pre_launch_rowmin(const PreArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_pre_rowmin, dim3(HX, (unsigned)a.n_frames), dim3(PB), 0, st, a);
    SG_CHECK_LAUNCH();
    return 0;
}

int sg_pre_launch_mean32(SgPrepassScratch *s, const PreArgs &a, int64_t max_frame, double *thr_poly, hipStream_t st)
{
    hipLaunchKernelGGL(k_pre_mean32, dim3((unsigned)a.n_frames), dim3(PB), 0, st, a, (int *)s->buf[B_LEAF], pre_max_leaves(max_frame), thr_poly);
    SG_CHECK_LAUNCH();
    return 0;
}

// ---- the lean chain's three entries share: their PreArgs, their buffers, their front, their float32 tail -----
static PreArgs lean_args(const void *rows, const int64_t *frame_off, int n_frames, int64_t max_frame, const double *plane)
{
    PreArgs a{};
    a.rows = rows; a.frame_off = frame_off; a.n_frames = n_frames; a.plane = plane; a.delta = 0.5; a.flat_earth = 0; a.cos_only = 1;
    a.max_tiles = sg_tiles(max_frame);
    return a;
}

// hist: the caller's histogram, or nullptr for the pool's.  float32 rows: also the ranges and leaves of NumPy's float32 mean (lean_mean32)
static int lean_reserve(SgPrepassScratch *s, PreArgs &a, int dtype, int64_t n_total, int64_t max_frame, int32_t *hist)
{
    const size_t n = (size_t)(n_total > 0 ? n_total : 1), nf = (size_t)a.n_frames;
    if (sg_pre_ensure(s, B_PART, nf * (size_t)a.max_tiles * LP_COLS * 8) || (!hist && sg_pre_ensure(s, B_HIST, nf * HX * HY * 4)) ||
        sg_pre_ensure(s, B_ROWMIN, nf * HX * 8) || sg_pre_ensure(s, B_FRAME, nf * sizeof(PreFrame)) ||
        (dtype == 0 && (sg_pre_ensure(s, B_CDIST, n * 4) || sg_pre_ensure(s, B_LEAF, nf * 3 * (size_t)pre_max_leaves(max_frame) * 4))))
        return -1;
    a.part = (double *)s->buf[B_PART]; a.hist = hist ? hist : (int32_t *)s->buf[B_HIST]; a.rowmin = (double *)s->buf[B_ROWMIN];
    a.fr = (PreFrame *)s->buf[B_FRAME]; a.cdist = (float *)s->buf[B_CDIST];
    return 0;
}

static int lean_stats(const PreArgs &a, int dtype, hipStream_t st)
{
    return sg_by_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_lean_stats<decltype(t)>, dim3((unsigned)a.max_tiles, (unsigned)a.n_frames), dim3(PB), 0, st, a);
        SG_CHECK_LAUNCH();
        return 0;
    });
}

// tile statistics (unless the tiles hold them already) -> per-frame means -> histogram
static int lean_front(const PreArgs &a, int dtype, bool tiles_done, hipStream_t st)
{
    if (!tiles_done)
        if (int rc = lean_stats(a, dtype, st)) return rc;
    hipLaunchKernelGGL(k_lean_means, dim3((unsigned)a.n_frames), dim3(64), 0, st, a, 3, 7 /* SNOWGPU_E_GROUND */);
    SG_CHECK_LAUNCH();
    return sg_by_dtype(dtype, [&](auto t) {
        hipLaunchKernelGGL(k_lean_hist<decltype(t)>, dim3((unsigned)a.max_tiles, (unsigned)a.n_frames), dim3(PB), 0, st, a);
        SG_CHECK_LAUNCH();
        return 0;
    });
}

// float32 rows: NumPy's float32 mean of the ground ranges for the frames that asked for it (need_mean32); the two kernels leave at once
// for every other frame
static int lean_mean32(SgPrepassScratch *s, const PreArgs &a, int64_t max_frame, double *thr_poly, hipStream_t st)
{
    hipLaunchKernelGGL(k_lean_gather<float>, dim3((unsigned)a.max_tiles, (unsigned)a.n_frames), dim3(PB), 0, st, a);
    SG_CHECK_LAUNCH();
    return sg_pre_launch_mean32(s, a, max_frame, thr_poly, st);
}

// The snowfall prepass without per-row scratch: two passes over the rows (statistics; histogram), the rest per frame.
// (the tile partials' buffer, for a caller whose own row-streaming kernel fills it: sg_launch_sort with statistics)
extern "C" double *sg_prepass_reserve_tiles(SgPrepassScratch *s, int n_frames, int64_t max_frame)
{
    if (sg_pre_ensure(s, B_PART, (size_t)n_frames * (size_t)sg_tiles(max_frame) * LP_COLS * 8)) return nullptr;
    return (double *)s->buf[B_PART];
}

// The per-tile statistics as a kernel of their own, ahead of the prepass proper (the tiles are reserved: sg_prepass_reserve_tiles; the plane is
// known): on the prepass stream beside the sort and the scan instead of inside the sort's first pass.  sg_prepass_run is then told tiles_done = 1.
extern "C" int sg_prepass_stats_early(SgPrepassScratch *s, const void *rows, int dtype, const int64_t *frame_off, int n_frames, int64_t max_frame,
                                      const double *plane, void *stream)
{
    PreArgs a = lean_args(rows, frame_off, n_frames, max_frame, plane);
    a.part = (double *)s->buf[B_PART];
    if (!a.part) return -1;
    return lean_stats(a, dtype, (hipStream_t)stream);
}

// The histogram of the snowfall prepass, cleared ahead of time: the fill depends on nothing of the batch, so it can run on the prepass
// stream beside the sort instead of in the prepass' own chain (sg_prepass_run is then told with hist_cleared = 1).
extern "C" int sg_prepass_clear_hist(SgPrepassScratch *s, int n_frames, void *stream)
{
    const size_t nf = (size_t)n_frames;
    if (sg_pre_ensure(s, B_HIST, nf * HX * HY * 4)) return -1;
    hipError_t e = hipMemsetAsync(s->buf[B_HIST], 0, nf * HX * HY * 4, (hipStream_t)stream);
    return e == hipSuccess ? 0 : (int)e;
}

// The snowfall path's prepass: thr_poly (n_frames x 3) receives every frame's quadratic (simulation.py:467).
// Returns 0, a positive hipError_t, or -1 on allocation failure.  plane: n_frames x 4 (wx, wy, wz, h).
extern "C" int sg_prepass_run(SgPrepassScratch *s, const void *rows, int dtype, const int64_t *frame_off, int n_frames,
                              int64_t n_total, int64_t max_frame, const double *plane, double noise_floor, double *thr_poly,
                              int32_t *status, void *stream, int tiles_done, const void *srows, const int32_t *frame_unsorted, int hist_cleared,
                              const double *weather)
{
    hipStream_t st = (hipStream_t)stream;
    PreArgs a = lean_args(rows, frame_off, n_frames, max_frame, plane);
    a.noise_floor = noise_floor; a.power_factor = 15.0; a.status = status; a.weather = weather;
    a.srows = srows; a.frame_unsorted = srows ? frame_unsorted : nullptr;
    if (lean_reserve(s, a, dtype, n_total, max_frame, nullptr)) return -1;
    if (!hist_cleared) {
        hipError_t e = hipMemsetAsync(a.hist, 0, (size_t)n_frames * HX * HY * 4, st);
        if (e != hipSuccess) return (int)e;
    }
    // (tiles_done: the channel sort's first kernel, or sg_prepass_stats_early, left the tile partials on its way over the rows)
    if (int rc = lean_front(a, dtype, tiles_done != 0, st)) return rc;
    if (n_frames <= 16) {
        hipLaunchKernelGGL(k_lean_rowmin_solve, dim3(HX, (unsigned)n_frames), dim3(PB), 0, st, a, dtype == 0 ? 1 : 0, thr_poly);
        SG_CHECK_LAUNCH();
    } else {
        if (int rc = sg_pre_launch_rowmin(a, st)) return rc;
        hipLaunchKernelGGL(k_lean_lines_solve, dim3((unsigned)n_frames), dim3(64), 0, st, a, dtype == 0 ? 1 : 0, thr_poly);
        SG_CHECK_LAUNCH();
    }
    // only frames whose noise line fell back to p = linregress(range, I / cos) need the float32 mean (and their quadratic waits for it)
    if (dtype == 0) return lean_mean32(s, a, max_frame, thr_poly, st);
    return 0;
}

// Per-frame record of the lean prepass for a caller that finishes the fit itself (snowgpu_prepass_stats): SG_PRE_REC doubles.
__global__ void k_lean_export(PreArgs a, double *out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n_frames) return;
    const PreFrame &fr = a.fr[f];
    double *o = out + (int64_t)f * SG_PRE_REC;
    o[0] = fr.n_ground; o[1] = fr.xmean; o[2] = fr.xmean32; o[3] = fr.ymean; o[4] = fr.ymax; o[5] = fr.p0; o[6] = fr.p1;
    for (int k = 0; k < 11; ++k) o[7 + k] = fr.q[k];
}

// hist[hist == 0] = len(pointcloud_planes) (augmentation.py:234-235) where the histogram is made: the caller converts and selects only
__global__ __launch_bounds__(PB) void k_lean_fill_empty(PreArgs a)
{
    const int f = blockIdx.y;
    const int ng = (int)a.fr[f].n_ground;
    int32_t *h = a.hist + (int64_t)f * HX * HY;
    for (int i = blockIdx.x * PB + threadIdx.x; i < HX * HY; i += gridDim.x * PB)
        if (h[i] == 0) h[i] = ng;
}

__global__ void k_lean_force_mean32(PreArgs a)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < a.n_frames) a.fr[f].need_mean32 = 1;
}

// The lean prepass up to the histogram and the regression line p, for a caller that takes the per-row minima of the histogram
// with its own code (quirk Q8: np.argpartition): d_hist receives n_frames x 50 x 2555 int32, d_rec n_frames x SG_PRE_REC doubles
// (n_ground, mean range, NumPy's float32 mean of the ranges, mean I / cos, max I / cos, p slope, p intercept, the 11 sums of the
// quadratic fit in LQ_* order).
extern "C" int sg_prepass_stats_run(SgPrepassScratch *s, const void *rows, int dtype, const int64_t *frame_off, int n_frames,
                                    int64_t n_total, int64_t max_frame, const double *plane, int32_t *d_hist, double *d_rec,
                                    int32_t *status, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    PreArgs a = lean_args(rows, frame_off, n_frames, max_frame, plane);
    a.noise_floor = 0.7; a.power_factor = 15.0; a.status = status;
    if (lean_reserve(s, a, dtype, n_total, max_frame, d_hist)) return -1;
    hipError_t e = hipMemsetAsync(a.hist, 0, (size_t)n_frames * HX * HY * 4, st);
    if (e != hipSuccess) return (int)e;
    const unsigned fb = (unsigned)((n_frames + 63) / 64);
    if (int rc = lean_front(a, dtype, false, st)) return rc;
    if (int rc = sg_pre_launch_rowmin(a, st)) return rc;
    hipLaunchKernelGGL(k_lean_lines, dim3(fb), dim3(64), 0, st, a, dtype == 0 ? 1 : 0);
    SG_CHECK_LAUNCH();
    if (dtype == 0) {        // NumPy's float32 mean of the ranges for EVERY frame: the caller's line may fall back to p (augmentation.py:250-251)
        hipLaunchKernelGGL(k_lean_force_mean32, dim3(fb), dim3(64), 0, st, a);
        SG_CHECK_LAUNCH();
        if (int rc = lean_mean32(s, a, max_frame, nullptr, st)) return rc;
    }
    hipLaunchKernelGGL(k_lean_export, dim3(fb), dim3(64), 0, st, a, d_rec);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_lean_fill_empty, dim3(32, (unsigned)n_frames), dim3(PB), 0, st, a);     // (after the row minima: they read the raw counts)
    SG_CHECK_LAUNCH();
    return 0;
}
