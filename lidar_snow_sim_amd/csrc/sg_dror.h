// sg_dror.h -- dynamic radius outlier removal (snowgpu_dror_mask_device): the definition's arithmetic and the binning of the neighbour
// search.  snowgpu_dror.hip runs these functions on the device, tests/host_harness/dror_cells.cpp the same code on the host (as sg_weather.h
// is compiled for both), and tests/dror_reference.py restates the DEFINITION below in float64 NumPy.
//
// Definition (Charron et al., CRV 2018; pointcloud_viewer.py:2258-2299 calls cadc_devkit's dror.py, which is not part of the reference
// checkout -- the edge conventions here are this library's).  Host constants, in double: c = beta (alpha (pi / 180)), c2 = c c,
// s2min = sr_min sr_min.  A row is USABLE iff it is present (keep-in byte non-zero, or no mask) and |x|, |y|, |z| <= 1e6 (false for NaN).
// With q = x x + y y and s2 = max(s2min, c2 q), usable row j != i of the same frame is a NEIGHBOUR of usable row i iff
// (dx dx + dy dy) + dz dz <= s2_i.  keep_i = usable_i and count_i >= k_min; neighbours_i = min(count_i, k_min).  No square root and no
// fused multiply-add takes part in a decision.
//
// The search.  Every usable row is filed in ONE cell of its frame's grid, which has two parts:
//   * a square Cartesian grid over |x|, |y| <= rc for the rows with q <= rc^2, rc a little beyond (sr_min / c) + sr_min: the disc in
//     which the radius is the constant sr_min, and the rim a query of that disc can reach;
//   * a log-polar grid over (ln r_xy, azimuth) for the rows beyond (q > rc^2), where the radius grows with the range: rings of equal
//     ratio from max(rc, 5 cm) to 300 m -- what lies nearer or farther (out to the 1e6 m limit) is filed in the first / last ring.
// Cells are about one search radius wide and are made wider, by one factor for both coordinates, until the part fits its share of the
// caller's cell budget: a wider cell costs candidates, never a neighbour.
// A query walks a WINDOW of cells computed from its own radius (sg_dror_window): the cells of the square x +- R, y +- R and of the
// annular sector r_xy +- R, azimuth +- asin(R / r_xy), with R = the radius, inflated by SG_DROR_MARGIN relative and 1e-9 of the range.
// The window is conservative -- the index functions are monotone in their argument up to the rounding of log / atan2 (1e-16), the margin
// is 1e-9 and more -- and the exact test above alone decides what is counted.  The row itself always lies in its window and passes the
// test (d2 = 0), so the kernel counts it and takes it off again: the sorted copy needs no row index.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SG_DROR_LIMIT 1e6          /* a coordinate beyond this (or NaN) makes the row unusable */
#define SG_DROR_MARGIN 1e-6        /* relative inflation of a query's radius for its window */
#define SG_DROR_C_MAX 0.25         /* domain: 0 < c <= 0.25 */
#define SG_DROR_K_MAX 65535        /* domain: 0 <= k_min <= 65535 */
#define SG_DROR_RING_FAR 300.0     /* m: the log-polar rings end here; farther rows are filed in the last ring */
#define SG_DROR_RING_NEAR 0.05     /* m: ... and begin here, or at rc if that is farther out */
#define SG_DROR_SR_GRID_MAX 4e6    /* m: a larger sr_min reaches every usable row of the frame; the grid is laid out for this one */
#define SG_DROR_MIN_CELLS 1024     /* cell budget per frame: at least this, */
#define SG_DROR_MAX_CELLS 81920    /* at most this (sg_dror_cell_budget): 4 bytes of scratch per cell and frame */
#define SG_NO_CELL 0xffffffffu     /* in a per-row cell entry: this row files nowhere (here and in sg_ball.h's cells, which include this header) */
#define SG_DROR_NO_CELL SG_NO_CELL /* the name the host harnesses (tests/host_harness/dror_cells.cpp, ball_cells.cpp) know it by */

struct SgDrorGrid {
    double c2, s2min;              // the definition's constants
    int32_t k_min;
    int32_t cart_m;                // Cartesian part: cart_m x cart_m cells of width 1 / cart_inv over [-rc, rc]^2
    double rc, rc2, cart_inv;
    int32_t n_ring, n_az;          // log-polar part: ring = (ln r_xy - ln_org) ring_inv, azimuth bin = (atan2(y, x) + pi) az_inv
    double ln_org, ring_inv, az_inv;
    int32_t cells;                 // cells per frame: cart_m^2 + n_ring n_az
};

struct SgDrorWindow {
    int32_t cart, ix0, ix1, iy0, iy1;      // cart != 0: Cartesian cells [ix0, ix1] x [iy0, iy1]
    int32_t polar, ring0, ring1, az0, n_az; // polar != 0: rings [ring0, ring1], n_az azimuth bins from az0 on, wrapping over the seam
};

// cells per frame for a batch whose longest frame has max_frame rows: about four cells per row, within the two limits
static inline int32_t sg_dror_cell_budget(int64_t max_frame)
{
    const int64_t want = 4 * max_frame;
    return (int32_t)(want < SG_DROR_MIN_CELLS ? SG_DROR_MIN_CELLS : want > SG_DROR_MAX_CELLS ? SG_DROR_MAX_CELLS : want);
}

// The grid of one call.  0, or 1: a parameter outside the domain (0 < c <= 0.25, sr_min >= 0 and finite, 0 <= k_min <= 65535).
static inline int sg_dror_make_grid(double alpha_deg, double beta, double sr_min, int64_t k_min, int32_t budget, SgDrorGrid *g)
{
    const double c = beta * (alpha_deg * (3.141592653589793 / 180.0));
    if (!(c > 0.0 && c <= SG_DROR_C_MAX) || !(sr_min >= 0.0) || !(sr_min <= 1.7976931348623157e308) || k_min < 0 || k_min > SG_DROR_K_MAX) return 1;
    if (budget < SG_DROR_MIN_CELLS) budget = SG_DROR_MIN_CELLS;
    g->c2 = c * c;
    g->s2min = sr_min * sr_min;
    g->k_min = (int32_t)k_min;
    // Cartesian part: a fifth of the budget
    const double sr = sr_min < SG_DROR_SR_GRID_MAX ? sr_min : SG_DROR_SR_GRID_MAX;
    g->rc = (sr / c + sr) * (1.0 + 1e-5) + 1e-9;
    g->rc2 = g->rc * g->rc;
    const int side_max = (int)floor(sqrt((double)(budget / 5)));
    double cell = sr * (1.0 + SG_DROR_MARGIN);
    if (cell < 2.0 * g->rc / side_max) cell = 2.0 * g->rc / side_max;
    g->cart_inv = 1.0 / cell;
    int m = (int)floor(2.0 * g->rc * g->cart_inv) + 1;
    g->cart_m = m > side_max ? side_max : m < 1 ? 1 : m;
    // log-polar part: what is left
    const int64_t polar_budget = (int64_t)budget - (int64_t)g->cart_m * g->cart_m;
    const double org = g->rc > SG_DROR_RING_NEAR ? g->rc : SG_DROR_RING_NEAR;
    const double span = org < SG_DROR_RING_FAR ? log(SG_DROR_RING_FAR / org) : 0.0;
    const double w = -log1p(-c);
    double k = 1.0;
    for (;;) {
        const double nr = floor(span / (w * k)) + 2.0, na = floor(2.0 * 3.141592653589793 / (w * k));
        if (na < 1.0 || nr * na <= (double)polar_budget) {
            g->n_ring = (int32_t)nr;
            g->n_az = na < 1.0 ? 1 : (int32_t)na;
            break;
        }
        const double need = sqrt(nr * na / (double)polar_budget);
        k *= need > 1.05 ? need : 1.05;
    }
    if ((int64_t)g->n_ring * g->n_az > polar_budget) g->n_ring = (int32_t)(polar_budget / g->n_az);      // (one azimuth bin: rings alone)
    if (g->n_ring < 1) g->n_ring = 1;
    g->ln_org = log(org);
    g->ring_inv = 1.0 / (w * k);
    g->az_inv = (double)g->n_az / (2.0 * 3.141592653589793);
    g->cells = g->cart_m * g->cart_m + g->n_ring * g->n_az;
    return 0;
}

__host__ __device__ inline bool sg_dror_usable(double x, double y, double z)
{
    return fabs(x) <= SG_DROR_LIMIT && fabs(y) <= SG_DROR_LIMIT && fabs(z) <= SG_DROR_LIMIT;
}

// the squared search radius of a row with q = x x + y y
__host__ __device__ inline double sg_dror_s2(const SgDrorGrid &g, double q)
{
    const double d = g.c2 * q;
    return d > g.s2min ? d : g.s2min;
}

__host__ __device__ inline int32_t sg_dror_clampi(double t, int32_t n)
{
    t = floor(t);
    return t >= (double)(n - 1) ? n - 1 : t > 0.0 ? (int32_t)t : 0;      // (-inf, and NaN, give 0)
}

__host__ __device__ inline int32_t sg_dror_cart_index(const SgDrorGrid &g, double v) { return sg_dror_clampi((v + g.rc) * g.cart_inv, g.cart_m); }

// ring of the squared range q (q = 0: the first ring)
__host__ __device__ inline int32_t sg_dror_ring(const SgDrorGrid &g, double q) { return sg_dror_clampi((0.5 * log(q) - g.ln_org) * g.ring_inv, g.n_ring); }

// azimuth bin of an angle in [-pi, pi], unwrapped: floor((phi + pi) az_inv), which may be -1 or n_az for a window's end
__host__ __device__ inline double sg_dror_az(const SgDrorGrid &g, double phi) { return floor((phi + 3.141592653589793) * g.az_inv); }

// the cell of a usable row, in [0, g.cells)
__host__ __device__ inline int32_t sg_dror_cell(const SgDrorGrid &g, double x, double y)
{
    const double q = x * x + y * y;
    if (q <= g.rc2) return sg_dror_cart_index(g, y) * g.cart_m + sg_dror_cart_index(g, x);
    int32_t a = (int32_t)sg_dror_az(g, atan2(y, x));
    if (a >= g.n_az) a -= g.n_az;                      // (phi = pi is phi = -pi)
    if (a < 0) a = 0;
    return g.cart_m * g.cart_m + sg_dror_ring(g, q) * g.n_az + a;
}

// the cells a query at (x, y) with squared radius s2 has to look at
__host__ __device__ inline void sg_dror_window(const SgDrorGrid &g, double x, double y, double s2, SgDrorWindow *w)
{
    const double r = sqrt(x * x + y * y);
    const double R = sqrt(s2) * (1.0 + SG_DROR_MARGIN) + 1e-9 * r + 1e-12;
    w->cart = r - R <= g.rc * (1.0 + 1e-9);
    w->polar = r + R >= g.rc * (1.0 - 1e-9);
    w->ix0 = w->ix1 = w->iy0 = w->iy1 = w->ring0 = w->ring1 = w->az0 = w->n_az = 0;
    if (w->cart) {
        w->ix0 = sg_dror_cart_index(g, x - R); w->ix1 = sg_dror_cart_index(g, x + R);
        w->iy0 = sg_dror_cart_index(g, y - R); w->iy1 = sg_dror_cart_index(g, y + R);
    }
    if (w->polar) {
        const double lo = r - R, hi = r + R;
        w->ring0 = lo > 0.0 ? sg_dror_ring(g, lo * lo) : 0;
        w->ring1 = sg_dror_ring(g, hi * hi);
        const double t = R / r;
        w->az0 = 0; w->n_az = g.n_az;
        if (t < 0.5) {                                  // (false for r = 0)
            const double da = asin(t) * (1.0 + SG_DROR_MARGIN) + 1e-9, phi = atan2(y, x);
            const double a0 = sg_dror_az(g, phi - da), a1 = sg_dror_az(g, phi + da);
            if (a1 - a0 + 1.0 < (double)g.n_az) {
                int32_t a = (int32_t)a0;
                w->n_az = (int32_t)(a1 - a0) + 1;
                w->az0 = a < 0 ? a + g.n_az : a >= g.n_az ? a - g.n_az : a;
            }
        }
    }
}

// whether cell `cell` (sg_dror_cell) lies in window w: the kernel walks exactly these cells
__host__ __device__ inline bool sg_dror_in_window(const SgDrorGrid &g, const SgDrorWindow &w, int32_t cell)
{
    const int32_t nc = g.cart_m * g.cart_m;
    if (cell < nc) {
        const int32_t iy = cell / g.cart_m, ix = cell - iy * g.cart_m;
        return w.cart && ix >= w.ix0 && ix <= w.ix1 && iy >= w.iy0 && iy <= w.iy1;
    }
    const int32_t ring = (cell - nc) / g.n_az, a = (cell - nc) - ring * g.n_az;
    int32_t d = a - w.az0;
    if (d < 0) d += g.n_az;
    return w.polar && ring >= w.ring0 && ring <= w.ring1 && d < w.n_az;
}
