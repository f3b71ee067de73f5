// sg_ball.h -- ball-query neighbour groups around keypoints (snowgpu_ball_query_device; the DEFINITION: include/snowgpu.h): the grid in
// which the usable rows of a frame are filed, the window of a centre, the compare-exchange network of the selection and the sizes of the
// scratch.  snowgpu_ball.hip runs these functions on the device, tests/host_harness/ball_cells.cpp and ball_select.cpp the same code on
// the host (as sg_dror.h and sg_fps.h are compiled for both), and tests/ball_reference.py restates the definition as brute-force NumPy.
// The usable test and the distance are the keypoint stage's (sg_fps_usable, sg_fps_dist in sg_fps.h): they are not restated here.
//
// The grid.  One uniform x-y grid per frame, nx x ny square cells, cell number iy nx + ix: a grid row of a window is ONE contiguous span
// of the sorted copy.  Its domain is the x-y rectangle of the range where the range gives finite bounds within 1e6, and
// |x|, |y| <= SG_BALL_SENSOR (120 m, the sensor's limit) where it does not.  The index functions clamp -- what lies beyond the domain is
// filed in the border cells -- and are monotone in their argument (a subtraction, a product with a positive constant, a floor), so the
// window [index(c - r'), index(c + r')] holds the cell of every row within r' of the centre on that axis whatever the cell width.
// r' = r_max (1 + SG_DROR_MARGIN) + 1e-9 max(|cx|, |cy|) + 1e-12: the rounding of the membership test in float32 (the radius, its square,
// three differences, three products and two sums: below 4e-7 relative on the distance) and of the window's own double arithmetic lie far
// inside it.  The exact test alone decides membership.
//
// The cell edge.  A call has up to four radii and walks ONE window per centre, that of the largest radius r_max: every distance is
// computed once and compared against all radii.  The edge is r_max / 2: spans are contiguous along x, so narrower cells cost no more
// spans along x and trim the window to (2 r' + up to one edge)^2 -- 6.25 r_max^2 on average, against 9 r_max^2 at an edge of r_max --, and
// five short grid rows instead of three is what a wave's 64 lanes take in one or two strides anyway.  A smaller radius of the same call
// only tests the candidates of the large one: its work is a compare and a ballot per candidate batch.  Where nx ny would exceed the cell
// budget (sg_ball_cell_budget: DROR's bounds) the edge is made wider by one factor for both axes: more candidates, never fewer neighbours.
//
// The selection.  Per (radius, samples) pair a wave keeps the 64 smallest row indices seen so far, ascending, one per lane, INT32_MAX in
// an empty lane.  A batch of 64 candidates (INT32_MAX in the lanes outside the ball) is sorted by the bitonic network of
// SG_BALL_SORT_STEPS compare-exchange steps below, then merged: min(kept[l], batch[63 - l]) is a bitonic sequence of the 64 smallest of
// both, and six half-cleaner steps (distances 32 .. 1, all ascending) sort it.  sg_ball_cx is the one compare-exchange; the kernel runs it
// with its partner's value fetched across the wave, the host walkers below over an array of 64 "lanes".
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_dror.h"        // SG_DROR_MARGIN, SG_DROR_MIN_CELLS, SG_DROR_MAX_CELLS, sg_dror_clampi
#include "sg_fps.h"         // SgFpsRange, sg_fps_usable, sg_fps_dist, SG_FPS_BOUND

#define SG_BALL_MAX_RADII 4        /* (radius, samples) pairs of a call */
#define SG_BALL_MAX_SAMPLES 64     /* samples of a pair: one lane each */
#define SG_BALL_RADIUS_MAX 1e6     /* domain: 0 < radius <= 1e6, finite */
#define SG_BALL_SENSOR 120.0       /* m: the grid's domain on an axis without a finite range bound */
#define SG_BALL_EMPTY 0x7fffffff   /* the index of an empty lane: above every row index */
#define SG_BALL_SORT_STEPS 21      /* compare-exchange steps of the bitonic sort of 64 */

struct SgBallGrid {
    double x0, y0, inv;            // cell (ix, iy) of a point: floor((x - x0) inv), floor((y - y0) inv), clamped
    int32_t nx, ny, cells;         // cells = nx ny
    double reach;                  // r_max, as a double at least the largest radius in the rows' dtype
};

struct SgBallWindow {
    int32_t ix0, ix1, iy0, iy1;    // the cells [ix0, ix1] x [iy0, iy1]
};

// the (radius, samples) pairs of a call for rows of type T: r2 = fl(fl(radius) fl(radius)), first output slot and number of slots per pair
template <typename T> struct SgBallPairs {
    T r2[SG_BALL_MAX_RADII];
    int32_t samples[SG_BALL_MAX_RADII], seg[SG_BALL_MAX_RADII];
    int32_t n_radii, total;        // total = the sum of the samples: S
};

// cells per frame for a batch whose longest frame has max_frame rows (sg_dror_cell_budget's shape and bounds)
static inline int32_t sg_ball_cell_budget(int64_t max_frame) { return sg_dror_cell_budget(max_frame); }

// elements of the entry table: per frame one first position and one per cell
static inline size_t sg_ball_entries(int n_frames, int32_t cells) { return (size_t)n_frames * ((size_t)cells + 1); }
// elements of the cell-of-row array and of each array of the sorted copy (x, y, z in the rows' dtype, the source row as int32)
static inline size_t sg_ball_scratch(int64_t n) { return (size_t)n; }

template <typename T>
static inline void sg_ball_make_pairs(int n_radii, const double *radii, const int *n_samples, SgBallPairs<T> *p)
{
    p->n_radii = n_radii;
    p->total = 0;
    for (int i = 0; i < SG_BALL_MAX_RADII; ++i) {
        const volatile T r = i < n_radii ? (T)radii[i] : (T)0;      // (volatile: the product is rounded to T, never kept wider)
        const volatile T r2 = r * r;
        p->r2[i] = r2;
        p->samples[i] = i < n_radii ? n_samples[i] : 0;
        p->seg[i] = p->total;
        p->total += p->samples[i];
    }
}

// The grid of one call: range6 = (x0, y0, z0, x1, y1, z1) or NULL, radii within the domain.  budget: cells per frame at most.
static inline void sg_ball_make_grid(const double *range6, int n_radii, const double *radii, int32_t budget, SgBallGrid *g)
{
    double lo[2], hi[2];
    for (int j = 0; j < 2; ++j) {
        lo[j] = range6 && fabs(range6[j]) <= SG_FPS_BOUND ? range6[j] : -SG_BALL_SENSOR;          // (false for an infinite bound)
        hi[j] = range6 && fabs(range6[3 + j]) <= SG_FPS_BOUND ? range6[3 + j] : SG_BALL_SENSOR;
        if (!(lo[j] < hi[j])) hi[j] = lo[j] + 2.0 * SG_BALL_SENSOR;                               // (one bound finite beyond the sensor's limit)
    }
    double rmax = 0.0;
    for (int i = 0; i < n_radii; ++i) rmax = radii[i] > rmax ? radii[i] : rmax;
    g->reach = rmax * (1.0 + 1e-7);                    // (float32 may round a radius up)
    if (budget < SG_DROR_MIN_CELLS) budget = SG_DROR_MIN_CELLS;
    const double edge = 0.5 * rmax, wx = hi[0] - lo[0], wy = hi[1] - lo[1];
    double k = 1.0;
    for (;;) {
        const double fx = floor(wx / (edge * k)) + 1.0, fy = floor(wy / (edge * k)) + 1.0;
        if (fx * fy <= (double)budget) {
            g->nx = (int32_t)fx;
            g->ny = (int32_t)fy;
            break;
        }
        const double need = sqrt(fx * fy / (double)budget);
        k *= need > 1.05 ? need : 1.05;
    }
    g->x0 = lo[0];
    g->y0 = lo[1];
    g->inv = 1.0 / (edge * k);
    g->cells = g->nx * g->ny;
}

__host__ __device__ inline int32_t sg_ball_ix(const SgBallGrid &g, double x) { return sg_dror_clampi((x - g.x0) * g.inv, g.nx); }
__host__ __device__ inline int32_t sg_ball_iy(const SgBallGrid &g, double y) { return sg_dror_clampi((y - g.y0) * g.inv, g.ny); }

// the cell of a usable row, in [0, g.cells)
__host__ __device__ inline int32_t sg_ball_cell(const SgBallGrid &g, double x, double y) { return sg_ball_iy(g, y) * g.nx + sg_ball_ix(g, x); }

// a centre is usable iff |x|, |y|, |z| <= 1e6 (false for NaN); it need not lie in the range
template <typename T> __host__ __device__ inline bool sg_ball_centre_usable(T x, T y, T z)
{
    return fabs((double)x) <= SG_FPS_BOUND && fabs((double)y) <= SG_FPS_BOUND && fabs((double)z) <= SG_FPS_BOUND;
}

// the cells a usable centre at (x, y) has to look at
__host__ __device__ inline void sg_ball_window(const SgBallGrid &g, double x, double y, SgBallWindow *w)
{
    const double ax = fabs(x), ay = fabs(y);
    const double R = g.reach * (1.0 + SG_DROR_MARGIN) + 1e-9 * (ax > ay ? ax : ay) + 1e-12;
    w->ix0 = sg_ball_ix(g, x - R); w->ix1 = sg_ball_ix(g, x + R);
    w->iy0 = sg_ball_iy(g, y - R); w->iy1 = sg_ball_iy(g, y + R);
}

// whether cell `cell` (sg_ball_cell) lies in window w: the kernel walks exactly these cells
__host__ __device__ inline bool sg_ball_in_window(const SgBallGrid &g, const SgBallWindow &w, int32_t cell)
{
    const int32_t iy = cell / g.nx, ix = cell - iy * g.nx;
    return ix >= w.ix0 && ix <= w.ix1 && iy >= w.iy0 && iy <= w.iy1;
}

// ---- the selection network ------------------------------------------------------------------------------------------------------------------
// Step s of the bitonic sort of 64 lanes: lanes l and l ^ j exchange, within blocks of k lanes that sort ascending where (l & k) == 0 and
// descending elsewhere (k = 64: ascending everywhere).  k = 2, 4, 4, 8, 8, 8, ...; j = k / 2 down to 1.
__host__ __device__ constexpr int sg_ball_step_k(int s)
{
    int k = 2;
    for (int stage = 1; s >= stage; ++stage) { s -= stage; k <<= 1; }
    return k;
}
__host__ __device__ constexpr int sg_ball_step_j(int s)
{
    int stage = 1;
    for (; s >= stage; ++stage) s -= stage;
    return 1 << (stage - 1 - s);
}

// what lane `lane` keeps of its own value and that of lane ^ j in a block of k
__host__ __device__ inline int32_t sg_ball_cx(int32_t mine, int32_t other, int lane, int j, int k)
{
    const bool lower = (lane & j) == 0, ascending = (lane & k) == 0;
    const int32_t lo = other < mine ? other : mine, hi = other < mine ? mine : other;
    return lower == ascending ? lo : hi;
}

// the sort over an array of 64 lanes
__host__ __device__ inline void sg_ball_sort_lanes(int32_t v[64])
{
    for (int s = 0; s < SG_BALL_SORT_STEPS; ++s) {
        const int j = sg_ball_step_j(s), k = sg_ball_step_k(s);
        int32_t nv[64];
        for (int l = 0; l < 64; ++l) nv[l] = sg_ball_cx(v[l], v[l ^ j], l, j, k);
        for (int l = 0; l < 64; ++l) v[l] = nv[l];
    }
}

// what lane `lane` holds before the half-cleaner steps of a merge: the smaller of its kept value and the batch's value of lane 63 - lane
__host__ __device__ inline int32_t sg_ball_meet(int32_t kept, int32_t mirrored) { return mirrored < kept ? mirrored : kept; }

// kept (ascending) and batch (ascending) over arrays of 64 lanes: kept becomes the 64 smallest of both, ascending
__host__ __device__ inline void sg_ball_merge_lanes(int32_t kept[64], const int32_t batch[64])
{
    int32_t v[64], nv[64];
    for (int l = 0; l < 64; ++l) v[l] = sg_ball_meet(kept[l], batch[63 - l]);
    for (int j = 32; j > 0; j >>= 1) {
        for (int l = 0; l < 64; ++l) nv[l] = sg_ball_cx(v[l], v[l ^ j], l, j, 64);
        for (int l = 0; l < 64; ++l) v[l] = nv[l];
    }
    for (int l = 0; l < 64; ++l) kept[l] = v[l];
}

// whether a batch has to be taken up: some lane is in the ball with an index below the S-th kept one
__host__ __device__ inline bool sg_ball_wanted(bool in_ball, int32_t index, int32_t kept_sth) { return in_ball && index < kept_sth; }
