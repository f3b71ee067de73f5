// sg_nn.h -- nearest centres of every row (snowgpu_nearest_centres_device; the DEFINITION: include/snowgpu.h): the grid in which the usable
// centres of a frame are filed, the ring walk of a row, its stopping bound, the k-best insertion, the weights and the sizes of the
// scratch.  snowgpu_nn.hip runs these functions on the device, tests/host_harness/nn_walk.cpp the same code on the host (as sg_ball.h
// and sg_fps.h are compiled for both), and tests/nn_reference.py restates the definition as brute-force NumPy.  The usable tests and the
// distance are the siblings' (sg_fps_usable, sg_fps_dist in sg_fps.h; sg_ball_centre_usable in sg_ball.h): they are not restated here.
//
// The grid.  One uniform x-y grid per frame, nx x ny square cells, cell number iy nx + ix: the cells [a, b] of one grid row are ONE
// contiguous span of the sorted copy.  Its domain is sg_ball_make_grid's: the x-y rectangle of the range where the range gives finite
// bounds within 1e6, |x|, |y| <= SG_BALL_SENSOR where it does not.  The index functions clamp -- what lies beyond the domain, rows and
// centres alike, is filed in the border cells -- and are monotone in their argument (a subtraction, a product with a positive constant, a
// floor).  There is no radius: the cells are sized by the number of centres.  budget = K / SG_NN_PER_CELL (rounded up) within
// SG_NN_MIN_CELLS .. SG_NN_MAX_CELLS, edge = sqrt(area / budget), nx = ceil(width / edge), ny = ceil(height / edge), and the edge grows by
// 5 % at a time while nx ny is above the budget.  Two centres per cell on average: with centres spread evenly the third nearest lies 0.7
// edges away, so a row ends after the 9 cells of rings 0 and 1 (some 18 candidates); at one per cell it would need ring 2 half of the
// time (25 cells), at four per cell ring 1 still (36 candidates).  The upper end keeps the counters of one frame in 8 KiB of LDS, so one
// workgroup files a frame in one kernel.  The grid depends on K and the range alone, never on the data.
//
// The walk.  One row walks rings of growing Chebyshev radius s around its own cell (ix, iy): the cells of the block
// [ix - s, ix + s] x [iy - s, iy + s] that the block of ring s - 1 did not hold -- the full top and bottom grid rows as one span each, the
// two end cells of every grid row between them --, all clipped to the OCCUPIED BOX of the frame (the smallest rectangle of cells that
// holds every usable centre).  The first ring is the Chebyshev distance from the row's cell to that box: a row far from every centre
// walks no empty ring.
//
// The stopping bound.  After ring s the visited cells are the block, clipped.  A side of the block that lies on or beyond the matching
// side of the occupied box has no usable centre behind it: its gap is +inf.  Behind any other side -- say the left one, column
// j = ix - s > box.ix0 >= 0 -- every unvisited centre has an index below j, so by monotonicity its x lies below the cell boundary
// L = x0 + j edge, while the row, whose index is at least j, lies at or above it: |x - x_c| >= x - L.  b = the smallest of the four gaps
// bounds the x-y distance, hence the distance, of EVERY unvisited centre from below.  What the arithmetic adds:
//   * the index is floor(fl(fl(v - x0) inv)), L is fl(x0 + fl(j edge)) and the gap one more subtraction: relative errors of 1.2e-16 on
//     numbers no larger than |x0| + the domain's width + |v|, v the row's coordinate.  SG_NN_SLACK (1e-9) times (reach + max(|x|, |y|)),
//     reach = the largest absolute coordinate of the domain's corners, plus 1e-12 m covers them a million times over;
//   * the distance in T is d = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) with dx = fl(x - x_c).  Rounding is monotone and the terms are
//     not negative, so d >= fl(dx dx) >= (|x - x_c| (1 - 2^-24))^2 (1 - 2^-24) in float32: 1.8e-7 relative below the true square, inside
//     (1 - SG_NN_MARGIN)^2 = 1 - 2e-6.  (No product is subnormal where the bound is positive: the slack keeps b > 0 to gaps above 1e-12 m.)
// So with B = max(0, b (1 - SG_NN_MARGIN) - slack), B^2 <= d(row, c) in T for every unvisited centre c.  The walk stops when all four
// gaps are +inf (everything is visited), or when (double)d_k < B^2, d_k the k-th kept distance (+inf while a slot is empty): STRICT, so an
// unvisited centre can neither beat nor tie a kept one, and the kept ones are the definition's first k whatever the ring order and the
// order inside the cells.  tests/host_harness/nn_walk.cpp checks B^2 <= d over millions of (row, block, outside centre) triples.
//
// The k best.  A lane keeps its KK = k best keys ascending in registers; KK is a template argument (one instance per k in 1 .. 8: a
// run-time k below KK would have the k-th slot chosen by a run-time number, which the compiler turns into an indexed array in memory)
// and every loop over the slots unrolls, so no slot is indexed by a run-time number.  float32: one 64-bit key, bits(d) << 32 | centre (d is neither negative nor NaN,
// so its bits order as an integer).  float64: the pair, compared in turn.  An empty slot is (+inf, -1), above every real key, and is
// what the outputs of an unfilled slot are read from.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_ball.h"        // SG_BALL_SENSOR, sg_ball_centre_usable; sg_dror_clampi; SgFpsRange, sg_fps_usable, sg_fps_dist, sg_fps_bits

#define SG_NN_MAX_K 8              /* neighbours of a row: 1 <= k <= 8 */
#define SG_NN_PER_CELL 2           /* centres per cell the grid aims at */
#define SG_NN_MIN_CELLS 16         /* cell budget per frame: at least this, */
#define SG_NN_MAX_CELLS 2048       /* at most this: the counters of a frame stay in LDS */
#define SG_NN_MARGIN 1e-6          /* relative deflation of the stopping bound: the rounding of the distance in T */
#define SG_NN_SLACK 1e-9           /* ... and, times (reach + max(|x|, |y|)), its absolute deflation: the double arithmetic of the cells */
#define SG_NN_EPS 1e-8             /* weights: u = 1 / (sqrt(d) + 1e-8), pointnet2's three_nn */

struct SgNnGrid {
    double x0, y0, inv, edge;      // cell (ix, iy) of a point: floor((x - x0) inv), floor((y - y0) inv), clamped; edge = the cell's width
    double reach;                  // the largest |coordinate| of the domain's corners
    int32_t nx, ny, cells;         // cells = nx ny
};

struct SgNnBox {
    int32_t ix0, ix1, iy0, iy1;    // the occupied cells [ix0, ix1] x [iy0, iy1] of a frame; ix0 > ix1: no usable centre
};

// one usable centre in the sorted copy: a candidate costs one load
template <typename T> struct SgNnRec;
template <> struct alignas(16) SgNnRec<float> { float x, y, z; int32_t c; };
template <> struct alignas(32) SgNnRec<double> { double x, y, z; int64_t c; };

// cells per frame for K centres per frame
static inline int32_t sg_nn_cell_budget(int64_t K)
{
    const int64_t want = (K + SG_NN_PER_CELL - 1) / SG_NN_PER_CELL;
    return (int32_t)(want < SG_NN_MIN_CELLS ? SG_NN_MIN_CELLS : want > SG_NN_MAX_CELLS ? SG_NN_MAX_CELLS : want);
}

// elements of the entry table (per frame the first position of every cell, then the number of usable centres), of the boxes (int32) and
// of the sorted copy (records)
static inline size_t sg_nn_entries(int n_frames, int32_t cells) { return (size_t)n_frames * ((size_t)cells + 1); }
static inline size_t sg_nn_boxes(int n_frames) { return (size_t)n_frames * 4; }
static inline size_t sg_nn_records(int n_frames, int64_t K) { return (size_t)n_frames * (size_t)K; }

// The grid of one call: range6 = (x0, y0, z0, x1, y1, z1) or NULL, K >= 1 centres per frame.
static inline void sg_nn_make_grid(const double *range6, int64_t K, SgNnGrid *g)
{
    double lo[2], hi[2];
    for (int j = 0; j < 2; ++j) {                                                                 // (sg_ball_make_grid's domain)
        lo[j] = range6 && fabs(range6[j]) <= SG_FPS_BOUND ? range6[j] : -SG_BALL_SENSOR;
        hi[j] = range6 && fabs(range6[3 + j]) <= SG_FPS_BOUND ? range6[3 + j] : SG_BALL_SENSOR;
        if (!(lo[j] < hi[j])) hi[j] = lo[j] + 2.0 * SG_BALL_SENSOR;
    }
    const double budget = (double)sg_nn_cell_budget(K), wx = hi[0] - lo[0], wy = hi[1] - lo[1];
    double edge = sqrt(wx * wy / budget);
    for (;;) {
        const double fx = fmax(1.0, ceil(wx / edge)), fy = fmax(1.0, ceil(wy / edge));
        if (fx * fy <= budget) {
            g->nx = (int32_t)fx;
            g->ny = (int32_t)fy;
            break;
        }
        edge *= 1.05;
    }
    g->x0 = lo[0];
    g->y0 = lo[1];
    g->edge = edge;
    g->inv = 1.0 / edge;
    g->cells = g->nx * g->ny;
    const double cx = fmax(fabs(lo[0]), fabs(lo[0] + g->nx * edge)), cy = fmax(fabs(lo[1]), fabs(lo[1] + g->ny * edge));
    g->reach = fmax(cx, cy);
}

__host__ __device__ inline int32_t sg_nn_ix(const SgNnGrid &g, double x) { return sg_dror_clampi((x - g.x0) * g.inv, g.nx); }
__host__ __device__ inline int32_t sg_nn_iy(const SgNnGrid &g, double y) { return sg_dror_clampi((y - g.y0) * g.inv, g.ny); }

// (The functions that take the k best by reference are __forceinline__: a call that is not inlined would put the slots in memory.)
// ---- the keys ---------------------------------------------------------------------------------------------------------------------------
template <typename T> struct SgNnKey;
template <> struct SgNnKey<float> {
    uint64_t w;                    // bits of d << 32 | centre
};
template <> struct SgNnKey<double> {
    double d;
    int32_t c;
};

__host__ __device__ inline SgNnKey<float> sg_nn_key(float d, int32_t c) { return SgNnKey<float>{((uint64_t)sg_fps_bits(d) << 32) | (uint32_t)c}; }
__host__ __device__ inline SgNnKey<double> sg_nn_key(double d, int32_t c) { return SgNnKey<double>{d, c}; }
// the empty slot: (+inf, -1)
template <typename T> __host__ __device__ inline SgNnKey<T> sg_nn_no_key();
template <> __host__ __device__ inline SgNnKey<float> sg_nn_no_key<float>() { return SgNnKey<float>{0x7f800000ffffffffull}; }
template <> __host__ __device__ inline SgNnKey<double> sg_nn_no_key<double>() { return SgNnKey<double>{(double)INFINITY, -1}; }

// (d, centre) of a before that of b
__host__ __device__ inline bool sg_nn_less(SgNnKey<float> a, SgNnKey<float> b) { return a.w < b.w; }
__host__ __device__ inline bool sg_nn_less(SgNnKey<double> a, SgNnKey<double> b) { return a.d < b.d || (a.d == b.d && (uint32_t)a.c < (uint32_t)b.c); }

// a if take else b, member by member (a conditional expression on the whole pair would select between two addresses: memory)
__host__ __device__ inline SgNnKey<float> sg_nn_pick(bool take, SgNnKey<float> a, SgNnKey<float> b) { return SgNnKey<float>{take ? a.w : b.w}; }
__host__ __device__ inline SgNnKey<double> sg_nn_pick(bool take, SgNnKey<double> a, SgNnKey<double> b) { return SgNnKey<double>{take ? a.d : b.d, take ? a.c : b.c}; }

__host__ __device__ inline float sg_nn_key_d(SgNnKey<float> k) { return sg_fps_unbits((uint32_t)(k.w >> 32)); }
__host__ __device__ inline double sg_nn_key_d(SgNnKey<double> k) { return k.d; }
__host__ __device__ inline int32_t sg_nn_key_c(SgNnKey<float> k) { return (int32_t)(uint32_t)k.w; }
__host__ __device__ inline int32_t sg_nn_key_c(SgNnKey<double> k) { return k.c; }

template <typename T, int KK> __host__ __device__ __forceinline__ void sg_nn_clear(SgNnKey<T> (&best)[KK])
{
#pragma unroll
    for (int j = 0; j < KK; ++j) best[j] = sg_nn_no_key<T>();
}

// best (ascending) takes `key` up if it comes before its last slot: the insertion, every slot from its old neighbours
template <typename T, int KK> __host__ __device__ __forceinline__ void sg_nn_insert(SgNnKey<T> (&best)[KK], SgNnKey<T> key)
{
    if (!sg_nn_less(key, best[KK - 1])) return;
#pragma unroll
    for (int j = KK - 1; j > 0; --j) best[j] = sg_nn_pick(sg_nn_less(key, best[j - 1]), best[j - 1], sg_nn_pick(sg_nn_less(key, best[j]), key, best[j]));
    best[0] = sg_nn_pick(sg_nn_less(key, best[0]), key, best[0]);
}

// the KK-th kept distance as a double (+inf while the last slot is empty)
template <typename T, int KK> __host__ __device__ __forceinline__ double sg_nn_kth(const SgNnKey<T> (&best)[KK]) { return (double)sg_nn_key_d(best[KK - 1]); }

// ---- the stopping bound -------------------------------------------------------------------------------------------------------------------
// B^2 for a row at (x, y) after the cells [jx0, jx1] x [jy0, jy1] (around the row's own cell; not clipped) are visited: no usable centre
// of the frame outside them is nearer than B.  +inf: there is none outside them.
__host__ __device__ inline double sg_nn_bound(const SgNnGrid &g, const SgNnBox &box, double x, double y, int32_t jx0, int32_t jx1, int32_t jy0, int32_t jy1)
{
    double b = (double)INFINITY;
    if (jx0 > box.ix0) b = fmin(b, x - (g.x0 + (double)jx0 * g.edge));
    if (jx1 < box.ix1) b = fmin(b, (g.x0 + (double)(jx1 + 1) * g.edge) - x);
    if (jy0 > box.iy0) b = fmin(b, y - (g.y0 + (double)jy0 * g.edge));
    if (jy1 < box.iy1) b = fmin(b, (g.y0 + (double)(jy1 + 1) * g.edge) - y);
    if (b == (double)INFINITY) return b;
    const double ax = fabs(x), ay = fabs(y);
    b = b * (1.0 - SG_NN_MARGIN) - (SG_NN_SLACK * (g.reach + (ax > ay ? ax : ay)) + 1e-12);
    return b > 0.0 ? b * b : 0.0;
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------------
// the records [p0, p1) of the frame's sorted copy against the row
template <typename T, int KK>
__host__ __device__ __forceinline__ void sg_nn_span(const SgNnRec<T> *__restrict__ rec, uint32_t p0, uint32_t p1, T x, T y, T z, SgNnKey<T> (&best)[KK])
{
    for (uint32_t p = p0; p < p1; ++p) {
        const SgNnRec<T> r = rec[p];
        sg_nn_insert<T, KK>(best, sg_nn_key(sg_fps_dist<T>(x, y, z, r.x, r.y, r.z), (int32_t)r.c));
    }
}

// The KK nearest usable centres of a usable row at (x, y, z) into best (cleared by the caller).
// entry: the frame's cells + 1 first positions; rec: the frame's sorted copy; box: its occupied cells.
template <typename T, int KK>
__host__ __device__ __forceinline__ void sg_nn_walk(const SgNnGrid &g, const SgNnBox &box, const uint32_t *__restrict__ entry, const SgNnRec<T> *__restrict__ rec,
                                           T x, T y, T z, SgNnKey<T> (&best)[KK])
{
    if (box.ix0 > box.ix1) return;
    const int32_t ix = sg_nn_ix(g, (double)x), iy = sg_nn_iy(g, (double)y);
    int32_t s = 0;                                                         // the first ring that meets the occupied box
    s = box.ix0 - ix > s ? box.ix0 - ix : s;
    s = ix - box.ix1 > s ? ix - box.ix1 : s;
    s = box.iy0 - iy > s ? box.iy0 - iy : s;
    s = iy - box.iy1 > s ? iy - box.iy1 : s;
    for (;; ++s) {
        const int32_t jx0 = ix - s, jx1 = ix + s, jy0 = iy - s, jy1 = iy + s;
        const int32_t xa = jx0 > box.ix0 ? jx0 : box.ix0, xb = jx1 < box.ix1 ? jx1 : box.ix1;
        const int32_t ya = jy0 > box.iy0 ? jy0 : box.iy0, yb = jy1 < box.iy1 ? jy1 : box.iy1;
        for (int32_t jy = ya; jy <= yb; ++jy) {
            const uint32_t *e = entry + jy * g.nx;
            if (jy == jy0 || jy == jy1) {                                  // the ring's top or bottom grid row: one span
                if (xa <= xb) sg_nn_span<T, KK>(rec, e[xa], e[xb + 1], x, y, z, best);
            } else {                                                       // between them: the ring's two end cells
                if (jx0 >= box.ix0) sg_nn_span<T, KK>(rec, e[jx0], e[jx0 + 1], x, y, z, best);
                if (jx1 <= box.ix1) sg_nn_span<T, KK>(rec, e[jx1], e[jx1 + 1], x, y, z, best);
            }
        }
        const double bb = sg_nn_bound(g, box, (double)x, (double)y, jx0, jx1, jy0, jy1);
        if (bb == (double)INFINITY || sg_nn_kth<T, KK>(best) < bb) return;
    }
}

// ---- the weights --------------------------------------------------------------------------------------------------------------------------
// u_j = 1 / (sqrt((double)d_j) + 1e-8) over the filled slots, n = ((u_0 + u_1) + u_2) + ..., weight_j = T(u_j / n): every operation in
// float64 and rounded on its own; 0 for an empty slot.
template <typename T, int KK> __host__ __device__ __forceinline__ void sg_nn_weights(const SgNnKey<T> (&best)[KK], T (&w)[KK])
{
    double u[KK], n = 0.0;
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        const bool filled = sg_nn_key_c(best[j]) >= 0;
        u[j] = filled ? 1.0 / (sqrt((double)sg_nn_key_d(best[j])) + SG_NN_EPS) : 0.0;
        n = j == 0 ? u[0] : n + u[j];                                      // (+ 0.0 changes nothing: the sum of the filled slots, in slot order)
    }
#pragma unroll
    for (int j = 0; j < KK; ++j) w[j] = u[j] > 0.0 ? (T)(u[j] / n) : (T)0;
}
