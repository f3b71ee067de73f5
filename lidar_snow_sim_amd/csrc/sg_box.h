// sg_box.h -- points in 3D boxes (snowgpu_points_in_boxes_device; the DEFINITION: include/snowgpu.h): which boxes are present, the pose, the
// record of a box, the membership test, the grid in which the present boxes of a frame are marked and the sizes of the scratch.
// snowgpu_box.hip runs these functions on the device, tests/host_harness/box_cells.cpp the same code on the host (as sg_nn.h is compiled
// for both), and tests/box_reference.py restates the definition as brute-force NumPy.
//
// The record.  One per box, eight doubles: centre, half extents -- hx = dx / 2 + 1e-5 and hy likewise (the margin of pcdet's
// check_pt_in_box3d folded in: dx / 2 is exact, the sum is the definition's own rounded operand), hz = dz / 2 -- and the pose (c, s).
// An absent box has a record of zeros: no row is strictly inside a half extent of 0.
//
// The membership test is the definition's expression and nothing else: sx = x - cx, sy = y - cy, sz = z - cz, lx = sx c + sy s,
// ly = sy c - sx s, inside iff |sz| <= hz, |lx| < hx, |ly| < hy; float64, every operation rounded on its own.
//
// The grid.  One uniform x-y grid per frame, SG_BOX_SIDE x SG_BOX_SIDE square cells over |x|, |y| <= SG_BALL_SENSOR (120 m, the domain of
// the nearest-centres grid without a range), cell number iy SG_BOX_SIDE + ix.  The index function clamps -- rows and boxes beyond the
// domain alike fall into the border cells, which so extend to infinity on their open sides -- and is monotone in its argument (a sum
// with a constant, a product with a positive constant, a floor).  A cell holds SG_BOX_WORDS(B) 64-bit words, bit b % 64 of word b / 64 for
// box b: its size does not depend on the boxes' sizes.  One more "cell" behind them, number SG_BOX_CELLS, holds the present boxes of
// the frame.
//
// The footprint.  A present box is marked in every cell of [index(cx - wx), index(cx + wx)] x [index(cy - wy), index(cy + wy)],
//   wx = (|c| hx + |s| hy) (1 + SG_BOX_INFLATE) + SG_BOX_ROUND,     wy = (|s| hx + |c| hy) (1 + SG_BOX_INFLATE) + SG_BOX_ROUND.
// Why no member is lost: with n2 = c c + s s the rotation inverts exactly to sx = (lx c - ly s) / n2, sy = (lx s + ly c) / n2, so a row
// with |lx| < hx and |ly| < hy in exact arithmetic has |sx| < (|c| hx + |s| hy) / n2.  Three terms widen this:
//   * the 1e-5 margin: it is part of hx and hy already;
//   * the pose tolerance: n2 >= 1 - 1e-6, so 1 / n2 <= 1 + 1.1e-6, inside 1 + SG_BOX_INFLATE = 1 + 2e-6 (the other 0.9e-6 pays for the
//     five roundings of wx itself, 1.2e-16 relative each);
//   * the float64 rounding of lx and ly: sx = fl(x - cx) is within 1.2e-16 of the true difference, at most 2e6 in size; lx is two
//     products and a sum of terms no larger than 2e6 (1 + 1e-6) each: an absolute error below 4 x 1.2e-16 x 4e6 = 2e-9 m, so the computed
//     test |lx| < hx admits an exact |lx| below hx + 2e-9, which moves |sx| by at most (|c| + |s|) 2e-9 / n2 < 3e-9 m; the difference
//     cx - wx is rounded once more, 1.2e-16 x 3.5e6 = 4e-10 m.  SG_BOX_ROUND = 1e-6 m covers their sum more than a hundred times over.
// The row's cell is index((double)x): by monotonicity it lies in the marked span.  Candidates, never a lost member -- what a cell's
// bits admit beyond the members is decided by the membership test.  tests/host_harness/box_cells.cpp holds this on millions of
// (row, box) pairs.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_ball.h"        // SG_BALL_SENSOR; sg_dror_clampi; SG_FPS_BOUND

#define SG_BOX_MAX 256             /* boxes per frame: 1 <= B <= 256 */
#define SG_BOX_SIDE 64             /* cells per axis */
#define SG_BOX_CELLS (SG_BOX_SIDE * SG_BOX_SIDE)
#define SG_BOX_MARGIN 1e-5         /* check_pt_in_box3d: |lx| < dx / 2 + 1e-5 */
#define SG_BOX_POSE_TOL 1e-6       /* a pose is accepted while |c c + s s - 1| <= 1e-6 */
#define SG_BOX_INFLATE 2e-6        /* relative growth of the footprint: the pose tolerance */
#define SG_BOX_ROUND 1e-6          /* m, its absolute growth: the float64 rounding at |coordinates| <= 1e6 */

struct SgBoxRec {
    double cx, cy, cz, hx, hy, hz, c, s;
};

// 64-bit words of a cell for B boxes per frame, and the elements of the scratch: words of the bit tables (per frame SG_BOX_CELLS cells and
// the present boxes behind them) and records
__host__ __device__ inline int32_t sg_box_words(int32_t B) { return (B + 63) / 64; }
static inline size_t sg_box_table(int n_frames, int32_t B) { return (size_t)n_frames * (size_t)(SG_BOX_CELLS + 1) * (size_t)sg_box_words(B); }
static inline size_t sg_box_records(int n_frames, int32_t B) { return (size_t)n_frames * (size_t)B; }

// a row is usable iff |x|, |y|, |z| <= 1e6 (false for NaN)
template <typename T> __host__ __device__ inline bool sg_box_row_usable(T x, T y, T z)
{
    return fabs((double)x) <= SG_FPS_BOUND && fabs((double)y) <= SG_FPS_BOUND && fabs((double)z) <= SG_FPS_BOUND;
}

// The record of the box b[0 .. 6] = (cx, cy, cz, dx, dy, dz, heading) under the caller's pose (pose_in[0 .. 1]) or, with NULL, under
// cos / sin of the heading in float64.  True: the box is present.  An absent box leaves a record of zeros.
template <typename T> __host__ __device__ inline bool sg_box_make(const T *b, const double *pose_in, SgBoxRec *r)
{
    const double cx = (double)b[0], cy = (double)b[1], cz = (double)b[2], dx = (double)b[3], dy = (double)b[4], dz = (double)b[5], h = (double)b[6];
    bool ok = fabs(cx) <= SG_FPS_BOUND && fabs(cy) <= SG_FPS_BOUND && fabs(cz) <= SG_FPS_BOUND && dx > 0.0 && dx <= SG_FPS_BOUND && dy > 0.0 &&
              dy <= SG_FPS_BOUND && dz > 0.0 && dz <= SG_FPS_BOUND && fabs(h) <= SG_FPS_BOUND;                    // (false for NaN and inf)
    double c = 0.0, s = 0.0;
    if (ok) {
        c = pose_in ? pose_in[0] : cos(h);
        s = pose_in ? pose_in[1] : sin(h);
        ok = fabs((c * c + s * s) - 1.0) <= SG_BOX_POSE_TOL;                                                      // (false for NaN and inf)
    }
    r->cx = ok ? cx : 0.0; r->cy = ok ? cy : 0.0; r->cz = ok ? cz : 0.0;
    r->hx = ok ? dx * 0.5 + SG_BOX_MARGIN : 0.0; r->hy = ok ? dy * 0.5 + SG_BOX_MARGIN : 0.0; r->hz = ok ? dz * 0.5 : 0.0;
    r->c = ok ? c : 0.0; r->s = ok ? s : 0.0;
    return ok;
}

// the membership test of a present box; the local coordinates come back whatever the answer
__host__ __device__ inline bool sg_box_inside(const SgBoxRec &r, double x, double y, double z, double *lx, double *ly, double *sz)
{
    const double sx = x - r.cx, sy = y - r.cy;
    *sz = z - r.cz;
    *lx = sx * r.c + sy * r.s;
    *ly = sy * r.c - sx * r.s;
    return fabs(*sz) <= r.hz && fabs(*lx) < r.hx && fabs(*ly) < r.hy;
}

// the cell index of a coordinate on either axis, in [0, SG_BOX_SIDE)
__host__ __device__ inline int32_t sg_box_index(double v) { return sg_dror_clampi((v + SG_BALL_SENSOR) * (SG_BOX_SIDE / (2.0 * SG_BALL_SENSOR)), SG_BOX_SIDE); }

// the cell of a usable row
__host__ __device__ inline int32_t sg_box_cell(double x, double y) { return sg_box_index(y) * SG_BOX_SIDE + sg_box_index(x); }

// the cells [ix0, ix1] x [iy0, iy1] that the footprint of a present box can touch
__host__ __device__ inline void sg_box_footprint(const SgBoxRec &r, int32_t *ix0, int32_t *ix1, int32_t *iy0, int32_t *iy1)
{
    const double ac = fabs(r.c), as = fabs(r.s);
    const double wx = (ac * r.hx + as * r.hy) * (1.0 + SG_BOX_INFLATE) + SG_BOX_ROUND;
    const double wy = (as * r.hx + ac * r.hy) * (1.0 + SG_BOX_INFLATE) + SG_BOX_ROUND;
    *ix0 = sg_box_index(r.cx - wx); *ix1 = sg_box_index(r.cx + wx);
    *iy0 = sg_box_index(r.cy - wy); *iy1 = sg_box_index(r.cy + wy);
}
