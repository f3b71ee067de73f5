// sg_centers.h -- centre heatmap targets (snowgpu_assign_centers_device; the DEFINITION: include/snowgpu.h): which gt boxes are present, the
// centre pixel and its fractional offset, the Gaussian radius, the slot of a gt in its head, the value of a pixel under a gt and which gts
// can reach a tile of the map.  snowgpu_centers.hip runs these functions on the device, tests/host_harness/centers_walk.cpp runs
// sg_centers_frame, the same code in one thread, on the host (as sg_anchors.h is compiled for both), and tests/centers_reference.py restates
// the definition as sequential NumPy.
//
// Everything is float64 computed from (double) of the inputs, every operation rounded on its own (-ffp-contract=off).  Divisions and square
// roots are correctly rounded on both sides; the one transcendental function is the exp of a pixel's value, whose float64 result is
// rounded to float32 -- include/snowgpu.h says why the float32 is the same on both sides.  Presence is sg_box_make's rule under the unit
// pose (1, 0), whose pose check always holds.
//
// The record.  One per gt, 24 bytes: den = 2 sigma^2 of its Gaussian, the centre pixel, the radius and the class -- 0 for a gt that is not
// drawn (absent, dropped or without a slot).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_box.h"         // presence: sg_box_make; SG_BOX_MAX

#define SG_CENTERS_GT_MAX SG_BOX_MAX    /* gt boxes per frame: 1 <= B <= 256 */
#define SG_CENTERS_CLASSES_MAX 16       /* 1 <= NC <= 16 */
#define SG_CENTERS_HEADS_MAX 16         /* 1 <= NH <= 16 */
#define SG_CENTERS_OBJS_MAX 512         /* 1 <= M <= 512 */
#define SG_CENTERS_RADIUS_MAX 512       /* the cap of the radius: tests/test_centers_reference.py walks every radius up to it */
#define SG_CENTERS_TILE_W 64            /* a tile of the map: 64 pixels of a row are one wave's store of 256 bytes ... */
#define SG_CENTERS_TILE_H 16            /* ... and 16 rows share one list of gts: a workgroup of 256 lanes, four rows a lane */

#define SG_CENTERS_ABSENT 0
#define SG_CENTERS_DRAWN 1
#define SG_CENTERS_DROPPED 2
#define SG_CENTERS_NO_SLOT 3

struct SgCenterCfg {                    // the settings as the kernels take them
    double x0, y0, vx, vy, stride, overlap;
    int32_t W, H, n_classes, n_heads, max_objs, min_radius, drop;       // drop: outside == 'drop'
    int32_t class_head[SG_CENTERS_CLASSES_MAX];                         // class c at [c - 1]
};

struct SgCenterRec {                    // cls 0: not drawn
    double den;
    int32_t cix, ciy, r, cls;
};

struct SgCenterGt {                     // what a gt is before its slot is known; state: ABSENT, DROPPED or DRAWN (a slot permitting)
    double offx, offy, den;
    int32_t cix, ciy, r, cls, head, state;
};

template <typename T> struct SgCenterOut {      // the outputs of the whole batch
    float *heatmap;
    int32_t *gt_index, *ind;
    uint8_t *mask;
    T *offset;
    int32_t *radius, *count;
    uint8_t *state;
};

// c = min(max(coord, 0), size - 0.5) (0 for NaN), its whole part and the rest, which is exact: 0 <= c < 2^31 and c - trunc(c) has no more
// bits than c
__host__ __device__ inline void sg_centers_pixel(double coord, int32_t size, int32_t *ci, double *off)
{
    const double hi = (double)size - 0.5;
    double c = coord > 0.0 ? coord : 0.0;
    c = c < hi ? c : hi;
    *ci = (int32_t)c;
    *off = c - (double)*ci;
}

// The Gaussian radius of a box of h x w pixels: the smallest of pcdet's three roots, truncated, at least min_radius, at most
// SG_CENTERS_RADIUS_MAX.  A NaN (inf - inf of a box of more than 1e154 pixels) fails every comparison and gives min_radius.
__host__ __device__ inline int32_t sg_centers_radius(double h, double w, double o, int32_t min_radius)
{
    const double b1 = h + w, c1 = w * h * (1.0 - o) / (1.0 + o);
    const double r1 = (b1 + sqrt(b1 * b1 - 4.0 * c1)) / 2.0;
    const double b2 = 2.0 * (h + w), c2 = (1.0 - o) * w * h;
    const double r2 = (b2 + sqrt(b2 * b2 - 16.0 * c2)) / 2.0;
    const double b3 = -2.0 * o * (h + w), c3 = (o - 1.0) * w * h;
    const double r3 = (b3 + sqrt(b3 * b3 - 16.0 * o * c3)) / 2.0;
    double m = r1;
    if (r2 < m) m = r2;
    if (r3 < m) m = r3;
    if (!(m >= (double)min_radius)) return min_radius;
    return m >= (double)SG_CENTERS_RADIUS_MAX ? SG_CENTERS_RADIUS_MAX : (int32_t)m;
}

// The gt b[0 .. 7]: present iff sg_box_make's rule holds and column 7 is integral with a value in 1 .. NC (sg_anchors_gt's rule).
template <typename T> __host__ __device__ inline void sg_centers_gt(const T *b, const SgCenterCfg &c, SgCenterGt *g)
{
    const double unit[2] = {1.0, 0.0};
    const double k = (double)b[7];
    SgBoxRec box;
    int32_t cls = 0;
    if (k >= 1.0 && k <= (double)c.n_classes && floor(k) == k) cls = (int32_t)k;            // (false for NaN)
    g->offx = g->offy = g->den = 0.0;
    g->cix = g->ciy = g->r = g->cls = g->head = 0;
    g->state = SG_CENTERS_ABSENT;
    if (!sg_box_make<T>(b, unit, &box) || cls == 0) return;
    g->cls = cls;
    g->head = c.class_head[cls - 1];
    const double coord_x = (((double)b[0] - c.x0) / c.vx) / c.stride, coord_y = (((double)b[1] - c.y0) / c.vy) / c.stride;
    if (c.drop && !(coord_x >= 0.0 && coord_x < (double)c.W && coord_y >= 0.0 && coord_y < (double)c.H)) {
        g->state = SG_CENTERS_DROPPED;
        return;
    }
    sg_centers_pixel(coord_x, c.W, &g->cix, &g->offx);
    sg_centers_pixel(coord_y, c.H, &g->ciy, &g->offy);
    const double h = ((double)b[3] / c.vx) / c.stride, w = ((double)b[4] / c.vy) / c.stride;
    g->r = sg_centers_radius(h, w, c.overlap, c.min_radius);
    const double d = (double)(2 * g->r + 1), sigma = d / 6.0;
    g->den = 2.0 * sigma * sigma;
    g->state = SG_CENTERS_DRAWN;
}

// the record of a gt whose slot in its head is `rank` (ascending g among the head's present gts that were not dropped), and its state
__host__ __device__ inline uint8_t sg_centers_record(const SgCenterGt &g, int32_t rank, int32_t max_objs, SgCenterRec *r)
{
    const bool drawn = g.state == SG_CENTERS_DRAWN && rank < max_objs;
    r->den = drawn ? g.den : 0.0;
    r->cix = drawn ? g.cix : 0; r->ciy = drawn ? g.ciy : 0; r->r = drawn ? g.r : 0;
    r->cls = drawn ? g.cls : 0;
    return (uint8_t)(g.state == SG_CENTERS_DRAWN && !drawn ? SG_CENTERS_NO_SLOT : g.state);
}

// Whether the drawn gt g of class cls reaches the tile whose first pixel is (tx0, ty0): cix + r >= tx0 and cix - r <= tx0 + 63, and the
// rows likewise -- as differences of two pixel numbers, which never leave int32.
__host__ __device__ inline bool sg_centers_near(const SgCenterRec &g, int32_t cls, int32_t tx0, int32_t ty0)
{
    return g.cls == cls && tx0 - g.cix <= g.r && g.cix - tx0 <= g.r + (SG_CENTERS_TILE_W - 1) && ty0 - g.ciy <= g.r &&
           g.ciy - ty0 <= g.r + (SG_CENTERS_TILE_H - 1);
}

// the value of pixel (px, py) under the drawn gt g: float32(exp(-(ex ex + ey ey) / den)) inside its patch, 0 outside
__host__ __device__ inline float sg_centers_value(const SgCenterRec &g, int32_t px, int32_t py)
{
    const int32_t ex = px - g.cix, ey = py - g.ciy;
    if (ex > g.r || -ex > g.r || ey > g.r || -ey > g.r) return 0.0f;
    return (float)exp(-(double)(ex * ex + ey * ey) / g.den);                // (ex ex + ey ey <= 2 x 512^2: an exact integer)
}

// the slot (h, m) of frame f as one element of the (F, NH, M) outputs; g: the gt of the slot or -1, gts: the frame's
template <typename T>
__host__ __device__ inline void sg_centers_slot(const SgCenterCfg &c, int64_t at, int32_t g, int32_t cix, int32_t ciy, int32_t r, double offx, double offy,
                                                const SgCenterOut<T> &o)
{
    const bool full = g >= 0;
    o.gt_index[at] = g;
    o.ind[at] = full ? ciy * c.W + cix : 0;
    o.mask[at] = full ? 1 : 0;
    o.offset[at * 2] = (T)(full ? offx : 0.0);
    o.offset[at * 2 + 1] = (T)(full ? offy : 0.0);
    o.radius[at] = full ? r : 0;
}

static inline int32_t sg_centers_tiles_x(int32_t W) { return (W + SG_CENTERS_TILE_W - 1) / SG_CENTERS_TILE_W; }
static inline int32_t sg_centers_tiles_y(int32_t H) { return (H + SG_CENTERS_TILE_H - 1) / SG_CENTERS_TILE_H; }

// The whole of frame f in one thread.  gt (B, Cg): the frame's own; recs: B records.  The heat is made as the kernel makes it: a tile at a
// time, over the ascending list of the class's gts that reach the tile.
template <typename T>
__host__ __device__ inline void sg_centers_frame(const SgCenterCfg &c, int64_t f, int32_t B, const T *gt, int32_t Cg, SgCenterRec *recs, const SgCenterOut<T> &o)
{
    const int32_t NH = c.n_heads, M = c.max_objs;
    int32_t taken[SG_CENTERS_HEADS_MAX];
    for (int32_t h = 0; h < NH; ++h) taken[h] = 0;
    for (int64_t s = 0; s < (int64_t)NH * M; ++s) sg_centers_slot<T>(c, f * NH * M + s, -1, 0, 0, 0, 0.0, 0.0, o);
    for (int32_t g = 0; g < B; ++g) {
        SgCenterGt me;
        sg_centers_gt<T>(gt + (int64_t)g * Cg, c, &me);
        int32_t rank = 0;
        if (me.state == SG_CENTERS_DRAWN) rank = taken[me.head]++;
        o.state[f * B + g] = sg_centers_record(me, rank, M, &recs[g]);
        if (recs[g].cls != 0) sg_centers_slot<T>(c, (f * NH + me.head) * M + rank, g, me.cix, me.ciy, me.r, me.offx, me.offy, o);
    }
    for (int32_t h = 0; h < NH; ++h) o.count[f * NH + h] = taken[h] < M ? taken[h] : M;
    for (int32_t cls = 1; cls <= c.n_classes; ++cls)
        for (int64_t ty0 = 0; ty0 < c.H; ty0 += SG_CENTERS_TILE_H)
            for (int64_t tx0 = 0; tx0 < c.W; tx0 += SG_CENTERS_TILE_W) {
                uint16_t list[SG_CENTERS_GT_MAX];
                int32_t near = 0;
                for (int32_t g = 0; g < B; ++g)
                    if (sg_centers_near(recs[g], cls, (int32_t)tx0, (int32_t)ty0)) list[near++] = (uint16_t)g;
                for (int64_t py = ty0; py < ty0 + SG_CENTERS_TILE_H && py < c.H; ++py)
                    for (int64_t px = tx0; px < tx0 + SG_CENTERS_TILE_W && px < c.W; ++px) {
                        float best = 0.0f;
                        for (int32_t k = 0; k < near; ++k) {
                            const float v = sg_centers_value(recs[list[k]], (int32_t)px, (int32_t)py);
                            best = v > best ? v : best;
                        }
                        o.heatmap[((f * c.n_classes + (cls - 1)) * c.H + py) * c.W + px] = best;
                    }
            }
}
