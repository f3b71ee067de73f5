// sg_anchors.h -- anchor target assignment (snowgpu_assign_anchors_device; the DEFINITION: include/snowgpu.h): which anchors and gt boxes are
// present, the nearest axis-aligned BEV box of a box, the overlap of two such boxes, the walk of an anchor over the gts of its frame and the
// label rule.  snowgpu_anchors.hip runs these functions on the device -- only the largest overlap of every gt (`top`) is gathered another
// way there, by a cross-lane maximum and an integer atomic maximum on the bits --, tests/host_harness/anchors_walk.cpp runs
// sg_anchors_frame, the same code in one thread, on the host (as sg_targets.h is compiled for both), and tests/anchors_reference.py restates
// the definition as brute-force NumPy.
//
// Everything is float64 computed from (double) of the inputs, every operation rounded on its own (-ffp-contract=off), and there is no
// transcendental function: presence is sg_box_make's rule under the unit pose (1, 0), whose pose check always holds.
//
// The record.  One per gt, 48 bytes: x0, x1, y0, y1 and the area of its BEV box and its class, 0 for an absent gt.  An anchor's record is
// built by the lane that owns the anchor and never stored.
//
// The bits.  An overlap is a non-negative double that is no NaN, so its bits, read as an unsigned 64-bit integer, order as the values do:
// the maximum of the bits is the bits of the maximum, whatever the order of arrival.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "sg_box.h"         // presence: sg_box_make; SG_BOX_MAX

#define SG_ANCHORS_GT_MAX SG_BOX_MAX    /* gt boxes per frame: 1 <= B <= 256 */
#define SG_ANCHORS_CLASSES_MAX 16       /* 1 <= NC <= 16 */
#define SG_ANCHORS_PI 3.141592653589793         /* np.pi */
#define SG_ANCHORS_PI_4 0.7853981633974483      /* np.pi / 4 */
#define SG_ANCHORS_EPS 1e-6             /* the smallest union */

struct SgAnchorCfg {                    // the thresholds as the kernels take them: class c at [c - 1]
    int32_t n_classes;
    double matched[SG_ANCHORS_CLASSES_MAX], unmatched[SG_ANCHORS_CLASSES_MAX];
};

struct SgAnchorRec {                    // the nearest axis-aligned BEV box, its area and the class; cls 0: absent
    double x0, x1, y0, y1, area;
    int32_t cls, pad;
};

template <typename T> struct SgAnchorOut {      // the outputs of the whole batch; iou may be null
    int32_t *label, *gt_index, *count, *gt_count;
    T *iou;
};

// the bits of a non-negative double
__host__ __device__ inline unsigned long long sg_anchors_bits(double v)
{
    unsigned long long u;
    memcpy(&u, &v, 8);
    return u;
}

// the BEV box of the present box b[0 .. 6] into r (cls is the caller's)
template <typename T> __host__ __device__ inline void sg_anchors_bev(const T *b, SgAnchorRec *r)
{
    const double cx = (double)b[0], cy = (double)b[1], dx = (double)b[3], dy = (double)b[4], h = (double)b[6];
    const double k = floor(h / SG_ANCHORS_PI + 0.5);
    const double turn = fabs(h - k * SG_ANCHORS_PI);
    const bool keep = turn < SG_ANCHORS_PI_4;
    const double ex = keep ? dx : dy, ey = keep ? dy : dx;
    const double hx = ex / 2.0, hy = ey / 2.0;
    r->x0 = cx - hx; r->x1 = cx + hx;
    r->y0 = cy - hy; r->y1 = cy + hy;
    r->area = (r->x1 - r->x0) * (r->y1 - r->y0);
}

// The record of anchor b[0 .. 6] of class number cls: present iff sg_box_make's rule holds and 1 <= cls <= NC.  An absent anchor has cls 0.
template <typename T> __host__ __device__ inline bool sg_anchors_anchor(const T *b, int32_t cls, int32_t n_classes, SgAnchorRec *r)
{
    const double unit[2] = {1.0, 0.0};
    SgBoxRec box;
    const bool ok = sg_box_make<T>(b, unit, &box) && cls >= 1 && cls <= n_classes;
    r->x0 = r->x1 = r->y0 = r->y1 = r->area = 0.0;
    r->cls = 0; r->pad = 0;
    if (ok) {
        sg_anchors_bev<T>(b, r);
        r->cls = cls;
    }
    return ok;
}

// The record of gt b[0 .. 7]: present iff sg_box_make's rule holds and column 7 is integral with a value in 1 .. NC.
template <typename T> __host__ __device__ inline bool sg_anchors_gt(const T *b, int32_t n_classes, SgAnchorRec *r)
{
    const double c = (double)b[7];
    int32_t cls = 0;
    if (c >= 1.0 && c <= (double)n_classes && floor(c) == c) cls = (int32_t)c;          // (false for NaN)
    return sg_anchors_anchor<T>(b, cls, n_classes, r);
}

// the overlap of two BEV boxes
__host__ __device__ inline double sg_anchors_iou(const SgAnchorRec &a, const SgAnchorRec &g)
{
    const double rx = (a.x1 < g.x1 ? a.x1 : g.x1) - (a.x0 > g.x0 ? a.x0 : g.x0);
    const double ry = (a.y1 < g.y1 ? a.y1 : g.y1) - (a.y0 > g.y0 ? a.y0 : g.y0);
    const double ix = rx > 0.0 ? rx : 0.0, iy = ry > 0.0 ? ry : 0.0;
    const double inter = ix * iy;
    const double uni = (a.area + g.area) - inter;
    return inter / (uni > SG_ANCHORS_EPS ? uni : SG_ANCHORS_EPS);
}

// Whether the gt g can meet, at an overlap > 0, an anchor whose BEV box lies inside bb = (the smallest x0, the largest x1, the smallest y0, the
// largest y1) of a set of anchors.  Exact, not a tolerance: g.x1 <= bb[0] <= a.x0 gives min(a.x1, g.x1) <= max(a.x0, g.x0), a width that is not
// > 0, an intersection of 0 and an overlap of exactly 0; the other three sides alike.  An empty set (bb = +inf, -inf, +inf, -inf) meets nothing.
__host__ __device__ inline bool sg_anchors_near(const SgAnchorRec &g, const double *bb)
{
    return g.cls != 0 && g.x1 > bb[0] && g.x0 < bb[1] && g.y1 > bb[2] && g.y0 < bb[3];
}

// The walk of the present anchor a over the records of its frame in ascending g: best, the largest overlap with a gt of its class; arg, the
// smallest g that reaches it, -1 if best is not > 0; forced: some gt of its class has top > 0 (top: the bits of every gt's largest overlap)
// and meets the anchor at exactly top.  With list == NULL the walk visits g = 0 .. n - 1; otherwise the n gt numbers of list, which must be
// ascending and may leave out any gt that meets the anchor at 0: such a gt changes none of the three (0 is not > best, and its bits are
// not those of a top > 0).
template <typename Rec, typename Word, typename Item>
__host__ __device__ inline void sg_anchors_walk(const SgAnchorRec &a, const Rec *gts, const Item *list, int32_t n, const Word *top, double *best, int32_t *arg,
                                                bool *forced)
{
    double b = 0.0;
    int32_t at = -1;
    bool f = false;
    for (int32_t k = 0; k < n; ++k) {
        const int32_t g = list ? (int32_t)list[k] : k;
        if (gts[g].cls != a.cls) continue;              // (an absent gt has class 0, a present anchor none below 1)
        const SgAnchorRec rec = gts[g];
        const double v = sg_anchors_iou(a, rec);
        const unsigned long long t = (unsigned long long)top[g];
        if (v > b) { b = v; at = g; }
        f = f || (t != 0ull && sg_anchors_bits(v) == t);              // (v >= 0 and never -0: inter / positive; bits 0 is the value 0)
    }
    *best = b; *arg = at; *forced = f;
}

// the label of a present anchor of class cls: cls for a positive, 0 for background, -1 for ignored
__host__ __device__ inline int32_t sg_anchors_label(const SgAnchorCfg &c, int32_t cls, double best, bool forced)
{
    if (forced || best >= c.matched[cls - 1]) return cls;
    return best < c.unmatched[cls - 1] ? 0 : -1;
}

// the box around the BEV boxes of a set of anchors: start from sg_anchors_bb_empty, add every present anchor
#define SG_ANCHORS_GROUP 256            /* anchors that share one box and one list of near gts: a workgroup of the kernels */
static inline int32_t sg_anchors_groups(int32_t A) { return (int32_t)(((int64_t)A + SG_ANCHORS_GROUP - 1) / SG_ANCHORS_GROUP); }
__host__ __device__ inline void sg_anchors_bb_empty(double *bb) { bb[0] = bb[2] = HUGE_VAL; bb[1] = bb[3] = -HUGE_VAL; }
__host__ __device__ inline void sg_anchors_bb_add(const SgAnchorRec &a, double *bb)
{
    bb[0] = a.x0 < bb[0] ? a.x0 : bb[0]; bb[1] = a.x1 > bb[1] ? a.x1 : bb[1];
    bb[2] = a.y0 < bb[2] ? a.y0 : bb[2]; bb[3] = a.y1 > bb[3] ? a.y1 : bb[3];
}

// The whole of frame f in one thread.  anchors (A, Ca), anchor_class (A): the batch's; gt (B, Cg): the frame's own; recs: B records; top: B words.
// top is gathered over every (anchor, gt) pair; the labels are made as the kernels make them: SG_ANCHORS_GROUP anchors at a time, walking the
// ascending list of the gts near the group's box.
template <typename T>
__host__ __device__ inline void sg_anchors_frame(const SgAnchorCfg &c, int64_t f, int32_t A, const T *anchors, int32_t Ca, const int32_t *anchor_class, int32_t B,
                                                 const T *gt, int32_t Cg, SgAnchorRec *recs, unsigned long long *top, const SgAnchorOut<T> &o)
{
    for (int32_t g = 0; g < B; ++g) {
        (void)sg_anchors_gt<T>(gt + (int64_t)g * Cg, c.n_classes, &recs[g]);
        top[g] = 0ull;
        o.gt_count[f * B + g] = 0;
    }
    for (int32_t a = 0; a < A; ++a) {
        SgAnchorRec rec;
        if (!sg_anchors_anchor<T>(anchors + (int64_t)a * Ca, anchor_class[a], c.n_classes, &rec)) continue;
        for (int32_t g = 0; g < B; ++g) {
            if (recs[g].cls != rec.cls) continue;
            const unsigned long long v = sg_anchors_bits(sg_anchors_iou(rec, recs[g]));
            if (v > top[g]) top[g] = v;
        }
    }
    int32_t n[3] = {0, 0, 0};
    for (int32_t first = 0; first < A; first += SG_ANCHORS_GROUP) {
        const int32_t last = first + SG_ANCHORS_GROUP < A ? first + SG_ANCHORS_GROUP : A;
        double bb[4];
        uint16_t list[SG_ANCHORS_GT_MAX];
        int32_t near = 0;
        sg_anchors_bb_empty(bb);
        for (int32_t a = first; a < last; ++a) {
            SgAnchorRec rec;
            if (sg_anchors_anchor<T>(anchors + (int64_t)a * Ca, anchor_class[a], c.n_classes, &rec)) sg_anchors_bb_add(rec, bb);
        }
        for (int32_t g = 0; g < B; ++g)
            if (sg_anchors_near(recs[g], bb)) list[near++] = (uint16_t)g;
        for (int32_t a = first; a < last; ++a) {
            SgAnchorRec rec;
            int32_t label = -1, arg = -1;
            double best = 0.0;
            if (sg_anchors_anchor<T>(anchors + (int64_t)a * Ca, anchor_class[a], c.n_classes, &rec)) {
                bool forced;
                sg_anchors_walk(rec, recs, list, near, top, &best, &arg, &forced);
                label = sg_anchors_label(c, rec.cls, best, forced);
                if (label <= 0) arg = -1;
                n[label > 0 ? 0 : (label == 0 ? 1 : 2)] += 1;
                if (label > 0) o.gt_count[f * B + arg] += 1;
            }
            o.label[f * A + a] = label;
            o.gt_index[f * A + a] = arg;
            if (o.iou) o.iou[f * A + a] = (T)best;
        }
    }
    o.count[f * 3] = n[0]; o.count[f * 3 + 1] = n[1]; o.count[f * 3 + 2] = n[2];
}
