// sg_targets.h -- proposal target sampling (snowgpu_sample_rois_device; the DEFINITION: include/snowgpu.h): which rois are candidates, the
// three overlap classes, the Philox words of the slots, how the slots are split, the walk without replacement, the pick of a slot and
// everything a slot stores.  snowgpu_targets.hip runs these functions on the device -- only the three ordered lists are built another way
// there, by ballots --, tests/host_harness/targets_walk.cpp runs sg_targets_frame, the same code in one thread, on the host (as sg_weather.h
// is compiled for both), and tests/targets_reference.py restates the definition in NumPy and Python integers.
//
// The lists.  fg holds the roi numbers of class FG ascending; bg those of class HARD ascending and BEHIND them, from bg[n_hard] on, those
// of class EASY ascending.  HARD and EASY exclude each other, FG may meet either (reg_fg_thresh > cls_fg_thresh; cls_bg_thresh_lo above the
// foreground threshold): fg and bg hold at most M entries each.
//
// The words.  r_k = word k % 4 of Philox4x32-10 under key seed at counter (step lo, step hi, frame, "ROIS" + k / 4): sg_weather_block's
// rounds under another tag.  Slot k uses r_k whatever the other slots do.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_box.h"         // presence and the pose: sg_box_make
#include "sg_weather.h"     // the Philox block: sg_weather_block

#define SG_TARGETS_MAX 9216             /* rois and gt boxes per frame: 1 <= M, B <= 9216 (the limit of the IoU stage) */
#define SG_TARGETS_SLOTS_MAX 1024       /* 1 <= S <= 1024 */
#define SG_TARGETS_TAG 0x524F4953u      /* "ROIS" */
#define SG_TARGETS_FG 1
#define SG_TARGETS_HARD 2
#define SG_TARGETS_EASY 4
#define SG_TARGETS_PI 3.141592653589793         /* np.pi */
#define SG_TARGETS_2PI 6.283185307179586        /* 2 * np.pi */
#define SG_TARGETS_PI_2 1.5707963267948966      /* 0.5 * np.pi */
#define SG_TARGETS_3PI_2 4.71238898038469       /* 1.5 * np.pi */

struct SgTargetCfg {                    // snowgpu_roi_sampler as the kernel takes it
    int32_t S, fg_per_image;
    double reg_fg, cls_fg, cls_bg, cls_bg_lo, hard_ratio;
    int32_t cls_mode;
};

template <typename T> struct SgTargetOut {      // the outputs of the whole batch; pose and gt_local may be null
    int32_t *index;
    T *rois, *roi_iou;
    int32_t *gt_index;
    T *gt_of_rois;
    uint8_t *reg_valid;
    T *cls_label;
    int32_t *segments, *class_count;
    double *pose;
    T *gt_local;
};

struct SgTargetSplit {                  // how the S slots of a frame are used: fg picks, then hard picks, then easy picks
    int32_t fg_this, hard_this, easy_this;
    bool fg_replace;                    // the fg picks are drawn with replacement (branch b)
};

// block b of frame f: the four words of slots 4 b .. 4 b + 3
__host__ __device__ inline void sg_targets_block(uint64_t seed, uint64_t step, uint32_t f, uint32_t b, uint32_t (&out)[4])
{
    sg_weather_block(seed, step, f, (SG_TARGETS_TAG - SG_WEATHER_TAG) + b, out);       // (uint32 arithmetic: the tag becomes "ROIS" + b)
}

// a pick with replacement from a list of n: (r n) >> 32, below n
__host__ __device__ inline int32_t sg_targets_pick(uint32_t r, int32_t n) { return (int32_t)(((uint64_t)r * (uint64_t)(uint32_t)n) >> 32); }

// The classes of roi b[0 .. 6] with overlap ov under the caller's pose or (NULL) cos / sin of the heading: 0 for a roi that is no candidate,
// else the OR of SG_TARGETS_FG / HARD / EASY.  rec receives the record with the pose that was used.
template <typename T> __host__ __device__ inline int sg_targets_classes(const SgTargetCfg &c, const T *b, const double *pose_in, T overlap, SgBoxRec *rec)
{
    const double ov = (double)overlap;
    if (!sg_box_make<T>(b, pose_in, rec) || ov != ov) return 0;
    const double fg_thresh = c.reg_fg < c.cls_fg ? c.reg_fg : c.cls_fg;
    return (ov >= fg_thresh ? SG_TARGETS_FG : 0) | ((ov < c.reg_fg && ov >= c.cls_bg_lo) ? SG_TARGETS_HARD : 0) | (ov < c.cls_bg_lo ? SG_TARGETS_EASY : 0);
}

// the background picks of count n
__host__ __device__ inline void sg_targets_background(const SgTargetCfg &c, int32_t n, int32_t n_hard, int32_t n_easy, SgTargetSplit *s)
{
    if (n_hard > 0 && n_easy > 0) {
        const int32_t want = (int32_t)((double)n * c.hard_ratio);                     // one float64 product, truncated
        s->hard_this = want < n_hard ? want : n_hard;
        s->easy_this = n - s->hard_this;
    } else {
        s->hard_this = n_hard > 0 ? n : 0;
        s->easy_this = n_easy > 0 ? n : 0;
    }
}

// branches (a) .. (d) of the definition
__host__ __device__ inline SgTargetSplit sg_targets_split(const SgTargetCfg &c, int32_t n_fg, int32_t n_hard, int32_t n_easy)
{
    SgTargetSplit s{0, 0, 0, false};
    const int32_t n_bg = n_hard + n_easy;
    if (n_fg > 0 && n_bg > 0) {
        s.fg_this = c.fg_per_image < n_fg ? c.fg_per_image : n_fg;
        sg_targets_background(c, c.S - s.fg_this, n_hard, n_easy, &s);
    } else if (n_fg > 0) {
        s.fg_this = c.S;
        s.fg_replace = true;
    } else if (n_bg > 0) {
        sg_targets_background(c, c.S, n_hard, n_easy, &s);
    }
    return s;
}

// The fg picks without replacement: the first fg_this steps of a forward Fisher-Yates walk over fg[0 .. n_fg); step i uses r_i.  Afterwards
// fg[i] is pick i.
template <typename Word, typename Item>
__host__ __device__ inline void sg_targets_walk(int32_t fg_this, int32_t n_fg, const Word *words, Item *fg)
{
    for (int32_t i = 0; i < fg_this; ++i) {
        const int32_t j = i + sg_targets_pick(words[i], n_fg - i);
        const Item t = fg[i]; fg[i] = fg[j]; fg[j] = t;
    }
}

// the roi of slot k (after the walk), -1 for an empty slot
template <typename Word, typename Item>
__host__ __device__ inline int32_t sg_targets_slot(const SgTargetSplit &s, int32_t k, int32_t n_fg, int32_t n_hard, int32_t n_easy, const Word *words,
                                                   const Item *fg, const Item *bg)
{
    if (k < s.fg_this) return (int32_t)(s.fg_replace ? fg[sg_targets_pick(words[k], n_fg)] : fg[k]);
    if (k < s.fg_this + s.hard_this) return n_hard > 0 ? (int32_t)bg[sg_targets_pick(words[k], n_hard)] : -1;
    if (k < s.fg_this + s.hard_this + s.easy_this) return n_easy > 0 ? (int32_t)bg[n_hard + sg_targets_pick(words[k], n_easy)] : -1;
    return -1;
}

// the classification target of overlap ov
__host__ __device__ inline double sg_targets_label(const SgTargetCfg &c, double ov)
{
    if (ov > c.cls_fg) return 1.0;
    if (c.cls_mode == 0) return ov < c.cls_bg ? 0.0 : (ov - c.cls_bg) / (c.cls_fg - c.cls_bg);
    return (ov > c.cls_bg && ov < c.cls_fg) ? -1.0 : 0.0;
}

// fmod(x, 2 pi) moved into [0, 2 pi]: plus 2 pi when negative, +0 when zero
__host__ __device__ inline double sg_targets_pmod(double x)
{
    double r = fmod(x, SG_TARGETS_2PI);
    if (r < 0.0) r += SG_TARGETS_2PI;
    return r == 0.0 ? 0.0 : r;
}

// the heading label of a gt of heading h_gt in a roi of heading h_roi, in [-pi / 2, pi / 2]
__host__ __device__ inline double sg_targets_heading(double h_roi, double h_gt)
{
    const double ry = sg_targets_pmod(h_roi);
    double hl = sg_targets_pmod(h_gt - ry);
    if (hl > SG_TARGETS_PI_2 && hl < SG_TARGETS_3PI_2) hl = sg_targets_pmod(hl + SG_TARGETS_PI);
    if (hl > SG_TARGETS_PI) hl -= SG_TARGETS_2PI;
    return hl < -SG_TARGETS_PI_2 ? -SG_TARGETS_PI_2 : (hl > SG_TARGETS_PI_2 ? SG_TARGETS_PI_2 : hl);
}

// the gt g[0 .. 6] in the frame of the roi b[0 .. 6] of pose (c, s): out[0 .. 6]; zeros for a gt whose seven values are not all within 1e6
template <typename T> __host__ __device__ inline void sg_targets_local(const T *b, double c, double s, const T *g, T *out)
{
    bool ok = true;
    for (int j = 0; j < 7; ++j) ok = ok && fabs((double)g[j]) <= SG_FPS_BOUND;        // (false for NaN and inf)
    if (!ok) {
        for (int j = 0; j < 7; ++j) out[j] = (T)0;
        return;
    }
    const double sx = (double)g[0] - (double)b[0], sy = (double)g[1] - (double)b[1], lz = (double)g[2] - (double)b[2];
    const double lx = sx * c + sy * s, ly = sy * c - sx * s;
    out[0] = (T)lx; out[1] = (T)ly; out[2] = (T)lz;
    out[3] = g[3]; out[4] = g[4]; out[5] = g[5];
    out[6] = (T)sg_targets_heading((double)b[6], (double)g[6]);
}

// Everything slot k of frame f stores for the picked roi m (-1: an empty slot).  rois, overlap, assign, gt, pose_in: the frame's own.
template <typename T>
__host__ __device__ inline void sg_targets_fill(const SgTargetCfg &c, int64_t f, int32_t k, int32_t m, const T *rois, int32_t Cb, const T *overlap,
                                                const int32_t *assign, int32_t B, const T *gt, int32_t Cg, const double *pose_in,
                                                const SgTargetOut<T> &o)
{
    const int64_t t = f * c.S + k;
    T *roi = o.rois + t * Cb, *own = o.gt_of_rois + t * Cg;
    int32_t a = -1;
    double ov = 0.0, pc = 0.0, ps = 0.0;
    const T *b = nullptr, *g = nullptr;
    if (m >= 0) {
        SgBoxRec rec;
        b = rois + (int64_t)m * Cb;
        (void)sg_box_make<T>(b, pose_in ? pose_in + (int64_t)m * 2 : nullptr, &rec);  // (present: m is a candidate)
        pc = rec.c; ps = rec.s;
        a = assign[m];
        if (a < 0 || a >= B) a = -1;
        if (a >= 0) g = gt + (int64_t)a * Cg;
        ov = (double)overlap[m];
    }
    o.index[t] = m;
    for (int32_t j = 0; j < Cb; ++j) roi[j] = b ? b[j] : (T)0;
    o.roi_iou[t] = b ? overlap[m] : (T)0;
    o.gt_index[t] = a;
    for (int32_t j = 0; j < Cg; ++j) own[j] = g ? g[j] : (T)0;
    o.reg_valid[t] = (uint8_t)(b && ov > c.reg_fg ? 1 : 0);
    o.cls_label[t] = b ? (T)sg_targets_label(c, ov) : (T)-1;
    if (o.pose) { o.pose[t * 2] = pc; o.pose[t * 2 + 1] = ps; }
    if (o.gt_local) {
        T *l = o.gt_local + t * 7;
        if (g) sg_targets_local<T>(b, pc, ps, g, l);
        else
            for (int j = 0; j < 7; ++j) l[j] = (T)0;
    }
}

// The whole of frame f in one thread.  rois (M, Cb), overlap (M), assign (M), gt (B, Cg), pose_in (M, 2) or NULL: the frame's own; fg and bg:
// M items each; words: 4 ceil(S / 4).
template <typename T>
__host__ __device__ inline void sg_targets_frame(const SgTargetCfg &c, uint64_t seed, uint64_t step, uint32_t f, int32_t M, const T *rois, int32_t Cb,
                                                 const T *overlap, const int32_t *assign, int32_t B, const T *gt, int32_t Cg, const double *pose_in,
                                                 uint16_t *fg, uint16_t *bg, uint32_t *words, const SgTargetOut<T> &o)
{
    int32_t n_fg = 0, n_hard = 0, n_easy = 0;
    for (int pass = 0; pass < 2; ++pass)                                             // FG and HARD, then EASY behind HARD
        for (int32_t m = 0; m < M; ++m) {
            SgBoxRec rec;
            const int cls = sg_targets_classes<T>(c, rois + (int64_t)m * Cb, pose_in ? pose_in + (int64_t)m * 2 : nullptr, overlap[m], &rec);
            if (pass == 0 && (cls & SG_TARGETS_FG)) fg[n_fg++] = (uint16_t)m;
            if (pass == 0 && (cls & SG_TARGETS_HARD)) bg[n_hard++] = (uint16_t)m;
            if (pass == 1 && (cls & SG_TARGETS_EASY)) bg[n_hard + n_easy++] = (uint16_t)m;
        }
    for (int32_t b = 0; 4 * b < c.S; ++b) {
        uint32_t w[4];
        sg_targets_block(seed, step, f, (uint32_t)b, w);
        for (int k = 0; k < 4; ++k) words[4 * b + k] = w[k];
    }
    const SgTargetSplit s = sg_targets_split(c, n_fg, n_hard, n_easy);
    if (!s.fg_replace) sg_targets_walk(s.fg_this, n_fg, words, fg);
    for (int32_t k = 0; k < c.S; ++k)
        sg_targets_fill<T>(c, (int64_t)f, k, sg_targets_slot(s, k, n_fg, n_hard, n_easy, words, fg, bg), rois, Cb, overlap, assign, B, gt, Cg, pose_in, o);
    o.segments[(int64_t)f * 3] = s.fg_this; o.segments[(int64_t)f * 3 + 1] = s.hard_this; o.segments[(int64_t)f * 3 + 2] = s.easy_this;
    o.class_count[(int64_t)f * 3] = n_fg; o.class_count[(int64_t)f * 3 + 1] = n_hard; o.class_count[(int64_t)f * 3 + 2] = n_easy;
}
