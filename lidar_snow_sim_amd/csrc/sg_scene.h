// sg_scene.h -- scene transforms (snowgpu_transform_scene_device; the DEFINITION: include/snowgpu.h): the Philox words of the world draw and
// of every try of every box, the uniform value of a word, the candidate of a try, the sweep that settles the boxes of a frame, what a row
// and what a box become, and the sizes of the scratch.  snowgpu_scene.hip runs these functions on the device -- only the collision bits of
// a box's tries are built another way there, spread over a workgroup --, tests/host_harness/scene_sweep.cpp runs the same code in one
// thread on the host (as sg_paste.h is compiled for both), and tests/scene_reference.py restates the definition in NumPy.
//
// The records, eight doubles each.  WORLD (per frame): flip_x, flip_y, cos theta, sin theta, theta, sigma, 0, 0.  TRY (per box and try):
// tx, ty, tz, cos delta, sin delta, delta, s, collided (0 or 1).  The draw functions here leave (cos, sin) = (1, 0); the caller fills them
// in where the part is on -- the device from its math library, the host harness from its input -- so that nothing in this file is
// transcendental.  The ROW record (per box, ten doubles): the ORIGINAL centre, cos delta, sin delta, s, tx, ty, tz, moved (0 or 1).
//
// A part that is switched off draws nothing and has the identity's values (0, (1, 0), 1); the arithmetic below is the same either way, so
// an identity part can at most turn a -0 into +0.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_iou.h"         // presence and the record: sg_iou_make; the overlap: sg_iou_area
#include "sg_weather.h"     // the Philox block: sg_weather_block

#define SG_SCENE_TAG 0x5846524Du        /* "XFRM" */
#define SG_SCENE_TRIES_MAX 16           /* 0 <= T <= 16: one bit per try in the collision word; 0: no local part */
#define SG_SCENE_REC 8
#define SG_SCENE_ROWREC 10
#define SG_SCENE_FLIP_X 1
#define SG_SCENE_FLIP_Y 2
#define SG_SCENE_PI 3.141592653589793   /* float64 nearest pi: the flip about y turns the heading into -(heading + pi) */
#define SG_SCENE_STILL 0
#define SG_SCENE_MOVED 1
#define SG_SCENE_BLOCKED 2

struct SgSceneCfg {                     // the ranges as the kernel takes them
    int32_t flip;                       // SG_SCENE_FLIP_X | SG_SCENE_FLIP_Y: the axes asked for
    int32_t rot_on, scale_on;           // the world parts
    int32_t tries;                      // T; 0: no local part
    int32_t ltrans_on, lrot_on, lscale_on;
    double rot[2], scale[2];            // lo, hi
    double ltrans[3];                   // ax, ay, az: a component is uniform in -a .. a
    double lrot[2], lscale[2];
};

// elements of the scratch: doubles of the row records and of the try records (when the caller takes no d_out_tries)
static inline size_t sg_scene_rowrecs(int n_frames, int32_t B) { return (size_t)n_frames * (size_t)B * SG_SCENE_ROWREC; }
static inline size_t sg_scene_tries(int n_frames, int32_t B, int32_t T) { return (size_t)n_frames * (size_t)B * (size_t)T * SG_SCENE_REC; }

// block b of frame f
__host__ __device__ inline void sg_scene_block(uint64_t seed, uint64_t step, uint32_t f, uint32_t b, uint32_t (&out)[4])
{
    sg_weather_block(seed, step, f, (SG_SCENE_TAG - SG_WEATHER_TAG) + b, out);         // (uint32 arithmetic: the tag becomes "XFRM" + b)
}

// lo + (w 2^-32) (hi - lo): the scaling is exact, the difference, the product and the sum are rounded each
__host__ __device__ inline double sg_scene_uniform(uint32_t w, double lo, double hi)
{
    const double u = (double)w * 0x1p-32, d = hi - lo, p = u * d;
    return lo + p;
}

// block 0: the world record of frame f, cos / sin left at (1, 0)
__host__ __device__ inline void sg_scene_world_draw(const SgSceneCfg &k, uint64_t seed, uint64_t step, uint32_t f, double *rec)
{
    uint32_t w[4];
    sg_scene_block(seed, step, f, 0u, w);
    rec[0] = ((k.flip & SG_SCENE_FLIP_X) && w[0] < 0x80000000u) ? 1.0 : 0.0;
    rec[1] = ((k.flip & SG_SCENE_FLIP_Y) && w[1] < 0x80000000u) ? 1.0 : 0.0;
    rec[2] = 1.0; rec[3] = 0.0;
    rec[4] = k.rot_on ? sg_scene_uniform(w[2], k.rot[0], k.rot[1]) : 0.0;
    rec[5] = k.scale_on ? sg_scene_uniform(w[3], k.scale[0], k.scale[1]) : 1.0;
    rec[6] = 0.0; rec[7] = 0.0;
}

// blocks 1 + 2 (i T + t) and the next: the record of try t of box i, cos / sin left at (1, 0), collided at 0
__host__ __device__ inline void sg_scene_try_draw(const SgSceneCfg &k, uint64_t seed, uint64_t step, uint32_t f, int32_t i, int32_t t, double *rec)
{
    uint32_t a[4], b[4];
    const uint32_t blk = 1u + 2u * (uint32_t)(i * k.tries + t);
    sg_scene_block(seed, step, f, blk, a);
    sg_scene_block(seed, step, f, blk + 1u, b);
    for (int j = 0; j < 3; ++j) rec[j] = k.ltrans_on ? sg_scene_uniform(a[j], -k.ltrans[j], k.ltrans[j]) : 0.0;
    rec[3] = 1.0; rec[4] = 0.0;
    rec[5] = k.lrot_on ? sg_scene_uniform(a[3], k.lrot[0], k.lrot[1]) : 0.0;
    rec[6] = k.lscale_on ? sg_scene_uniform(b[0], k.lscale[0], k.lscale[1]) : 1.0;
    rec[7] = 0.0;
}

__host__ __device__ inline void sg_scene_identity(double *rec)
{
    rec[0] = 0.0; rec[1] = 0.0; rec[2] = 0.0; rec[3] = 1.0; rec[4] = 0.0; rec[5] = 0.0; rec[6] = 1.0; rec[7] = 0.0;
}

// the candidate of a try: the box o with centre + t, dims s and the pose turned by delta (the angle-addition formulas); float64 throughout
__host__ __device__ inline void sg_scene_candidate(const SgIouRec &o, const double *r, SgIouRec *c)
{
    c->cx = o.cx + r[0]; c->cy = o.cy + r[1]; c->cz = o.cz + r[2];
    c->dx = o.dx * r[6]; c->dy = o.dy * r[6]; c->dz = o.dz * r[6];
    c->c = o.c * r[3] - o.s * r[4];
    c->s = o.s * r[3] + o.c * r[4];
    c->ok = 1.0;
}

// The sweep of one frame over i ascending by plain loops (the host's route; the kernel spreads the (t, j) pairs of a box over a workgroup).
// cur[B]: the records of the boxes, settled in place; tries: B T records, cos / sin filled in, `collided` written for every try of every
// present box; state[i] and tried[i] are written for every i < B.
__host__ __device__ inline void sg_scene_sweep(int32_t B, int32_t T, SgIouRec *cur, double *tries, int32_t *state, int32_t *tried)
{
    for (int32_t i = 0; i < B; ++i) {
        state[i] = SG_SCENE_STILL; tried[i] = -1;
        if (T < 1 || cur[i].ok == 0.0) continue;
        int32_t taken = -1;
        for (int32_t t = 0; t < T; ++t) {
            double *r = tries + ((size_t)i * T + t) * SG_SCENE_REC;
            SgIouRec cand;
            sg_scene_candidate(cur[i], r, &cand);
            bool hit = false;
            for (int32_t j = 0; j < B && !hit; ++j)
                hit = j != i && cur[j].ok != 0.0 && sg_iou_area(cand, cur[j], nullptr) > 0.0;
            r[7] = hit ? 1.0 : 0.0;
            if (!hit && taken < 0) taken = t;
        }
        if (taken >= 0) {
            SgIouRec cand;
            sg_scene_candidate(cur[i], tries + ((size_t)i * T + taken) * SG_SCENE_REC, &cand);
            cur[i] = cand;
            state[i] = SG_SCENE_MOVED; tried[i] = taken;
        } else {
            state[i] = SG_SCENE_BLOCKED;
        }
    }
}

// `local` and the row record of box i from its state, the try it took (r: that try's record, not read unless moved) and its ORIGINAL centre
__host__ __device__ inline void sg_scene_box_records(int32_t state, const double *r, double cx, double cy, double cz, double *local, double *rowrec)
{
    sg_scene_identity(local);
    if (state == SG_SCENE_MOVED)
        for (int j = 0; j < 7; ++j) local[j] = r[j];
    rowrec[0] = cx; rowrec[1] = cy; rowrec[2] = cz;
    rowrec[3] = local[3]; rowrec[4] = local[4]; rowrec[5] = local[6];
    rowrec[6] = local[0]; rowrec[7] = local[1]; rowrec[8] = local[2];
    rowrec[9] = state == SG_SCENE_MOVED ? 1.0 : 0.0;
}

// A present, usable row: the local part of its box (rr: the row record of a MOVED box, or NULL), then the world part in pcdet's order
__host__ __device__ inline void sg_scene_row(double *x, double *y, double *z, const double *rr, const double *w)
{
    double px = *x, py = *y, pz = *z;
    if (rr) {
        const double sx = px - rr[0], sy = py - rr[1], sz = pz - rr[2];
        const double rx = sx * rr[3] - sy * rr[4], ry = sx * rr[4] + sy * rr[3];
        px = (rx * rr[5] + rr[0]) + rr[6];
        py = (ry * rr[5] + rr[1]) + rr[7];
        pz = (sz * rr[5] + rr[2]) + rr[8];
    }
    if (w[0] != 0.0) py = -py;
    if (w[1] != 0.0) px = -px;
    const double nx = px * w[2] - py * w[3], ny = px * w[3] + py * w[2];
    *x = nx * w[5]; *y = ny * w[5]; *z = pz * w[5];
}

// A present box: columns 0 .. 6 and the pose of the output from the ORIGINAL heading h, the settled record (centre, dims and pose behind
// the local part), the delta of the try taken (not read unless moved) and the world record
__host__ __device__ inline void sg_scene_box(double h, const SgIouRec &cur, bool moved, double delta, const double *w, double *out, double *pose)
{
    double cx = cur.cx, cy = cur.cy, c = cur.c, s = cur.s;
    if (moved) h = h + delta;
    if (w[0] != 0.0) { cy = -cy; h = -h; s = -s; }
    if (w[1] != 0.0) { cx = -cx; h = -(h + SG_SCENE_PI); c = -c; }
    const double nx = cx * w[2] - cy * w[3], ny = cx * w[3] + cy * w[2];
    h = h + w[4];
    pose[0] = c * w[2] - s * w[3];
    pose[1] = s * w[2] + c * w[3];
    out[0] = nx * w[5]; out[1] = ny * w[5]; out[2] = cur.cz * w[5];
    out[3] = cur.dx * w[5]; out[4] = cur.dy * w[5]; out[5] = cur.dz * w[5];
    out[6] = h;
}
