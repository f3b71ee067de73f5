// sg_iou.h -- rotated box IoU and NMS (snowgpu_boxes_iou_device, snowgpu_nms_device; the DEFINITION: include/snowgpu.h): which boxes are
// present, the record of a box, the overlap area of two boxes by clipping in a fixed order, the two IoUs and the sizes of the scratch.
// snowgpu_iou.hip runs these functions on the device, tests/host_harness/iou_clip.cpp the same code on the host (as sg_box.h is compiled
// for both), and tests/iou_reference.py restates the definition in NumPy.
//
// The record.  One per box, nine doubles: the centre, the three extents as they came (dx, dy, dz: the half extents are dx * 0.5 and so on,
// exact, WITHOUT the 1e-5 margin of the membership test -- pcdet's IoU has none), the pose (c, s) and ok = 1.  An absent box has a record
// of zeros; ok = 0 makes every IoU with it exactly 0.  Presence and pose follow sg_box_make to the letter.
//
// The area.  area(a, b): the four corners of a, in the order (+,+), (-,+), (-,-), (+,-), are moved into b's frame as the membership test
// moves a row, and the quadrilateral is clipped against u <= hxb, -u <= hxb, v <= hyb, -v <= hyb in this order (Sutherland-Hodgman); a
// point on the boundary is inside.  Then the shoelace sum, sequentially from vertex 0.  Only + - x / and comparisons in float64, every
// operation rounded on its own (-ffp-contract=off), so NumPy gives the same bytes.  No atan2, no angular sort.
//
// The capacity.  In exact arithmetic a convex quadrilateral clipped by four half-planes has at most 8 vertices.  In floating point it has
// more: two equal boxes, or two whose headings are 1 ulp apart, put several vertices within rounding of one clip line, and a pass can meet
// two runs of outside vertices where geometry has one -- the host harness sees up to 10.  What can be said for every input: a pass over n
// vertices emits the inside ones and two crossings per run of outside ones, and there are no more runs than inside or outside vertices,
// so it emits at most n + floor(n / 2): 4 -> 6 -> 9 -> 13 -> 19.  A polygon is held in SG_IOU_CAP = 20 slots, so NO VERTEX IS EVER DROPPED
// and the definition needs no rule for it.  (The emit is guarded all the same; the harness asserts that the guard never acts.)
//
// area(a, b) and area(b, a) differ in their last bits.  The IoU matrix uses area(a_m, b_b), NMS area(candidate, kept).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_box.h"         // SG_BOX_POSE_TOL; SG_FPS_BOUND

#define SG_IOU_MAX 9216            /* boxes per frame on either side: 1 <= M, B <= 9216 */
#define SG_IOU_CAP 20              /* vertices of a clipped polygon: more than any input can produce (above) */
#define SG_IOU_EPS_BEV 1e-8        /* pcdet: max(Aa + Ab - inter, 1e-8) */
#define SG_IOU_EPS_3D 1e-6         /* pcdet: max(Va + Vb - I3, 1e-6) */
#define SG_IOU_MODE_BEV 0
#define SG_IOU_MODE_3D 1

struct SgIouRec {
    double cx, cy, cz, dx, dy, dz, c, s, ok;
};
#define SG_IOU_REC_DOUBLES 9

// elements (doubles) of the record scratch for n boxes in all
static inline size_t sg_iou_records(size_t n) { return n * (size_t)SG_IOU_REC_DOUBLES; }

// The record of the box b[0 .. 6] = (cx, cy, cz, dx, dy, dz, heading) under the caller's pose (pose_in[0 .. 1]) or, with NULL, under
// cos / sin of the heading in float64.  True: the box is present.  An absent box leaves a record of zeros.
template <typename T> __host__ __device__ inline bool sg_iou_make(const T *b, const double *pose_in, SgIouRec *r)
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
    r->dx = ok ? dx : 0.0; r->dy = ok ? dy : 0.0; r->dz = ok ? dz : 0.0;
    r->c = ok ? c : 0.0; r->s = ok ? s : 0.0; r->ok = ok ? 1.0 : 0.0;
    return ok;
}

// area(a, b) of two present boxes.  *most, when given, is raised to the largest number of vertices a pass wanted to emit (the harness).
__host__ __device__ inline double sg_iou_area(const SgIouRec &a, const SgIouRec &b, int *most)
{
    const double hxa = a.dx * 0.5, hya = a.dy * 0.5, hxb = b.dx * 0.5, hyb = b.dy * 0.5;
    double pu[SG_IOU_CAP], pv[SG_IOU_CAP], qu[SG_IOU_CAP], qv[SG_IOU_CAP];
    for (int k = 0; k < 4; ++k) {
        const double lx = (k == 0 || k == 3) ? hxa : -hxa, ly = k < 2 ? hya : -hya;
        const double x = a.cx + (lx * a.c - ly * a.s), y = a.cy + (lx * a.s + ly * a.c);
        const double sx = x - b.cx, sy = y - b.cy;
        pu[k] = sx * b.c + sy * b.s;
        pv[k] = sy * b.c - sx * b.s;
    }
    int n = 4;
    for (int pass = 0; pass < 4; ++pass) {
        const bool on_v = pass >= 2, neg = (pass & 1) != 0;
        const double h = on_v ? hyb : hxb;
        const double *su = (pass & 1) ? qu : pu, *sv = (pass & 1) ? qv : pv;
        double *du = (pass & 1) ? pu : qu, *dv = (pass & 1) ? pv : qv;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 == n ? 0 : i + 1;
            const double p_c = on_v ? sv[i] : su[i], p_o = on_v ? su[i] : sv[i];
            const double q_c = on_v ? sv[j] : su[j], q_o = on_v ? su[j] : sv[j];
            const double dp = neg ? -p_c : p_c, dq = neg ? -q_c : q_c;
            const bool in_p = dp <= h, in_q = dq <= h;
            if (in_p) {
                if (m < SG_IOU_CAP) { du[m] = su[i]; dv[m] = sv[i]; }
                ++m;
            }
            if (in_p != in_q) {
                const double t = (h - dp) / (dq - dp);
                const double o = p_o + t * (q_o - p_o), e = neg ? -h : h;
                if (m < SG_IOU_CAP) { du[m] = on_v ? o : e; dv[m] = on_v ? e : o; }
                ++m;
            }
        }
        if (most && m > *most) *most = m;
        n = m < SG_IOU_CAP ? m : SG_IOU_CAP;
        if (n == 0) return 0.0;
    }
    // (four passes: the polygon is back in pu, pv)
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        sum = sum + (pu[i] * pv[j] - pu[j] * pv[i]);
    }
    return 0.5 * fabs(sum);
}

// iou(a, b) with area(a, b); either box absent: exactly 0
__host__ __device__ inline double sg_iou_pair(const SgIouRec &a, const SgIouRec &b, int mode, int *most)
{
    if (a.ok == 0.0 || b.ok == 0.0) return 0.0;
    const double inter = sg_iou_area(a, b, most);
    const double Aa = a.dx * a.dy, Ab = b.dx * b.dy;
    if (mode == SG_IOU_MODE_BEV) {
        const double u = Aa + Ab - inter;
        return inter / (u > SG_IOU_EPS_BEV ? u : SG_IOU_EPS_BEV);
    }
    const double hza = a.dz * 0.5, hzb = b.dz * 0.5;
    const double ta = a.cz + hza, tb = b.cz + hzb, ba = a.cz - hza, bb = b.cz - hzb;
    const double top = ta < tb ? ta : tb, bot = ba > bb ? ba : bb;
    const double d = top - bot, h = d > 0.0 ? d : 0.0;
    const double i3 = inter * h, Va = Aa * a.dz, Vb = Ab * b.dz;
    const double u = Va + Vb - i3;
    return i3 / (u > SG_IOU_EPS_3D ? u : SG_IOU_EPS_3D);
}
