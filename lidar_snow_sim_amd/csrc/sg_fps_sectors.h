// sg_fps_sectors.h -- sectorized, proposal-centric keypoint sampling (snowgpu_fps_sectors_device; the DEFINITION: include/snowgpu.h): which
// rois are present and their reach, the near test, the sector of a row, the quotas of a frame's sectors, the ranks of a tile's rows within
// their sectors and the layout of the scratch.  snowgpu_fps.hip runs these functions on the device, tests/host_harness/fps_sectors.cpp the
// same code on the host (as sg_fps.h is compiled for both), and tests/fps_sectors_reference.py restates the definition in NumPy.
//
// The reach.  float64, every operation rounded on its own (the build has -ffp-contract=off):
//     reach = sqrt(((dx/2)(dx/2) + (dy/2)(dy/2)) + (dz/2)(dz/2)) + margin,   reach2 = reach reach
// sqrt is IEEE's, correctly rounded on the host and on the device alike (sg_range.h relies on the same).  A row is near the roi iff
// ((sx sx) + (sy sy)) + (sz sz) < reach2, STRICT.  An absent roi has the record (0, 0, 0, 0): no distance is below 0.
//
// The sector.  a = sg_atan2_cr(y, x) + pi in [0, 2 pi] (atan2 >= -pi, and -pi + pi = 0 exactly), s = min((int)floor(a / ((2 pi) / S)), S - 1).
// With S = 1 that is 0 for every row, and no angle is evaluated.
//
// The quota.  int64 throughout: n_s K < 2^30 2^31.  m >= K: q_s = floor(n_s K / m), r_s = n_s K mod m, L = K - sum q_s, and the L sectors
// first in the order (larger r_s, then smaller s) get one more.  include/snowgpu.h argues sum q_s = K, q_s <= n_s and r_s > 0 for the winners.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_atan_cr.h"
#include "sg_fps.h"

#define SG_FPSS_MAX_SECTORS 16
#define SG_FPSS_MAX_ROIS 256
#define SG_FPSS_PI 3.141592653589793        /* the double nearest pi: NumPy's np.pi */
// elements of scratch between the compacted frames: every one of a frame's up to 16 segments starts on a multiple of 4 and is padded to one
#define SG_FPSS_GAP (4 * SG_FPSS_MAX_SECTORS + 4)

struct SgFpsRoi {
    double cx, cy, cz, reach2;
};

// where the segments of frame f (first row `a`) begin in the scratch arrays, and the elements of every scratch array
__host__ __device__ inline int64_t sg_fpss_base(int64_t a, int f) { return (a + (int64_t)SG_FPSS_GAP * f) & ~(int64_t)3; }
static inline size_t sg_fpss_scratch(int64_t n, int n_frames) { return (size_t)n + (size_t)SG_FPSS_GAP * ((size_t)n_frames + 1); }

// The record of the roi b[0 .. 5] = (cx, cy, cz, dx, dy, dz).  True: the roi is present (the box stage's rule on these six values).
template <typename T> __host__ __device__ inline bool sg_fpss_roi(const T *b, double margin, SgFpsRoi *r)
{
    const double cx = (double)b[0], cy = (double)b[1], cz = (double)b[2], dx = (double)b[3], dy = (double)b[4], dz = (double)b[5];
    const bool ok = fabs(cx) <= SG_FPS_BOUND && fabs(cy) <= SG_FPS_BOUND && fabs(cz) <= SG_FPS_BOUND && dx > 0.0 && dx <= SG_FPS_BOUND && dy > 0.0 &&
                    dy <= SG_FPS_BOUND && dz > 0.0 && dz <= SG_FPS_BOUND;                                       // (false for NaN and inf)
    double reach2 = 0.0;
    if (ok) {
        const double hx = dx / 2.0, hy = dy / 2.0, hz = dz / 2.0;
        const double reach = sqrt(((hx * hx) + (hy * hy)) + (hz * hz)) + margin;
        reach2 = reach * reach;
    }
    r->cx = ok ? cx : 0.0; r->cy = ok ? cy : 0.0; r->cz = ok ? cz : 0.0; r->reach2 = reach2;
    return ok;
}

__host__ __device__ inline bool sg_fpss_near(const SgFpsRoi &r, double x, double y, double z)
{
    const double sx = x - r.cx, sy = y - r.cy, sz = z - r.cz;
    return ((sx * sx) + (sy * sy)) + (sz * sz) < r.reach2;
}

__host__ __device__ inline int sg_fpss_sector(double x, double y, int S)
{
    if (S == 1) return 0;
    const double a = sg_atan2_cr(y, x) + SG_FPSS_PI;
    const int s = (int)floor(a / ((2 * SG_FPSS_PI) / (double)S));
    return s < S - 1 ? s : S - 1;
}

// q[0 .. S - 1] from n[0 .. S - 1]; returns m = the sum of the n_s
__host__ __device__ inline int64_t sg_fpss_quota(const int64_t *n, int S, int64_t K, int32_t *q)
{
    int64_t m = 0;
    for (int s = 0; s < S; ++s) m += n[s];
    if (m < K) {
        for (int s = 0; s < S; ++s) q[s] = (int32_t)n[s];
        return m;
    }
    int64_t r[SG_FPSS_MAX_SECTORS], given = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t nk = n[s] * K;
        q[s] = (int32_t)(nk / m);
        r[s] = nk % m;
        given += q[s];
    }
    const int64_t L = K - given;
    for (int s = 0; s < S; ++s) {
        int before = 0;                    // the sectors in front of s in the order (larger r, then smaller s)
        for (int o = 0; o < S; ++o) before += (r[o] > r[s] || (r[o] == r[s] && o < s)) ? 1 : 0;
        if (before < L) q[s] += 1;
    }
    return m;
}

// The rank of a row among the rows of ITS sector within its wave, from the wave's ballot for that sector (lane = its lane), and the
// rows of the sector in the wave.
__host__ __device__ inline int sg_fpss_rank(unsigned long long ballot, int lane) { return __builtin_popcountll(ballot & ((1ull << lane) - 1ull)); }
