// sg_range.h -- range-image projection (snowgpu_range_image_device): the usable test, the range, the column, the image row and the key of
// a row.  snowgpu_range.hip runs these functions on the device, tests/host_harness/range_pixels.cpp the same code on the host (as
// sg_voxel.h and sg_ball.h are compiled for both), and tests/range_reference.py restates the DEFINITION of include/snowgpu.h in NumPy.
//
// Everything is float64 on (double)x, (double)y, (double)z, every operation rounded on its own -- no reciprocal, no fused multiply-add --
// and both angles are sg_atan2_cr's (sg_atan_cr.h: correctly rounded, the double that NumPy's arctan2 returns) -- evaluated by the math
// library's atan2 wherever that decides the same pixel, see "the guard" below:
//   r     = T(sqrt((x x + y y) + z z))                          rounded once more to the rows' dtype T: the value the image stores
//   col   = clip(floor((0.5 (-atan2(y, x) / pi + 1)) W), 0, W - 1)
//   row   = clip(floor((1 - (atan2(z, sqrt(x x + y y)) - fov_down) / (fov_up - fov_down)) H), 0, H - 1)        or ring[i]
// sqrt, the division and floor are correctly rounded on the host and on the device alike.
//
// The key.  float32: bits(r) << 32 | batch row.  r > 0 for a usable row, so its bits order as an unsigned integer does, and the minimum of
// the keys of a pixel is its smallest r and, among equal r, its smallest row: one 64-bit atomic min per row, whatever their arrival.
// float64: the key is bits(r) alone; a second pass takes the smallest row among those whose r equals the pixel's minimum.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "sg_atan_cr.h"

#define SG_RANGE_EMPTY 0xffffffffffffffffull      /* a pixel without a row: what the memset in front of the projection leaves */
#define SG_RANGE_PI 3.141592653589793             /* the double nearest pi: NumPy's np.pi */
#define SG_RANGE_MAX_ABS 1e6

struct SgRangeGeom {
    int32_t H, W;
    int32_t by_ring;                 // rows by channel (ring[i]) instead of by elevation
    double fov_up, fov_down;         // radians; not read with by_ring
    double lo, hi;                   // (double)T(lo), (double)T(hi): the limits rounded to the rows' dtype (exact in double, so
                                     // lo < (double)r < hi decides what T(lo) < r < T(hi) decides)
};

// the limits as the rows' dtype sees them (dtype 0: float32)
static inline void sg_range_limits(int dtype, const double *limits2, double *lo, double *hi)
{
    const double l = limits2 ? limits2[0] : 0.0, h = limits2 ? limits2[1] : INFINITY;
    *lo = dtype == 0 ? (double)(float)l : l;
    *hi = dtype == 0 ? (double)(float)h : h;
}

// |x|, |y|, |z| <= 1e6 (false for NaN)
__host__ __device__ inline bool sg_range_finite(double x, double y, double z)
{
    return fabs(x) <= SG_RANGE_MAX_ABS && fabs(y) <= SG_RANGE_MAX_ABS && fabs(z) <= SG_RANGE_MAX_ABS;
}

// the range in the rows' dtype
template <typename T> __host__ __device__ inline T sg_range_r(double x, double y, double z)
{
    return (T)sqrt((x * x + y * y) + z * z);
}

// ---- the two angles: a fast evaluation that decides the pixel away from its edges, the correctly rounded one near them -------------------
// px and py as functions of the angle, the arithmetic of the definition
__host__ __device__ inline double sg_range_px_at(double yaw, int32_t W) { return (0.5 * (yaw / SG_RANGE_PI + 1.0)) * (double)W; }
__host__ __device__ inline double sg_range_py_at(const SgRangeGeom &g, double pitch)
{
    return (1.0 - (pitch - g.fov_down) / (g.fov_up - g.fov_down)) * (double)g.H;
}

// THE DEFINITION: both angles from sg_atan2_cr
__host__ __device__ inline double sg_range_px_exact(double x, double y, int32_t W) { return sg_range_px_at(-sg_atan2_cr(y, x), W); }
__host__ __device__ inline double sg_range_py_exact(const SgRangeGeom &g, double x, double y, double z)
{
    return sg_range_py_at(g, sg_atan2_cr(z, sqrt(x * x + y * y)));
}

// The guard.  atan2() below is the math library's float64 atan2: the ROCm device library's on the device, libm's on the host.  The OpenCL C
// specification, whose accuracy table the device library's functions are written to, bounds its error by 6 ulp (the HIP math API
// reference reports 1 ulp measured); against the correctly rounded value that is E <= 6.5 ulp of the result.  With e = 2^-52:
//   px:  |yaw| <= pi < 4, so the two yaws differ by at most 6.5 * 2 e = 13 e.  t = yaw / pi, |t| <= 1: 13 e / pi + 2 * e / 4 < 4.7 e.
//        u = t + 1 in [0, 2]: + 2 * e / 2 -> 5.7 e.  0.5 u is exact.  px = (0.5 u) W <= W: 2.85 e W + 2 * e W / 2 < 4 e W.
//   py:  |pitch| <= pi / 2 < 2: 6.5 e.  a = pitch - fov_down, |a| <= pi: + 2 e -> 8.5 e.  q = a / D, D = fov_up - fov_down:
//        8.5 e / D + e |q|.  w = 1 - q: + e |w|.  py = w H: H (8.5 e / D + e |q| + e |w|) + e H |w| <= e H (8.5 / D + 3 |q| + 2).
// The bands taken are 2^-44 W = 256 e W and 2^-46 H (1 / D + |q| + 1) = 64 e H (1 / D + |q| + 1): 64 and 7 times the bounds above, and
// still sound for an atan2 that is 60 ulp off.  A fast p farther than its band from every integer has the floor of the exact p, so the
// same pixel after the clip; anything else -- p on an integer (the seam, the axis), p not finite, a band of 0.5 or more -- is decided by
// sg_atan2_cr.  At W = 2048 the column's band holds 2^-32 of the rows.  Measured on one MI355X (scripts/probe/range_ab.py, 256 C2
// sweeps): 0.88 ms by elevation and 0.84 ms by channel, against 1.38 and 0.98 ms with every angle from sg_atan2_cr; the bytes are the same.
#define SG_RANGE_BAND_X 0x1p-44
#define SG_RANGE_BAND_Y 0x1p-46

// p lies farther than `band` from every integer (false for a p that is not finite and for band >= 0.5)
__host__ __device__ inline bool sg_range_decided(double p, double band)
{
    const double d = p - floor(p);                         // exact
    return d > band && d < 1.0 - band;
}

__host__ __device__ inline double sg_range_px(double x, double y, int32_t W)
{
    const double px = sg_range_px_at(-atan2(y, x), W);
    return sg_range_decided(px, SG_RANGE_BAND_X * (double)W) ? px : sg_range_px_exact(x, y, W);
}

__host__ __device__ inline double sg_range_py(const SgRangeGeom &g, double x, double y, double z)
{
    const double pitch = atan2(z, sqrt(x * x + y * y)), D = g.fov_up - g.fov_down;
    const double py = sg_range_py_at(g, pitch);
    const double band = SG_RANGE_BAND_Y * (double)g.H * ((1.0 / D + fabs((pitch - g.fov_down) / D)) + 1.0);
    return sg_range_decided(py, band) ? py : sg_range_py_exact(g, x, y, z);
}

// clip(floor(p), 0, n - 1); p is finite for a row that passed sg_range_finite
__host__ __device__ inline int32_t sg_range_clip(double p, int32_t n)
{
    const double t = floor(p);
    return t <= 0.0 ? 0 : (t >= (double)(n - 1) ? n - 1 : (int32_t)t);
}

__host__ __device__ inline int32_t sg_range_col(const SgRangeGeom &g, double x, double y)
{
    return sg_range_clip(sg_range_px(x, y, g.W), g.W);
}
__host__ __device__ inline int32_t sg_range_row(const SgRangeGeom &g, double x, double y, double z)
{
    return sg_range_clip(sg_range_py(g, x, y, z), g.H);
}

// The pixel of a PRESENT row inside its frame's image, row W + col, and its range; -1 for a row that is not usable.  `ring`: the row's
// channel, read with g.by_ring only.
template <typename T> __host__ __device__ inline int32_t sg_range_pixel(const SgRangeGeom &g, T tx, T ty, T tz, int32_t ring, T *r_out)
{
    const double x = (double)tx, y = (double)ty, z = (double)tz;
    if (!sg_range_finite(x, y, z)) return -1;
    const T r = sg_range_r<T>(x, y, z);
    if (!(g.lo < (double)r && (double)r < g.hi)) return -1;
    if (g.by_ring && (ring < 0 || ring >= g.H)) return -1;
    *r_out = r;
    const int32_t row = g.by_ring ? ring : sg_range_row(g, x, y, z);
    return row * g.W + sg_range_col(g, x, y);
}

__host__ __device__ inline uint32_t sg_range_bits(float r)
{
    uint32_t b;
    memcpy(&b, &r, 4);
    return b;
}
__host__ __device__ inline unsigned long long sg_range_bits(double r)
{
    unsigned long long b;
    memcpy(&b, &r, 8);
    return b;
}
__host__ __device__ inline float sg_range_unbits(uint32_t b)
{
    float r;
    memcpy(&r, &b, 4);
    return r;
}
__host__ __device__ inline double sg_range_unbits(unsigned long long b)
{
    double r;
    memcpy(&r, &b, 8);
    return r;
}

// the key of batch row i (below 2^31) with range r > 0
__host__ __device__ inline unsigned long long sg_range_key(float r, uint32_t i) { return ((unsigned long long)sg_range_bits(r) << 32) | i; }
__host__ __device__ inline unsigned long long sg_range_key(double r, uint32_t) { return sg_range_bits(r); }

// `word` into *p if it is below what *p holds
__host__ __device__ inline void sg_range_lower(unsigned long long *p, unsigned long long word)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, word);
#else
    if (word < *p) *p = word;
#endif
}
__host__ __device__ inline void sg_range_lower(uint32_t *p, uint32_t word)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, word);
#else
    if (word < *p) *p = word;
#endif
}
