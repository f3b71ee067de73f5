// sg_fps.h -- farthest point sampling of aligned batches (snowgpu_fps_device): the usable test, the distance, the candidate key and its
// fold, and the capacities of the resident tiers.  snowgpu_fps.hip runs these functions on the device, tests/host_harness/fps_walk.cpp the
// same code on the host (as sg_voxel.h is compiled for both), and tests/fps_reference.py restates the DEFINITION of include/snowgpu.h as
// a sequential NumPy program.
//
// The distance.  d(a, b) = ((dx dx) + (dy dy)) + (dz dz), dx = x_a - x_b, in the rows' dtype, every operation rounded on its own: no fused
// multiply-add (the build has -ffp-contract=off), no square root, no reciprocal.  Usable coordinates are within 1e6: no square overflows.
//
// The key.  A running minimum t is never negative and never NaN, so its bits order as an unsigned integer.  The candidate of a round is
// the pair (bits of t, ~p), p = the row's position among the usable rows of its frame, compared as one number: larger t first, then the
// SMALLER position.  float32: one 64-bit word, bits << 32 | ~p.  float64: two words compared in turn.  The all-zero key stands for "no
// candidate": every real key is larger (p < 2^30, so ~p > 0).  The fold is the maximum -- associative and commutative: how lanes, waves
// and tiles are combined decides nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#define SG_FPS_BLOCK 1024                   /* threads of the one workgroup that walks a frame */
#define SG_FPS_WAVES (SG_FPS_BLOCK / 64)
#define SG_FPS_BOUND 1e6                    /* |x|, |y|, |z| of a usable row (DROR's bound) */
#define SG_FPS_MAX_FRAME ((int64_t)1 << 30) /* usable rows of a frame: a position and its complement fit 32 bits */
// Resident tiers: x, y, z and t of every usable row of the frame stay in registers, 32 or 64 of them per lane (of the 128 a lane has with
// sixteen waves on a compute unit).  Beyond them x, y, z stream from scratch; t stays in LDS while the frame's usable rows fit 156 of the
// 160 KiB of a compute unit (tier 2), and streams from scratch too for a frame of more.
#define SG_FPS_TIER0_REGS 32
#define SG_FPS_TIER1_REGS 64
#define SG_FPS_TIER2_BYTES (156 * 1024)
#define SG_FPS_TIER0_ROWS_F32 (SG_FPS_BLOCK * (SG_FPS_TIER0_REGS / 4))      /*  8192:  8 rows per lane */
#define SG_FPS_TIER1_ROWS_F32 (SG_FPS_BLOCK * (SG_FPS_TIER1_REGS / 4))      /* 16384: 16 rows per lane */
#define SG_FPS_TIER2_ROWS_F32 (SG_FPS_TIER2_BYTES / 4)                      /* 39936 */
#define SG_FPS_TIER0_ROWS_F64 (SG_FPS_BLOCK * (SG_FPS_TIER0_REGS / 8))      /*  4096:  4 rows per lane */
#define SG_FPS_TIER1_ROWS_F64 (SG_FPS_BLOCK * (SG_FPS_TIER1_REGS / 8))      /*  8192:  8 rows per lane */
#define SG_FPS_TIER2_ROWS_F64 (SG_FPS_TIER2_BYTES / 8)                      /* 19968 */
#define SG_FPS_GAP 8                        /* elements of scratch between the compacted frames: each starts on a multiple of 4 and is padded to one */

// rows per lane of resident tier `tier` (0, 1) for rows of type T
template <typename T> struct SgFpsTier {
    static constexpr int P0 = SG_FPS_TIER0_REGS / (int)sizeof(T), P1 = SG_FPS_TIER1_REGS / (int)sizeof(T);
    static constexpr int ROWS2 = SG_FPS_TIER2_BYTES / (int)sizeof(T);      // usable rows whose t fit LDS
};

struct SgFpsRange {
    double lo[3], hi[3];           // x, y, z; -inf / +inf without a range
};

// where the compacted rows of the frame whose first row is `a` begin in the scratch arrays (frame f of the batch)
__host__ __device__ inline int64_t sg_fps_base(int64_t a, int f) { return (a + (int64_t)SG_FPS_GAP * f) & ~(int64_t)3; }

// elements of every scratch array for a batch of n rows in n_frames frames
static inline size_t sg_fps_scratch(int64_t n, int n_frames) { return (size_t)n + (size_t)SG_FPS_GAP * ((size_t)n_frames + 1); }

template <typename T>
__host__ __device__ inline bool sg_fps_usable(const SgFpsRange &r, T x, T y, T z)
{
    if (!(fabs((double)x) <= SG_FPS_BOUND && fabs((double)y) <= SG_FPS_BOUND && fabs((double)z) <= SG_FPS_BOUND)) return false;      // (false for NaN)
    return r.lo[0] <= (double)x && (double)x < r.hi[0] && r.lo[1] <= (double)y && (double)y < r.hi[1] && r.lo[2] <= (double)z && (double)z < r.hi[2];
}

template <typename T>
__host__ __device__ inline T sg_fps_dist(T xa, T ya, T za, T xb, T yb, T zb)
{
    const T dx = xa - xb, dy = ya - yb, dz = za - zb;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// min(t, d) as np.minimum gives it for numbers that are not NaN
template <typename T> __host__ __device__ inline T sg_fps_min(T t, T d) { return d < t ? d : t; }

__host__ __device__ inline uint32_t sg_fps_bits(float t)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(t);
#else
    uint32_t b; memcpy(&b, &t, 4); return b;
#endif
}
__host__ __device__ inline uint64_t sg_fps_bits(double t)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(t);
#else
    uint64_t b; memcpy(&b, &t, 8); return b;
#endif
}
__host__ __device__ inline float sg_fps_unbits(uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(b);
#else
    float t; memcpy(&t, &b, 4); return t;
#endif
}
__host__ __device__ inline double sg_fps_unbits(uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double t; memcpy(&t, &b, 8); return t;
#endif
}

template <typename T> struct SgFpsKey;
template <> struct SgFpsKey<float> {
    uint64_t w;                    // bits of t << 32 | ~p
};
template <> struct SgFpsKey<double> {
    uint64_t t;                    // bits of t
    uint32_t np;                   // ~p
};

__host__ __device__ inline SgFpsKey<float> sg_fps_key(float t, uint32_t p) { return SgFpsKey<float>{((uint64_t)sg_fps_bits(t) << 32) | (uint32_t)~p}; }
__host__ __device__ inline SgFpsKey<double> sg_fps_key(double t, uint32_t p) { return SgFpsKey<double>{sg_fps_bits(t), (uint32_t)~p}; }
template <typename T> __host__ __device__ inline SgFpsKey<T> sg_fps_no_key();
template <> __host__ __device__ inline SgFpsKey<float> sg_fps_no_key<float>() { return SgFpsKey<float>{0}; }
template <> __host__ __device__ inline SgFpsKey<double> sg_fps_no_key<double>() { return SgFpsKey<double>{0, 0}; }

// the larger of two keys
__host__ __device__ inline SgFpsKey<float> sg_fps_fold(SgFpsKey<float> a, SgFpsKey<float> b) { return b.w > a.w ? b : a; }
__host__ __device__ inline SgFpsKey<double> sg_fps_fold(SgFpsKey<double> a, SgFpsKey<double> b)
{
    return (b.t > a.t || (b.t == a.t && b.np > a.np)) ? b : a;
}

__host__ __device__ inline uint32_t sg_fps_key_pos(SgFpsKey<float> k) { return ~(uint32_t)k.w; }
__host__ __device__ inline uint32_t sg_fps_key_pos(SgFpsKey<double> k) { return ~k.np; }
__host__ __device__ inline float sg_fps_key_t(SgFpsKey<float> k) { return sg_fps_unbits((uint32_t)(k.w >> 32)); }
__host__ __device__ inline double sg_fps_key_t(SgFpsKey<double> k) { return sg_fps_unbits(k.t); }
