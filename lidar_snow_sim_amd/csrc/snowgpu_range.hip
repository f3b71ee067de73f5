// snowgpu_range.hip -- range-image projection of an aligned batch (snowgpu_range_image_device; definition: include/snowgpu.h; the usable
// test, the range, the column, the image row and the key: sg_range.h).  One 8-byte key per pixel, preset to all ones by a memset; then,
// on one stream:
//   k_range_project  one thread per row, coalesced over the batch: the row's pixel into pixel_of, its key into the pixel by ONE 64-bit
//                    atomic min, the pixel's count bumped when asked.  float32: the key is bits(r) << 32 | row, so the minimum IS the
//                    winner.  float64: the key is bits(r), the minimum is the winner's range.  The two angles of a row come from the
//                    device library's atan2 and, inside a guard band around every pixel edge, from sg_atan2_cr (sg_range.h: the guard).
//   k_range_tie      float64 only: every row whose range equals its pixel's minimum lowers the pixel's index (preset to all ones by a
//                    memset of the index output) by a 32-bit atomic min.  The pixel comes from pixel_of: no angle is evaluated twice.
//   k_range_finish   one thread per pixel: decodes the winner, gathers its row and writes the 1 + C planes and the index, every plane
//                    coalesced along W; -1 in an empty pixel.  Without keys (a batch without a row) every pixel is empty.
// Minima of integers: the result does not depend on the arrival of the atomics.  Whether a row is present and which frame it lies in:
// sg_rowkit.h.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_range.h"
#include "sg_rowkit.h"

#define SG_RANGE_BLOCK 256

template <typename T>
__global__ __launch_bounds__(SG_RANGE_BLOCK) void k_range_project(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                                 const uint8_t *__restrict__ keep_in, const int32_t *__restrict__ ring, SgRangeGeom g,
                                                                 unsigned long long *__restrict__ key, int32_t *__restrict__ pixel_of,
                                                                 int32_t *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * SG_RANGE_BLOCK + threadIdx.x;
    if (i >= n) return;
    int32_t p = -1;
    if (sg_row_present(frame_off, n_frames, keep_in, i, n)) {
        const T *row = rows + i * 5;
        T r;
        const int32_t q = sg_range_pixel<T>(g, row[0], row[1], row[2], g.by_ring ? ring[i] : 0, &r);
        if (q >= 0) {
            p = sg_find_frame(frame_off, n_frames, i) * (g.H * g.W) + q;      // (below F H W <= 2^31 - 1)
            sg_range_lower(&key[p], sg_range_key(r, (uint32_t)i));
            if (count) atomicAdd(&count[p], 1);
        }
    }
    pixel_of[i] = p;
}

__global__ __launch_bounds__(SG_RANGE_BLOCK) void k_range_tie(const double *__restrict__ rows, int64_t n, const int32_t *__restrict__ pixel_of,
                                                             const unsigned long long *__restrict__ key, uint32_t *__restrict__ index)
{
    const int64_t i = (int64_t)blockIdx.x * SG_RANGE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t p = pixel_of[i];
    if (p < 0) return;
    const double *row = rows + i * 5;
    if (sg_range_bits(sg_range_r<double>(row[0], row[1], row[2])) == key[p]) sg_range_lower(&index[p], (uint32_t)i);
}

// the winner of a pixel, -1 without one (float64: the tie pass left it in the index output)
__device__ __forceinline__ int32_t range_winner(float, const unsigned long long *key, const int32_t *, int64_t p, float *r)
{
    const unsigned long long k = key[p];
    if (k == SG_RANGE_EMPTY) return -1;
    *r = sg_range_unbits((uint32_t)(k >> 32));
    return (int32_t)(uint32_t)k;
}
__device__ __forceinline__ int32_t range_winner(double, const unsigned long long *key, const int32_t *index, int64_t p, double *r)
{
    const unsigned long long k = key[p];
    if (k == SG_RANGE_EMPTY) return -1;
    *r = sg_range_unbits(k);
    return index[p];
}

template <typename T>
__global__ __launch_bounds__(SG_RANGE_BLOCK) void k_range_finish(const T *__restrict__ rows, int64_t pixels, int32_t hw, int32_t C,
                                                                const unsigned long long *__restrict__ key, T *__restrict__ image, int32_t *index)
{
    const int64_t p = (int64_t)blockIdx.x * SG_RANGE_BLOCK + threadIdx.x;
    if (p >= pixels) return;
    T r = (T)-1;
    const int32_t w = key ? range_winner(T{}, key, index, p, &r) : -1;
    const int64_t f = p / hw;
    T *plane = image + f * (int64_t)(1 + C) * hw + (p - f * hw);
    plane[0] = r;
    const T *row = rows + (int64_t)(w < 0 ? 0 : w) * 5;
    for (int c = 0; c < C; ++c) plane[(int64_t)(c + 1) * hw] = w < 0 ? (T)-1 : row[c];
    index[p] = w;
}

// The whole sequence on `stream`.  key: n_frames H W words (unused, and the finish kernel alone launched behind the memset of the count,
// for a batch without a row).
extern "C" int sg_launch_range(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const int32_t *ring,
                               const SgRangeGeom *g, int32_t n_features, unsigned long long *key, void *out_image, int32_t *out_index,
                               int32_t *out_pixel_of, int32_t *out_count, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int32_t hw = g->H * g->W;
    const int64_t pixels = (int64_t)n_frames * hw;
    const unsigned pblocks = (unsigned)((pixels + SG_RANGE_BLOCK - 1) / SG_RANGE_BLOCK);
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipError_t me = out_count ? hipMemsetAsync(out_count, 0, sizeof(int32_t) * (size_t)pixels, st) : hipSuccess;
        if (me != hipSuccess) return (int)me;
        if (n > 0) {
            me = hipMemsetAsync(key, 0xff, sizeof(unsigned long long) * (size_t)pixels, st);
            if (me != hipSuccess) return (int)me;
            const unsigned blocks = (unsigned)((n + SG_RANGE_BLOCK - 1) / SG_RANGE_BLOCK);
            hipLaunchKernelGGL(k_range_project<T>, dim3(blocks), dim3(SG_RANGE_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames, keep_in, ring, *g, key,
                               out_pixel_of, out_count);
            SG_CHECK_LAUNCH();
            if constexpr (sizeof(T) == 8) {
                me = hipMemsetAsync(out_index, 0xff, sizeof(int32_t) * (size_t)pixels, st);
                if (me != hipSuccess) return (int)me;
                hipLaunchKernelGGL(k_range_tie, dim3(blocks), dim3(SG_RANGE_BLOCK), 0, st, (const double *)rows, n, (const int32_t *)out_pixel_of,
                                   (const unsigned long long *)key, (uint32_t *)out_index);
                SG_CHECK_LAUNCH();
            }
        }
        hipLaunchKernelGGL(k_range_finish<T>, dim3(pblocks), dim3(SG_RANGE_BLOCK), 0, st, (const T *)rows, pixels, hw, n_features,
                           (const unsigned long long *)(n > 0 ? key : nullptr), (T *)out_image, out_index);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
