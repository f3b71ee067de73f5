// snowgpu_weather.hip -- the per-frame weather draw on gfx950 (wave64): k_draw_weather, one wave per frame, and its launch wrapper.
//
// Which weather a frame gets -- its two gates, its wet settings, its table set and the order of that set's tables over the lasers -- is
// drawn on the device from Philox4x32-10 keyed by (seed; step, frame), the step read from DEVICE memory: a captured graph that holds the
// draw, the augmentation and a `step += 1` draws anew on every replay.  The draw itself is written down once, in sg_weather.h.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>
#include "sg_weather.h"
#include "sg_launch.h"

// One wave per frame.  The words of the permutation come from up to 32 independent Philox blocks (lanes 0 .. 31, one block each) and
// land in LDS; the swaps depend on each other, so lane 0 walks them there (at most 127); then every lane gathers its table ids.
__global__ __launch_bounds__(64) void k_draw_weather(SgWeatherDraw p, uint64_t seed, const uint64_t *__restrict__ step, const int32_t *__restrict__ set_ids,
                                                     int32_t *__restrict__ table_ids, double *__restrict__ weather)
{
    __shared__ uint32_t words[SG_WEATHER_MAX_LASERS];
    __shared__ uint8_t order[SG_WEATHER_MAX_LASERS];
    __shared__ int s_set;
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x, L = p.n_lasers;
    const uint64_t st = step[0];
    if (p.shuffle && lane < 32 && 4 * lane < L - 1) {
        uint32_t w[4];
        sg_weather_block(seed, st, f, 2u + (uint32_t)lane, w);
        for (int k = 0; k < 4; ++k) words[4 * lane + k] = w[k];
    }
    for (int c = lane; c < L; c += 64) order[c] = (uint8_t)c;
    __syncthreads();
    if (lane == 0) {
        double rec[SG_WEATHER_REC];
        s_set = sg_weather_scalars(p, seed, st, f, rec);
        double *o = weather + (int64_t)f * SG_WEATHER_REC;
        for (int k = 0; k < SG_WEATHER_REC; ++k) o[k] = rec[k];
        if (p.shuffle) sg_weather_permute(L, words, order);
    }
    __syncthreads();
    const int set = s_set;
    for (int c = lane; c < L; c += 64) table_ids[(int64_t)f * L + c] = set_ids[(int64_t)set * L + order[c]];
}

// the wet flags of a batch without a single row: "not asked" (2) or "returned as it came" (1)
__global__ void k_weather_flags(const double *__restrict__ weather, int n_frames, int32_t *__restrict__ flags)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_frames) flags[f] = weather[(int64_t)f * SG_WEATHER_REC + SG_W_WET] == 0.0 ? 2 : 1;
}

extern "C" int sg_launch_weather_flags(const double *d_weather, int n_frames, int32_t *d_flags, void *stream)
{
    hipLaunchKernelGGL(k_weather_flags, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), 0, (hipStream_t)stream, d_weather, n_frames, d_flags);
    SG_CHECK_LAUNCH();
    return 0;
}

extern "C" int sg_launch_draw_weather(const SgWeatherDraw *p, int n_frames, uint64_t seed, const uint64_t *d_step, const int32_t *d_set_ids,
                                      int32_t *d_table_ids, double *d_weather, void *stream)
{
    hipLaunchKernelGGL(k_draw_weather, dim3((unsigned)n_frames), dim3(64), 0, (hipStream_t)stream, *p, seed, d_step, d_set_ids, d_table_ids, d_weather);
    SG_CHECK_LAUNCH();
    return 0;
}
