// sg_weather.h -- the per-frame weather draw (snowgpu_draw_weather_device) and the layout of a weather record.  k_draw_weather
// (snowgpu_weather.hip) runs these functions on the device, tests/host_harness/weather_draw.cpp the same code on the host
// (as sg_range_index.h is compiled for both), and tests/weather_reference.py restates the SPECIFICATION below in Python integers.
//
// A weather record: 8 doubles per frame, [snow, wet, water_height, pavement_depth, wet_noise_floor, power_factor, delta, 0].
//
// The draw of frame f at step `step` under key `seed`.  W(b) = the four words of Philox4x32-10 with key seed, counter
// (step lo, step hi, f, 0x57544852 + b)  -- philox_u32x4(seed, idx = step, group = f, tag = "WTHR" + b) of sg_philox.h:
//   block 0   snow = w0 < T(p_snow), wet = w1 < T(p_wet), T(p) = min(2^32, floor(p 2^32)) (0: never, 1: always);
//             set = (w2 n_sets) >> 32;  water index = (w3 n_water) >> 32
//   block 1   pavement index = (w0 n_pave) >> 32
//   permutation   order = 0 .. L-1; for i = L-1 down to 1, k = L-1-i: r = word k % 4 of block 2 + k / 4, j = (r (i + 1)) >> 32,
//             swap order[i], order[j].  shuffle = 0: the identity.
//   table_ids[f][c] = set_ids[set][order[c]]
// Every draw is made whether or not its gate is on: a gate never shifts another frame's or another field's draw.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SG_WEATHER_REC 8
#define SG_W_SNOW 0
#define SG_W_WET 1
#define SG_W_WATER 2
#define SG_W_PAVE 3
#define SG_W_NOISE 4
#define SG_W_POWER 5
#define SG_W_DELTA 6

#define SG_WEATHER_TAG 0x57544852u   /* "WTHR" */
#define SG_WEATHER_MAX_LASERS 128
#define SG_WEATHER_MAX_SETS 64
#define SG_WEATHER_MAX_CHOICES 16

struct SgWeatherDraw {               // snowgpu_weather_plan as the kernel takes it
    uint64_t t_snow, t_wet;          // T(p_snow), T(p_wet): 0 .. 2^32
    int32_t n_sets, n_lasers, n_water, n_pave, shuffle;
    double water[SG_WEATHER_MAX_CHOICES], pave[SG_WEATHER_MAX_CHOICES];
    double wet_noise_floor, power_factor, delta;
};

// Philox4x32-10 (sg_philox.h: philox_u32x4) with the high products from 64-bit multiplies, so that the host compiles it too
__host__ __device__ inline void sg_weather_block(uint64_t seed, uint64_t step, uint32_t f, uint32_t b, uint32_t (&out)[4])
{
    uint32_t c0 = (uint32_t)step, c1 = (uint32_t)(step >> 32), c2 = f, c3 = SG_WEATHER_TAG + b;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// blocks 0 and 1: the frame's record (rec: SG_WEATHER_REC doubles); returns the table set drawn
__host__ __device__ inline int sg_weather_scalars(const SgWeatherDraw &p, uint64_t seed, uint64_t step, uint32_t f, double *rec)
{
    uint32_t w[4], v[4];
    sg_weather_block(seed, step, f, 0, w);
    sg_weather_block(seed, step, f, 1, v);
    const int iw = (int)(((uint64_t)w[3] * (uint64_t)p.n_water) >> 32), ip = (int)(((uint64_t)v[0] * (uint64_t)p.n_pave) >> 32);
    rec[SG_W_SNOW] = (uint64_t)w[0] < p.t_snow ? 1.0 : 0.0;
    rec[SG_W_WET] = (uint64_t)w[1] < p.t_wet ? 1.0 : 0.0;
    rec[SG_W_WATER] = p.water[iw];
    rec[SG_W_PAVE] = p.pave[ip];
    rec[SG_W_NOISE] = p.wet_noise_floor;
    rec[SG_W_POWER] = p.power_factor;
    rec[SG_W_DELTA] = p.delta;
    rec[7] = 0.0;
    return (int)(((uint64_t)w[2] * (uint64_t)p.n_sets) >> 32);
}

// the swaps of the permutation from its L - 1 words (word k = word k % 4 of block 2 + k / 4); order holds 0 .. L-1 on entry
template <typename Word, typename Order>
__host__ __device__ inline void sg_weather_permute(int L, const Word *words, Order *order)
{
    for (int i = L - 1; i >= 1; --i) {
        const uint32_t r = words[L - 1 - i];
        const int j = (int)(((uint64_t)r * (uint64_t)(i + 1)) >> 32);
        const Order t = order[i]; order[i] = order[j]; order[j] = t;
    }
}

// The whole draw of frame f, one thread: rec (SG_WEATHER_REC doubles) and table_ids (n_lasers) from set_ids (n_sets x n_lasers).
__host__ __device__ inline void sg_weather_frame(const SgWeatherDraw &p, uint64_t seed, uint64_t step, uint32_t f, const int32_t *set_ids,
                                                 int32_t *table_ids, double *rec)
{
    const int L = p.n_lasers;
    uint32_t words[SG_WEATHER_MAX_LASERS];
    uint8_t order[SG_WEATHER_MAX_LASERS];
    for (int c = 0; c < L; ++c) order[c] = (uint8_t)c;
    if (p.shuffle) {
        for (int b = 0; 4 * b < L - 1; ++b) {
            uint32_t w[4];
            sg_weather_block(seed, step, f, 2u + (uint32_t)b, w);
            for (int k = 0; k < 4; ++k) words[4 * b + k] = w[k];
        }
        sg_weather_permute(L, words, order);
    }
    const int set = sg_weather_scalars(p, seed, step, f, rec);
    for (int c = 0; c < L; ++c) table_ids[c] = set_ids[(int64_t)set * L + order[c]];
}
