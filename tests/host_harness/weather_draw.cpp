// Host harness: the per-frame weather draw of csrc/sg_weather.h (sg_weather_frame -- the blocks, the scalars and the permutation that
// k_draw_weather runs on the device) compiled for the host, printed for tests/test_weather_reference.py to compare with the Python
// restatement of the specification (tests/weather_reference.py).
//   usage: weather_draw n_frames n_lasers n_sets step shuffle seed p_snow p_wet
//   plan:  water heights (0.0004, 0.0008, 0.002), pavement depths (0.001, 0.0012), noise floor 0.7, power factor 15, delta 0.5;
//          set_ids[s][c] = s * n_lasers + c; the thresholds T(p) = min(2^32, floor(p 2^32)) as snowgpu_draw_weather_device makes them
//   output: one line per frame: the n_lasers table ids, then the 8 doubles of the record (%.17g)
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sg_weather.h"

int main(int argc, char **argv)
{
    if (argc != 9) { fprintf(stderr, "usage: weather_draw n_frames n_lasers n_sets step shuffle seed p_snow p_wet\n"); return 2; }
    const int n_frames = atoi(argv[1]), n_lasers = atoi(argv[2]), n_sets = atoi(argv[3]);
    const uint64_t step = strtoull(argv[4], nullptr, 10);
    const int shuffle = atoi(argv[5]);
    const uint64_t seed = strtoull(argv[6], nullptr, 10);
    const double p_snow = atof(argv[7]), p_wet = atof(argv[8]);
    if (n_lasers < 1 || n_lasers > SG_WEATHER_MAX_LASERS || n_sets < 1 || n_sets > SG_WEATHER_MAX_SETS || n_frames < 1) return 2;
    auto threshold = [](double p) { const double t = std::floor(p * 4294967296.0); return t >= 4294967296.0 ? (uint64_t)1 << 32 : (uint64_t)t; };
    SgWeatherDraw d{};
    d.t_snow = threshold(p_snow); d.t_wet = threshold(p_wet);
    d.n_sets = n_sets; d.n_lasers = n_lasers; d.n_water = 3; d.n_pave = 2; d.shuffle = shuffle;
    d.water[0] = 0.0004; d.water[1] = 0.0008; d.water[2] = 0.002;
    d.pave[0] = 0.001; d.pave[1] = 0.0012;
    d.wet_noise_floor = 0.7; d.power_factor = 15.0; d.delta = 0.5;
    std::vector<int32_t> set_ids((size_t)n_sets * n_lasers), tids((size_t)n_lasers);
    for (size_t i = 0; i < set_ids.size(); ++i) set_ids[i] = (int32_t)i;
    for (int f = 0; f < n_frames; ++f) {
        double rec[SG_WEATHER_REC];
        sg_weather_frame(d, seed, step, (uint32_t)f, set_ids.data(), tids.data(), rec);
        for (int c = 0; c < n_lasers; ++c) printf("%d ", tids[c]);
        for (int k = 0; k < SG_WEATHER_REC; ++k) printf("%.17g%c", rec[k], k + 1 < SG_WEATHER_REC ? ' ' : '\n');
    }
    return 0;
}
