// snowgpu_mask.hip -- an input keep mask for the aligned snowfall entry on gfx950 (wave64), with its launch wrappers.
//
//   k_mask_count / k_mask_scan / k_mask_offsets   the front end: present rows (keep-in byte != 0) per 1024-row tile, the per-frame scan of
//                those counts, and the exclusive scan of the per-frame totals over the frames -- the offsets of the compacted batch, which
//                never leave the device.  The scatter itself is k_crop_scatter (snowgpu_compact.hip: sg_launch_crop_scatter).  With per-frame
//                weather records (sg_weather.h) a frame's snow gate is part of the mask: k_mask_count and the scatter leave such a frame out.
//   k_finish_aligned_masked   k_finish_aligned for a batch that was compacted by such a mask: the decision and the output row of every
//                sorted position of the COMPACTED frame, written to the row's index in the caller's INPUT frame through the scatter's map.
//   k_fov_mask   the camera-FOV test (sg_in_fov) as a producer of such a mask.
//
// Everything between the front end and the finish runs on the compacted rows with the kernels of the unmasked call, untouched: same tiles,
// same sums, same bytes as that call on frames the caller compacted.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "sg_common.h"
#include "sg_kutil.h"
#include "sg_row.h"
#include "sg_finish.h"
#include "sg_launch.h"
#include "sg_weather.h"

// Present rows per tile.  An absent row is finished here: its keep byte is 0 and -- out of place (out_rows != null) -- its five columns are
// copied as they are (plain loads and stores of the row type: bit for bit, NaNs included).  out_keep may BE keep_in: the byte written is
// the byte read.
// weather (optional, n_frames x SG_WEATHER_REC): a frame whose snow gate is 0 has no present row for the snowfall stage -- it reaches the
// per-beam kernels as an empty frame -- but its keep bytes stay the caller's (1 without a mask): the frame is not cropped, it is left out.
// keep_in may be null only with weather (every row present).
template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void k_mask_count(const T *__restrict__ rows, const uint8_t *keep_in, const double *__restrict__ weather,
                                                         const int64_t *__restrict__ frame_off, T *__restrict__ out_rows, uint8_t *out_keep,
                                                         int32_t *__restrict__ tile_cnt, int64_t max_tiles)
{
    const int f = blockIdx.y;
    const bool gated = weather && weather[(int64_t)f * SG_WEATHER_REC + SG_W_SNOW] == 0.0;
    const int64_t base = frame_off[f], n = frame_off[f + 1] - base;
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    int c = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * SG_BLOCK + threadIdx.x;
        if (r >= n) continue;
        const uint8_t k = keep_in ? keep_in[base + r] : (uint8_t)1;
        if (k && !gated) { ++c; continue; }
        out_keep[base + r] = k;                  // (0, or the byte that came in for a frame that is left out)
        if (out_rows) {
            const T *s = rows + (base + r) * 5;
            T *d = out_rows + (base + r) * 5;
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3]; d[4] = s[4];
        }
    }
    __shared__ int s[4];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[(int64_t)f * max_tiles + blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// per frame (one wave): where each tile's present rows start in the compacted frame, and how many the frame has
__global__ __launch_bounds__(64) void k_mask_scan(const int64_t *__restrict__ frame_off, const int32_t *__restrict__ tile_cnt, int32_t *__restrict__ tile_base,
                                                  int64_t *__restrict__ counts, int64_t max_tiles)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int64_t n = frame_off[f + 1] - frame_off[f];
    const int64_t tiles = std::min<int64_t>((n + SG_TILE - 1) / SG_TILE, max_tiles);      // (k_mask_count's grid has no more)
    int64_t run = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += 64) {
        const int64_t t = t0 + lane;
        const int c = t < tiles ? tile_cnt[(int64_t)f * max_tiles + t] : 0;
        int inc = c;
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o); if (lane >= o) inc += v; }
        if (t < tiles) tile_base[(int64_t)f * max_tiles + t] = (int32_t)run + inc - c;       // (a frame has fewer than 2^31 rows)
        run += __shfl(inc, 63);
    }
    if (lane == 0) counts[f] = run;
}

// The offsets of the compacted batch: the exclusive scan of the frames' present rows, new_off[0 .. n_frames].  ONE block, which walks the
// frames 256 at a time (n_frames may exceed any block) and carries the running total.
__global__ __launch_bounds__(256) void k_mask_offsets(const int64_t *__restrict__ counts, int n_frames, int64_t *__restrict__ new_off)
{
    __shared__ long long s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    long long carry = 0;
    for (int f0 = 0; f0 < n_frames; f0 += 256) {
        const int f = f0 + tid;
        const long long c = f < n_frames ? (long long)counts[f] : 0;
        long long inc = c;
        for (int o = 1; o < 64; o <<= 1) { const long long v = __shfl_up(inc, o); if (lane >= o) inc += v; }
        if (lane == 63) s_wave[w] = inc;
        __syncthreads();
        long long before = carry;
        for (int ww = 0; ww < w; ++ww) before += s_wave[ww];
        if (f < n_frames) new_off[f] = before + inc - c;
        carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (tid == 0) new_off[n_frames] = carry;
}

// k_finish_aligned (snowgpu_compact.hip) for a masked batch.  crows / srows / rec / rng / perm and c_off describe the COMPACTED batch the
// per-beam kernels ran on; sorted position g of compacted frame f is compacted row j = perm[g] (firing order) or g, which is row map[j] of
// the caller's frame, at in_off[f].  Its five columns and its keep byte go there; counts and statistics are those of the compacted frame.
// Nothing here reads the caller's rows (out_rows may be them: in place), and the rows absent from the mask are not written.
template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void k_finish_aligned_masked(const T *__restrict__ crows, const T *__restrict__ srows, const int32_t *__restrict__ frame_unsorted,
                                                                    const uint32_t *__restrict__ rec, const uint32_t *__restrict__ rec_q, const T *__restrict__ rng,
                                                                    const double *__restrict__ thr_poly, const int32_t *__restrict__ perm, const int64_t *__restrict__ c_off,
                                                                    const int64_t *__restrict__ in_off, const int32_t *__restrict__ map, T *__restrict__ out_rows,
                                                                    uint8_t *__restrict__ out_keep, int32_t *__restrict__ tile_cnt, int64_t max_tiles, SgFov fov,
                                                                    unsigned long long *__restrict__ tiles_done, int32_t *__restrict__ tile_base, int64_t *__restrict__ out_counts,
                                                                    int64_t *__restrict__ out_stats, const unsigned long long *__restrict__ diff2)
{
    const int f = blockIdx.y;
    const int64_t base = c_off[f], n = c_off[f + 1] - base;
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) {
        if (tiles_done && blockIdx.x == 0 && threadIdx.x == 0) {       // no present row: no tile completes the frame, its counts here
            out_counts[f] = 0; out_stats[f * 3 + 0] = 0; out_stats[f * 3 + 1] = 0; out_stats[f * 3 + 2] = 0;
        }
        return;
    }
    const int64_t in_base = in_off[f], in_n = in_off[f + 1] - in_base;
    const bool uns = frame_unsorted[f] != 0;
    const T *rows = uns ? srows : crows;
    const double p0 = thr_poly[(int64_t)f * 3], p1 = thr_poly[(int64_t)f * 3 + 1], p2 = thr_poly[(int64_t)f * 3 + 2];
    int c = 0;
    uint32_t rcs[4];
    T dds[4], rv[4][5];
    int64_t dst[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * SG_BLOCK + threadIdx.x;
        const bool in = r < n;
        rcs[q] = in ? rec[base + r] : 0u;
        dds[q] = (in && rng != nullptr) ? rng[base + r] : (T)0;
        dst[q] = (in && uns) ? (int64_t)perm[base + r] : r;
#pragma unroll
        for (int j = 0; j < 5; ++j) rv[q][j] = in ? rows[(base + r) * 5 + j] : (T)0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (rcs[q] & SG_REC_SLOT) rcs[q] = rec_q[rcs[q] & ~SG_REC_SLOT];
        const int64_t r = tile0 + q * SG_BLOCK + threadIdx.x;
        dst[q] = (r < n && (uint64_t)dst[q] < (uint64_t)n) ? (int64_t)map[base + dst[q]] : -1;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + q * SG_BLOCK + threadIdx.x;
        if (r >= n) continue;
        const uint32_t rc = rcs[q];
        const SgDecision d = sg_row_decision<T>(rv[q], rc, dds[q], rng != nullptr, fov, p0, p1, p2);
        const SgRow<T> o = sg_rebuild_row<T>(rv[q], rc);
        if ((uint64_t)dst[q] < (uint64_t)in_n) {
            T *w = out_rows + (in_base + dst[q]) * 5;
            w[0] = o.x; w[1] = o.y; w[2] = o.z; w[3] = o.i; w[4] = o.lab;
            out_keep[in_base + dst[q]] = d.keep ? 1 : 0;
        }
        c += d.keep;
        c += (d.noise_ok && d.is_att) ? (1 << 16) : 0;
    }
    sg_tile_counts_done(f, n, c, 0, tile_cnt, max_tiles, nullptr, tiles_done, tile_base, out_counts, out_stats, diff2, nullptr, nullptr);
}

// large batches: the per-frame scan for counts and statistics as a launch of its own (k_compact_scan on the compacted offsets)
__global__ __launch_bounds__(64) void k_mask_finish_scan(const int64_t *__restrict__ c_off, const int32_t *__restrict__ tile_cnt, int32_t *__restrict__ tile_base,
                                                         int64_t *__restrict__ out_counts, int64_t *__restrict__ out_stats, const unsigned long long *__restrict__ diff2,
                                                         int64_t max_tiles)
{
    const int f = blockIdx.x;
    sg_compact_scan_frame(f, c_off[f + 1] - c_off[f], tile_cnt, tile_base, out_counts, out_stats, diff2, max_tiles, nullptr, nullptr, nullptr);
}

// out_keep[i] = (keep_in ? keep_in[i] : 1) && get_fov_flag(row i).  A row whose keep-in byte is 0 is not loaded.  out_keep may be keep_in.
template <typename T>
__global__ __launch_bounds__(256) void k_fov_mask(const T *__restrict__ rows, int64_t n, const uint8_t *keep_in, uint8_t *out_keep, SgFov fov)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        bool k = keep_in ? keep_in[i] != 0 : true;
        if (k) {
            const T *row = rows + i * 5;
            k = sg_in_fov(fov, (double)row[0], (double)row[1], (double)row[2]);
        }
        out_keep[i] = k ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------
// launch wrappers (C linkage, called from snowgpu_batch.cpp and snowgpu_device.cpp)

// The front end of a masked aligned call, on `stream`: new_off[0 .. n_frames] (device), the present rows of frame f at crows[new_off[f] ..]
// in input order, map[new_off[f] + j] = frame-local input row of compacted row j.  out_rows: null in place, else the absent rows are copied.
// weather: optional per-frame records; their snow gate is part of the mask (keep_in may then be null).
extern "C" int sg_launch_mask_front(const void *rows, int dtype, const uint8_t *keep_in, const double *weather, const int64_t *frame_off, int n_frames, void *out_rows,
                                    uint8_t *out_keep, int32_t *tile_cnt, int32_t *tile_base, int64_t *counts, int64_t *new_off, void *crows,
                                    int32_t *map, int64_t max_tiles, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)max_tiles, (unsigned)n_frames);
    int e = sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_mask_count<T>, grid, dim3(SG_BLOCK), 0, st, (const T *)rows, keep_in, weather, frame_off, (T *)out_rows, out_keep, tile_cnt, max_tiles);
        SG_CHECK_LAUNCH();
        return 0;
    });
    if (e) return e;
    hipLaunchKernelGGL(k_mask_scan, dim3(n_frames), dim3(64), 0, st, frame_off, (const int32_t *)tile_cnt, tile_base, counts, max_tiles);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mask_offsets, dim3(1), dim3(256), 0, st, (const int64_t *)counts, n_frames, new_off);
    SG_CHECK_LAUNCH();
    return sg_launch_crop_scatter(rows, dtype, keep_in, weather, frame_off, new_off, n_frames, tile_base, crows, map, max_tiles, stream);
}

extern "C" int sg_launch_finish_aligned_masked(const void *crows, const void *srows, const int32_t *frame_unsorted, int dtype, const uint32_t *rec, const uint32_t *rec_q,
                                               const void *rng, const double *thr_poly, const int32_t *perm, const int64_t *c_off, const int64_t *in_off,
                                               const int32_t *map, int n_frames, int32_t *tile_cnt, int32_t *tile_base, void *out_rows, uint8_t *out_keep,
                                               int64_t *out_counts, int64_t *out_stats, const unsigned long long *diff2, const SgFov *fov, int64_t max_tiles,
                                               unsigned long long *tiles_done /* n_frames words, zero */, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)max_tiles, (unsigned)n_frames);
    SgFov fv{};
    if (fov) fv = *fov;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_finish_aligned_masked<T>, grid, dim3(SG_BLOCK), 0, st, (const T *)crows, (const T *)srows, frame_unsorted, rec, rec_q, (const T *)rng, thr_poly,
                           perm, c_off, in_off, map, (T *)out_rows, out_keep, tile_cnt, max_tiles, fv, tiles_done, tile_base, out_counts, out_stats, diff2);
        SG_CHECK_LAUNCH();
        if (!tiles_done) {
            hipLaunchKernelGGL(k_mask_finish_scan, dim3(n_frames), dim3(64), 0, st, c_off, (const int32_t *)tile_cnt, tile_base, out_counts, out_stats, diff2, max_tiles);
            SG_CHECK_LAUNCH();
        }
        return 0;
    });
}

extern "C" int sg_launch_fov_mask(const void *rows, int dtype, int64_t n, const uint8_t *keep_in, uint8_t *out_keep, const SgFov *fov, void *stream)
{
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)sg_cu_count() * 16);
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_fov_mask<T>, dim3(blocks), dim3(256), 0, st, (const T *)rows, n, keep_in, out_keep, *fov);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
