// snowgpu_ball.hip -- ball-query neighbour groups around keypoints (snowgpu_ball_query_device; definition: include/snowgpu.h; the grid, the
// window, the selection network and the scratch sizes: sg_ball.h).  Cell lists by count, scan and scatter -- the frame of a row, the
// presence test, the atomic per run of lanes and the scan are sg_rowkit.h's -- then one wave per centre; four kernels behind one memset,
// on one stream:
//   k_ball_count    every usable row: its cell (sg_ball_cell), kept per row, and one atomic on the cell's counter per run of lanes in it
//   k_ball_scan     one block per frame: the counters become the cells' first positions in the frame's slot of the sorted copy
//   k_ball_scatter  x, y, z AND THE SOURCE ROW of every usable row into its cell's span (the atomic that hands out the position turns the
//                   cell's entry into its END: cell c of a frame then spans [entry[c], entry[c + 1]), entry[0] the frame's first position)
//   k_ball_query    one wave per centre: the lanes stride over the span of every grid row of the window (coalesced: x, y, z and the source
//                   row are four arrays), one distance per candidate against the R squared radii, counts by ballot popcounts; per pair the
//                   wave keeps its 64 smallest indices ascending, one per lane, and takes a batch up only if a lane is in the ball with
//                   an index below the S-th kept one -- a wave-uniform branch -- by a bitonic sort of the batch and a bitonic merge.
//                   Then the padding with slot 0, -1 / 0 for an empty ball or an unusable centre, and the gather of the C columns.
// The order inside a span depends on the arrival of atomics; the result does not: counts are integers, and the kept set is the 64
// smallest indices of the ball whatever the order they are seen in.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sg_ball.h"
#include "sg_common.h"
#include "sg_launch.h"
#include "sg_rowkit.h"

#define SG_BALL_BLOCK 256
#define SG_BALL_SCAN_BLOCK 1024
#define SG_BALL_QUERY_WAVES 4       /* centres per block of k_ball_query */

// cell_of[i] = the entry of row i's cell (frame f, cell c: f (cells + 1) + 1 + c), or SG_NO_CELL for a row that is not usable
template <typename T>
__global__ __launch_bounds__(SG_BALL_BLOCK) void k_ball_count(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                             const uint8_t *__restrict__ keep_in, SgFpsRange range, SgBallGrid g,
                                                             uint32_t *__restrict__ entry, uint32_t *__restrict__ cell_of)
{
    const int64_t i = (int64_t)blockIdx.x * SG_BALL_BLOCK + threadIdx.x;
    uint32_t e = SG_NO_CELL;
    if (sg_row_present(frame_off, n_frames, keep_in, i, n)) {
        const T *row = rows + i * 5;
        const T x = row[0], y = row[1], z = row[2];
        if (sg_fps_usable<T>(range, x, y, z)) {
            const int f = sg_find_frame(frame_off, n_frames, i);
            e = (uint32_t)((int64_t)f * (g.cells + 1) + 1 + sg_ball_cell(g, (double)x, (double)y));
        }
    }
    sg_run_add(entry, e, SG_NO_CELL, threadIdx.x & 63);
    if (i < n) cell_of[i] = e;
}

// entry[f (cells + 1)] = frame_off[f]; entry[.. + 1 + c] = frame_off[f] + the rows filed in the cells before c
__global__ __launch_bounds__(SG_BALL_SCAN_BLOCK) void k_ball_scan(const int64_t *__restrict__ frame_off, int32_t cells, uint32_t *__restrict__ entry)
{
    uint32_t *e = entry + (int64_t)blockIdx.x * (cells + 1);
    const uint32_t first = (uint32_t)frame_off[blockIdx.x];
    if (threadIdx.x == 0) e[0] = first;
    sg_block_scan_excl<SG_BALL_SCAN_BLOCK>(e + 1, e + 1, cells, first);
}

template <typename T>
__global__ __launch_bounds__(SG_BALL_BLOCK) void k_ball_scatter(const T *__restrict__ rows, int64_t n, const uint32_t *__restrict__ cell_of,
                                                               uint32_t *__restrict__ entry, T *__restrict__ sx, T *__restrict__ sy, T *__restrict__ sz,
                                                               int32_t *__restrict__ ssrc)
{
    const int64_t i = (int64_t)blockIdx.x * SG_BALL_BLOCK + threadIdx.x;
    const uint32_t e = i < n ? cell_of[i] : SG_NO_CELL;
    const int64_t p = (int64_t)sg_run_claim(entry, e, SG_NO_CELL, threadIdx.x & 63);
    if (e == SG_NO_CELL) return;
    const T *row = rows + i * 5;                                      // (p below the frame's end: a frame files no more rows than it has)
    sx[p] = row[0]; sy[p] = row[1]; sz[p] = row[2];
    ssrc[p] = (int32_t)i;
}

// ---- the selection across the wave: sg_ball.h's network, the partner's value by DPP (distances 1, 2), ds_swizzle (4, 8, 16) and
// ds_bpermute (32, and the mirror of the merge) ---------------------------------------------------------------------------------------------
template <int J> __device__ __forceinline__ int32_t ball_partner(int32_t v, int lane)
{
    if constexpr (J == 1) return __builtin_amdgcn_update_dpp(v, v, 0xb1, 0xf, 0xf, false);            // quad_perm:[1,0,3,2]
    else if constexpr (J == 2) return __builtin_amdgcn_update_dpp(v, v, 0x4e, 0xf, 0xf, false);       // quad_perm:[2,3,0,1]
    else if constexpr (J <= 16) return __builtin_amdgcn_ds_swizzle(v, (J << 10) | 0x1f);              // bit mode: lane ^ J within 32 lanes
    else return __builtin_amdgcn_ds_bpermute((lane ^ J) << 2, v);
}
template <int S> __device__ __forceinline__ int32_t ball_sort_from(int32_t v, int lane)
{
    if constexpr (S < SG_BALL_SORT_STEPS) {
        constexpr int j = sg_ball_step_j(S), k = sg_ball_step_k(S);
        return ball_sort_from<S + 1>(sg_ball_cx(v, ball_partner<j>(v, lane), lane, j, k), lane);
    } else return v;
}
template <int J> __device__ __forceinline__ int32_t ball_clean_from(int32_t v, int lane)
{
    if constexpr (J >= 1) return ball_clean_from<J / 2>(sg_ball_cx(v, ball_partner<J>(v, lane), lane, J, 64), lane);
    else return v;
}
// kept (ascending over the lanes) and a batch in any order: the 64 smallest of both, ascending
__device__ __forceinline__ int32_t ball_take_up(int32_t kept, int32_t batch, int lane)
{
    batch = ball_sort_from<0>(batch, lane);
    const int32_t mirrored = __builtin_amdgcn_ds_bpermute((63 - lane) << 2, batch);
    return ball_clean_from<32>(sg_ball_meet(kept, mirrored), lane);
}

template <typename T>
__global__ __launch_bounds__(64 * SG_BALL_QUERY_WAVES) void k_ball_query(const T *__restrict__ rows, int n_frames, int32_t K, const T *__restrict__ centres,
                                                                         int32_t Cq, const uint32_t *__restrict__ entry, const T *__restrict__ sx,
                                                                         const T *__restrict__ sy, const T *__restrict__ sz, const int32_t *__restrict__ ssrc,
                                                                         SgBallGrid g, SgBallPairs<T> pr, int32_t C, int32_t *__restrict__ out_index,
                                                                         int32_t *__restrict__ out_count, T *__restrict__ out_points)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * SG_BALL_QUERY_WAVES + (threadIdx.x >> 6);      // the wave's centre
    if (q >= (int64_t)n_frames * K) return;                                                // (the whole wave)
    const int f = (int)(q / K);
    const T *c = centres + q * Cq;
    const T cx = c[0], cy = c[1], cz = c[2];
    int32_t kept[SG_BALL_MAX_RADII], cnt[SG_BALL_MAX_RADII];
#pragma unroll
    for (int i = 0; i < SG_BALL_MAX_RADII; ++i) { kept[i] = SG_BALL_EMPTY; cnt[i] = 0; }
    if (sg_ball_centre_usable<T>(cx, cy, cz)) {
        SgBallWindow w;
        sg_ball_window(g, (double)cx, (double)cy, &w);
        const uint32_t *e = entry + (int64_t)f * (g.cells + 1);
        for (int iy = w.iy0; iy <= w.iy1; ++iy) {
            const uint32_t b = e[iy * g.nx + w.ix0], end = e[iy * g.nx + w.ix1 + 1];
            for (uint32_t p0 = b; p0 < end; p0 += 64) {
                const uint32_t p = p0 + (uint32_t)lane;
                T d = (T)INFINITY;
                int32_t idx = SG_BALL_EMPTY;
                if (p < end) {
                    d = sg_fps_dist<T>(sx[p], sy[p], sz[p], cx, cy, cz);
                    idx = ssrc[p];
                }
#pragma unroll
                for (int i = 0; i < SG_BALL_MAX_RADII; ++i) {
                    if (i >= pr.n_radii) break;
                    const bool in = d < pr.r2[i];                                          // (false beyond the span's end)
                    cnt[i] += __popcll(__ballot(in));
                    const int32_t sth = __builtin_amdgcn_readlane(kept[i], pr.samples[i] - 1);
                    if (__ballot(sg_ball_wanted(in, idx, sth)) != 0ull) kept[i] = ball_take_up(kept[i], in ? idx : SG_BALL_EMPTY, lane);
                }
            }
        }
    }
    // the outputs of the centre: slots beyond the ball's rows repeat slot 0; -1 and 0 for an empty ball or an unusable centre
    const int64_t slot0 = q * pr.total;
#pragma unroll
    for (int i = 0; i < SG_BALL_MAX_RADII; ++i) {
        if (i >= pr.n_radii) break;
        const int32_t S = pr.samples[i], first = __builtin_amdgcn_readlane(kept[i], 0);
        const int32_t v = cnt[i] == 0 ? -1 : (lane < cnt[i] ? kept[i] : first);           // (lane < S <= 64 below: kept holds the 64 smallest)
        const int64_t base = slot0 + pr.seg[i];
        if (lane < S) out_index[base + lane] = v;
        if (lane == 0) out_count[q * pr.n_radii + i] = cnt[i];
        if (out_points)
            for (int32_t e0 = 0; e0 < S * C; e0 += 64) {
                const int32_t el = e0 + lane, slot = el / C, col = el - slot * C;
                const int32_t row = __shfl(v, slot & 63);
                if (el < S * C) out_points[(base + slot) * C + col] = row >= 0 ? rows[(int64_t)row * 5 + col] : (T)0;
            }
    }
}

// a batch without a row: every ball is empty
template <typename T>
__global__ __launch_bounds__(256) void k_ball_empty(int64_t slots, int64_t counts, int32_t C, int32_t *__restrict__ out_index, int32_t *__restrict__ out_count,
                                                   T *__restrict__ out_points)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < counts) out_count[e] = 0;
    if (e >= slots) return;
    out_index[e] = -1;
    if (out_points)
        for (int c = 0; c < C; ++c) out_points[e * C + c] = (T)0;
}

// The whole sequence on `stream`.  entry: sg_ball_entries(n_frames, g->cells) words; cell_of, ssrc: sg_ball_scratch(n) words; sx, sy, sz:
// as many values of the row dtype (all unused, and the fill kernel alone launched, for a batch without a row).
extern "C" int sg_launch_ball(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const SgFpsRange *range,
                              const SgBallGrid *g, int32_t n_centres, const void *centres, int32_t centre_features, int n_radii, const double *radii,
                              const int *n_samples, int32_t n_features, uint32_t *entry, uint32_t *cell_of, void *sx, void *sy, void *sz, int32_t *ssrc,
                              int32_t *out_index, int32_t *out_count, void *out_points, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        SgBallPairs<T> pr;
        sg_ball_make_pairs<T>(n_radii, radii, n_samples, &pr);
        const int64_t q = (int64_t)n_frames * n_centres, slots = q * pr.total, counts = q * n_radii;
        if (n <= 0) {
            hipLaunchKernelGGL(k_ball_empty<T>, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, slots, counts, n_features, out_index, out_count,
                               (T *)out_points);
            SG_CHECK_LAUNCH();
            return 0;
        }
        hipError_t me = hipMemsetAsync(entry, 0, sizeof(uint32_t) * sg_ball_entries(n_frames, g->cells), st);
        if (me != hipSuccess) return (int)me;
        const unsigned blocks = (unsigned)((n + SG_BALL_BLOCK - 1) / SG_BALL_BLOCK);
        hipLaunchKernelGGL(k_ball_count<T>, dim3(blocks), dim3(SG_BALL_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames, keep_in, *range, *g, entry, cell_of);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ball_scan, dim3(n_frames), dim3(SG_BALL_SCAN_BLOCK), 0, st, frame_off, g->cells, entry);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ball_scatter<T>, dim3(blocks), dim3(SG_BALL_BLOCK), 0, st, (const T *)rows, n, (const uint32_t *)cell_of, entry, (T *)sx, (T *)sy,
                           (T *)sz, ssrc);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_ball_query<T>, dim3((unsigned)((q + SG_BALL_QUERY_WAVES - 1) / SG_BALL_QUERY_WAVES)), dim3(64 * SG_BALL_QUERY_WAVES), 0, st,
                           (const T *)rows, n_frames, n_centres, (const T *)centres, centre_features, (const uint32_t *)entry, (const T *)sx, (const T *)sy,
                           (const T *)sz, (const int32_t *)ssrc, *g, pr, n_features, out_index, out_count, (T *)out_points);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
