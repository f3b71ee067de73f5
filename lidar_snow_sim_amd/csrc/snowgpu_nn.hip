// snowgpu_nn.hip -- nearest centres of every row (snowgpu_nearest_centres_device; definition: include/snowgpu.h; the grid, the ring walk,
// the stopping bound, the k-best insertion, the weights and the scratch sizes: sg_nn.h).  The K centres of a frame are filed, not its
// rows; two kernels on one stream, no memset:
//   k_nn_file   one workgroup per frame: the usable centres counted per cell in LDS (and the occupied box by LDS min / max), the counters
//               scanned into the cells' first positions, then every usable centre scattered as one record (x, y, z, centre number) into
//               its cell's span of the frame's slot of the sorted copy.  Cell c of a frame spans [entry[c], entry[c + 1]), positions
//               within the frame's K records; entry[cells] = its usable centres.
//   k_nn_walk   one LANE per row: sg_nn_walk over rings around the row's cell, the k best in registers (KK = k slots, one instance per k, every
//               loop over them unrolled), then index, dist2 and the weights.  Neighbouring lanes are neighbouring rows of the sensor's order
//               and walk neighbouring cells.  A row that is absent or not usable writes -1, +inf and 0.  Whether a row is present and
//               which frame it lies in: sg_rowkit.h.
// The order inside a span depends on the arrival of LDS atomics; the result does not (sg_nn.h: the bound is strict).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_nn.h"
#include "sg_common.h"
#include "sg_launch.h"
#include "sg_rowkit.h"

#define SG_NN_BLOCK 256

template <typename T>
__global__ __launch_bounds__(SG_NN_BLOCK) void k_nn_file(const T *__restrict__ centres, int32_t K, int32_t Cq, SgNnGrid g, uint32_t *__restrict__ entry,
                                                         int32_t *__restrict__ box, SgNnRec<T> *__restrict__ rec)
{
    __shared__ uint32_t cnt[SG_NN_MAX_CELLS];
    __shared__ uint32_t part[SG_NN_BLOCK];
    __shared__ int32_t bx[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const T *cen = centres + (int64_t)f * K * Cq;
    for (int32_t c = tid; c < g.cells; c += SG_NN_BLOCK) cnt[c] = 0u;
    if (tid == 0) { bx[0] = bx[2] = 0x7fffffff; bx[1] = bx[3] = -1; }
    __syncthreads();
    for (int64_t k = tid; k < K; k += SG_NN_BLOCK) {
        const T x = cen[k * Cq], y = cen[k * Cq + 1], z = cen[k * Cq + 2];
        if (!sg_ball_centre_usable<T>(x, y, z)) continue;
        const int32_t ix = sg_nn_ix(g, (double)x), iy = sg_nn_iy(g, (double)y);
        atomicAdd(&cnt[iy * g.nx + ix], 1u);
        atomicMin(&bx[0], ix); atomicMax(&bx[1], ix);
        atomicMin(&bx[2], iy); atomicMax(&bx[3], iy);
    }
    __syncthreads();
    // the counters become first positions: every thread takes `per` consecutive cells, the threads' sums are scanned through LDS
    const int32_t per = (g.cells + SG_NN_BLOCK - 1) / SG_NN_BLOCK, c0 = tid * per, c1 = c0 + per < g.cells ? c0 + per : g.cells;
    uint32_t sum = 0;
    for (int32_t c = c0; c < c1; ++c) sum += cnt[c];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < SG_NN_BLOCK; d <<= 1) {
        const uint32_t below = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += below;
        __syncthreads();
    }
    uint32_t *e = entry + (int64_t)f * (g.cells + 1);
    uint32_t run = part[tid] - sum;
    for (int32_t c = c0; c < c1; ++c) {
        const uint32_t v = cnt[c];
        e[c] = run;
        cnt[c] = run;                                                      // the cell's cursor for the scatter
        run += v;
    }
    if (tid == SG_NN_BLOCK - 1) e[g.cells] = part[tid];                    // the usable centres of the frame
    if (tid == 0) { box[f * 4] = bx[0]; box[f * 4 + 1] = bx[1]; box[f * 4 + 2] = bx[2]; box[f * 4 + 3] = bx[3]; }
    __syncthreads();
    SgNnRec<T> *out = rec + (int64_t)f * K;
    for (int64_t k = tid; k < K; k += SG_NN_BLOCK) {
        const T x = cen[k * Cq], y = cen[k * Cq + 1], z = cen[k * Cq + 2];
        if (!sg_ball_centre_usable<T>(x, y, z)) continue;
        const uint32_t p = atomicAdd(&cnt[sg_nn_iy(g, (double)y) * g.nx + sg_nn_ix(g, (double)x)], 1u);      // (p < K: a frame files no more than it has)
        SgNnRec<T> r;
        r.x = x; r.y = y; r.z = z; r.c = (int32_t)k;
        out[p] = r;
    }
}

template <typename T, int KK>
__global__ __launch_bounds__(SG_NN_BLOCK) void k_nn_walk(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                         const uint8_t *__restrict__ keep_in, SgFpsRange range, SgNnGrid g, int32_t K,
                                                         const uint32_t *__restrict__ entry, const int32_t *__restrict__ box,
                                                         const SgNnRec<T> *__restrict__ rec, int32_t *__restrict__ out_index,
                                                         T *__restrict__ out_dist, T *__restrict__ out_weight)
{
    const int64_t i = (int64_t)blockIdx.x * SG_NN_BLOCK + threadIdx.x;
    if (i >= n) return;
    SgNnKey<T> best[KK];
    sg_nn_clear<T, KK>(best);
    if (sg_row_present(frame_off, n_frames, keep_in, i, n)) {
        const T *row = rows + i * 5;
        const T x = row[0], y = row[1], z = row[2];
        if (sg_fps_usable<T>(range, x, y, z)) {
            const int f = sg_find_frame(frame_off, n_frames, i);
            const SgNnBox b{box[f * 4], box[f * 4 + 1], box[f * 4 + 2], box[f * 4 + 3]};
            sg_nn_walk<T, KK>(g, b, entry + (int64_t)f * (g.cells + 1), rec + (int64_t)f * K, x, y, z, best);
        }
    }
    T w[KK];
    if (out_weight) sg_nn_weights<T, KK>(best, w);
    const int64_t o = i * KK;
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        out_index[o + j] = sg_nn_key_c(best[j]);
        out_dist[o + j] = sg_nn_key_d(best[j]);
        if (out_weight) out_weight[o + j] = w[j];
    }
}

template <typename T, int KK>
static void nn_launch_walk(hipStream_t st, const void *rows, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const SgFpsRange *range,
                           const SgNnGrid *g, int32_t K, const uint32_t *entry, const int32_t *box, const void *rec, int32_t *out_index, void *out_dist,
                           void *out_weight)
{
    hipLaunchKernelGGL((k_nn_walk<T, KK>), dim3((unsigned)((n + SG_NN_BLOCK - 1) / SG_NN_BLOCK)), dim3(SG_NN_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames,
                       keep_in, *range, *g, K, entry, box, (const SgNnRec<T> *)rec, out_index, (T *)out_dist, (T *)out_weight);
}

// The whole sequence on `stream`.  entry: sg_nn_entries(n_frames, g->cells) words; box: sg_nn_boxes(n_frames) words; rec:
// sg_nn_records(n_frames, n_centres) records of the rows' dtype.  A batch without a row has no element to write: nothing is launched.
extern "C" int sg_launch_nn(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const SgFpsRange *range,
                            const SgNnGrid *g, int32_t n_centres, const void *centres, int32_t centre_features, int k, uint32_t *entry, int32_t *box, void *rec,
                            int32_t *out_index, void *out_dist, void *out_weight, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) return 0;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_nn_file<T>, dim3(n_frames), dim3(SG_NN_BLOCK), 0, st, (const T *)centres, n_centres, centre_features, *g, entry, box, (SgNnRec<T> *)rec);
        SG_CHECK_LAUNCH();
#define SG_NN_CASE(KK) \
    case KK: nn_launch_walk<T, KK>(st, rows, n, frame_off, n_frames, keep_in, range, g, n_centres, entry, box, rec, out_index, out_dist, out_weight); break
        switch (k) {
            SG_NN_CASE(1); SG_NN_CASE(2); SG_NN_CASE(3); SG_NN_CASE(4); SG_NN_CASE(5); SG_NN_CASE(6); SG_NN_CASE(7); SG_NN_CASE(8);
            default: return (int)hipErrorInvalidValue;                     // (the entry has refused it)
        }
#undef SG_NN_CASE
        SG_CHECK_LAUNCH();
        return 0;
    });
}
