// snowgpu_centers.hip -- centre heatmap targets (snowgpu_assign_centers_device; definition: include/snowgpu.h; presence, the centre, the
// radius, the record, the value of a pixel and which gts reach a tile: sg_centers.h).  Two kernels on one stream:
//   k_center_gts   one workgroup of 256 per frame, one lane per gt: presence, centre, radius and head (sg_centers_gt); the rank of the gt
//                  within its head by one wave ballot per head and a prefix over the four waves' counts in LDS -- ascending g, no B x B
//                  loop; the slot table of the frame, NH x M gt numbers in LDS, cleared to -1 and then filled by the gts that got a slot;
//                  then one lane per slot writes the slot's six outputs from the table, the empty slots included: every element of the
//                  (F, NH, M) outputs gets exactly one store, and none depends on an order.  `state`, `count` and the gt's record of
//                  24 bytes (den, cix, ciy, r, the class or 0 when not drawn) into scratch;
//   k_center_heat  one workgroup per (tile of 64 x 16 pixels, class, frame) -- class and frame on grid.y and grid.z, the tile origin
//                  computed from blockIdx: all of them in scalar registers; the frame's records into LDS, lane = gt; the drawn gts of
//                  the class whose patch meets the tile listed in ascending g by a ballot and a prefix sum (sg_centers_near); wave w owns
//                  the rows w, w + 4, w + 8 and w + 12 of the tile, a lane one pixel of each: a wave's store is 64 consecutive float32,
//                  256 bytes of one row.  Every lane takes the maximum over the list and stores its four pixels, 0 included: no memset.
//                  A maximum of floats does not depend on the order.
// No atomics, no sort, no host read, no allocation: two calls give identical bytes.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_centers.h"

#define SG_CEN_BLOCK 256
#define SG_CEN_WAVES (SG_CEN_BLOCK / 64)
#define SG_CEN_ROWS (SG_CENTERS_TILE_H / SG_CEN_WAVES)         /* rows of a tile per wave */
#define SG_CEN_GRID_Z 65535
#define SG_CEN_GRID_X 1048576           /* tiles of one launch along grid.x; a workgroup walks the rest */

static_assert(SG_CENTERS_GT_MAX <= SG_CEN_BLOCK && SG_CENTERS_TILE_W == 64 && SG_CENTERS_TILE_H % SG_CEN_WAVES == 0, "one lane per gt, one wave per row");

template <typename T>
__global__ __launch_bounds__(SG_CEN_BLOCK) void k_center_gts(SgCenterCfg c, int32_t B, const T *__restrict__ gt, int32_t Cg, SgCenterRec *__restrict__ recs,
                                                             SgCenterOut<T> o)
{
    __shared__ int16_t s_slot[SG_CENTERS_HEADS_MAX * SG_CENTERS_OBJS_MAX];      // the gt of every slot, -1: empty
    __shared__ int32_t s_cnt[SG_CEN_WAVES][SG_CENTERS_HEADS_MAX];
    __shared__ int32_t s_cix[SG_CENTERS_GT_MAX], s_ciy[SG_CENTERS_GT_MAX], s_r[SG_CENTERS_GT_MAX];
    __shared__ double s_offx[SG_CENTERS_GT_MAX], s_offy[SG_CENTERS_GT_MAX];
    const int64_t f = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t NH = c.n_heads, M = c.max_objs, slots = NH * M;
    for (int32_t s = tid; s < slots; s += SG_CEN_BLOCK) s_slot[s] = -1;
    SgCenterGt me;
    me.state = SG_CENTERS_ABSENT; me.head = 0;
    if (tid < B) sg_centers_gt<T>(gt + (f * B + tid) * Cg, c, &me);         // (B <= SG_CENTERS_GT_MAX <= SG_CEN_BLOCK)
    const bool mine = tid < B && me.state == SG_CENTERS_DRAWN;
    int32_t below = 0;                                                      // the head's gts before this one in the wave
    for (int32_t h = 0; h < NH; ++h) {                                      // (uniform)
        const unsigned long long votes = __ballot(mine && me.head == h);
        if (lane == 0) s_cnt[wave][h] = (int32_t)__popcll(votes);
        if (me.head == h) below = (int32_t)__popcll(votes & ((1ull << lane) - 1ull));
    }
    __syncthreads();                                                        // the counts are in; the table is clear
    int32_t rank = below;
#pragma unroll
    for (int w = 0; w < SG_CEN_WAVES; ++w) rank += w < wave ? s_cnt[w][me.head] : 0;
    if (tid < B) {
        SgCenterRec r;
        o.state[f * B + tid] = sg_centers_record(me, mine ? rank : 0, M, &r);
        recs[f * B + tid] = r;
        s_cix[tid] = me.cix; s_ciy[tid] = me.ciy; s_r[tid] = me.r;
        s_offx[tid] = me.offx; s_offy[tid] = me.offy;
        if (r.cls != 0) s_slot[me.head * M + rank] = (int16_t)tid;          // (rank < M: a slot of its own, by the ranks)
    }
    if (tid < NH) {
        int32_t n = 0;
#pragma unroll
        for (int w = 0; w < SG_CEN_WAVES; ++w) n += s_cnt[w][tid];
        o.count[f * NH + tid] = n < M ? n : M;
    }
    __syncthreads();                                                        // the table is filled
    for (int32_t s = tid; s < slots; s += SG_CEN_BLOCK) {
        const int32_t g = s_slot[s], at = g < 0 ? 0 : g;
        sg_centers_slot<T>(c, f * slots + s, g, s_cix[at], s_ciy[at], s_r[at], s_offx[at], s_offy[at], o);
    }
}

__global__ __launch_bounds__(SG_CEN_BLOCK) void k_center_heat(int32_t F, int32_t NC, int32_t H, int32_t W, int32_t tiles_x, int32_t tiles, int32_t B,
                                                              const SgCenterRec *__restrict__ recs, float *__restrict__ heat)
{
    __shared__ SgCenterRec s[SG_CENTERS_GT_MAX];
    __shared__ uint16_t list[SG_CENTERS_GT_MAX];
    __shared__ int32_t wave_cnt[SG_CEN_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t cls = (int32_t)blockIdx.y + 1;                            // (uniform, as f, tile, tx0 and ty0 below)
    for (int32_t f = blockIdx.z; f < F; f += gridDim.z) {                   // (one frame per workgroup unless F > 65535)
        for (int32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (one tile per workgroup unless the map has more than 2^20)
            const int32_t tx0 = (tile % tiles_x) * SG_CENTERS_TILE_W, ty0 = (tile / tiles_x) * SG_CENTERS_TILE_H;
            bool hit = false;
            __syncthreads();                                                // the last tile's records and list are read before these are written
            if (tid < B) {                                                  // (B <= SG_CENTERS_GT_MAX <= SG_CEN_BLOCK)
                const SgCenterRec r = recs[(int64_t)f * B + tid];
                s[tid] = r;
                hit = sg_centers_near(r, cls, tx0, ty0);
            }
            const unsigned long long votes = __ballot(hit);
            if (lane == 0) wave_cnt[wave] = (int32_t)__popcll(votes);
            __syncthreads();
            int32_t before = 0, near = 0;
#pragma unroll
            for (int w = 0; w < SG_CEN_WAVES; ++w) {
                const int32_t n = wave_cnt[w];
                before += w < wave ? n : 0;
                near += n;
            }
            if (hit) list[before + (int32_t)__popcll(votes & ((1ull << lane) - 1ull))] = (uint16_t)tid;       // (below near <= B)
            __syncthreads();
            const int32_t px = tx0 + lane;
            float best[SG_CEN_ROWS];
#pragma unroll
            for (int j = 0; j < SG_CEN_ROWS; ++j) best[j] = 0.0f;
            for (int32_t k = 0; k < near; ++k) {                            // (the workgroup's)
                const SgCenterRec g = s[list[k]];
#pragma unroll
                for (int j = 0; j < SG_CEN_ROWS; ++j) {
                    const float v = sg_centers_value(g, px, ty0 + wave + j * SG_CEN_WAVES);
                    best[j] = v > best[j] ? v : best[j];
                }
            }
#pragma unroll
            for (int j = 0; j < SG_CEN_ROWS; ++j) {
                const int32_t py = ty0 + wave + j * SG_CEN_WAVES;
                if (px < W && py < H) heat[(((int64_t)f * NC + (cls - 1)) * H + py) * W + px] = best[j];
            }
        }
    }
}

// The stage on `stream`: two kernels.  recs: F B records of 24 bytes.
extern "C" int sg_launch_assign_centers(const SgCenterCfg *cfg, int n_frames, int32_t n_gt, const void *gt, int32_t gt_features, int dtype, void *recs,
                                        float *out_heatmap, int32_t *out_gt_index, int32_t *out_ind, uint8_t *out_mask, void *out_offset, int32_t *out_radius,
                                        int32_t *out_count, uint8_t *out_state, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const SgCenterOut<T> o{out_heatmap, out_gt_index, out_ind, out_mask, (T *)out_offset, out_radius, out_count, out_state};
        const int32_t tiles_x = sg_centers_tiles_x(cfg->W);
        const int64_t tiles = (int64_t)tiles_x * sg_centers_tiles_y(cfg->H);                 // (< 2^31: W H <= 2^31 - 1)
        const dim3 grid((unsigned)(tiles < SG_CEN_GRID_X ? tiles : SG_CEN_GRID_X), (unsigned)cfg->n_classes,
                        (unsigned)(n_frames < SG_CEN_GRID_Z ? n_frames : SG_CEN_GRID_Z));
        hipLaunchKernelGGL(k_center_gts<T>, dim3((unsigned)n_frames), dim3(SG_CEN_BLOCK), 0, st, *cfg, n_gt, (const T *)gt, gt_features, (SgCenterRec *)recs, o);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_center_heat, grid, dim3(SG_CEN_BLOCK), 0, st, (int32_t)n_frames, cfg->n_classes, cfg->H, cfg->W, tiles_x, (int32_t)tiles, n_gt,
                           (const SgCenterRec *)recs, out_heatmap);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
