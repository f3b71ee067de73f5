// snowgpu_targets.hip -- proposal target sampling (snowgpu_sample_rois_device; definition: include/snowgpu.h; the classes, the words, the
// split of the slots, the walk, the pick and what a slot stores: sg_targets.h; presence and the pose: sg_box.h).  One kernel, ONE WORKGROUP
// PER FRAME, everything between its steps in LDS:
//   classes   every lane decides the classes of its rois (sg_targets_classes) into one byte per roi;
//   lists     FG, HARD and -- behind HARD -- EASY are written in ascending roi number: SG_TGT_BLOCK rois a step, the ballot of a class's
//             members per wave, the waves' counts through LDS, a member's place = the members before this step + those of lower waves +
//             those in lower lanes.  uint16 entries: fg and bg hold at most M = 9216 each, 36 KB;
//   words     lane b draws Philox block b: the words of slots 4 b .. 4 b + 3;
//   walk      branch (a): lane 0 makes the fg_this <= S dependent swaps of the walk without replacement in LDS (sg_targets_walk);
//   slots     one lane per slot: the pick (sg_targets_slot) and every per-slot output (sg_targets_fill).
// No atomics, no memset, no scratch in global memory; the step is read from device memory by the kernel, so a captured graph draws anew
// when the caller advances it.  Integer sums in a fixed order and float64 operations rounded on their own: two calls give identical bytes.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_targets.h"

#define SG_TGT_BLOCK 512
#define SG_TGT_WAVES (SG_TGT_BLOCK / 64)

// The rois whose class byte has `bit`, ascending, into dest; returns their number.  Every lane of the block arrives; wave_cnt: SG_TGT_WAVES.
__device__ __forceinline__ int32_t tgt_list(const uint8_t *cls, int32_t M, int bit, uint16_t *dest, int32_t *wave_cnt)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t base = 0;
    for (int32_t start = 0; start < M; start += SG_TGT_BLOCK) {            // (uniform: M is the block's)
        const int32_t m = start + tid;
        const bool in = m < M && (cls[m] & bit) != 0;
        const unsigned long long votes = __ballot(in);
        if (lane == 0) wave_cnt[wave] = (int32_t)__popcll(votes);
        __syncthreads();
        int32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SG_TGT_WAVES; ++w) {
            const int32_t n = wave_cnt[w];
            before += w < wave ? n : 0;
            all += n;
        }
        if (in) dest[base + before + (int32_t)__popcll(votes & below)] = (uint16_t)m;      // (below the class's size <= M)
        base += all;
        __syncthreads();                                                   // the counts are read before the next step writes them
    }
    return base;
}

template <typename T>
__global__ __launch_bounds__(SG_TGT_BLOCK) void k_sample_rois(SgTargetCfg c, uint64_t seed, const uint64_t *__restrict__ step_p, int32_t M,
                                                              const T *__restrict__ rois, int32_t Cb, const T *__restrict__ overlap,
                                                              const int32_t *__restrict__ assign, int32_t B, const T *__restrict__ gt, int32_t Cg,
                                                              const double *__restrict__ pose_in, SgTargetOut<T> o)
{
    __shared__ uint16_t fg[SG_TARGETS_MAX], bg[SG_TARGETS_MAX];
    __shared__ uint8_t cls[SG_TARGETS_MAX];
    __shared__ uint32_t words[SG_TARGETS_SLOTS_MAX];
    __shared__ int32_t wave_cnt[SG_TGT_WAVES];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    rois += f * M * Cb; overlap += f * M; assign += f * M; gt += f * B * Cg;
    if (pose_in) pose_in += f * M * 2;
    for (int32_t m = tid; m < M; m += SG_TGT_BLOCK) {
        SgBoxRec rec;
        cls[m] = (uint8_t)sg_targets_classes<T>(c, rois + (int64_t)m * Cb, pose_in ? pose_in + (int64_t)m * 2 : nullptr, overlap[m], &rec);
    }
    const uint64_t step = *step_p;
    for (int32_t b = tid; 4 * b < c.S; b += SG_TGT_BLOCK) {                // (4 b + 3 < SG_TARGETS_SLOTS_MAX: S <= 1024)
        uint32_t w[4];
        sg_targets_block(seed, step, (uint32_t)f, (uint32_t)b, w);
        words[4 * b] = w[0]; words[4 * b + 1] = w[1]; words[4 * b + 2] = w[2]; words[4 * b + 3] = w[3];
    }
    __syncthreads();
    const int32_t n_fg = tgt_list(cls, M, SG_TARGETS_FG, fg, wave_cnt);
    const int32_t n_hard = tgt_list(cls, M, SG_TARGETS_HARD, bg, wave_cnt);
    const int32_t n_easy = tgt_list(cls, M, SG_TARGETS_EASY, bg + n_hard, wave_cnt);       // (n_hard + n_easy <= M: the two exclude each other)
    const SgTargetSplit s = sg_targets_split(c, n_fg, n_hard, n_easy);     // (the block's: every lane has the same counts)
    if (!s.fg_replace && s.fg_this > 0) {
        if (tid == 0) sg_targets_walk(s.fg_this, n_fg, words, fg);
        __syncthreads();
    }
    for (int32_t k = tid; k < c.S; k += SG_TGT_BLOCK)
        sg_targets_fill<T>(c, f, k, sg_targets_slot(s, k, n_fg, n_hard, n_easy, words, fg, bg), rois, Cb, overlap, assign, B, gt, Cg, pose_in, o);
    if (tid == 0) {
        o.segments[f * 3] = s.fg_this; o.segments[f * 3 + 1] = s.hard_this; o.segments[f * 3 + 2] = s.easy_this;
        o.class_count[f * 3] = n_fg; o.class_count[f * 3 + 1] = n_hard; o.class_count[f * 3 + 2] = n_easy;
    }
}

// The stage on `stream`: one kernel.  pose_in, out_pose and out_gt_local may be null.
extern "C" int sg_launch_sample_rois(const SgTargetCfg *cfg, int n_frames, int32_t n_rois, const void *rois, int32_t roi_features, const void *overlap,
                                     const int32_t *assign, int32_t n_gt, const void *gt, int32_t gt_features, int dtype, uint64_t seed,
                                     const uint64_t *d_step, const double *pose_in, int32_t *out_index, void *out_rois, void *out_roi_iou,
                                     int32_t *out_gt_index, void *out_gt_of_rois, uint8_t *out_reg_valid, void *out_cls_label, int32_t *out_segments,
                                     int32_t *out_class_count, double *out_pose, void *out_gt_local, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const SgTargetOut<T> o{out_index,        (T *)out_rois, (T *)out_roi_iou, out_gt_index, (T *)out_gt_of_rois, out_reg_valid,
                               (T *)out_cls_label, out_segments,  out_class_count,  out_pose,     (T *)out_gt_local};
        hipLaunchKernelGGL(k_sample_rois<T>, dim3((unsigned)n_frames), dim3(SG_TGT_BLOCK), 0, st, *cfg, seed, d_step, n_rois, (const T *)rois, roi_features,
                           (const T *)overlap, assign, n_gt, (const T *)gt, gt_features, pose_in, o);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
