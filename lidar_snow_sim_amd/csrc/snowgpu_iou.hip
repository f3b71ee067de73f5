// snowgpu_iou.hip -- rotated box IoU and NMS (snowgpu_boxes_iou_device, snowgpu_nms_device; definition: include/snowgpu.h; presence, the
// record, the clip, the two IoUs and the capacity of a polygon: sg_iou.h).  One pair per LANE everywhere; no atomics, no memset:
//   k_iou_rec    one lane per box: present or absent, the pose taken or computed, one record of nine doubles.
//   k_iou_pairs  one WAVE per box a_m, four of them per workgroup.  The workgroup stages 64 records of the b side in LDS, lane l clips a_m
//                into b_l's frame, stores the IoU and keeps the largest it has seen (strictly larger wins, so the smallest b stays);
//                behind the last tile the 64 lanes fold (value descending, then box number ascending) and lane 0 writes best.
//   k_nms_rank   the rank of every candidate by counting: 256 candidates per workgroup walk the frame's scores tile by tile through LDS;
//                rank = the candidates with a larger score, or an equal one and a smaller number.  order[rank] = box.
//   k_nms_sweep  one workgroup of sixteen waves per frame walks the ranking in blocks of 64 candidates -- the lazy sweep: (1) lane l holds
//                candidate l and wave w tests it against the boxes kept so far, w, w + 16, ..., leaving at the first that suppresses
//                it; (2) the block's own 64 x 64 triangle, candidate j (uniform) against the earlier candidate i (the lane), one ballot
//                per j; (3) one lane resolves the block in rank order from the 64 masks.  It computes candidates x kept pairs
//                instead of B^2 / 2, keeps no mask in memory and leaves at post_max.  Then the workgroup writes every output in full.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_iou.h"
#include "sg_launch.h"

#define SG_IOU_BLOCK 256
#define SG_NMS_BLOCK 1024
#define SG_NMS_WAVES (SG_NMS_BLOCK / 64)
#define SG_NMS_TILE 1024

template <typename T>
__global__ __launch_bounds__(SG_IOU_BLOCK) void k_iou_rec(const T *__restrict__ boxes, int64_t n, int32_t Cb, const double *__restrict__ pose_in,
                                                          SgIouRec *__restrict__ rec)
{
    const int64_t q = (int64_t)blockIdx.x * SG_IOU_BLOCK + threadIdx.x;
    if (q >= n) return;
    SgIouRec r;
    sg_iou_make<T>(boxes + q * Cb, pose_in ? pose_in + q * 2 : nullptr, &r);
    rec[q] = r;
}

template <typename T>
__global__ __launch_bounds__(SG_IOU_BLOCK) void k_iou_pairs(const SgIouRec *__restrict__ rec_a, const SgIouRec *__restrict__ rec_b, int32_t M, int32_t B,
                                                            int32_t groups, int mode, T *__restrict__ out_iou, int32_t *__restrict__ out_best,
                                                            T *__restrict__ out_best_iou)
{
    __shared__ double tile[64 * SG_IOU_REC_DOUBLES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int32_t f = (int32_t)(blockIdx.x / (uint32_t)groups), m = (int32_t)(blockIdx.x % (uint32_t)groups) * (SG_IOU_BLOCK / 64) + w;
    const bool row = m < M;
    SgIouRec a = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (row) a = rec_a[(int64_t)f * M + m];
    const double *fb = (const double *)(rec_b + (int64_t)f * B);
    const int64_t total = (int64_t)B * SG_IOU_REC_DOUBLES;
    double best_v = 0.0;
    int32_t best_b = -1;
    for (int32_t b0 = 0; b0 < B; b0 += 64) {                              // (uniform across the workgroup)
        __syncthreads();                                                  // the tile of the step before has been read
        for (int32_t i = tid; i < 64 * SG_IOU_REC_DOUBLES; i += SG_IOU_BLOCK) {
            const int64_t at = (int64_t)b0 * SG_IOU_REC_DOUBLES + i;
            tile[i] = at < total ? fb[at] : 0.0;
        }
        __syncthreads();
        const int32_t b = b0 + lane;
        if (row && b < B) {
            const SgIouRec rb = *(const SgIouRec *)&tile[lane * SG_IOU_REC_DOUBLES];
            const double v = sg_iou_pair(a, rb, mode, nullptr);
            if (out_iou) out_iou[((int64_t)f * M + m) * B + b] = (T)v;
            if (v > best_v) { best_v = v; best_b = b; }
        }
    }
    if (!out_best && !out_best_iou) return;
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best_v, off);
        const int32_t ob = __shfl_xor(best_b, off);
        if (ov > best_v || (ov == best_v && ob >= 0 && (best_b < 0 || ob < best_b))) { best_v = ov; best_b = ob; }
    }
    if (row && lane == 0) {
        if (out_best) out_best[(int64_t)f * M + m] = best_b;
        if (out_best_iou) out_best_iou[(int64_t)f * M + m] = (T)best_v;
    }
}

// the key of box i of a frame: its score in float64 (the conversion keeps the order of T), NaN for a box that is no candidate
template <typename T> __device__ __forceinline__ double nms_key(const SgIouRec *__restrict__ rec, const T *__restrict__ scores, int64_t at, double score_thresh)
{
    const double s = (double)scores[at];
    return (rec[at].ok != 0.0 && s >= score_thresh) ? s : __longlong_as_double(0x7ff8000000000000ll);      // (s >= ... is false for NaN)
}

template <typename T>
__global__ __launch_bounds__(SG_IOU_BLOCK) void k_nms_rank(const SgIouRec *__restrict__ rec, const T *__restrict__ scores, int32_t B, int32_t groups,
                                                           double score_thresh, int32_t *__restrict__ order, int32_t *__restrict__ n_cand)
{
    __shared__ double tile[SG_NMS_TILE];
    const int tid = threadIdx.x;
    const int32_t f = (int32_t)(blockIdx.x / (uint32_t)groups), g = (int32_t)(blockIdx.x % (uint32_t)groups), j = g * SG_IOU_BLOCK + tid;
    const int64_t base = (int64_t)f * B;
    const double kj = j < B ? nms_key<T>(rec, scores, base + j, score_thresh) : __longlong_as_double(0x7ff8000000000000ll);
    int32_t before = 0, cands = 0;
    for (int32_t t0 = 0; t0 < B; t0 += SG_NMS_TILE) {
        __syncthreads();
        for (int32_t i = tid; i < SG_NMS_TILE; i += SG_IOU_BLOCK)
            tile[i] = t0 + i < B ? nms_key<T>(rec, scores, base + t0 + i, score_thresh) : __longlong_as_double(0x7ff8000000000000ll);
        __syncthreads();
        const int32_t n = B - t0 < SG_NMS_TILE ? B - t0 : SG_NMS_TILE;
        for (int32_t i = 0; i < n; ++i) {
            const double ki = tile[i];
            before += (ki > kj || (ki == kj && t0 + i < j)) ? 1 : 0;
            cands += ki == ki ? 1 : 0;
        }
    }
    if (kj == kj) order[base + before] = j;
    if (g == 0 && tid == 0) n_cand[f] = cands;
}

template <typename T>
__global__ __launch_bounds__(SG_NMS_BLOCK) void k_nms_sweep(const T *__restrict__ boxes, int32_t B, int32_t Cb, const T *__restrict__ scores,
                                                            const SgIouRec *__restrict__ rec, const int32_t *__restrict__ order,
                                                            const int32_t *__restrict__ n_cand, int mode, double iou_thresh, int32_t post_max,
                                                            int32_t *__restrict__ out_index, int32_t *__restrict__ out_count, T *__restrict__ out_boxes,
                                                            T *__restrict__ out_scores, uint8_t *__restrict__ out_kept)
{
    __shared__ int32_t kept_idx[SG_IOU_MAX];
    __shared__ uint8_t flag[SG_IOU_MAX];
    __shared__ double crec[64 * SG_IOU_REC_DOUBLES];
    __shared__ unsigned long long mask[64];
    __shared__ int32_t cidx[64], alive[64];
    __shared__ int32_t s_nk;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int32_t f = blockIdx.x;
    const int64_t base = (int64_t)f * B;
    const SgIouRec *fr = rec + base;
    const int32_t nc = n_cand[f];
    if (tid == 0) s_nk = 0;
    for (int32_t i = tid; i < B; i += SG_NMS_BLOCK) flag[i] = 0;
    __syncthreads();
    for (int32_t r0 = 0; r0 < nc; r0 += 64) {                             // (uniform: nc and s_nk are the workgroup's)
        const int32_t nk0 = s_nk;
        if (nk0 >= post_max) break;
        if (tid < 64) {
            const int32_t j = r0 + tid < nc ? order[base + r0 + tid] : -1;
            cidx[tid] = j;
            alive[tid] = j >= 0 ? 1 : 0;
            if (j >= 0) *(SgIouRec *)&crec[tid * SG_IOU_REC_DOUBLES] = fr[j];
        }
        __syncthreads();
        // (1) the candidate of this lane against the boxes kept in the blocks before
        const bool valid = cidx[lane] >= 0;
        SgIouRec mine = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (valid) mine = *(const SgIouRec *)&crec[lane * SG_IOU_REC_DOUBLES];
        bool dead = false;
        for (int32_t k = w; k < nk0; k += SG_NMS_WAVES) {
            if (valid && !dead) {
                const SgIouRec kb = fr[kept_idx[k]];
                dead = sg_iou_pair(mine, kb, mode, nullptr) > iou_thresh;
            }
        }
        if (dead) alive[lane] = 0;                                        // (every writer writes 0)
        __syncthreads();
        // (2) the block's own triangle: candidate j against the earlier candidate of this lane
        const bool me = valid && alive[lane] != 0;
        for (int32_t j = w; j < 64; j += SG_NMS_WAVES) {
            bool hit = false;
            if (me && lane < j && alive[j] != 0) {
                const SgIouRec cj = *(const SgIouRec *)&crec[j * SG_IOU_REC_DOUBLES];
                hit = sg_iou_pair(cj, mine, mode, nullptr) > iou_thresh;
            }
            const unsigned long long m = __ballot(hit);
            if (lane == 0) mask[j] = m;
        }
        __syncthreads();
        // (3) in rank order: kept iff alive and suppressed by no kept candidate of this block
        if (tid == 0) {
            unsigned long long kept_bits = 0ull;
            int32_t nk = nk0;
            for (int32_t j = 0; j < 64 && nk < post_max; ++j) {
                if (alive[j] != 0 && (mask[j] & kept_bits) == 0ull) {
                    kept_bits |= 1ull << j;
                    kept_idx[nk++] = cidx[j];
                    flag[cidx[j]] = 1;
                }
            }
            s_nk = nk;
        }
        __syncthreads();
    }
    __syncthreads();
    const int32_t nk = s_nk;
    if (tid == 0) out_count[f] = nk;
    for (int32_t k = tid; k < post_max; k += SG_NMS_BLOCK) {
        const int32_t j = k < nk ? kept_idx[k] : -1;
        out_index[(int64_t)f * post_max + k] = j;
        if (out_scores) out_scores[(int64_t)f * post_max + k] = j >= 0 ? scores[base + j] : (T)0;
    }
    if (out_boxes) {
        const int64_t cells = (int64_t)post_max * Cb;
        for (int64_t e = tid; e < cells; e += SG_NMS_BLOCK) {
            const int32_t k = (int32_t)(e / Cb), c = (int32_t)(e % Cb);
            out_boxes[(int64_t)f * cells + e] = k < nk ? boxes[(base + kept_idx[k]) * Cb + c] : (T)0;
        }
    }
    if (out_kept)
        for (int32_t i = tid; i < B; i += SG_NMS_BLOCK) out_kept[base + i] = flag[i];
}

// The records of n boxes on `stream`.
template <typename T> static int iou_records(const void *boxes, int64_t n, int32_t Cb, const double *pose_in, SgIouRec *rec, hipStream_t st)
{
    hipLaunchKernelGGL(k_iou_rec<T>, dim3((unsigned)((n + SG_IOU_BLOCK - 1) / SG_IOU_BLOCK)), dim3(SG_IOU_BLOCK), 0, st, (const T *)boxes, n, Cb, pose_in, rec);
    SG_CHECK_LAUNCH();
    return 0;
}

// The IoU matrix and the best box of every row: three kernels on `stream`.  rec: sg_iou_records(n_frames (M + B)) doubles.
extern "C" int sg_launch_iou(int n_frames, int32_t M, const void *boxes_a, int32_t a_features, int32_t B, const void *boxes_b, int32_t b_features, int dtype,
                             int mode, const double *pose_a, const double *pose_b, double *rec, void *out_iou, int32_t *out_best, void *out_best_iou,
                             void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    SgIouRec *ra = (SgIouRec *)rec, *rb = ra + (int64_t)n_frames * M;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (int e = iou_records<T>(boxes_a, (int64_t)n_frames * M, a_features, pose_a, ra, st)) return e;
        if (int e = iou_records<T>(boxes_b, (int64_t)n_frames * B, b_features, pose_b, rb, st)) return e;
        const int32_t groups = (M + SG_IOU_BLOCK / 64 - 1) / (SG_IOU_BLOCK / 64);
        hipLaunchKernelGGL(k_iou_pairs<T>, dim3((unsigned)((int64_t)n_frames * groups)), dim3(SG_IOU_BLOCK), 0, st, ra, rb, M, B, groups, mode, (T *)out_iou,
                           out_best, (T *)out_best_iou);
        SG_CHECK_LAUNCH();
        return 0;
    });
}

// NMS: three kernels on `stream`.  rec: sg_iou_records(n_frames B) doubles; order: n_frames B; n_cand: n_frames.
extern "C" int sg_launch_nms(int n_frames, int32_t B, const void *boxes, int32_t box_features, const void *scores, int dtype, int mode, double iou_thresh,
                             double score_thresh, int32_t post_max, const double *pose_in, double *rec, int32_t *order, int32_t *n_cand,
                             int32_t *out_index, int32_t *out_count, void *out_boxes, void *out_scores, uint8_t *out_kept, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    SgIouRec *r = (SgIouRec *)rec;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (int e = iou_records<T>(boxes, (int64_t)n_frames * B, box_features, pose_in, r, st)) return e;
        const int32_t groups = (B + SG_IOU_BLOCK - 1) / SG_IOU_BLOCK;
        hipLaunchKernelGGL(k_nms_rank<T>, dim3((unsigned)((int64_t)n_frames * groups)), dim3(SG_IOU_BLOCK), 0, st, r, (const T *)scores, B, groups, score_thresh,
                           order, n_cand);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_nms_sweep<T>, dim3((unsigned)n_frames), dim3(SG_NMS_BLOCK), 0, st, (const T *)boxes, B, box_features, (const T *)scores, r, order,
                           n_cand, mode, iou_thresh, post_max, out_index, out_count, (T *)out_boxes, (T *)out_scores, out_kept);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
