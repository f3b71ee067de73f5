// snowgpu_anchors.hip -- anchor target assignment (snowgpu_assign_anchors_device; definition: include/snowgpu.h; presence, the BEV box, the
// overlap, the walk and the label rule: sg_anchors.h).  Four kernels on one stream:
//   k_anchor_gts    one workgroup per frame, one lane per gt: the gt's record (48 bytes) into scratch; the frame's `top` words and `gt_count`
//                   zeroed -- no memset anywhere;
//   k_anchor_best   one lane per (frame, anchor), the frame on grid.y: the box around the workgroup's 256 anchors (two cross-lane and
//                   cross-wave minima and maxima, once), the frame's records in LDS (12 KB at B = 256) and, by a ballot and a prefix sum,
//                   the ascending list of the gts NEAR that box (sg_anchors_near: every other gt meets every anchor of the workgroup at
//                   exactly 0 and decides nothing); per listed gt of the lane's class the overlap, the wave's maximum by a cross-lane
//                   reduction -- only where some lane of the wave has an overlap > 0 -- and ONE 64-bit integer atomicMax on the bits of
//                   that non-negative double per (wave, gt): a maximum does not depend on the order of arrival;
//   k_anchor_label  the same lanes, the same box and list: the walk (sg_anchors_walk), by the same function on the same records, hence with
//                   the same bits, compared with `top`; label, gt_index and iou written by the lane; `gt_count` by one integer atomic add
//                   per positive; the workgroup's positives, backgrounds and ignored by three wave ballots and a sum through LDS into
//                   scratch, one plain store each;
//   k_anchor_count  one workgroup per frame: `count` = the sums of the workgroups' three counts.  (One atomic add per wave on `count`
//                   was measured first: the 3 300 waves of a frame all add to the same word, and the label kernel took 423 us of the
//                   call's 520 at SECOND's head -- DESIGN.md section 9.)
// The anchors' records are rebuilt by each of the two kernels from the anchor's seven values (one row of at most 80 bytes) instead of being
// stored: F x A records of 48 bytes would be 162 MB at SECOND's head.  No sort, no host read, no allocation, no floating-point atomic:
// integer sums and maxima, float64 operations rounded on their own -- two calls give identical bytes.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_anchors.h"

#define SG_ANC_BLOCK SG_ANCHORS_GROUP
#define SG_ANC_WAVES (SG_ANC_BLOCK / 64)
#define SG_ANC_GRID_Y 65535

template <typename T>
__global__ __launch_bounds__(SG_ANC_BLOCK) void k_anchor_gts(int32_t n_classes, int32_t B, const T *__restrict__ gt, int32_t Cg, SgAnchorRec *__restrict__ recs,
                                                             unsigned long long *__restrict__ top, int32_t *__restrict__ gt_count)
{
    const int64_t f = blockIdx.x;
    const int g = threadIdx.x;
    if (g < B) {                                                            // (B <= SG_ANCHORS_GT_MAX = SG_ANC_BLOCK)
        SgAnchorRec r;
        (void)sg_anchors_gt<T>(gt + (f * B + g) * Cg, n_classes, &r);
        recs[f * B + g] = r;
        top[f * B + g] = 0ull;
        gt_count[f * B + g] = 0;
    }
}

// the record of the lane's anchor; class 0 for an absent anchor and for a lane behind the last anchor
template <typename T>
__device__ __forceinline__ SgAnchorRec anc_own(int32_t n_classes, int64_t a, int32_t A, const T *anchors, int32_t Ca, const int32_t *anchor_class)
{
    SgAnchorRec me;
    me.x0 = me.x1 = me.y0 = me.y1 = me.area = 0.0;
    me.cls = 0; me.pad = 0;
    if (a < A) (void)sg_anchors_anchor<T>(anchors + a * Ca, anchor_class[a], n_classes, &me);
    return me;
}

// The box around the workgroup's present anchors into bb (every lane gets it).  Every lane of the workgroup arrives; s_bb: SG_ANC_WAVES x 4.
__device__ __forceinline__ void anc_box(const SgAnchorRec &me, double (*s_bb)[4], double *bb)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    sg_anchors_bb_empty(bb);
    if (me.cls != 0) sg_anchors_bb_add(me, bb);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double x0 = __shfl_xor(bb[0], off), x1 = __shfl_xor(bb[1], off), y0 = __shfl_xor(bb[2], off), y1 = __shfl_xor(bb[3], off);
        bb[0] = x0 < bb[0] ? x0 : bb[0]; bb[1] = x1 > bb[1] ? x1 : bb[1];
        bb[2] = y0 < bb[2] ? y0 : bb[2]; bb[3] = y1 > bb[3] ? y1 : bb[3];
    }
    if (lane == 0) { s_bb[wave][0] = bb[0]; s_bb[wave][1] = bb[1]; s_bb[wave][2] = bb[2]; s_bb[wave][3] = bb[3]; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SG_ANC_WAVES; ++w) {
        bb[0] = s_bb[w][0] < bb[0] ? s_bb[w][0] : bb[0]; bb[1] = s_bb[w][1] > bb[1] ? s_bb[w][1] : bb[1];
        bb[2] = s_bb[w][2] < bb[2] ? s_bb[w][2] : bb[2]; bb[3] = s_bb[w][3] > bb[3] ? s_bb[w][3] : bb[3];
    }
}

// The frame's records into s and the gts near the workgroup's box, ascending, into list; returns their number.  Every lane of the workgroup
// arrives; wave_cnt: SG_ANC_WAVES.  Ends behind a barrier: s and list are ready.
__device__ __forceinline__ int32_t anc_near(const SgAnchorRec *__restrict__ recs, int32_t B, const double *bb, SgAnchorRec *s, uint16_t *list, int32_t *wave_cnt)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    bool hit = false;
    __syncthreads();                                                        // the last frame's records and list are read before these are written
    if (tid < B) {                                                          // (B <= SG_ANCHORS_GT_MAX = SG_ANC_BLOCK)
        const SgAnchorRec r = recs[tid];
        s[tid] = r;
        hit = sg_anchors_near(r, bb);
    }
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) wave_cnt[wave] = (int32_t)__popcll(votes);
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SG_ANC_WAVES; ++w) {
        const int32_t n = wave_cnt[w];
        before += w < wave ? n : 0;
        all += n;
    }
    if (hit) list[before + (int32_t)__popcll(votes & ((1ull << lane) - 1ull))] = (uint16_t)tid;       // (below all <= B)
    __syncthreads();
    return all;
}

template <typename T>
__global__ __launch_bounds__(SG_ANC_BLOCK) void k_anchor_best(int32_t n_classes, int32_t F, int32_t A, const T *__restrict__ anchors, int32_t Ca,
                                                              const int32_t *__restrict__ anchor_class, int32_t B, const SgAnchorRec *__restrict__ recs,
                                                              unsigned long long *__restrict__ top)
{
    __shared__ SgAnchorRec s[SG_ANCHORS_GT_MAX];
    __shared__ uint16_t list[SG_ANCHORS_GT_MAX];
    __shared__ double s_bb[SG_ANC_WAVES][4];
    __shared__ int32_t wave_cnt[SG_ANC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const SgAnchorRec me = anc_own<T>(n_classes, (int64_t)blockIdx.x * SG_ANC_BLOCK + tid, A, anchors, Ca, anchor_class);
    double bb[4];
    anc_box(me, s_bb, bb);
    for (int32_t f = blockIdx.y; f < F; f += gridDim.y) {                   // (uniform: one frame per workgroup unless F > 65535)
        const int32_t near = anc_near(recs + (int64_t)f * B, B, bb, s, list, wave_cnt);
        for (int32_t k = 0; k < near; ++k) {                                // (the workgroup's: every branch below is taken by whole waves)
            const int32_t g = list[k];
            double v = 0.0;
            if (me.cls == s[g].cls) v = sg_anchors_iou(me, s[g]);           // (a listed gt is present: its class is none of an absent anchor)
            if (__ballot(v > 0.0) == 0ull) continue;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double o = __shfl_xor(v, off);
                v = o > v ? o : v;
            }
            if (lane == 0) atomicMax(&top[(int64_t)f * B + g], sg_anchors_bits(v));
        }
    }
}

template <typename T>
__global__ __launch_bounds__(SG_ANC_BLOCK) void k_anchor_label(SgAnchorCfg c, int32_t F, int32_t A, const T *__restrict__ anchors, int32_t Ca,
                                                               const int32_t *__restrict__ anchor_class, int32_t B, const SgAnchorRec *__restrict__ recs,
                                                               const unsigned long long *__restrict__ top, int32_t *__restrict__ blk, SgAnchorOut<T> o)
{
    __shared__ int32_t s_cnt[SG_ANC_WAVES][3];
    __shared__ SgAnchorRec s[SG_ANCHORS_GT_MAX];
    __shared__ unsigned long long s_top[SG_ANCHORS_GT_MAX];
    __shared__ uint16_t list[SG_ANCHORS_GT_MAX];
    __shared__ double s_bb[SG_ANC_WAVES][4];
    __shared__ int32_t wave_cnt[SG_ANC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t a = (int64_t)blockIdx.x * SG_ANC_BLOCK + tid;
    const SgAnchorRec me = anc_own<T>(c.n_classes, a, A, anchors, Ca, anchor_class);
    double bb[4];
    anc_box(me, s_bb, bb);
    for (int32_t f = blockIdx.y; f < F; f += gridDim.y) {
        __syncthreads();                                                    // the last frame's words are read before these are written
        if (tid < B) s_top[tid] = top[(int64_t)f * B + tid];
        const int32_t near = anc_near(recs + (int64_t)f * B, B, bb, s, list, wave_cnt);      // (its barriers stand behind the store above)
        int32_t label = -1, arg = -1;
        double best = 0.0;
        if (me.cls != 0) {
            bool forced;
            sg_anchors_walk(me, s, list, near, s_top, &best, &arg, &forced);
            label = sg_anchors_label(c, me.cls, best, forced);
            if (label <= 0) arg = -1;
            if (label > 0) atomicAdd(&o.gt_count[(int64_t)f * B + arg], 1);        // (0 <= arg < B: a positive has best > 0)
        }
        if (a < A) {
            const int64_t at = (int64_t)f * A + a;
            o.label[at] = label;
            o.gt_index[at] = arg;
            if (o.iou) o.iou[at] = (T)best;
        }
        const unsigned long long pos = __ballot(me.cls != 0 && label > 0), neg = __ballot(me.cls != 0 && label == 0),
                                 ign = __ballot(me.cls != 0 && label < 0);
        if (lane == 0) {
            s_cnt[tid >> 6][0] = (int32_t)__popcll(pos); s_cnt[tid >> 6][1] = (int32_t)__popcll(neg); s_cnt[tid >> 6][2] = (int32_t)__popcll(ign);
        }
        __syncthreads();                                                    // (the next frame's barriers stand between this read and its next write)
        if (tid < 3) {
            int32_t n = 0;
#pragma unroll
            for (int w = 0; w < SG_ANC_WAVES; ++w) n += s_cnt[w][tid];
            blk[((int64_t)f * gridDim.x + blockIdx.x) * 3 + tid] = n;
        }
    }
}

// count[f] = the sums of the workgroups' three counts of frame f: one workgroup per frame, integer sums
__global__ __launch_bounds__(SG_ANC_BLOCK) void k_anchor_count(int32_t n_blocks, const int32_t *__restrict__ blk, int32_t *__restrict__ count)
{
    __shared__ int32_t s_cnt[SG_ANC_WAVES][3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t f = blockIdx.x;
    int32_t n[3] = {0, 0, 0};
    for (int32_t b = tid; b < n_blocks; b += SG_ANC_BLOCK) {
        const int32_t *p = blk + (f * n_blocks + b) * 3;
        n[0] += p[0]; n[1] += p[1]; n[2] += p[2];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n[0] += __shfl_xor(n[0], off); n[1] += __shfl_xor(n[1], off); n[2] += __shfl_xor(n[2], off);
    }
    if (lane == 0) { s_cnt[tid >> 6][0] = n[0]; s_cnt[tid >> 6][1] = n[1]; s_cnt[tid >> 6][2] = n[2]; }
    __syncthreads();
    if (tid < 3) {
        int32_t sum = 0;
#pragma unroll
        for (int w = 0; w < SG_ANC_WAVES; ++w) sum += s_cnt[w][tid];
        count[f * 3 + tid] = sum;
    }
}

// The stage on `stream`: four kernels.  recs: F B records; top: F B words; blk: F x sg_anchors_groups(A) x 3 int32; out_iou may be null.
extern "C" int sg_launch_assign_anchors(const SgAnchorCfg *cfg, int n_frames, int32_t n_anchors, const void *anchors, int32_t anchor_features,
                                        const int32_t *anchor_class, int32_t n_gt, const void *gt, int32_t gt_features, int dtype, void *recs,
                                        unsigned long long *top, int32_t *blk, int32_t *out_label, int32_t *out_gt_index, int32_t *out_count, int32_t *out_gt_count,
                                        void *out_iou, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        const SgAnchorOut<T> o{out_label, out_gt_index, out_count, out_gt_count, (T *)out_iou};
        const int32_t groups = sg_anchors_groups(n_anchors);
        const dim3 grid((unsigned)groups, (unsigned)(n_frames < SG_ANC_GRID_Y ? n_frames : SG_ANC_GRID_Y));
        hipLaunchKernelGGL(k_anchor_gts<T>, dim3((unsigned)n_frames), dim3(SG_ANC_BLOCK), 0, st, cfg->n_classes, n_gt, (const T *)gt, gt_features,
                           (SgAnchorRec *)recs, top, out_gt_count);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_anchor_best<T>, grid, dim3(SG_ANC_BLOCK), 0, st, cfg->n_classes, (int32_t)n_frames, n_anchors, (const T *)anchors, anchor_features,
                           anchor_class, n_gt, (const SgAnchorRec *)recs, top);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_anchor_label<T>, grid, dim3(SG_ANC_BLOCK), 0, st, *cfg, (int32_t)n_frames, n_anchors, (const T *)anchors, anchor_features, anchor_class,
                           n_gt, (const SgAnchorRec *)recs, (const unsigned long long *)top, blk, o);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_anchor_count, dim3((unsigned)n_frames), dim3(SG_ANC_BLOCK), 0, st, groups, (const int32_t *)blk, out_count);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
