// snowgpu_roipool.hip -- RoI point pooling (snowgpu_roi_point_pool_device; definition: include/snowgpu.h; the enlarged roi, the runs and
// the scratch sizes: sg_roipool.h; presence, the record, the membership test, the grid and the footprint: sg_box.h).  The M rois of a frame
// are filed as the boxes of points_in_boxes are; then the members of every roi are counted and ranked IN ROW ORDER without a sort.  Five
// kernels on one stream, no memset:
//   k_roi_file    one workgroup per frame: k_box_file's steps for up to SG_ROI_MAX rois -- every roi enlarged and decided present or
//                 absent, its record and the used pose written, the frame's bit table cleared and every present roi marked by atomicOr in
//                 the cells its footprint can touch.
//   k_roi_count   one WAVE per run of SG_ROI_RUN consecutive rows of one frame (sg_roipool.h), 64 rows a step.  The wave ORs its lanes'
//                 cell words and visits the set bits of the union ascending: every lane whose own word has the bit makes the membership
//                 test, and the ballot of the members is that roi's members among these 64 rows, in lane = row order.  Its population
//                 is added to the wave's count of the roi in LDS; at the end the M counts go to the run's row of the scratch table.
//   k_roi_scan    one lane per (frame, roi): the runs' counts become exclusive prefixes in place, their sum is `count`.
//   k_roi_rank    the walk of k_roi_count again, the wave's LDS counts started from the run's prefix: a member's rank is that running
//                 count plus the members in lower lanes, __popcll(ballot & lanemask_lt); index[f, m, rank] = row if rank < S.
//   k_roi_finish  one lane per (f, m, j): the wrap-around fill j >= cnt -> slot j mod cnt, -1 for cnt = 0, the gather of `points` and
//                 `local` recomputed by sg_box_inside from the record and the row: the only full write of the big outputs, consecutive
//                 lanes at consecutive j.
// The walk visits a roi ONCE per step for the whole wave (not every lane its own lowest bit, as k_box_rows does): only then do the members
// of one roi meet in one ballot, which is what makes the lane order the row order.  A wave owns its run, so there is no scan across the
// waves of a block and no barrier inside the walk.  The marks are ORs, the counts integer sums in a fixed order: two calls give identical
// bytes.  The first four kernels are a launcher of their own, sg_launch_roi_members: the RoI-aware voxel pooling (snowgpu_roiaware.hip) starts
// from the same members in the same order.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_roipool.h"

#define SG_ROI_BLOCK 256
#define SG_ROI_WAVES (SG_ROI_BLOCK / 64)

template <typename T>
__global__ __launch_bounds__(SG_ROI_BLOCK) void k_roi_file(const T *__restrict__ rois, int32_t M, int32_t Cb, double ewx, double ewy, double ewz,
                                                           const double *__restrict__ pose_in, SgBoxRec *__restrict__ rec,
                                                           unsigned long long *__restrict__ table, double *__restrict__ out_pose)
{
    __shared__ int32_t rect[SG_ROI_MAX][4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int32_t W = sg_box_words(M);
    unsigned long long *tab = table + (int64_t)f * (SG_BOX_CELLS + 1) * W;
    for (int32_t i = tid; i < (SG_BOX_CELLS + 1) * W; i += SG_ROI_BLOCK) tab[i] = 0ull;
    for (int32_t b = tid; b < M; b += SG_ROI_BLOCK) {
        const int64_t q = (int64_t)f * M + b;
        SgBoxRec r;
        const bool present = sg_roi_make<T>(rois + q * Cb, ewx, ewy, ewz, pose_in ? pose_in + q * 2 : nullptr, &r);
        rec[q] = r;
        if (out_pose) { out_pose[q * 2] = r.c; out_pose[q * 2 + 1] = r.s; }
        int32_t ix0 = 1, ix1 = 0, iy0 = 1, iy1 = 0;                        // an absent roi: no cell
        if (present) sg_box_footprint(r, &ix0, &ix1, &iy0, &iy1);          // (the bound of sg_box.h holds as it is: sg_roipool.h)
        rect[b][0] = ix0; rect[b][1] = ix1; rect[b][2] = iy0; rect[b][3] = iy1;
    }
    __threadfence();                                                       // the cleared words before any mark
    __syncthreads();
    for (int32_t b = 0; b < M; ++b) {
        const int32_t ix0 = rect[b][0], ix1 = rect[b][1], iy0 = rect[b][2], iy1 = rect[b][3];
        if (ix0 > ix1) continue;
        const int32_t w = ix1 - ix0 + 1, cells = w * (iy1 - iy0 + 1);
        const unsigned long long bit = 1ull << (b & 63);
        if (tid == 0) atomicOr(&tab[(int64_t)SG_BOX_CELLS * W + (b >> 6)], bit);           // the frame's present rois
        for (int32_t i = tid; i < cells; i += SG_ROI_BLOCK)
            atomicOr(&tab[(int64_t)((iy0 + i / w) * SG_BOX_SIDE + ix0 + i % w) * W + (b >> 6)], bit);
    }
}

// the OR of a 64-bit word over the wave, in every lane
__device__ __forceinline__ unsigned long long roi_wave_or(unsigned long long v)
{
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, d);
        hi |= (uint32_t)__shfl_xor((int)hi, d);
    }
    return ((unsigned long long)hi << 32) | lo;
}

// The walk of one run by one wave: hit(m, members, mine) for every roi m that holds rows of the current 64, ascending in m within a step,
// the steps in row order; members is the ballot of the member lanes, mine whether this lane is one, row its global row.  Uniform across
// the wave: every lane arrives at every hit.
template <typename T, typename Hit>
__device__ __forceinline__ void roi_walk(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int f, int64_t run,
                                         const uint8_t *__restrict__ keep_in, int32_t M, const SgBoxRec *__restrict__ rec,
                                         const unsigned long long *__restrict__ table, Hit hit)
{
    const int lane = threadIdx.x & 63;
    const int32_t W = sg_box_words(M);
    int64_t a = frame_off[f], b = frame_off[f + 1];
    a = a < 0 ? 0 : a; b = b > n ? n : b;
    const int64_t start = a + run * SG_ROI_RUN, end = b < start + SG_ROI_RUN ? b : start + SG_ROI_RUN;
    const SgBoxRec *fr = rec + (int64_t)f * M;
    const unsigned long long *cells = table + (int64_t)f * (SG_BOX_CELLS + 1) * W;
    for (int64_t base = start; base < end; base += 64) {                   // (start and end are the wave's: a uniform loop)
        const int64_t i = base + lane;
        bool usable = i < end && (!keep_in || keep_in[i] != 0);
        double x = 0.0, y = 0.0, z = 0.0;
        if (usable) {
            const T *row = rows + i * 5;
            const T tx = row[0], ty = row[1], tz = row[2];
            usable = sg_box_row_usable<T>(tx, ty, tz);
            x = (double)tx; y = (double)ty; z = (double)tz;
        }
        const unsigned long long *words = cells + (usable ? (int64_t)sg_box_cell(x, y) * W : 0);
        for (int32_t w = 0; w < W; ++w) {
            const unsigned long long own = usable ? words[w] : 0ull;
            unsigned long long any = roi_wave_or(own);
            while (any != 0ull) {
                const int bit = __ffsll((long long)any) - 1;
                any &= any - 1ull;
                const int32_t m = w * 64 + bit;                            // (< M: only rois are marked)
                bool mine = false;
                if ((own >> bit) & 1ull) {
                    double lx, ly, sz;
                    mine = sg_box_inside(fr[m], x, y, z, &lx, &ly, &sz);
                }
                const unsigned long long members = __ballot(mine);
                if (members != 0ull) hit(m, members, mine, i);
            }
        }
    }
}

// grid ceil(runs / SG_ROI_WAVES) blocks per frame, frame after frame: wave w of a frame's block x owns its run x SG_ROI_WAVES + w
template <typename T>
__global__ __launch_bounds__(SG_ROI_BLOCK) void k_roi_count(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int64_t runs,
                                                            const uint8_t *__restrict__ keep_in, int32_t M, const SgBoxRec *__restrict__ rec,
                                                            const unsigned long long *__restrict__ table, int32_t *__restrict__ run_cnt)
{
    __shared__ int32_t cnt[SG_ROI_WAVES][SG_ROI_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t per_frame = (runs + SG_ROI_WAVES - 1) / SG_ROI_WAVES;
    const int f = (int)(blockIdx.x / per_frame);
    const int64_t run = (int64_t)(blockIdx.x % per_frame) * SG_ROI_WAVES + wave;
    for (int32_t m = lane; m < M; m += 64) cnt[wave][m] = 0;
    __syncthreads();
    if (run < runs)
        roi_walk<T>(rows, n, frame_off, f, run, keep_in, M, rec, table, [&](int32_t m, unsigned long long members, bool, int64_t) {
            if (lane == 0) cnt[wave][m] += (int32_t)__popcll(members);     // (lane 0 alone touches the wave's counts)
        });
    __syncthreads();
    if (run < runs) {
        int32_t *out = run_cnt + ((int64_t)f * runs + run) * M;
        for (int32_t m = lane; m < M; m += 64) out[m] = cnt[wave][m];
    }
}

// one lane per (frame, roi): exclusive prefixes over the frame's runs, in place; the sum is the count
__global__ __launch_bounds__(SG_ROI_BLOCK) void k_roi_scan(int32_t *__restrict__ run_cnt, int64_t runs, int32_t M, int64_t slots, int32_t *__restrict__ out_count)
{
    const int64_t q = (int64_t)blockIdx.x * SG_ROI_BLOCK + threadIdx.x;
    if (q >= slots) return;
    const int64_t f = q / M, m = q % M;
    int32_t *p = run_cnt + f * runs * M + m;
    int32_t sum = 0;
    for (int64_t r = 0; r < runs; ++r) {
        const int32_t c = p[r * M];
        p[r * M] = sum;
        sum += c;
    }
    out_count[q] = sum;
}

template <typename T>
__global__ __launch_bounds__(SG_ROI_BLOCK) void k_roi_rank(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int64_t runs,
                                                           const uint8_t *__restrict__ keep_in, int32_t M, int32_t S, const SgBoxRec *__restrict__ rec,
                                                           const unsigned long long *__restrict__ table, const int32_t *__restrict__ run_base,
                                                           int32_t *__restrict__ out_index)
{
    __shared__ int32_t cnt[SG_ROI_WAVES][SG_ROI_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t per_frame = (runs + SG_ROI_WAVES - 1) / SG_ROI_WAVES;
    const int f = (int)(blockIdx.x / per_frame);
    const int64_t run = (int64_t)(blockIdx.x % per_frame) * SG_ROI_WAVES + wave;
    if (run < runs) {
        const int32_t *in = run_base + ((int64_t)f * runs + run) * M;
        for (int32_t m = lane; m < M; m += 64) cnt[wave][m] = in[m];
    }
    __syncthreads();
    if (run >= runs) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t *index = out_index + (int64_t)f * M * S;
    roi_walk<T>(rows, n, frame_off, f, run, keep_in, M, rec, table, [&](int32_t m, unsigned long long members, bool mine, int64_t i) {
        int32_t before = 0;
        if (lane == 0) {                                                   // (lane 0 alone touches the wave's counts)
            before = cnt[wave][m];
            cnt[wave][m] = before + (int32_t)__popcll(members);
        }
        before = __shfl(before, 0);
        const int32_t rank = before + (int32_t)__popcll(members & below);
        if (mine && rank < S) index[(int64_t)m * S + rank] = (int32_t)i;
    });
}

// one lane per (f, m, j).  blank: a batch without a row -- the counts are written here, 0.
template <typename T>
__global__ __launch_bounds__(SG_ROI_BLOCK) void k_roi_finish(const T *__restrict__ rows, int64_t n, int32_t S, int32_t C, int64_t total, const SgBoxRec *__restrict__ rec,
                                                             int blank, int32_t *__restrict__ out_count, int32_t *__restrict__ out_index,
                                                             T *__restrict__ out_points, T *__restrict__ out_local)
{
    const int64_t t = (int64_t)blockIdx.x * SG_ROI_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int64_t q = t / S;
    const int32_t j = (int32_t)(t - q * S);
    int32_t cnt = 0;
    if (blank) {
        if (j == 0) out_count[q] = 0;
    } else {
        cnt = out_count[q];
    }
    int32_t at = -1;
    if (cnt > 0) {
        at = out_index[q * S + (j < cnt ? j : j % cnt)];                   // (slots below min(cnt, S) are k_roi_rank's; this kernel writes those from cnt on)
        if (at < 0 || at >= n) at = -1;                                    // (never: no row is read outside the batch)
        if (j >= cnt) out_index[t] = at;
    } else {
        out_index[t] = -1;
    }
    const T *row = at >= 0 ? rows + (int64_t)at * 5 : nullptr;
    if (out_points) {
        T *p = out_points + t * C;
        for (int32_t c = 0; c < C; ++c) p[c] = row ? row[c] : (T)0;
    }
    if (out_local) {
        double lx = 0.0, ly = 0.0, sz = 0.0;
        if (row) (void)sg_box_inside(rec[q], (double)row[0], (double)row[1], (double)row[2], &lx, &ly, &sz);
        out_local[t * 3] = (T)lx; out_local[t * 3 + 1] = (T)ly; out_local[t * 3 + 2] = (T)sz;
    }
}

// The members of every roi on `stream`: the rois filed, the walk twice with the scan between.  count receives every roi's members, index
// (n_frames, n_rois, n_slots) its first n_slots of them in row order; slots from the count on are NOT written.  rec: sg_box_records(n_frames,
// n_rois) records; table: sg_box_table(n_frames, n_rois) words; run_cnt: sg_roi_table(n_frames, max_frame, n_rois) int32.  A batch without a
// row has the rois filed and the pose written; nothing is launched over rows and count is not written.  snowgpu_roiaware.hip starts here too.
extern "C" int sg_launch_roi_members(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                                     int32_t n_rois, const void *rois, int32_t roi_features, const double *ew, int32_t n_slots, const double *pose_in,
                                     SgBoxRec *rec, unsigned long long *table, int32_t *run_cnt, int32_t *out_index, int32_t *out_count, double *out_pose,
                                     void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int64_t runs = sg_roi_runs(max_frame), slots = (int64_t)n_frames * n_rois;
    const dim3 walk((unsigned)((runs + SG_ROI_WAVES - 1) / SG_ROI_WAVES * n_frames));          // (below 2^31: sg_check_roipool_args)
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_roi_file<T>, dim3(n_frames), dim3(SG_ROI_BLOCK), 0, st, (const T *)rois, n_rois, roi_features, ew[0], ew[1], ew[2], pose_in, rec, table,
                           out_pose);
        SG_CHECK_LAUNCH();
        if (n > 0) {
            hipLaunchKernelGGL(k_roi_count<T>, walk, dim3(SG_ROI_BLOCK), 0, st, (const T *)rows, n, frame_off, runs, keep_in, n_rois, rec, table, run_cnt);
            SG_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_roi_scan, dim3((unsigned)((slots + SG_ROI_BLOCK - 1) / SG_ROI_BLOCK)), dim3(SG_ROI_BLOCK), 0, st, run_cnt, runs, n_rois, slots, out_count);
            SG_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_roi_rank<T>, walk, dim3(SG_ROI_BLOCK), 0, st, (const T *)rows, n, frame_off, runs, keep_in, n_rois, n_slots, rec, table, run_cnt,
                               out_index);
            SG_CHECK_LAUNCH();
        }
        return 0;
    });
}

// The whole sequence on `stream`: the members, then the finish.  A batch without a row has its pose written by the first kernel and
// everything else by the last; nothing is launched over rows.
extern "C" int sg_launch_roipool(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                                 int32_t n_rois, const void *rois, int32_t roi_features, const double *ew, int32_t n_samples, int32_t num_features,
                                 const double *pose_in, SgBoxRec *rec, unsigned long long *table, int32_t *run_cnt, int32_t *out_index, int32_t *out_count,
                                 void *out_points, void *out_local, double *out_pose, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = (int64_t)n_frames * n_rois * n_samples;
    if (int e = sg_launch_roi_members(rows, dtype, n, max_frame, frame_off, n_frames, keep_in, n_rois, rois, roi_features, ew, n_samples, pose_in, rec, table, run_cnt,
                                      out_index, out_count, out_pose, stream))
        return e;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_roi_finish<T>, dim3((unsigned)((total + SG_ROI_BLOCK - 1) / SG_ROI_BLOCK)), dim3(SG_ROI_BLOCK), 0, st, (const T *)rows, n, n_samples,
                           num_features, total, rec, n > 0 ? 0 : 1, out_count, out_index, (T *)out_points, (T *)out_local);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
