// snowgpu_roiaware.hip -- RoI-aware voxel pooling (snowgpu_roi_voxel_pool_device; definition: include/snowgpu.h; the sub-voxel of a member
// and the scratch sizes: sg_roiaware.h).  The members of every roi come from the pooling stage's own kernels (sg_launch_roi_members of
// snowgpu_roipool.hip: the rois filed, the walk twice with the scan between), which leave a roi's first P = roi_capacity members IN ROW
// ORDER in the scratch `list`.  Behind them, on the same stream, no memset:
//   k_roiaware_bucket  one WAVE per (frame, roi) groups its list by voxel, stably.  Pass A: every member's voxel is counted in LDS (integer
//                      adds: the order of arrival does not show).  The wave scans the G counts to exclusive offsets, writes `count` and the
//                      offset table, and leaves the offsets in LDS as the voxels' cursors.  Pass B: the list again in chunks of 64 members,
//                      chunk after chunk; within a chunk the distinct voxels are visited one by one -- the first lane still to be served
//                      names the voxel, the ballot of the lanes with that voxel gives every one of them its place behind the cursor
//                      (__popcll(ballot & lanemask_lt): lane order is row order), and the cursor moves on by the ballot's population.
//                      The voxel is recomputed by sg_roiaware_voxel from what the membership test saw: both passes see the same number.
//   k_roiaware_pool    one lane per (f, m, g, channel), consecutive lanes at consecutive channels: the voxel's first min(count, T) rows
//                      in order -- the running maximum with its row, and the float32 sum, one add per member -- then max, argmax and avg.
//                      With Cf a multiple of 4 and aligned buffers a lane takes four channels: 16-byte loads and stores.
//   k_roiaware_index   one lane per (f, m, g, t): the voxel's t-th row or -1; four consecutive elements per lane into an aligned output.
//   k_roiaware_blank   a batch without a row: the zero counts (nothing is launched over rows; the two kernels above then write zeros and -1).
// No atomic's arrival order reaches an output: two calls give identical bytes.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_roiaware.h"

#define SG_RA_BLOCK 256

template <typename T>
__global__ __launch_bounds__(64) void k_roiaware_bucket(const T *__restrict__ rows, int64_t n, const T *__restrict__ rois, int32_t Cb, double ewx, double ewy,
                                                        double ewz, int32_t gx, int32_t gy, int32_t gz, int32_t P, const SgBoxRec *__restrict__ rec,
                                                        const int32_t *__restrict__ roi_count, const int32_t *__restrict__ list, int32_t *__restrict__ sorted,
                                                        int32_t *__restrict__ offset, int32_t *__restrict__ out_count)
{
    extern __shared__ int32_t next[];                                      // G int32: the voxels' counts, then their cursors
    const int64_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int32_t G = gx * gy * gz;
    const SgBoxRec r = rec[q];
    double dx, dy, dz;
    sg_roiaware_sizes<T>(rois + q * Cb, ewx, ewy, ewz, &dx, &dy, &dz);
    int32_t members = roi_count[q];
    members = members < 0 ? 0 : (members > P ? P : members);               // (only the first P were listed)
    const int32_t *mine = list + q * P;
    int32_t *out = sorted + q * P;
    auto voxel_of = [&](int32_t row) {
        const T *p = rows + (int64_t)row * 5;
        double lx, ly, sz;
        (void)sg_box_inside(r, (double)p[0], (double)p[1], (double)p[2], &lx, &ly, &sz);
        return sg_roiaware_voxel(lx, ly, sz, dx, dy, dz, gx, gy, gz);
    };
    for (int32_t g = lane; g < G; g += 64) next[g] = 0;
    __syncthreads();
    for (int32_t j = lane; j < members; j += 64) {                         // pass A
        const int32_t row = mine[j];
        if (row >= 0 && row < n) atomicAdd(&next[voxel_of(row)], 1);       // (always: no row is read outside the batch)
    }
    __syncthreads();
    for (int32_t g = lane; g < G; g += 64) out_count[q * G + g] = next[g];
    // the exclusive scan: every lane its stretch of consecutive voxels, the stretches' sums scanned across the wave
    const int32_t per = (G + 63) / 64, a = lane * per < G ? lane * per : G, b = a + per < G ? a + per : G;
    int32_t sum = 0;
    for (int32_t g = a; g < b; ++g) sum += next[g];
    int32_t upto = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t v = __shfl_up(upto, d);
        if (lane >= d) upto += v;
    }
    int32_t at = upto - sum;
    __syncthreads();                                                       // (the counts are read: they may be overwritten)
    for (int32_t g = a; g < b; ++g) {
        const int32_t c = next[g];
        next[g] = at;
        at += c;
    }
    __syncthreads();
    for (int32_t g = lane; g < G; g += 64) offset[q * G + g] = next[g];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int32_t base = 0; base < members; base += 64) {                   // pass B (members is the wave's: a uniform loop)
        const int32_t j = base + lane;
        int32_t row = j < members ? mine[j] : -1;
        if (row >= n) row = -1;                                            // (never)
        const int32_t g = row >= 0 ? voxel_of(row) : -1;
        unsigned long long todo = __ballot(row >= 0);
        int32_t slot = -1;
        while (todo != 0ull) {
            const int first = __ffsll((long long)todo) - 1;
            const int32_t key = __shfl(g, first);
            const bool same = g == key;                                    // (key >= 0: lanes without a row are not among them)
            const unsigned long long group = __ballot(same);
            int32_t before = 0;
            if (lane == first) {                                           // (this lane alone touches the voxel's cursor)
                before = next[key];
                next[key] = before + (int32_t)__popcll(group);
            }
            before = __shfl(before, first);
            if (same) slot = before + (int32_t)__popcll(group & below);
            todo &= ~group;
        }
        if (slot >= 0 && slot < members) out[slot] = row;                  // (always for a lane with a row: pass A counted the same voxels)
    }
}

// the first min(count, T) rows of voxel v of roi q, or 0 of them
__device__ __forceinline__ int32_t roiaware_span(uint32_t v, uint32_t q, int32_t T, int32_t P, const int32_t *__restrict__ count, const int32_t *__restrict__ offset,
                                                 const int32_t *__restrict__ sorted, const int32_t **at)
{
    int32_t c = count[v];
    c = c < T ? c : T;
    if (c <= 0) return 0;
    const int32_t off = offset[v];
    if (off < 0 || off + c > P) return 0;                                  // (never: the offsets and counts of a roi end within its list)
    *at = sorted + (int64_t)q * P + off;
    return c;
}

// W = 1: one lane per (f, m, g, channel).  W = 4: one lane per four consecutive channels, loaded and stored as 16 bytes -- for Cf a multiple
// of 4 and 16-byte aligned features and outputs (the launcher decides); every channel goes through the same operations in the same order.
template <int W>
__global__ __launch_bounds__(SG_RA_BLOCK) void k_roiaware_pool(const float *__restrict__ features, int64_t n, int32_t G, int32_t Cf, int32_t T, int32_t P, int64_t total,
                                                               const int32_t *__restrict__ count, const int32_t *__restrict__ offset,
                                                               const int32_t *__restrict__ sorted, float *__restrict__ out_max, int32_t *__restrict__ out_argmax,
                                                               float *__restrict__ out_avg)
{
    const uint32_t t = blockIdx.x * SG_RA_BLOCK + threadIdx.x;             // (total <= 2^31 - 1: 32-bit divisions, a fraction of the 64-bit ones' cost)
    if ((int64_t)t * W >= total) return;
    const uint32_t per = (uint32_t)Cf / W, v = t / per, q = v / (uint32_t)G;
    const int32_t ch = (int32_t)(t - v * per) * W;
    const int32_t *at = nullptr;
    const int32_t c = roiaware_span(v, q, T, P, count, offset, sorted, &at);
    float best[W], sum[W], x[W];
    int32_t arg[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { best[k] = 0.0f; sum[k] = 0.0f; arg[k] = -1; }
    for (int32_t i = 0; i < c; ++i) {
        const int32_t row = at[i];
        if (row < 0 || row >= n) continue;                                 // (never)
        const float *p = features + (int64_t)row * Cf + ch;
        if (W == 4) {
            const float4 f = *reinterpret_cast<const float4 *>(p);
            x[0] = f.x; x[1 % W] = f.y; x[2 % W] = f.z; x[3 % W] = f.w;
        } else {
            x[0] = p[0];
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if ((arg[k] < 0 && x[k] == x[k]) || x[k] > best[k]) { best[k] = x[k]; arg[k] = row; }      // pcdet's loop: the first of equal maxima, never NaN
            sum[k] = sum[k] + x[k];
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        best[k] = arg[k] >= 0 ? best[k] : 0.0f;
        sum[k] = c > 0 ? __fdiv_rn(sum[k], (float)c) : 0.0f;
    }
    const int64_t e = (int64_t)t * W;
    if (W == 4) {
        if (out_max) *reinterpret_cast<float4 *>(out_max + e) = make_float4(best[0], best[1 % W], best[2 % W], best[3 % W]);
        if (out_argmax) *reinterpret_cast<int4 *>(out_argmax + e) = make_int4(arg[0], arg[1 % W], arg[2 % W], arg[3 % W]);
        if (out_avg) *reinterpret_cast<float4 *>(out_avg + e) = make_float4(sum[0], sum[1 % W], sum[2 % W], sum[3 % W]);
    } else {
        if (out_max) out_max[e] = best[0];
        if (out_argmax) out_argmax[e] = arg[0];
        if (out_avg) out_avg[e] = sum[0];
    }
}

// W = 1: one lane per (f, m, g, t).  W = 4: one lane per four consecutive elements of the flat index, stored as 16 bytes where all four
// exist -- for a 16-byte aligned output (the launcher decides); T need be no multiple of 4: the four may belong to two voxels.
template <int W>
__global__ __launch_bounds__(SG_RA_BLOCK) void k_roiaware_index(int64_t n, int32_t G, int32_t T, int32_t P, int64_t total, const int32_t *__restrict__ count,
                                                                const int32_t *__restrict__ offset, const int32_t *__restrict__ sorted, int32_t *__restrict__ out_index)
{
    const int64_t e0 = ((int64_t)blockIdx.x * SG_RA_BLOCK + threadIdx.x) * W;
    if (e0 >= total) return;
    int32_t row[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        row[k] = -1;
        if (e0 + k >= total) continue;
        const uint32_t t = (uint32_t)(e0 + k);                             // (as above)
        const uint32_t v = t / (uint32_t)T, q = v / (uint32_t)G;
        const int32_t i = (int32_t)(t - v * (uint32_t)T);
        const int32_t *at = nullptr;
        const int32_t c = roiaware_span(v, q, T, P, count, offset, sorted, &at);
        if (i < c) row[k] = at[i];
        if (row[k] >= n) row[k] = -1;                                      // (never)
    }
    if (W == 4 && e0 + 3 < total) {
        *reinterpret_cast<int4 *>(out_index + e0) = make_int4(row[0], row[1 % W], row[2 % W], row[3 % W]);
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k)
            if (e0 + k < total) out_index[e0 + k] = row[k];
    }
}

__global__ __launch_bounds__(SG_RA_BLOCK) void k_roiaware_blank(int64_t slots, int64_t voxels, int32_t *__restrict__ out_roi_count, int32_t *__restrict__ out_count)
{
    const int64_t t = (int64_t)blockIdx.x * SG_RA_BLOCK + threadIdx.x;
    if (t < slots) out_roi_count[t] = 0;
    if (t < voxels) out_count[t] = 0;
}

extern "C" int sg_launch_roiaware(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                                  int32_t n_rois, const void *rois, int32_t roi_features, const double *ew, const int32_t *grid, int32_t max_points, int32_t cap,
                                  const float *features, int32_t channels, const double *pose_in, SgBoxRec *rec, unsigned long long *table, int32_t *run_cnt,
                                  int32_t *list, int32_t *sorted, int32_t *offset, int32_t *out_roi_count, int32_t *out_count, int32_t *out_index, float *out_max,
                                  int32_t *out_argmax, float *out_avg, double *out_pose, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int32_t G = grid[0] * grid[1] * grid[2];
    const int64_t slots = (int64_t)n_frames * n_rois, voxels = slots * G;                      // (below 2^31: sg_check_roiaware_args)
    if (int e = sg_launch_roi_members(rows, dtype, n, max_frame, frame_off, n_frames, keep_in, n_rois, rois, roi_features, ew, cap, pose_in, rec, table, run_cnt, list,
                                      out_roi_count, out_pose, stream))
        return e;
    if (n > 0) {
        const int e = sg_by_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL(k_roiaware_bucket<T>, dim3((unsigned)slots), dim3(64), (size_t)G * sizeof(int32_t), st, (const T *)rows, n, (const T *)rois, roi_features,
                               ew[0], ew[1], ew[2], grid[0], grid[1], grid[2], cap, rec, out_roi_count, list, sorted, offset, out_count);
            SG_CHECK_LAUNCH();
            return 0;
        });
        if (e) return e;
    } else {
        hipLaunchKernelGGL(k_roiaware_blank, dim3((unsigned)((voxels + SG_RA_BLOCK - 1) / SG_RA_BLOCK)), dim3(SG_RA_BLOCK), 0, st, slots, voxels, out_roi_count, out_count);
        SG_CHECK_LAUNCH();
    }
    auto aligned = [](const void *p) { return ((uintptr_t)p & 15) == 0; };                    // (a null pointer counts: it is not written)
    const dim3 block(SG_RA_BLOCK);
    if (out_max || out_argmax || out_avg) {
        const int64_t total = voxels * channels;
        if (channels % 4 == 0 && aligned(features) && aligned(out_max) && aligned(out_argmax) && aligned(out_avg))
            hipLaunchKernelGGL(k_roiaware_pool<4>, dim3((unsigned)((total / 4 + SG_RA_BLOCK - 1) / SG_RA_BLOCK)), block, 0, st, features, n, G, channels, max_points, cap,
                               total, out_count, offset, sorted, out_max, out_argmax, out_avg);
        else
            hipLaunchKernelGGL(k_roiaware_pool<1>, dim3((unsigned)((total + SG_RA_BLOCK - 1) / SG_RA_BLOCK)), block, 0, st, features, n, G, channels, max_points, cap,
                               total, out_count, offset, sorted, out_max, out_argmax, out_avg);
        SG_CHECK_LAUNCH();
    }
    if (out_index) {
        const int64_t total = voxels * max_points;
        if (aligned(out_index))
            hipLaunchKernelGGL(k_roiaware_index<4>, dim3((unsigned)(((total + 3) / 4 + SG_RA_BLOCK - 1) / SG_RA_BLOCK)), block, 0, st, n, G, max_points, cap, total,
                               out_count, offset, sorted, out_index);
        else
            hipLaunchKernelGGL(k_roiaware_index<1>, dim3((unsigned)((total + SG_RA_BLOCK - 1) / SG_RA_BLOCK)), block, 0, st, n, G, max_points, cap, total, out_count,
                               offset, sorted, out_index);
        SG_CHECK_LAUNCH();
    }
    return 0;
}
