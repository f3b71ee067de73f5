// sg_rowkit.h -- what the row stages have in common (snowgpu_dror.hip, snowgpu_ball.hip, snowgpu_voxel.hip, snowgpu_nn.hip, snowgpu_box.hip,
// snowgpu_range.hip; through sg_kutil.h the snowfall kernels take sg_find_frame from here): the frame of a row, whether a row is present,
// one atomic per run of lanes with the same id, and the block-wide exclusive scan that turns counters into first positions.  Device code
// only, nothing of the beam code; every function is inlined into its kernel.  A new row stage starts from these.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// largest f with off[f] <= i (0 if there is none; the frame of row i where off[0] <= i < off[n_frames])
__device__ __forceinline__ int sg_find_frame(const int64_t *__restrict__ off, int n_frames, int64_t i)
{
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// row i of an n-row buffer belongs to the batch
__device__ __forceinline__ bool sg_row_in_batch(const int64_t *off, int n_frames, int64_t i, int64_t n)
{
    return i < n && i >= off[0] && i < off[n_frames];
}

// ... and is present: its keep byte (no mask: every row) is read only for a row of the batch
__device__ __forceinline__ bool sg_row_present(const int64_t *off, int n_frames, const uint8_t *keep_in, int64_t i, int64_t n)
{
    return sg_row_in_batch(off, n_frames, i, n) && (!keep_in || keep_in[i] != 0);
}

// Rows that follow one another in a sweep fall into the same cell, and atomics of one wave on one address queue behind one another in L2:
// a run of consecutive lanes with the same id is served by ONE atomic, made by its first lane.  *head = the run's first lane, *len = its
// lanes; the id is one word or the pair (a, b).  An id equal to the caller's sentinel ("files nowhere") forms runs like any other.
// Every lane of the wave must call this.
__device__ __forceinline__ void sg_lane_run(uint32_t a, uint32_t b, int lane, int *head, int *len)
{
    const uint32_t pa = __shfl_up(a, 1), pb = __shfl_up(b, 1);
    const unsigned long long heads = __ballot(lane == 0 || pa != a || pb != b);
    const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
    *head = 63 - __clzll((long long)(heads & upto));
    const unsigned long long after = heads & ~upto;
    *len = (after ? __ffsll((long long)after) - 1 : 64) - *head;
}
__device__ __forceinline__ void sg_lane_run(uint32_t id, int lane, int *head, int *len)
{
    sg_lane_run(id, 0u, lane, head, len);      // (the constant key costs nothing: its shuffle folds away)
}

// counter[id] += the lanes of the run, by the run's head; nothing for the run of `none`.  Every lane of the wave must call this.
__device__ __forceinline__ void sg_run_add(uint32_t *counter, uint32_t id, uint32_t none, int lane)
{
    int head, len;
    sg_lane_run(id, lane, &head, &len);
    if (id != none && lane == head) atomicAdd(&counter[id], (uint32_t)len);
}

// The same add hands out the run's positions, consecutive from the counter's old value: every lane gets its own (a lane of the run of
// `none` gets no position: its result means nothing).  Every lane of the wave must call this.
__device__ __forceinline__ uint32_t sg_run_claim(uint32_t *counter, uint32_t id, uint32_t none, int lane)
{
    int head, len;
    uint32_t *slot = &counter[id];      // (an address only for `none`: never touched)
    sg_lane_run(id, lane, &head, &len);
    uint32_t base = 0;
    if (id != none && lane == head) base = atomicAdd(slot, (uint32_t)len);
    return __shfl(base, head) + (uint32_t)(lane - head);
}

// out[j] = carry + in[0] + .. + in[j - 1] for j < m, BLOCK elements a trip with the running total carried from trip to trip; returns
// carry + the sum of all m.  in and out may be the same array.  The whole block (BLOCK threads) must call this.
template <int BLOCK, typename T, typename N>
__device__ __forceinline__ T sg_block_scan_excl(const T *in, T *out, N m, T carry)
{
    __shared__ T wave_sum[BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (N j0 = 0; j0 < m; j0 += BLOCK) {
        const N j = j0 + tid;
        const T v = j < m ? in[j] : (T)0;
        T incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const T up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        T before = 0, total = 0;
        for (int w = 0; w < BLOCK / 64; ++w) {
            const T s = wave_sum[w];
            before += w < wave ? s : (T)0;
            total += s;
        }
        if (j < m) out[j] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    return carry;
}
