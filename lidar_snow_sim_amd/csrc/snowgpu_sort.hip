// snowgpu_sort.hip -- channel sort and launch order of the snowfall-augmentation engine on gfx950, with their launch wrappers.
//
//   k_sort_*          stable counting sort of every frame's rows by channel                 (simulation.py:447)
//   k_gather_rows     the sorted copy for a caller-supplied permutation
//   k_seg_*           launch order of the first pass: (table, frame, channel) segments
//   k_expand_rows     compact input (x, y, z, intensity + channel byte) -> the rows every kernel reads
//   k_resolve_tables  table_ids[frame][channel] -> table descriptors
//
// The per-beam kernels that run in this order are in snowgpu_kernels.hip, the compaction of their results in snowgpu_compact.hip.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "sg_common.h"
#include "sg_kutil.h"
#include "sg_lean.h"
#include "sg_launch.h"

// ------------------------------------------------------------------------------------------------
// Stable counting sort by channel, per frame.  grid = (tiles per frame, frames), 256 threads, a tile
// is 1024 consecutive rows; wave w owns rows [256 w, 256 w + 256) of the tile in 4 rounds of 64 so
// that "earlier row" == "earlier (wave, round, lane)".
// STATS: the tile's rows are here anyway -- the per-tile statistics of the noise-threshold prepass (sg_lean.h; needs the ground plane,
// i.e. a plane that is known when the sort starts) ride along: one pass over the rows less per step (0.67 GB of 256 sweeps).
// Ranks: every lane finds the lanes of its wave that hold the same channel by eight ballots, one per bit of the channel byte -- the
// same cost whether the 64 rows are of one channel (a channel-major sweep) or of 64 (firing order: an STF .bin interleaves the
// channels, precompute.py:78).  A loop with one round per DISTINCT channel of the wave took 1.23 ms of a 256-sweep step on firing-order
// rows against 0.35 ms on channel-major ones (profiles/r05_C2fire_*).
// tile_unsorted: 1 if a row of this tile has a smaller channel than the row before it (k_sort_scan folds the tiles of a frame: a
// frame without such a row is channel-sorted as it stands, its permutation is the identity and nobody makes or reads a copy of it).
template <typename T, bool STATS>
__global__ __launch_bounds__(SG_BLOCK) void k_sort_hist(const T *__restrict__ rows, const int64_t *__restrict__ frame_off,
                                                        int32_t *__restrict__ tile_hist, uint16_t *__restrict__ rank,
                                                        uint8_t *__restrict__ ch8, int32_t *__restrict__ status, int64_t max_tiles, SgLeanTile lean,
                                                        int32_t *__restrict__ tile_unsorted)
{
    const int f = blockIdx.y;
    // status[1] ("first offending row", -1 = none: nobody writes it before the per-beam kernels) is set here, so that ONE fill clears the
    // status words of a batch instead of two (each fill is a launch on the chain of a small batch)
    if (blockIdx.x == 0 && f == 0 && threadIdx.x == 0) status[1] = -1;
    const int64_t base = frame_off[f], n = frame_off[f + 1] - base;
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    __shared__ volatile int cnt[4][256];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    for (int i = tid; i < 4 * 256; i += SG_BLOCK) ((volatile int *)cnt)[i] = 0;
    __syncthreads();
    int my_bucket[4], my_rank[4];
    [[maybe_unused]] T sx[4], sy[4], sz[4], si[4];
    [[maybe_unused]] bool sv[4];
    int descends = 0;
    // every load of the thread's four rows first (the rounds below are chains of ballots and LDS updates: a load inside one waits its turn)
    T sc[4], scp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + w * 256 + q * 64 + lane;
        const bool valid = r < n;
        const T *p = rows + (base + (valid ? r : 0)) * 5;
        if constexpr (STATS) { sx[q] = p[0]; sy[q] = p[1]; sz[q] = p[2]; si[q] = p[3]; sv[q] = valid; }
        sc[q] = p[4];
        scp[q] = (valid && lane == 0 && r > 0) ? p[-1] : (T)0;        // lane 0: the channel of the row before this round's first (earlier round, wave or tile)
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + w * 256 + q * 64 + lane;
        const bool valid = r < n;
        int bucket = -1;
        const T c_prev = scp[q];
        if (valid) {
            const T c = sc[q];
            const int ci = (int)c;
            if ((T)ci == c && ci >= 0 && ci < 256) bucket = ci;
            else { atomicCAS(&status[0], 0, 5 /* SNOWGPU_E_CHANNELS */); bucket = 255; }
        }
        {
            int before_b = __shfl_up(bucket, 1);
            if (lane == 0) before_b = r > 0 ? (int)c_prev : bucket;
            if (valid && bucket < before_b) descends = 1;
        }
        my_bucket[q] = bucket;
        my_rank[q] = 0;
        if (valid) ch8[base + r] = (uint8_t)bucket;     // the scatter pass reads 1 byte per row instead of the row again
        unsigned long long same = __ballot(valid);      // lanes of this wave with my channel
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (bucket >> bit) & 1;
            const unsigned long long bb = __ballot(set);
            same &= set ? bb : ~bb;
        }
        if (valid) {
            const int before = cnt[w][bucket];          // (a wave's LDS operations keep their order: every read precedes the leaders' writes)
            my_rank[q] = before + __popcll(same & sg_lanemask_lt());
            if ((same & sg_lanemask_lt()) == 0) cnt[w][bucket] = before + __popcll(same);
        }
    }
    const int any_descends = __syncthreads_or(descends);
    for (int q = 0; q < 4; ++q) {
        const int64_t r = tile0 + w * 256 + q * 64 + lane;
        if (r < n) {
            int off = my_rank[q];
            for (int ww = 0; ww < w; ++ww) off += cnt[ww][my_bucket[q]];
            rank[base + r] = (uint16_t)off;
        }
    }
    int32_t *h = tile_hist + ((int64_t)f * max_tiles + blockIdx.x) * 256;
    h[tid] = cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
    if (tid == 0) tile_unsorted[(int64_t)f * max_tiles + blockIdx.x] = any_descends ? 1 : 0;
    if constexpr (STATS) {
        __shared__ double sm[58];
        lean_tile_stats<T>(lean, f, blockIdx.x, sx, sy, sz, si, sv, sm);
    }
}

// One block per frame, thread v owns bucket v: tile_base[t][v] = (rows of smaller buckets) + (rows of
// bucket v in earlier tiles); frame_unsorted[f] = some tile of the frame saw a descending channel.
__global__ __launch_bounds__(SG_BLOCK) void k_sort_scan(const int64_t *__restrict__ frame_off,
                                                        const int32_t *__restrict__ tile_hist,
                                                        int32_t *__restrict__ tile_base, int64_t max_tiles,
                                                        const int32_t *__restrict__ tile_unsorted, int32_t *__restrict__ frame_unsorted)
{
    const int f = blockIdx.x, v = threadIdx.x;
    const int64_t n = frame_off[f + 1] - frame_off[f];
    const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
    const int32_t *h = tile_hist + (int64_t)f * max_tiles * 256;
    int32_t *b = tile_base + (int64_t)f * max_tiles * 256;
    int total = 0, uns = 0;
    for (int64_t t = v; t < tiles; t += SG_BLOCK) uns |= tile_unsorted[(int64_t)f * max_tiles + t];
#pragma unroll 8                                  // eight loads in flight: the loop is a chain of global-load latencies otherwise
    for (int64_t t = 0; t < tiles; ++t) total += h[t * 256 + v];
    __shared__ int s[256];
    s[v] = total;
    uns = __syncthreads_or(uns);
    if (v == 0) frame_unsorted[f] = uns ? 1 : 0;
    for (int d = 1; d < 256; d <<= 1) {          // Hillis-Steele inclusive scan over the 256 buckets
        int add = v >= d ? s[v - d] : 0;
        __syncthreads();
        s[v] += add;
        __syncthreads();
    }
    int run = s[v] - total;
#pragma unroll 8
    for (int64_t t = 0; t < tiles; ++t) { b[t * 256 + v] = run; run += h[t * 256 + v]; }
}

// Second pass of the sort, for the frames that need it (frame_unsorted[f]; a channel-sorted frame is read in place): the tile's rows
// go to their places in the SORTED COPY of the frame, and perm gets their source rows.  The tile is staged through LDS in sorted
// order first, so that the stores walk whole runs -- in firing order a tile holds 16 rows of each of 64 channels, i.e. 64 runs of
// 320 contiguous bytes -- instead of scattering 20-byte rows lane by lane.  The per-beam kernels and the compaction then read sorted
// position g as row g of the copy: no gather through perm anywhere (measured on firing-order rows before this: the scan 1.83 instead of
// 1.60 ms, the compaction's scatter 0.69 instead of 0.36 ms, this pass -- 4-byte stores scattered over 64 channel runs -- 0.32 ms).
// identity_perm: the debug tap wants the permutation of every frame, sorted ones too.
template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void k_sort_scatter(const T *__restrict__ rows, const uint8_t *__restrict__ ch8, const int64_t *__restrict__ frame_off,
                                                           const int32_t *__restrict__ tile_hist, const int32_t *__restrict__ tile_base,
                                                           const uint16_t *__restrict__ rank, int32_t *__restrict__ perm, T *__restrict__ srows,
                                                           const int32_t *__restrict__ frame_unsorted, int identity_perm, int64_t max_tiles)
{
    const int f = blockIdx.y;
    const int64_t base = frame_off[f], n = frame_off[f + 1] - base;
    const int64_t tile0 = (int64_t)blockIdx.x * SG_TILE;
    if (tile0 >= n) return;
    const int tid = threadIdx.x;
    if (!frame_unsorted[f]) {
        if (identity_perm)
            for (int q = 0; q < 4; ++q) { const int64_t r = tile0 + q * SG_BLOCK + tid; if (r < n) perm[base + r] = (int32_t)r; }
        return;
    }
    __shared__ T stage[SG_TILE * 5];
    __shared__ int s_dest[SG_TILE];
    __shared__ uint16_t s_src[SG_TILE];
    __shared__ int s_start[256];
    const int32_t *b = tile_base + ((int64_t)f * max_tiles + blockIdx.x) * 256;
    {   // where each channel's run starts inside the tile's sorted image: exclusive scan of the tile's histogram
        const int c = tile_hist[((int64_t)f * max_tiles + blockIdx.x) * 256 + tid];
        s_start[tid] = c;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int add = tid >= d ? s_start[tid - d] : 0;
            __syncthreads();
            s_start[tid] += add;
            __syncthreads();
        }
        const int excl = s_start[tid] - c;
        __syncthreads();
        s_start[tid] = excl;
        __syncthreads();
    }
    const int m = (int)(n - tile0 < SG_TILE ? n - tile0 : SG_TILE);      // rows of this tile
    for (int q = 0; q < 4; ++q) {
        const int i = q * SG_BLOCK + tid;
        if (i < m) {
            const int64_t r = tile0 + i;
            const int ch = ch8[base + r], rk = rank[base + r];
            const int sp = s_start[ch] + rk;                                 // position in the tile's sorted image
            const T *p = rows + (base + r) * 5;
            const T v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3], v4 = p[4];
            T *d = stage + sp * 5;
            d[0] = v0; d[1] = v1; d[2] = v2; d[3] = v3; d[4] = v4;
            s_dest[sp] = b[ch] + rk;                                         // frame-local sorted position
            s_src[sp] = (uint16_t)i;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < m * 5; idx += SG_BLOCK) {
        const int sp = idx / 5, j = idx - sp * 5;
        srows[(base + s_dest[sp]) * 5 + j] = stage[idx];
    }
    for (int sp = tid; sp < m; sp += SG_BLOCK) perm[base + s_dest[sp]] = (int32_t)(tile0 + s_src[sp]);
}

// The sorted copy for a caller-supplied permutation (no device sort): a plain gather; every frame counts as unsorted.
template <typename T>
__global__ __launch_bounds__(SG_BLOCK) void k_gather_rows(const T *__restrict__ rows, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ perm,
                                                          T *__restrict__ srows, int32_t *__restrict__ frame_unsorted, int32_t *__restrict__ status)
{
    const int f = blockIdx.y;
    const int64_t base = frame_off[f], n = frame_off[f + 1] - base;
    if (blockIdx.x == 0 && threadIdx.x == 0) frame_unsorted[f] = 1;
    if (blockIdx.x == 0 && f == 0 && threadIdx.x == 0) status[1] = -1;       // (see k_sort_hist)
    for (int64_t r = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x; r < n; r += (int64_t)gridDim.x * SG_BLOCK) {
        const T *p = rows + (base + perm[base + r]) * 5;
        T *d = srows + (base + r) * 5;
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2]; d[3] = p[3]; d[4] = p[4];
    }
}

// ------------------------------------------------------------------------------------------------
// Segment order of the first pass.  A segment = the rows of one (frame, channel) pair in the channel-sorted order,
// i.e. all beams of a frame that look up the same flake table.  Segments are ordered by table, so that the ~1000
// blocks resident at any moment use one or two tables (2-3 MB each: L2-resident) instead of all 64 of a frame.
// Three small kernels over the n_frames * 256 pairs: count segments and blocks per table (one packed 64-bit atomic
// per pair: segments << 32 | blocks), exclusive scan over the tables, place every pair (a second packed atomic gives
// its segment slot and its first block inside the table's range).  The order inside a table is whatever the atomics
// give -- results do not depend on the launch order.
struct SgPair { int64_t start; int rows; int key; };

__device__ __forceinline__ SgPair sg_pair(int p, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ tile_base, int64_t max_tiles,
                                          const int32_t *__restrict__ table_ids, int n_las, int n_tables)
{
    SgPair r;
    const int f = p >> 8, c = p & 255;
    const int64_t n = frame_off[f + 1] - frame_off[f];
    r.start = frame_off[f]; r.rows = 0; r.key = n_tables;
    if (n <= 0) return r;                             // the sort wrote nothing for an empty frame
    const int32_t *b = tile_base + (int64_t)f * max_tiles * 256;
    const int64_t s0 = b[c], s1 = c < 255 ? (int64_t)b[c + 1] : n;
    r.start += s0;
    r.rows = (int)(s1 - s0);
    if (c < n_las) {
        const int id = table_ids[(int64_t)f * n_las + c];
        if (id >= 0 && id < n_tables) r.key = id;     // unknown ids and channels without a laser go last
    }
    return r;
}

__global__ __launch_bounds__(256) void k_seg_count(const int64_t *__restrict__ frame_off, int n_frames, const int32_t *__restrict__ tile_base,
                                                   int64_t max_tiles, const int32_t *__restrict__ table_ids, int n_las, int n_tables, int blk,
                                                   unsigned long long *__restrict__ tbl_cnt, const SgTable *__restrict__ tables,
                                                   SgTable *__restrict__ resolved)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_frames * 256) return;
    if (resolved && (p & 255) < n_las) {              // table descriptor of (frame, channel): what k_resolve_tables does, one launch less
        const int64_t i = (int64_t)(p >> 8) * n_las + (p & 255);
        const int t = table_ids[i];
        SgTable d{};
        if (t >= 0 && t < n_tables) d = tables[t];
        resolved[i] = d;
    }
    const SgPair r = sg_pair(p, frame_off, tile_base, max_tiles, table_ids, n_las, n_tables);
    if (r.rows > 0) atomicAdd(&tbl_cnt[(size_t)r.key * SG_TBL_STRIDE], (1ull << 32) | (unsigned long long)((r.rows + blk - 1) / blk));
}

// exclusive scan of the packed per-table counts (both halves at once: neither overflows 32 bits); leaves the counts zero
// so that k_seg_place can use them as cursors
__global__ __launch_bounds__(1024) void k_seg_scan(unsigned long long *__restrict__ tbl_cnt, unsigned long long *__restrict__ tbl_base, int n,
                                                   int32_t *__restrict__ seg_n, int32_t *__restrict__ one_chunk_blk)
{
    __shared__ unsigned long long sc[1024];
    const int t = threadIdx.x;
    const int per = (n + 1023) / 1024, b0 = t * per, b1 = b0 + per < n ? b0 + per : n;
    unsigned long long sum = 0;
    for (int k = b0; k < b1; ++k) sum += tbl_cnt[(size_t)k * SG_TBL_STRIDE];
    sc[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { const unsigned long long add = t >= d ? sc[t - d] : 0; __syncthreads(); sc[t] += add; __syncthreads(); }
    unsigned long long run = sc[t] - sum;
    for (int k = b0; k < b1; ++k) { const unsigned long long c = tbl_cnt[(size_t)k * SG_TBL_STRIDE]; tbl_base[k] = run; run += c; tbl_cnt[(size_t)k * SG_TBL_STRIDE] = 0; }
    if (t == 1023) {
        seg_n[0] = (int32_t)(sc[1023] >> 32); seg_n[1] = (int32_t)(sc[1023] & 0xffffffffull);
        if (one_chunk_blk) { one_chunk_blk[0] = 0; one_chunk_blk[1] = (int32_t)(sc[1023] & 0xffffffffull); }   // the pass as ONE launch: all blocks
    }
}

__global__ __launch_bounds__(256) void k_seg_place(const int64_t *__restrict__ frame_off, int n_frames, const int32_t *__restrict__ tile_base,
                                                   int64_t max_tiles, const int32_t *__restrict__ table_ids, int n_las, int n_tables, int blk,
                                                   const unsigned long long *__restrict__ tbl_base, unsigned long long *__restrict__ tbl_cur,
                                                   int64_t *__restrict__ seg_start, int32_t *__restrict__ seg_cnt, int32_t *__restrict__ seg_frame,
                                                   int32_t *__restrict__ seg_blk, int32_t *__restrict__ seg_of_blk)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_frames * 256) return;
    const SgPair r = sg_pair(p, frame_off, tile_base, max_tiles, table_ids, n_las, n_tables);
    if (r.rows <= 0) return;
    const int nb = (r.rows + blk - 1) / blk;
    const unsigned long long c = atomicAdd(&tbl_cur[(size_t)r.key * SG_TBL_STRIDE], (1ull << 32) | (unsigned long long)nb), base = tbl_base[r.key];
    const int slot = (int)(base >> 32) + (int)(c >> 32);
    const int b0 = (int)(base & 0xffffffffull) + (int)(c & 0xffffffffull);
    seg_start[slot] = r.start; seg_cnt[slot] = r.rows; seg_frame[slot] = (p >> 8) | ((p & 255) << 22); seg_blk[slot] = b0;
    for (int q = 0; q < nb; ++q) {                               // block -> what k_beams needs of its segment: one round trip per block there
        int32_t *br = seg_of_blk + (int64_t)(b0 + q) * SG_BLKREC;
        br[0] = slot; br[1] = (int32_t)r.start; br[2] = r.rows; br[3] = (p >> 8) | ((p & 255) << 22); br[4] = b0;
    }
}

// The three kernels above as ONE block for batches of up to four frames (1024 (frame, channel) pairs) and up to SG_SEG_SMALL_TABLES
// tables: per-table counts, their scan and the placement through LDS, and on the way the fill that clears everything the step counts up
// from zero (`zero`, n_zero 64-bit words).  A small batch is bound by its chain of dependent launches: this is one link instead of five
// (fill, three kernels, fill) and it runs on the caller's stream, so the scan needs no hop to a side stream and back (55 us between the
// end of the sort and the start of the scan in a single sweep's trace, ~10 us now).  Same segments as the three kernels build (the order
// inside a table is whatever the atomics give, there as here).
#define SG_SEG_SMALL_TABLES 4096
__global__ __launch_bounds__(1024) void k_seg_small(const int64_t *__restrict__ frame_off, int n_frames, const int32_t *__restrict__ tile_base,
                                                    int64_t max_tiles, const int32_t *__restrict__ table_ids, int n_las, int n_tables, int blk,
                                                    int64_t *__restrict__ seg_start, int32_t *__restrict__ seg_cnt, int32_t *__restrict__ seg_frame,
                                                    int32_t *__restrict__ seg_blk, int32_t *__restrict__ seg_of_blk, int32_t *__restrict__ seg_n,
                                                    int32_t *__restrict__ one_chunk_blk, const SgTable *__restrict__ tables, SgTable *__restrict__ resolved,
                                                    unsigned long long *__restrict__ zero, int64_t n_zero)
{
    __shared__ unsigned long long cnt[SG_SEG_SMALL_TABLES + 1], sc[1024];
    const int t = threadIdx.x, p = t;
    for (int64_t i = t; i < n_zero; i += 1024) zero[i] = 0ull;
    for (int i = t; i <= n_tables; i += 1024) cnt[i] = 0ull;
    __syncthreads();
    const bool mine = p < n_frames * 256;
    SgPair r{};
    int nb = 0;
    if (mine) {
        if ((p & 255) < n_las) {                      // table descriptor of (frame, channel)
            const int64_t i = (int64_t)(p >> 8) * n_las + (p & 255);
            const int id = table_ids[i];
            SgTable d{};
            if (id >= 0 && id < n_tables) d = tables[id];
            resolved[i] = d;
        }
        r = sg_pair(p, frame_off, tile_base, max_tiles, table_ids, n_las, n_tables);
        nb = (r.rows + blk - 1) / blk;
        if (r.rows > 0) atomicAdd(&cnt[r.key], (1ull << 32) | (unsigned long long)nb);
    }
    __syncthreads();
    // exclusive scan of the packed per-table counts (segments << 32 | blocks)
    const int n = n_tables + 1, per = (n + 1023) / 1024, b0 = t * per, b1 = b0 + per < n ? b0 + per : n;
    unsigned long long sum = 0;
    for (int k = b0; k < b1; ++k) sum += cnt[k];
    sc[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { const unsigned long long add = t >= d ? sc[t - d] : 0; __syncthreads(); sc[t] += add; __syncthreads(); }
    unsigned long long run = sc[t] - sum;
    for (int k = b0; k < b1; ++k) { const unsigned long long c = cnt[k]; cnt[k] = run; run += c; }     // cnt: now the table's base, bumped below as its cursor
    if (t == 1023) {
        seg_n[0] = (int32_t)(sc[1023] >> 32); seg_n[1] = (int32_t)(sc[1023] & 0xffffffffull);
        one_chunk_blk[0] = 0; one_chunk_blk[1] = (int32_t)(sc[1023] & 0xffffffffull);
    }
    __syncthreads();
    if (mine && r.rows > 0) {
        const unsigned long long c = atomicAdd(&cnt[r.key], (1ull << 32) | (unsigned long long)nb);
        const int slot = (int)(c >> 32), bb = (int)(c & 0xffffffffull);
        seg_start[slot] = r.start; seg_cnt[slot] = r.rows; seg_frame[slot] = (p >> 8) | ((p & 255) << 22); seg_blk[slot] = bb;
        for (int q = 0; q < nb; ++q) {
            int32_t *br = seg_of_blk + (int64_t)(bb + q) * SG_BLKREC;
            br[0] = slot; br[1] = (int32_t)r.start; br[2] = r.rows; br[3] = (p >> 8) | ((p & 255) << 22); br[4] = bb;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Compact input (snowgpu_augment_batch_compact): rows that crossed the link as (x, y, z, intensity) float32 + one channel BYTE -- 17 bytes
// per point instead of the STF row's 20 (precompute.py:78 keeps the channel as a fifth float32) -- become the (x, y, z, intensity,
// channel) rows every kernel reads.  One thread per row; the batch's only pass that exists for the link's sake (0.67 GB written per
// 256 sweeps, spread over the chunks of the pipeline).
__global__ __launch_bounds__(256) void k_expand_rows(const float4 *__restrict__ xyzi, const uint8_t *__restrict__ ch, float *__restrict__ rows, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 v = xyzi[i];
    float *r = rows + i * 5;
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; r[4] = (float)ch[i];
}


// table_ids[frame][channel] -> the table descriptor itself, so that a beam needs one load instead of two dependent ones
__global__ void k_resolve_tables(const SgTable *__restrict__ tables, int n_tables, const int32_t *__restrict__ table_ids,
                                 int64_t n, SgTable *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = table_ids[i];
    SgTable d{};
    if (t >= 0 && t < n_tables) d = tables[t];
    out[i] = d;
}

// ------------------------------------------------------------------------------------------------
// launch wrappers (C linkage, called from snowgpu_batch.cpp and snowgpu_host.cpp)

extern "C" int sg_launch_expand_rows(const void *xyzi, const uint8_t *ch, void *rows, int64_t n, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_expand_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4 *)xyzi, ch, (float *)rows, n);
    SG_CHECK_LAUNCH();
    return 0;
}

extern "C" int sg_launch_resolve_tables(const SgTable *tables, int n_tables, const int32_t *table_ids, int64_t n, SgTable *out,
                                        void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_resolve_tables, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tables, n_tables,
                       table_ids, n, out);
    SG_CHECK_LAUNCH();
    return 0;
}

// lean_plane / lean_part: optional -- the ground planes (n_frames x 4) and the tile-partials buffer of the noise-threshold prepass
// (sg_prepass_reserve_tiles): the first kernel then leaves the prepass' per-tile statistics on its way over the rows
extern "C" int sg_launch_sort(const void *rows, int dtype, const int64_t *frame_off, int n_frames, int64_t n_total,
                              int32_t *tile_hist, int32_t *tile_base, uint16_t *rank, uint8_t *ch8, int32_t *perm, int32_t *status,
                              int64_t max_tiles, const double *lean_plane, double *lean_part, int32_t *tile_unsorted, int32_t *frame_unsorted,
                              void *srows, int identity_perm, int phase /* 1: histogram + scan; 2: scatter; 3: both */, void *stream)
{
    (void)n_total;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)max_tiles, (unsigned)n_frames);
    SgLeanTile lt{};
    lt.plane = lean_plane; lt.delta = 0.5; lt.part = lean_part; lt.max_tiles = max_tiles;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (phase & 1) {
            if (lean_plane && lean_part) hipLaunchKernelGGL((k_sort_hist<T, true>), grid, dim3(SG_BLOCK), 0, st, (const T *)rows, frame_off, tile_hist, rank, ch8, status, max_tiles, lt, tile_unsorted);
            else hipLaunchKernelGGL((k_sort_hist<T, false>), grid, dim3(SG_BLOCK), 0, st, (const T *)rows, frame_off, tile_hist, rank, ch8, status, max_tiles, lt, tile_unsorted);
            SG_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_sort_scan, dim3(n_frames), dim3(SG_BLOCK), 0, st, frame_off, tile_hist, tile_base, max_tiles, tile_unsorted, frame_unsorted);
            SG_CHECK_LAUNCH();
        }
        if (phase & 2) {
            hipLaunchKernelGGL(k_sort_scatter<T>, grid, dim3(SG_BLOCK), 0, st, (const T *)rows, ch8, frame_off, tile_hist, tile_base, rank, perm, (T *)srows, frame_unsorted, identity_perm, max_tiles);
            SG_CHECK_LAUNCH();
        }
        return 0;
    });
}

extern "C" int sg_launch_gather_rows(const void *rows, int dtype, const int64_t *frame_off, int n_frames, int64_t n_total, int64_t max_frame,
                                     const int32_t *perm, void *srows, int32_t *frame_unsorted, int32_t *status, void *stream)
{
    (void)n_total;
    if (n_frames <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((max_frame + SG_BLOCK - 1) / SG_BLOCK, 256)), (unsigned)n_frames);
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_gather_rows<T>, grid, dim3(SG_BLOCK), 0, st, (const T *)rows, frame_off, perm, (T *)srows, frame_unsorted, status);
        SG_CHECK_LAUNCH();
        return 0;
    });
}

// the same for a small batch (see k_seg_small); returns -1 if the batch is not small (nothing launched)
extern "C" int sg_launch_segments_small(const int64_t *frame_off, int n_frames, const int32_t *tile_base, int64_t max_tiles, const int32_t *table_ids,
                                        int n_las, int n_tables, int block, int32_t *seg_blk, int64_t *seg_start, int32_t *seg_cnt, int32_t *seg_frame,
                                        int32_t *seg_n, int32_t *seg_of_blk, int32_t *chunk_blk, const SgTable *tables, SgTable *resolved,
                                        unsigned long long *zero, int64_t n_zero, void *stream)
{
    if (n_frames * 256 > 1024 || n_tables + 1 > SG_SEG_SMALL_TABLES || n_zero > (1 << 16)) return -1;
    hipLaunchKernelGGL(k_seg_small, dim3(1), dim3(1024), 0, (hipStream_t)stream, frame_off, n_frames, tile_base, max_tiles, table_ids, n_las, n_tables, block,
                       seg_start, seg_cnt, seg_frame, seg_blk, seg_of_blk, seg_n, chunk_blk, tables, resolved, zero, n_zero);
    SG_CHECK_LAUNCH();
    return 0;
}

extern "C" int sg_launch_segments(const int64_t *frame_off, int n_frames, const int32_t *tile_base, int64_t max_tiles, const int32_t *table_ids,
                                  int n_las, int n_tables, int block, unsigned long long *tbl_cnt, unsigned long long *tbl_base, int32_t *seg_blk,
                                  int64_t *seg_start, int32_t *seg_cnt, int32_t *seg_frame, int32_t *seg_n, int32_t *seg_of_blk,
                                  int32_t *chunk_blk, const SgTable *tables, SgTable *resolved, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)n_frames;         // 256 pairs per frame, one thread each
    if (hipMemsetAsync(tbl_cnt, 0, sizeof(unsigned long long) * ((size_t)n_tables + 1) * SG_TBL_STRIDE, st) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(k_seg_count, dim3(grid), dim3(256), 0, st, frame_off, n_frames, tile_base, max_tiles, table_ids, n_las, n_tables, block, tbl_cnt,
                       tables, resolved);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(1024), 0, st, tbl_cnt, tbl_base, n_tables + 1, seg_n, chunk_blk);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_seg_place, dim3(grid), dim3(256), 0, st, frame_off, n_frames, tile_base, max_tiles, table_ids, n_las, n_tables, block,
                       tbl_base, tbl_cnt, seg_start, seg_cnt, seg_frame, seg_blk, seg_of_blk);
    SG_CHECK_LAUNCH();
    return 0;
}
