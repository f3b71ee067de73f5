// snowgpu_voxel.hip -- point-to-voxel grouping of aligned batches (snowgpu_voxelize_device; definition: include/snowgpu.h, the cell and the
// table of open cells: sg_voxel.h).  Two memsets (the tables to "empty", the voxels to zero) and eleven kernels on one stream:
//   k_voxel_insert      every usable row into its frame's table (one insert per run of lanes with the same cell); its slot, per row
//   k_voxel_first       first[i] = row i is the smallest row of its cell -- it opens the cell -- and the firsts per 1024-row tile
//   k_voxel_tile_scan   one block: the exclusive scan of the tile counts over the batch
//   k_voxel_frame_cells one wave per frame: the firsts in front of the frame's first row, and m_f = min(cells of the frame, V)
//   k_voxel_offsets     one block: voxel_offsets = the exclusive scan of m_f
//   k_voxel_assign      every first row: its rank among the frame's firsts IS the voxel number v.  v < V: coords of the packed voxel, its
//                       row counter cleared, the packed index into the cell's slot; else the slot says "dropped"
//   k_voxel_count       every row: the packed voxel of its cell (voxel_of), one atomic on its row counter per run of lanes
//   k_voxel_span_scan   one block per frame: the counters become the voxels' first positions in the frame's slice of `order`
//   k_voxel_scatter     row indices into their voxel's span (the atomic that hands out the position turns the counter into the span's END)
//   k_voxel_gather      every row: its rank among the rows of its span (the rows with a smaller index, counted up to T); below T it is
//                       STORED: its C columns go to slot `rank` of the voxel
//   k_voxel_finish      every packed index below F V: num_points = min(rows of the span, T); beyond voxel_offsets[F]: coords -1, 0 points
// A span's ORDER depends on the arrival of atomics; what is read from it -- how many of its row indices are smaller than a given one --
// does not.  Every output element is a function of integer row indices: results are identical from run to run.
// The offsets search, the in-batch test, the runs of lanes (sg_lane_run, sg_run_add, sg_run_claim) and the three scans
// (sg_block_scan_excl) are sg_rowkit.h's.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sg_common.h"
#include "sg_voxel.h"
#include "sg_launch.h"
#include "sg_rowkit.h"

#define SG_VOX_BLOCK 256
#define SG_VOX_TILE 1024          /* rows per tile: four per thread */
#define SG_VOX_SCAN_BLOCK 1024

// The frame of row i (off[0] <= i < off[n_frames]) where the lanes of a wave hold consecutive rows: the frame of the wave's first row
// serves every lane in front of that frame's end.
__device__ __forceinline__ int vox_frame(const int64_t *__restrict__ off, int n_frames, int64_t i, int lane)
{
    const int f0 = sg_find_frame(off, n_frames, i - lane);
    return i < off[f0 + 1] && i >= off[f0] ? f0 : sg_find_frame(off, n_frames, i);
}

// slot_of[i] = the slot of row i's cell in its frame's table, SG_VOXEL_NONE for a row that is not usable
template <typename T>
__global__ __launch_bounds__(SG_VOX_BLOCK) void k_voxel_insert(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                              const uint8_t *__restrict__ keep_in, SgVoxelGrid g, unsigned long long *__restrict__ table,
                                                              uint32_t *__restrict__ slot_of)
{
    const int64_t i = (int64_t)blockIdx.x * SG_VOX_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t key = SG_VOXEL_NONE, f = 0;
    if (sg_row_present(frame_off, n_frames, keep_in, i, n)) {
        const T *row = rows + i * 5;
        key = sg_voxel_key(g, (double)row[0], (double)row[1], (double)row[2]);
        if (key != SG_VOXEL_NONE) f = (uint32_t)vox_frame(frame_off, n_frames, i, lane);
    }
    int head, len;
    sg_lane_run(key, f, lane, &head, &len);
    uint32_t slot = SG_VOXEL_NONE;
    if (lane == head && key != SG_VOXEL_NONE)          // the run's first lane holds its smallest row
        slot = sg_voxel_insert(table + (int64_t)f * g.cap, g.cap, g.shift, key, (uint32_t)i);
    slot = __shfl(slot, head);
    if (i < n) slot_of[i] = slot;
}

// the low word of row i's slot: the first row of the cell (after k_voxel_insert), the packed voxel or SG_VOXEL_NONE (after k_voxel_assign)
__device__ __forceinline__ uint32_t vox_slot_low(const unsigned long long *__restrict__ table, uint32_t cap, int f, uint32_t slot)
{
    return (uint32_t)table[(int64_t)f * cap + slot];
}

__global__ __launch_bounds__(SG_VOX_BLOCK) void k_voxel_first(int64_t n, const int64_t *__restrict__ frame_off, int n_frames, const uint32_t *__restrict__ slot_of,
                                                             const unsigned long long *__restrict__ table, uint32_t cap, uint8_t *__restrict__ first,
                                                             int32_t *__restrict__ tile_cnt)
{
    const int lane = threadIdx.x & 63;
    int c = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = (int64_t)blockIdx.x * SG_VOX_TILE + q * SG_VOX_BLOCK + threadIdx.x;
        if (i >= n) continue;
        const uint32_t slot = slot_of[i];
        bool is_first = false;
        if (slot != SG_VOXEL_NONE) is_first = vox_slot_low(table, cap, vox_frame(frame_off, n_frames, i, lane), slot) == (uint32_t)i;
        first[i] = is_first ? 1 : 0;
        c += is_first ? 1 : 0;
    }
    __shared__ int s[4];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if (lane == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s[0] + s[1] + s[2] + s[3];
}

// tile_base[t] = the firsts in the tiles in front of tile t, t = 0 .. n_tiles (the last: all of them)
__global__ __launch_bounds__(SG_VOX_SCAN_BLOCK) void k_voxel_tile_scan(const int32_t *__restrict__ tile_cnt, int64_t n_tiles, int32_t *__restrict__ tile_base)
{
    const int32_t all = sg_block_scan_excl<SG_VOX_SCAN_BLOCK>(tile_cnt, tile_base, n_tiles, (int32_t)0);
    if (threadIdx.x == 0) tile_base[n_tiles] = all;
}

// the firsts among the rows [0, x) of the batch, 0 <= x <= n; the whole wave calls it and every lane gets the sum
__device__ __forceinline__ int32_t vox_firsts_before(const int32_t *__restrict__ tile_base, const uint8_t *__restrict__ first, int64_t x, int lane)
{
    const int64_t tile = x / SG_VOX_TILE;
    int32_t c = 0;
    for (int64_t j = tile * SG_VOX_TILE + lane; j < x; j += 64) c += first[j];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    return tile_base[tile] + c;
}

// fbase[f] = the firsts in front of frame f; m[f] = min(cells of frame f, V)
__global__ __launch_bounds__(64) void k_voxel_frame_cells(int64_t n, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ tile_base,
                                                          const uint8_t *__restrict__ first, int32_t max_voxels, int32_t *__restrict__ fbase,
                                                          int32_t *__restrict__ m)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int64_t a = std::min<int64_t>(std::max<int64_t>(frame_off[f], 0), n), b = std::min<int64_t>(std::max<int64_t>(frame_off[f + 1], a), n);
    const int32_t before = vox_firsts_before(tile_base, first, a, lane), upto = vox_firsts_before(tile_base, first, b, lane);
    if (lane == 0) {
        fbase[f] = before;
        m[f] = std::min<int32_t>(upto - before, max_voxels);
    }
}

// voxel_offsets[0 .. n_frames]: the exclusive scan of m.  ONE block, which walks the frames 256 at a time and carries the running total
// (F V <= 2^31 - 1 by the entry's domain: the sums fit).
__global__ __launch_bounds__(256) void k_voxel_offsets(const int32_t *__restrict__ m, int n_frames, int32_t *__restrict__ voxel_offsets)
{
    const int32_t all = sg_block_scan_excl<256>(m, voxel_offsets, n_frames, (int32_t)0);
    if (threadIdx.x == 0) voxel_offsets[n_frames] = all;
}

// Every first row: v = its rank among the firsts of its frame, in row order.  The low word of its cell's slot becomes the packed voxel
// voxel_offsets[f] + v, or SG_VOXEL_NONE for a dropped cell (v >= V): only the first row of a cell writes the cell's slot.
__global__ __launch_bounds__(SG_VOX_BLOCK) void k_voxel_assign(int64_t n, const int64_t *__restrict__ frame_off, int n_frames, const uint32_t *__restrict__ slot_of,
                                                              const uint8_t *__restrict__ first, const int32_t *__restrict__ tile_base,
                                                              const int32_t *__restrict__ fbase, const int32_t *__restrict__ voxel_offsets, SgVoxelGrid g,
                                                              unsigned long long *__restrict__ table, int32_t *__restrict__ out_coords, uint32_t *__restrict__ span)
{
    __shared__ int s_cnt[16];      // firsts per (quarter of the tile, wave)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    bool is_first[4];
    int in_wave[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = (int64_t)blockIdx.x * SG_VOX_TILE + q * SG_VOX_BLOCK + threadIdx.x;
        is_first[q] = i < n && first[i] != 0;
        const unsigned long long b = __ballot(is_first[q]);
        in_wave[q] = __popcll(b & below);
        if (lane == 0) s_cnt[q * 4 + wave] = __popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!is_first[q]) continue;
        const int64_t i = (int64_t)blockIdx.x * SG_VOX_TILE + q * SG_VOX_BLOCK + threadIdx.x;
        int before = in_wave[q];
        for (int k = 0; k < q * 4 + wave; ++k) before += s_cnt[k];
        const int f = sg_find_frame(frame_off, n_frames, i);
        const int32_t v = tile_base[blockIdx.x] + before - fbase[f];
        unsigned long long *slot = table + (int64_t)f * g.cap + slot_of[i];
        const uint32_t key = (uint32_t)(*slot >> 32);
        uint32_t packed = SG_VOXEL_NONE;
        if (v < g.max_voxels) {
            packed = (uint32_t)(voxel_offsets[f] + v);
            int32_t cx, cy, cz;
            sg_voxel_unkey(g, key, &cx, &cy, &cz);
            int32_t *c = out_coords + (int64_t)packed * 4;
            c[0] = f; c[1] = cz; c[2] = cy; c[3] = cx;
            span[packed] = 0;
        }
        *slot = ((unsigned long long)key << 32) | packed;
    }
}

// vox[i] = the packed voxel of row i's cell, or -1 (vox may be slot_of itself: a row reads its own element, then writes it)
__global__ __launch_bounds__(SG_VOX_BLOCK) void k_voxel_count(int64_t n, const int64_t *__restrict__ frame_off, int n_frames, const uint32_t *slot_of,
                                                             const unsigned long long *__restrict__ table, uint32_t cap, uint32_t *vox,
                                                             int32_t *__restrict__ out_voxel_of, uint32_t *__restrict__ span)
{
    const int64_t i = (int64_t)blockIdx.x * SG_VOX_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t v = SG_VOXEL_NONE;
    if (i < n) {
        const uint32_t slot = slot_of[i];
        if (slot != SG_VOXEL_NONE) v = vox_slot_low(table, cap, vox_frame(frame_off, n_frames, i, lane), slot);
    }
    sg_run_add(span, v, SG_VOXEL_NONE, lane);
    if (i < n) {
        vox[i] = v;
        if (out_voxel_of) out_voxel_of[i] = (int32_t)v;
    }
}

// span[voxel_offsets[f] + v] = frame_off[f] + the rows of the frame's voxels in front of v
__global__ __launch_bounds__(SG_VOX_SCAN_BLOCK) void k_voxel_span_scan(const int64_t *__restrict__ frame_off, const int32_t *__restrict__ voxel_offsets,
                                                                      uint32_t *__restrict__ span)
{
    const int f = blockIdx.x;
    uint32_t *e = span + voxel_offsets[f];
    sg_block_scan_excl<SG_VOX_SCAN_BLOCK>(e, e, voxel_offsets[f + 1] - voxel_offsets[f], (uint32_t)frame_off[f]);
}

// (a frame's voxels hold no more rows than the frame has: every position lies inside the frame's slice of `order`)
__global__ __launch_bounds__(SG_VOX_BLOCK) void k_voxel_scatter(int64_t n, const uint32_t *__restrict__ vox, uint32_t *__restrict__ span, uint32_t *__restrict__ order)
{
    const int64_t i = (int64_t)blockIdx.x * SG_VOX_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t v = i < n ? vox[i] : SG_VOXEL_NONE;
    const uint32_t pos = sg_run_claim(span, v, SG_VOXEL_NONE, lane);
    if (v == SG_VOXEL_NONE) return;
    if ((int64_t)pos < n) order[pos] = (uint32_t)i;
}

// the span of packed voxel v of frame f after the scatter: [*b, *e)
__device__ __forceinline__ void vox_span(const uint32_t *__restrict__ span, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ voxel_offsets, int f,
                                         uint32_t v, uint32_t *b, uint32_t *e)
{
    *b = v == (uint32_t)voxel_offsets[f] ? (uint32_t)frame_off[f] : span[v - 1];
    *e = span[v];
}

template <typename T>
__global__ __launch_bounds__(SG_VOX_BLOCK) void k_voxel_gather(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                              const uint32_t *__restrict__ vox, const uint32_t *__restrict__ span,
                                                              const uint32_t *__restrict__ order, const int32_t *__restrict__ voxel_offsets,
                                                              int32_t max_points, int32_t n_features, T *__restrict__ out_voxels)
{
    const int64_t i = (int64_t)blockIdx.x * SG_VOX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = vox[i];
    if (v == SG_VOXEL_NONE) return;
    uint32_t b, e;
    vox_span(span, frame_off, voxel_offsets, vox_frame(frame_off, n_frames, i, threadIdx.x & 63), v, &b, &e);
    if ((int64_t)e > n) e = (uint32_t)n;
    int32_t rank = 0;
    for (uint32_t p = b; p < e && rank < max_points; ++p) rank += order[p] < (uint32_t)i ? 1 : 0;
    if (rank >= max_points) return;                    // it belongs to the voxel and is not stored
    const T *row = rows + i * 5;
    T *dst = out_voxels + ((int64_t)v * max_points + rank) * n_features;
    for (int j = 0; j < n_features; ++j) dst[j] = row[j];
}

__global__ __launch_bounds__(SG_VOX_BLOCK) void k_voxel_finish(int64_t slots, const int64_t *__restrict__ frame_off, int n_frames, const uint32_t *__restrict__ span,
                                                              const int32_t *__restrict__ voxel_offsets, int32_t max_points, int32_t *__restrict__ out_coords,
                                                              int32_t *__restrict__ out_num_points)
{
    const int64_t v = (int64_t)blockIdx.x * SG_VOX_BLOCK + threadIdx.x;
    if (v >= slots) return;
    if (v >= voxel_offsets[n_frames]) {
        int32_t *c = out_coords + v * 4;
        c[0] = -1; c[1] = -1; c[2] = -1; c[3] = -1;
        out_num_points[v] = 0;
        return;
    }
    uint32_t b, e;
    vox_span(span, frame_off, voxel_offsets, out_coords[v * 4], (uint32_t)v, &b, &e);
    out_num_points[v] = (int32_t)std::min<uint32_t>(e - b, (uint32_t)max_points);
}

// The whole sequence on `stream`.  Scratch: table n_frames g->cap words of 64 bits; slot_of, order n words; first n bytes; tile_cnt
// ceil(n / 1024) and tile_base one more; fbase, m n_frames; span n_frames g->max_voxels words.
extern "C" int sg_launch_voxelize(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const SgVoxelGrid *g,
                                  unsigned long long *table, uint32_t *slot_of, uint8_t *first, uint32_t *order, int32_t *tile_cnt, int32_t *tile_base,
                                  int32_t *fbase, int32_t *m, uint32_t *span, void *out_voxels, int32_t *out_coords, int32_t *out_num_points,
                                  int32_t *out_voxel_offsets, int32_t *out_voxel_of, void *stream)
{
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t slots = (int64_t)n_frames * g->max_voxels;
    const size_t esz = dtype == 0 ? 4 : 8;
    hipError_t me = hipMemsetAsync(table, 0xff, sizeof(unsigned long long) * (size_t)n_frames * (size_t)g->cap, st);
    if (me != hipSuccess) return (int)me;
    me = hipMemsetAsync(out_voxels, 0, esz * (size_t)slots * (size_t)g->max_points * (size_t)g->n_features, st);
    if (me != hipSuccess) return (int)me;
    const unsigned blocks = (unsigned)((n + SG_VOX_BLOCK - 1) / SG_VOX_BLOCK);
    const int64_t n_tiles = (n + SG_VOX_TILE - 1) / SG_VOX_TILE;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_voxel_insert<T>, dim3(blocks), dim3(SG_VOX_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames, keep_in, *g, table, slot_of);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_first, dim3((unsigned)n_tiles), dim3(SG_VOX_BLOCK), 0, st, n, frame_off, n_frames, (const uint32_t *)slot_of,
                           (const unsigned long long *)table, g->cap, first, tile_cnt);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_tile_scan, dim3(1), dim3(SG_VOX_SCAN_BLOCK), 0, st, (const int32_t *)tile_cnt, n_tiles, tile_base);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_frame_cells, dim3(n_frames), dim3(64), 0, st, n, frame_off, (const int32_t *)tile_base, (const uint8_t *)first, g->max_voxels,
                           fbase, m);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_offsets, dim3(1), dim3(256), 0, st, (const int32_t *)m, n_frames, out_voxel_offsets);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_assign, dim3((unsigned)n_tiles), dim3(SG_VOX_BLOCK), 0, st, n, frame_off, n_frames, (const uint32_t *)slot_of,
                           (const uint8_t *)first, (const int32_t *)tile_base, (const int32_t *)fbase, (const int32_t *)out_voxel_offsets, *g, table, out_coords,
                           span);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_count, dim3(blocks), dim3(SG_VOX_BLOCK), 0, st, n, frame_off, n_frames, (const uint32_t *)slot_of,
                           (const unsigned long long *)table, g->cap, slot_of, out_voxel_of, span);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_span_scan, dim3(n_frames), dim3(SG_VOX_SCAN_BLOCK), 0, st, frame_off, (const int32_t *)out_voxel_offsets, span);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_scatter, dim3(blocks), dim3(SG_VOX_BLOCK), 0, st, n, (const uint32_t *)slot_of, span, order);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_gather<T>, dim3(blocks), dim3(SG_VOX_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames, (const uint32_t *)slot_of,
                           (const uint32_t *)span, (const uint32_t *)order, (const int32_t *)out_voxel_offsets, g->max_points, g->n_features, (T *)out_voxels);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_voxel_finish, dim3((unsigned)((slots + SG_VOX_BLOCK - 1) / SG_VOX_BLOCK)), dim3(SG_VOX_BLOCK), 0, st, slots, frame_off, n_frames,
                           (const uint32_t *)span, (const int32_t *)out_voxel_offsets, g->max_points, out_coords, out_num_points);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
