// snowgpu_dror.hip -- dynamic radius outlier removal as a producer of a keep mask (snowgpu_dror_mask_device; definition, grid and the
// argument for the window: sg_dror.h).  A fixed-radius neighbour count by cell lists, four kernels behind one memset, on one stream:
//   k_dror_count    every usable row: its cell (sg_dror_cell), kept per row, and one atomic on the cell's counter per run of lanes in it
//   k_dror_scan     one block per frame: the counters become the cells' first positions in the frame's slot of the sorted copy
//   k_dror_scatter  x, y, z of every usable row into its cell's span (the atomic that hands out the position turns the cell's entry into
//                   its END: cell c of a frame then spans [entry[c], entry[c + 1]), entry[0] the frame's first position)
//   k_dror_query    one thread per row: the spans of its window, the exact test, out as soon as k_min neighbours (and itself) are counted
// Counts are integers: neither the order of a span nor that of the walk changes a result.
// The frame of a row, the presence test, the atomic per run of lanes and the scan are sg_rowkit.h's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sg_common.h"
#include "sg_dror.h"
#include "sg_launch.h"
#include "sg_rowkit.h"

#define SG_DROR_BLOCK 256
#define SG_DROR_SCAN_BLOCK 1024

// cell_of[i] = the entry of row i's cell (frame f, cell c: f (cells + 1) + 1 + c), or SG_NO_CELL for a row that is not usable
template <typename T>
__global__ __launch_bounds__(SG_DROR_BLOCK) void k_dror_count(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                             const uint8_t *__restrict__ keep_in, SgDrorGrid g, uint32_t *__restrict__ entry,
                                                             uint32_t *__restrict__ cell_of)
{
    const int64_t i = (int64_t)blockIdx.x * SG_DROR_BLOCK + threadIdx.x;
    uint32_t e = SG_NO_CELL;
    if (sg_row_present(frame_off, n_frames, keep_in, i, n)) {
        const T *row = rows + i * 5;
        const double x = (double)row[0], y = (double)row[1], z = (double)row[2];
        if (sg_dror_usable(x, y, z)) {
            const int f = sg_find_frame(frame_off, n_frames, i);
            e = (uint32_t)((int64_t)f * (g.cells + 1) + 1 + sg_dror_cell(g, x, y));
        }
    }
    sg_run_add(entry, e, SG_NO_CELL, threadIdx.x & 63);
    if (i < n) cell_of[i] = e;
}

// entry[f (cells + 1)] = frame_off[f]; entry[.. + 1 + c] = frame_off[f] + the rows filed in the cells before c
__global__ __launch_bounds__(SG_DROR_SCAN_BLOCK) void k_dror_scan(const int64_t *__restrict__ frame_off, int32_t cells, uint32_t *__restrict__ entry)
{
    uint32_t *e = entry + (int64_t)blockIdx.x * (cells + 1);
    const uint32_t first = (uint32_t)frame_off[blockIdx.x];
    if (threadIdx.x == 0) e[0] = first;
    sg_block_scan_excl<SG_DROR_SCAN_BLOCK>(e + 1, e + 1, cells, first);
}

template <typename T>
__global__ __launch_bounds__(SG_DROR_BLOCK) void k_dror_scatter(const T *__restrict__ rows, int64_t n, const uint32_t *__restrict__ cell_of,
                                                               uint32_t *__restrict__ entry, T *__restrict__ sorted)
{
    const int64_t i = (int64_t)blockIdx.x * SG_DROR_BLOCK + threadIdx.x;
    const uint32_t e = i < n ? cell_of[i] : SG_NO_CELL;
    const uint32_t p = sg_run_claim(entry, e, SG_NO_CELL, threadIdx.x & 63);
    if (e == SG_NO_CELL) return;
    const T *row = rows + i * 5;
    T *dst = sorted + (int64_t)p * 3;     // (below the frame's end: a frame files no more rows than it has)
    dst[0] = row[0]; dst[1] = row[1]; dst[2] = row[2];
}

// the rows sorted[b .. e) against the query: counted up to `need`
template <typename T>
__device__ __forceinline__ int dror_walk(const T *__restrict__ sorted, uint32_t b, uint32_t e, double x, double y, double z, double s2, int cnt, int need)
{
    for (uint32_t p = b; p < e && cnt < need; ++p) {
        const T *s = sorted + (int64_t)p * 3;
        const double dx = (double)s[0] - x, dy = (double)s[1] - y, dz = (double)s[2] - z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        cnt += d2 <= s2 ? 1 : 0;
    }
    return cnt;
}

template <typename T>
__global__ __launch_bounds__(SG_DROR_BLOCK) void k_dror_query(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                             const uint32_t *__restrict__ cell_of, const uint32_t *__restrict__ entry,
                                                             const T *__restrict__ sorted, SgDrorGrid g, uint8_t *__restrict__ out_keep,
                                                             int32_t *__restrict__ out_nb)
{
    const int64_t i = (int64_t)blockIdx.x * SG_DROR_BLOCK + threadIdx.x;
    if (i >= n) return;
    int nb = 0;
    bool keep = false;
    const uint32_t own = cell_of[i];
    if (own != SG_NO_CELL) {                     // usable: present, finite and within the limit
        const T *row = rows + i * 5;
        const double x = (double)row[0], y = (double)row[1], z = (double)row[2];
        const double s2 = sg_dror_s2(g, x * x + y * y);
        const int need = g.k_min + 1;                  // the row itself is in its window and passes the test
        int cnt = 0;
        if (g.k_min == 0) cnt = 1;
        else {
            SgDrorWindow w;
            sg_dror_window(g, x, y, s2, &w);
            const uint32_t *e = entry + (int64_t)sg_find_frame(frame_off, n_frames, i) * (g.cells + 1);
            if (w.cart)
                for (int iy = w.iy0; iy <= w.iy1 && cnt < need; ++iy) {
                    const uint32_t *er = e + iy * g.cart_m;
                    cnt = dror_walk(sorted, er[w.ix0], er[w.ix1 + 1], x, y, z, s2, cnt, need);
                }
            if (w.polar)
                for (int ring = w.ring0; ring <= w.ring1 && cnt < need; ++ring) {
                    const uint32_t *er = e + g.cart_m * g.cart_m + ring * g.n_az;
                    const int end = w.az0 + w.n_az;
                    if (end <= g.n_az) cnt = dror_walk(sorted, er[w.az0], er[end], x, y, z, s2, cnt, need);
                    else {                             // over the seam: the bins up to the last, then the first ones
                        cnt = dror_walk(sorted, er[w.az0], er[g.n_az], x, y, z, s2, cnt, need);
                        cnt = dror_walk(sorted, er[0], er[end - g.n_az], x, y, z, s2, cnt, need);
                    }
                }
        }
        nb = cnt > 0 ? cnt - 1 : 0;
        keep = nb >= g.k_min;
    }
    out_keep[i] = keep ? 1 : 0;
    if (out_nb) out_nb[i] = nb;
}

// The whole sequence on `stream`.  entry: n_frames (g->cells + 1) words; cell_of: n words; sorted: 3 n values of the row dtype.
extern "C" int sg_launch_dror(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const SgDrorGrid *g,
                              uint32_t *entry, uint32_t *cell_of, void *sorted, uint8_t *out_keep, int32_t *out_nb, void *stream)
{
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipError_t me = hipMemsetAsync(entry, 0, sizeof(uint32_t) * (size_t)n_frames * (size_t)(g->cells + 1), st);
    if (me != hipSuccess) return (int)me;
    const unsigned blocks = (unsigned)((n + SG_DROR_BLOCK - 1) / SG_DROR_BLOCK);
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_dror_count<T>, dim3(blocks), dim3(SG_DROR_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames, keep_in, *g, entry, cell_of);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_dror_scan, dim3(n_frames), dim3(SG_DROR_SCAN_BLOCK), 0, st, frame_off, g->cells, entry);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_dror_scatter<T>, dim3(blocks), dim3(SG_DROR_BLOCK), 0, st, (const T *)rows, n, (const uint32_t *)cell_of, entry, (T *)sorted);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_dror_query<T>, dim3(blocks), dim3(SG_DROR_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames, (const uint32_t *)cell_of,
                           (const uint32_t *)entry, (const T *)sorted, *g, out_keep, out_nb);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
