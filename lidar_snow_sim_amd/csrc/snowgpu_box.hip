// snowgpu_box.hip -- points in 3D boxes (snowgpu_points_in_boxes_device; definition: include/snowgpu.h; presence, the record, the
// membership test, the grid, the footprint and the scratch sizes: sg_box.h).  The B boxes of a frame are filed, not its rows; two
// kernels on one stream, no memset:
//   k_box_file   one workgroup per frame: every box decided present or absent and its pose taken or computed, one record per box, the
//                pose and the zeroed counts written, the frame's bit table cleared by the workgroup itself and then every present box
//                marked by atomicOr in every cell its footprint can touch -- box after box, the lanes over the cells of its rectangle,
//                so a box that covers the whole frame costs 16 steps -- and in the frame's word of present boxes.
//   k_box_rows   one LANE per row: the presence test and the frame by the offsets search (both sg_rowkit.h's), the usable test, the words
//                of the row's cell, and for every set bit ascending the membership test from the box record.
//                The first hit is box_of and gives the local coordinates; every hit
//                counts.  The loop over candidates is uniform across the wave, so equal boxes are folded by ballot before one lane adds
//                their number to the count: rows of one object are neighbours in the sensor's order, and 64 adds become one.
// The counts are integer sums and the marks are ORs: the result depends on no arrival order.
// -DSG_BOX_BRUTE=1 (scripts/build_variant.sh, the A/B of DESIGN.md section 9): no grid; every row tests every present box of its frame.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_box.h"
#include "sg_common.h"
#include "sg_launch.h"
#include "sg_rowkit.h"

#define SG_BOX_BLOCK 256

template <typename T>
__global__ __launch_bounds__(SG_BOX_BLOCK) void k_box_file(const T *__restrict__ boxes, int32_t B, int32_t Cb, const double *__restrict__ pose_in,
                                                           SgBoxRec *__restrict__ rec, unsigned long long *__restrict__ table,
                                                           int32_t *__restrict__ out_count, double *__restrict__ out_pose)
{
    __shared__ int32_t rect[SG_BOX_MAX][4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int32_t W = sg_box_words(B);
    unsigned long long *tab = table + (int64_t)f * (SG_BOX_CELLS + 1) * W;
    bool present = false;
    if (tid < B) {                                                         // (B <= SG_BOX_MAX = the block)
        const int64_t q = (int64_t)f * B + tid;
        SgBoxRec r;
        present = sg_box_make<T>(boxes + q * Cb, pose_in ? pose_in + q * 2 : nullptr, &r);
        rec[q] = r;
        if (out_pose) { out_pose[q * 2] = r.c; out_pose[q * 2 + 1] = r.s; }
        if (out_count) out_count[q] = 0;
        int32_t ix0 = 1, ix1 = 0, iy0 = 1, iy1 = 0;                        // an absent box: no cell
        if (present) sg_box_footprint(r, &ix0, &ix1, &iy0, &iy1);
        rect[tid][0] = ix0; rect[tid][1] = ix1; rect[tid][2] = iy0; rect[tid][3] = iy1;
    }
#ifdef SG_BOX_BRUTE
    for (int32_t i = tid; i < W; i += SG_BOX_BLOCK) tab[(int64_t)SG_BOX_CELLS * W + i] = 0ull;
#else
    for (int32_t i = tid; i < (SG_BOX_CELLS + 1) * W; i += SG_BOX_BLOCK) tab[i] = 0ull;
#endif
    __threadfence();                                                       // the cleared words before any mark
    __syncthreads();
    if (present) atomicOr(&tab[(int64_t)SG_BOX_CELLS * W + (tid >> 6)], 1ull << (tid & 63));
#ifndef SG_BOX_BRUTE
    for (int32_t b = 0; b < B; ++b) {
        const int32_t ix0 = rect[b][0], ix1 = rect[b][1], iy0 = rect[b][2], iy1 = rect[b][3];
        if (ix0 > ix1) continue;
        const int32_t w = ix1 - ix0 + 1, cells = w * (iy1 - iy0 + 1);
        const unsigned long long bit = 1ull << (b & 63);
        for (int32_t i = tid; i < cells; i += SG_BOX_BLOCK)
            atomicOr(&tab[(int64_t)((iy0 + i / w) * SG_BOX_SIDE + ix0 + i % w) * W + (b >> 6)], bit);
    }
#endif
}

template <typename T>
__global__ __launch_bounds__(SG_BOX_BLOCK) void k_box_rows(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off, int n_frames,
                                                           const uint8_t *__restrict__ keep_in, int32_t B, const SgBoxRec *__restrict__ rec,
                                                           const unsigned long long *__restrict__ table, int32_t *__restrict__ out_box_of,
                                                           int32_t *__restrict__ out_count, T *__restrict__ out_local)
{
    const int64_t i = (int64_t)blockIdx.x * SG_BOX_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t W = sg_box_words(B);
    bool usable = sg_row_present(frame_off, n_frames, keep_in, i, n);
    double x = 0.0, y = 0.0, z = 0.0;
    if (usable) {
        const T *row = rows + i * 5;
        const T tx = row[0], ty = row[1], tz = row[2];
        usable = sg_box_row_usable<T>(tx, ty, tz);
        x = (double)tx; y = (double)ty; z = (double)tz;
    }
    int f = 0;
    const unsigned long long *words = table;
    if (usable) {
        f = sg_find_frame(frame_off, n_frames, i);
#ifdef SG_BOX_BRUTE
        const int32_t cell = SG_BOX_CELLS;
#else
        const int32_t cell = sg_box_cell(x, y);
#endif
        words = table + ((int64_t)f * (SG_BOX_CELLS + 1) + cell) * W;
    }
    const SgBoxRec *fr = rec + (int64_t)f * B;
    int32_t box_of = -1;
    double lx0 = 0.0, ly0 = 0.0, sz0 = 0.0;
    for (int32_t w = 0; w < W; ++w) {
        unsigned long long m = usable ? words[w] : 0ull;
        while (__ballot(m != 0ull) != 0ull) {                              // (uniform across the wave: the fold below meets every lane)
            int32_t key = -1;
            if (m != 0ull) {
                const int32_t b = w * 64 + (__ffsll((long long)m) - 1);
                m &= m - 1ull;
                double lx, ly, sz;
                if (sg_box_inside(fr[b], x, y, z, &lx, &ly, &sz)) {
                    key = f * B + b;
                    if (box_of < 0) { box_of = b; lx0 = lx; ly0 = ly; sz0 = sz; }
                }
            }
            if (out_count) {
                unsigned long long pend = __ballot(key >= 0);
                while (pend != 0ull) {
                    const int leader = __ffsll((long long)pend) - 1;
                    const int32_t k0 = __shfl(key, leader);
                    const unsigned long long same = __ballot(key == k0);
                    if (lane == leader) atomicAdd(&out_count[k0], (int32_t)__popcll(same));
                    pend &= ~same;
                }
            }
        }
    }
    if (i < n) {
        out_box_of[i] = box_of;
        if (out_local) {
            out_local[i * 3] = (T)lx0; out_local[i * 3 + 1] = (T)ly0; out_local[i * 3 + 2] = (T)sz0;
        }
    }
}

// The whole sequence on `stream`.  rec: sg_box_records(n_frames, n_boxes) records; table: sg_box_table(n_frames, n_boxes) words.  A
// batch without a row has its counts zeroed and its pose written by the first kernel; nothing is launched over rows.
extern "C" int sg_launch_box(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, int32_t n_boxes,
                             const void *boxes, int32_t box_features, const double *pose_in, SgBoxRec *rec, unsigned long long *table, int32_t *out_box_of,
                             int32_t *out_count, void *out_local, double *out_pose, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_box_file<T>, dim3(n_frames), dim3(SG_BOX_BLOCK), 0, st, (const T *)boxes, n_boxes, box_features, pose_in, rec, table, out_count, out_pose);
        SG_CHECK_LAUNCH();
        if (n <= 0) return 0;
        hipLaunchKernelGGL(k_box_rows<T>, dim3((unsigned)((n + SG_BOX_BLOCK - 1) / SG_BOX_BLOCK)), dim3(SG_BOX_BLOCK), 0, st, (const T *)rows, n, frame_off, n_frames,
                           keep_in, n_boxes, rec, table, out_box_of, out_count, (T *)out_local);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
