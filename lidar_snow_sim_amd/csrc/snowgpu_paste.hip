// snowgpu_paste.hip -- ground-truth object paste (snowgpu_paste_objects_device; definition: include/snowgpu.h; the slots, the draw, the
// conflict words, the sweep and the scratch: sg_paste.h; presence and the membership test: sg_box.h; the overlap: sg_iou.h).  Three kernels:
//   k_paste_count   ONE WAVE PER 512-ROW RUN counts the rows absent on input (ballot and popcount) into the (frame, run) table;
//   k_paste_frame   ONE WORKGROUP PER FRAME: the runs' counts become run bases and the free total (each lane sums a stretch of runs, lane 0
//                   scans the 256 sums, the lanes rewrite their stretches); the gts' records, their bit copies and the class counts (an
//                   integer LDS add per present gt); one lane per slot draws its object and builds the candidate's record; the Q x B and
//                   Q x Q clips are spread over the workgroup and folded into one 64-bit word per side by LDS atomicOr, whose order cannot
//                   show; lane 0 runs the sweep (sg_paste_frame); one lane per slot writes object, state, the box row and the pose, and
//                   the pasted slots' bases and enlarged records go to the frame's SgPasteFrame; the frame's 64 x 64 bit grid of
//                   sg_box.h -- one word per cell, bit k for pasted object k -- is cleared by the workgroup at the start and marked over
//                   each enlarged box's footprint by its lane (a 64-bit atomicOr, whose order cannot show);
//   k_paste_rows    ONE WAVE PER RUN, one lane per row: the row is copied as words; a present, usable row is tested against the pasted
//                   boxes whose bit its cell holds (records in LDS); an absent row takes its free rank from the run base plus the ballot
//                   prefix and, below the frame's pasted total, finds its object among at most 64 bases and copies the bank point.  The
//                   removed rows are summed per workgroup and added once (an integer add: the order cannot show).
// The row test by the grid was measured against a plain loop over the frame's records (profiles/paste_ab.jsonl, row_test "grid" / "loop"):
// 0.074 against 0.082 ms at 16 frames, 0.491 against 0.496 ms at 256 with about ten pasted boxes a frame; the loop was taken out.
// No memset, nothing read on the host; the step is read from device memory, so a captured graph draws anew when the caller advances it.
// Absent rows are moved as integer words and never looked at as numbers.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_paste.h"

#define SG_PASTE_BLOCK 256
#define SG_PASTE_WAVES (SG_PASTE_BLOCK / 64)

template <int N> struct PasteWord;
template <> struct PasteWord<4> { using type = uint32_t; };
template <> struct PasteWord<8> { using type = uint64_t; };

__global__ __launch_bounds__(SG_PASTE_BLOCK) void k_paste_count(const uint8_t *__restrict__ keep, const int64_t *__restrict__ off, int32_t n_frames, int32_t runs,
                                                                int32_t *__restrict__ table)
{
    const int64_t w = ((int64_t)blockIdx.x * SG_PASTE_BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int64_t f = w / runs;
    if (f >= n_frames) return;                                             // (the wave's: w is)
    const int64_t a = off[f], len = off[f + 1] - a, start = (w - f * runs) * SG_ROI_RUN;
    int32_t n = 0;
    for (int s = 0; s < SG_ROI_RUN / 64; ++s) {
        const int64_t i = start + s * 64 + lane;
        n += (int32_t)__popcll(__ballot(i < len && keep[a + i] == 0));
    }
    if (lane == 0) table[w] = n;
}

template <typename T>
__global__ __launch_bounds__(SG_PASTE_BLOCK) void k_paste_frame(SgPasteGroups g, double ewx, double ewy, double ewz, uint64_t seed, const uint64_t *__restrict__ step_p,
                                                                int32_t runs, int32_t *__restrict__ table, int32_t B, const T *__restrict__ gt, int32_t Cb,
                                                                const double *__restrict__ pose_in, const int64_t *__restrict__ bank_off,
                                                                const T *__restrict__ bank_boxes, const double *__restrict__ bank_pose,
                                                                const int32_t *__restrict__ class_off, T *__restrict__ out_gt, int32_t *__restrict__ out_object,
                                                                int32_t *__restrict__ out_state, int32_t *__restrict__ out_count, double *__restrict__ out_pose,
                                                                SgPasteFrame *__restrict__ frames, unsigned long long *__restrict__ grid)
{
    __shared__ SgIouRec gt_rec[SG_PASTE_BOXES_MAX], cand[SG_PASTE_SLOTS_MAX];
    __shared__ unsigned long long earlier[SG_PASTE_SLOTS_MAX], gt_hit, masks[3];          // masks: active, present, pasted
    __shared__ int32_t part[SG_PASTE_BLOCK], cnt[SG_PASTE_CLASSES_MAX], obj[SG_PASTE_SLOTS_MAX], pts[SG_PASTE_SLOTS_MAX], state[SG_PASTE_SLOTS_MAX],
        base[SG_PASTE_SLOTS_MAX], free_total;
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int32_t Q = g.Q, BQ = B + Q;
    gt += f * B * Cb;
    if (pose_in) pose_in += f * B * 2;
    // the run bases and the free total
    if (table) {
        int32_t *mine = table + f * runs;
        const int32_t chunk = (runs + SG_PASTE_BLOCK - 1) / SG_PASTE_BLOCK, lo = tid * chunk < runs ? tid * chunk : runs, hi = lo + chunk < runs ? lo + chunk : runs;
        int32_t sum = 0;
        for (int32_t r = lo; r < hi; ++r) sum += mine[r];
        part[tid] = sum;
        __syncthreads();
        if (tid == 0) {
            int32_t run = 0;
            for (int t = 0; t < SG_PASTE_BLOCK; ++t) { const int32_t n = part[t]; part[t] = run; run += n; }
            free_total = run;
        }
        __syncthreads();
        int32_t run = part[tid];
        for (int32_t r = lo; r < hi; ++r) { const int32_t n = mine[r]; mine[r] = run; run += n; }
    } else if (tid == 0) {
        free_total = 0;
    }
    for (int32_t i = tid; i < SG_BOX_CELLS; i += SG_PASTE_BLOCK) grid[f * SG_BOX_CELLS + i] = 0;          // (visible to the marks below: barriers lie between)
    if (tid < SG_PASTE_CLASSES_MAX) cnt[tid] = 0;
    if (tid < SG_PASTE_SLOTS_MAX) earlier[tid] = 0;
    if (tid == 0) gt_hit = 0;
    __syncthreads();
    // the gts: records, bit copies, the pose that was used, the class counts
    for (int32_t b = tid; b < B; b += SG_PASTE_BLOCK) {
        const T *row = gt + (int64_t)b * Cb;
        SgIouRec rec;
        const bool ok = sg_iou_make<T>(row, pose_in ? pose_in + (int64_t)b * 2 : nullptr, &rec);
        gt_rec[b] = rec;
        if (ok) {
            const int32_t c = sg_paste_class<T>(row[7]);
            if (c > 0) atomicAdd(&cnt[c - 1], 1);
        }
        const int64_t t = f * BQ + b;
        for (int32_t j = 0; j < Cb; ++j) out_gt[t * Cb + j] = row[j];
        if (out_pose) { out_pose[t * 2] = rec.c; out_pose[t * 2 + 1] = rec.s; }
    }
    __syncthreads();
    // the draws and the candidates: wave 0, one lane per slot
    if (tid < 64) {
        int32_t o = -1, n = 0;
        bool ok = false;
        SgIouRec rec{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (tid < Q) {
            o = sg_paste_draw(g, tid, cnt, class_off, seed, *step_p, (uint32_t)f);
            if (o >= 0) {
                ok = sg_iou_make<T>(bank_boxes + (int64_t)o * 8, bank_pose + (int64_t)o * 2, &rec);
                n = (int32_t)(bank_off[o + 1] - bank_off[o]);
            }
            obj[tid] = o; pts[tid] = n; cand[tid] = rec;
        }
        const unsigned long long act = __ballot(o >= 0), pres = __ballot(ok);
        if (tid == 0) { masks[0] = act; masks[1] = pres; }
    }
    __syncthreads();
    // the clips: Q x B against the gts, then Q x Q among the candidates
    const int32_t n_gt_pairs = Q * B, n_pairs = n_gt_pairs + Q * Q;
    for (int32_t i = tid; i < n_pairs; i += SG_PASTE_BLOCK) {
        if (i < n_gt_pairs) {
            const int32_t q = i / B, b = i - q * B;
            if (cand[q].ok != 0.0 && gt_rec[b].ok != 0.0 && sg_iou_area(cand[q], gt_rec[b], nullptr) > 0.0) atomicOr(&gt_hit, 1ull << q);
        } else {
            const int32_t k = i - n_gt_pairs, q = k / Q, p = k - q * Q;
            if (p < q && cand[q].ok != 0.0 && cand[p].ok != 0.0 && sg_iou_area(cand[q], cand[p], nullptr) > 0.0) atomicOr(&earlier[q], 1ull << p);
        }
    }
    __syncthreads();
    SgPasteFrame *fr = frames + f;
    if (tid == 0) {
        const int32_t rows = sg_paste_frame(Q, masks[0], masks[1], gt_hit, (const uint64_t *)earlier, pts, free_total, state, base);
        unsigned long long pasted = 0;
        for (int32_t q = 0; q < Q; ++q)
            if (state[q] == SG_PASTE_PASTED) pasted |= 1ull << q;
        masks[2] = pasted;
        fr->n_pasted = (int32_t)__popcll(pasted); fr->rows_pasted = rows;
        out_count[f * 4] = (int32_t)__popcll(pasted); out_count[f * 4 + 1] = rows; out_count[f * 4 + 2] = 0; out_count[f * 4 + 3] = free_total;
    }
    __syncthreads();
    // what a slot stores
    if (tid < Q) {
        const int32_t q = tid, o = obj[q], s = state[q];
        const bool pasted = s == SG_PASTE_PASTED;
        const int64_t t = f * BQ + B + q;
        out_object[f * Q + q] = o;
        out_state[f * Q + q] = s;
        for (int32_t j = 0; j < Cb; ++j) out_gt[t * Cb + j] = (pasted && j < 8) ? bank_boxes[(int64_t)o * 8 + j] : (T)0;
        if (out_pose) { out_pose[t * 2] = pasted ? cand[q].c : 0.0; out_pose[t * 2 + 1] = pasted ? cand[q].s : 0.0; }
        if (pasted) {
            const int32_t k = (int32_t)__popcll(masks[2] & ((1ull << q) - 1ull));
            fr->slot[k] = q; fr->base[k] = base[q]; fr->points[k] = pts[q]; fr->first[k] = (int32_t)bank_off[o];
            SgBoxRec r;
            const bool ok = sg_roi_make<T>(bank_boxes + (int64_t)o * 8, ewx, ewy, ewz, bank_pose + (int64_t)o * 2, &r);
            fr->rec[k] = r;
            if (ok) {                                                      // bit k in every cell the enlarged box can touch (sg_box.h)
                int32_t ix0, ix1, iy0, iy1;
                sg_box_footprint(r, &ix0, &ix1, &iy0, &iy1);
                for (int32_t iy = iy0; iy <= iy1; ++iy)
                    for (int32_t ix = ix0; ix <= ix1; ++ix) atomicOr(&grid[f * SG_BOX_CELLS + iy * SG_BOX_SIDE + ix], 1ull << k);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(SG_PASTE_BLOCK) void k_paste_rows(const T *__restrict__ rows, const uint8_t *__restrict__ keep, const int64_t *__restrict__ off,
                                                               int32_t runs, int32_t blocks_per_frame, const int32_t *__restrict__ table,
                                                               const SgPasteFrame *__restrict__ frames, const unsigned long long *__restrict__ grid,
                                                               const T *__restrict__ bank_points, int32_t B,
                                                               T *__restrict__ out_rows, uint8_t *__restrict__ out_keep, int32_t *__restrict__ out_source,
                                                               int32_t *__restrict__ out_count)
{
    using U = typename PasteWord<sizeof(T)>::type;
    __shared__ int32_t head[2 + 4 * SG_PASTE_SLOTS_MAX], removed_of[SG_PASTE_WAVES];
    __shared__ SgBoxRec rec[SG_PASTE_SLOTS_MAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t f = blockIdx.x / blocks_per_frame;
    const int32_t r = (int32_t)(blockIdx.x - f * blocks_per_frame) * SG_PASTE_WAVES + wave;
    const SgPasteFrame *fr = frames + f;
    for (int i = tid; i < 2 + 4 * SG_PASTE_SLOTS_MAX; i += SG_PASTE_BLOCK) head[i] = ((const int32_t *)fr)[i];
    __syncthreads();
    const int32_t n_pasted = head[0], rows_pasted = head[1];
    const int32_t *slot = head + 2, *base = slot + SG_PASTE_SLOTS_MAX, *points = base + SG_PASTE_SLOTS_MAX, *first = points + SG_PASTE_SLOTS_MAX;
    for (int i = tid; i < n_pasted * 8; i += SG_PASTE_BLOCK) ((double *)rec)[i] = ((const double *)fr->rec)[i];
    __syncthreads();
    const int64_t a = off[f], len = off[f + 1] - a, start = (int64_t)r * SG_ROI_RUN;
    const unsigned long long below = (1ull << lane) - 1ull;
    int32_t removed = 0;
    if (r < runs && start < len) {                                         // (the wave's)
        int32_t rank0 = keep ? table[f * runs + r] : 0;
        const U *in = (const U *)rows, *bank = (const U *)bank_points;
        U *out = (U *)out_rows;
        for (int s = 0; s < SG_ROI_RUN / 64; ++s) {
            const int64_t i = start + s * 64 + lane, row = a + i;
            const bool here = i < len, present = here && (!keep || keep[row] != 0);
            const unsigned long long votes = __ballot(here && !present);
            const int32_t rank = rank0 + (int32_t)__popcll(votes & below);
            rank0 += (int32_t)__popcll(votes);
            bool gone = false;
            if (here) {
                const U *src = in + row * 5;
                uint8_t k_out = 0;
                int32_t from = -1;
                if (present) {
                    const T *p = (const T *)src;
                    const T x = p[0], y = p[1], z = p[2];
                    if (sg_box_row_usable<T>(x, y, z)) {
                        double lx, ly, sz;
                        unsigned long long word = grid[f * SG_BOX_CELLS + sg_box_cell((double)x, (double)y)];      // the pasted boxes near the row
                        while (word && !gone) {
                            const int32_t k = __ffsll(word) - 1;
                            word &= word - 1ull;
                            gone = sg_box_inside(rec[k], (double)x, (double)y, (double)z, &lx, &ly, &sz);
                        }
                    }
                    k_out = gone ? 0 : 1;
                } else if (rank < rows_pasted) {
                    for (int32_t k = 0; k < n_pasted; ++k)
                        if (rank >= base[k] && rank - base[k] < points[k]) {
                            src = bank + ((int64_t)first[k] + (rank - base[k])) * 5;
                            from = B + slot[k];
                            k_out = 1;
                        }
                }
                const U w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3], w4 = src[4];
                U *dst = out + row * 5;
                dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3; dst[4] = w4;
                out_keep[row] = k_out;
                if (out_source) out_source[row] = from;
            }
            removed += (int32_t)__popcll(__ballot(gone));
        }
    }
    if (lane == 0) removed_of[wave] = removed;
    __syncthreads();
    if (tid == 0) {
        int32_t n = 0;
        for (int w = 0; w < SG_PASTE_WAVES; ++w) n += removed_of[w];
        if (n) atomicAdd(&out_count[f * 4 + 2], n);
    }
}

// The stage on `stream`.  groups, ew: host.  keep, pose_in, out_source and out_pose may be null; table: sg_paste_table int32, frames:
// sg_paste_frames records, grid: sg_paste_grid words.
extern "C" int sg_launch_paste(const void *rows, int dtype, int64_t n_total, int64_t max_frame, const int64_t *off, int n_frames, const uint8_t *keep, int32_t n_gt,
                               const void *gt, int32_t gt_features, const double *pose_in, const void *bank_points, const int64_t *bank_off, const void *bank_boxes,
                               const double *bank_pose, const int32_t *class_off, const SgPasteGroups *groups, const double *ew, uint64_t seed,
                               const uint64_t *d_step, int32_t *table, SgPasteFrame *frames, unsigned long long *grid, void *out_rows, uint8_t *out_keep, void *out_gt, int32_t *out_object,
                               int32_t *out_state, int32_t *out_source, int32_t *out_count, double *out_pose, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const int64_t runs = sg_roi_runs(max_frame), blocks_per_frame = (runs + SG_PASTE_WAVES - 1) / SG_PASTE_WAVES;
    const bool counted = keep && n_total > 0;
    if (counted) {
        const int64_t waves = (int64_t)n_frames * runs;
        hipLaunchKernelGGL(k_paste_count, dim3((unsigned)((waves + SG_PASTE_WAVES - 1) / SG_PASTE_WAVES)), dim3(SG_PASTE_BLOCK), 0, st, keep, off, n_frames, (int32_t)runs,
                           table);
        SG_CHECK_LAUNCH();
    }
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_paste_frame<T>, dim3((unsigned)n_frames), dim3(SG_PASTE_BLOCK), 0, st, *groups, ew[0], ew[1], ew[2], seed, d_step, (int32_t)runs,
                           counted ? table : nullptr, n_gt, (const T *)gt, gt_features, pose_in, bank_off, (const T *)bank_boxes, bank_pose, class_off, (T *)out_gt,
                           out_object, out_state, out_count, out_pose, frames, grid);
        SG_CHECK_LAUNCH();
        if (n_total > 0) {
            hipLaunchKernelGGL(k_paste_rows<T>, dim3((unsigned)((int64_t)n_frames * blocks_per_frame)), dim3(SG_PASTE_BLOCK), 0, st, (const T *)rows, keep, off,
                               (int32_t)runs, (int32_t)blocks_per_frame, counted ? table : nullptr, frames, grid, (const T *)bank_points, n_gt, (T *)out_rows, out_keep,
                               out_source, out_count);
            SG_CHECK_LAUNCH();
        }
        return 0;
    });
}
