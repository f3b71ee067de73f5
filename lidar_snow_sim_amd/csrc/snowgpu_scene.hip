// snowgpu_scene.hip -- scene transforms (snowgpu_transform_scene_device; definition: include/snowgpu.h; the draws, the candidate, the
// sweep, what a row and a box become and the scratch: sg_scene.h; presence and the record: sg_iou.h; the membership test that makes
// box_of: sg_box.h through sg_launch_box, the launcher of snowgpu_points_in_boxes_device itself).  Two kernels of its own:
//   k_scene_frame   ONE WORKGROUP PER FRAME: one lane per box builds its record in LDS; lane 0 makes the world draw and takes cos / sin of
//                   theta; with a local part the lanes draw the B T tries (cos / sin of every delta) into the try records, and the sweep
//                   runs over the present boxes in order: T lanes build the candidates of box i in LDS, the lanes take the (t, j) pairs
//                   and clip them, an LDS atomicOr per hit gives each try's collision bit (an OR: the order cannot show), lane 0 takes the
//                   first clear bit and settles record i.  One lane per box then writes state, tried, local, the box row, the pose and
//                   the box's row record.  Without a local part neither the draws nor the sweep run.
//   k_scene_rows    ONE LANE PER ROW, a workgroup per span of 2048 rows of one frame: the frame's world record comes through the scalar
//                   path (its address is the workgroup's), the frame's row records go into LDS once per workgroup; a row is read as five
//                   words, a present and usable one is transformed in float64 and rounded once, and five words are written.  The rows
//                   are 20-byte (40-byte) records read at a lane stride of one row, as snowgpu_paste.hip reads them: a wave's five loads
//                   touch the same 1280 contiguous bytes.  A lane reads its row before it writes it and touches no other row, which is
//                   what the in-place form rests on.
// With a local part and no box_of from the caller, the two kernels of snowgpu_box.hip run in front into scratch of this stage.
// No memset, nothing read on the host; the step is read from device memory, so a captured graph draws anew when the caller advances it.
// Absent rows are moved as integer words and never looked at as numbers.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include "sg_common.h"
#include "sg_launch.h"
#include "sg_scene.h"

#define SG_SCENE_BLOCK 256
#define SG_SCENE_SPAN 2048              /* rows of a workgroup of k_scene_rows */

template <int N> struct SceneWord;
template <> struct SceneWord<4> { using type = uint32_t; };
template <> struct SceneWord<8> { using type = uint64_t; };

template <typename T>
__global__ __launch_bounds__(SG_SCENE_BLOCK) void k_scene_frame(SgSceneCfg k, uint64_t seed, const uint64_t *__restrict__ step_p, int32_t B, const T *__restrict__ gt,
                                                                int32_t Cb, const double *__restrict__ pose_in, T *__restrict__ out_gt, double *__restrict__ out_world,
                                                                int32_t *__restrict__ out_state, int32_t *__restrict__ out_tried, double *__restrict__ out_local,
                                                                double *__restrict__ out_pose, double *tries, double *__restrict__ rowrec)
{
    __shared__ SgIouRec cur[SG_BOX_MAX], cand[SG_SCENE_TRIES_MAX];
    __shared__ double world[SG_SCENE_REC];
    __shared__ int32_t state[SG_BOX_MAX], tried[SG_BOX_MAX];
    __shared__ unsigned int hit;
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x;
    const int32_t Tn = k.tries;
    gt += f * B * Cb;
    if (pose_in) pose_in += f * B * 2;
    if (tid < B) {                                                         // (B <= SG_BOX_MAX = the block)
        SgIouRec rec;
        sg_iou_make<T>(gt + (int64_t)tid * Cb, pose_in ? pose_in + (int64_t)tid * 2 : nullptr, &rec);
        cur[tid] = rec;
        state[tid] = SG_SCENE_STILL; tried[tid] = -1;
    }
    if (tid == 0) {
        double w[SG_SCENE_REC];
        sg_scene_world_draw(k, seed, *step_p, (uint32_t)f, w);
        if (k.rot_on) { w[2] = cos(w[4]); w[3] = sin(w[4]); }
        for (int j = 0; j < SG_SCENE_REC; ++j) { world[j] = w[j]; out_world[f * SG_SCENE_REC + j] = w[j]; }
    }
    __syncthreads();
    double *tr = tries ? tries + f * B * Tn * SG_SCENE_REC : nullptr;
    if (Tn > 0) {
        // the draws of every try of every present box
        for (int32_t p = tid; p < B * Tn; p += SG_SCENE_BLOCK) {
            const int32_t i = p / Tn, t = p - i * Tn;
            double r[SG_SCENE_REC];
            sg_scene_identity(r);
            if (cur[i].ok != 0.0) {
                sg_scene_try_draw(k, seed, *step_p, (uint32_t)f, i, t, r);
                if (k.lrot_on) { r[3] = cos(r[5]); r[4] = sin(r[5]); }
            }
            for (int j = 0; j < SG_SCENE_REC; ++j) tr[(int64_t)p * SG_SCENE_REC + j] = r[j];
        }
        __syncthreads();
        // the sweep: i ascending over the present boxes (the test is the workgroup's: record i is settled in its own turn only)
        for (int32_t i = 0; i < B; ++i) {
            if (cur[i].ok == 0.0) continue;
            if (tid < Tn) {
                SgIouRec c;
                sg_scene_candidate(cur[i], tr + ((int64_t)i * Tn + tid) * SG_SCENE_REC, &c);
                cand[tid] = c;
            }
            if (tid == 0) hit = 0u;
            __syncthreads();
            for (int32_t p = tid; p < Tn * B; p += SG_SCENE_BLOCK) {
                const int32_t t = p / B, j = p - t * B;
                if (j != i && cur[j].ok != 0.0 && sg_iou_area(cand[t], cur[j], nullptr) > 0.0) atomicOr(&hit, 1u << t);
            }
            __syncthreads();
            const unsigned int bits = hit;                                 // (cleared again only behind the barrier below)
            if (tid < Tn) tr[((int64_t)i * Tn + tid) * SG_SCENE_REC + 7] = ((bits >> tid) & 1u) ? 1.0 : 0.0;
            if (tid == 0) {
                const unsigned int clear = ~bits & ((1u << Tn) - 1u);
                if (clear) {
                    const int32_t t = __ffs((int)clear) - 1;
                    cur[i] = cand[t];
                    state[i] = SG_SCENE_MOVED; tried[i] = t;
                } else {
                    state[i] = SG_SCENE_BLOCKED;
                }
            }
            __syncthreads();
        }
    }
    // what a box stores
    if (tid < B) {
        const int64_t q = f * B + tid;
        const T *row = gt + (int64_t)tid * Cb;
        const int32_t st = state[tid], tk = tried[tid];
        const bool moved = st == SG_SCENE_MOVED;
        double r[SG_SCENE_REC], local[SG_SCENE_REC], rr[SG_SCENE_ROWREC];
        sg_scene_identity(r);
        if (moved)
            for (int j = 0; j < SG_SCENE_REC; ++j) r[j] = tr[((int64_t)tid * Tn + tk) * SG_SCENE_REC + j];
        const SgIouRec me = cur[tid];
        const bool present = me.ok != 0.0;
        sg_scene_box_records(st, r, present ? (double)row[0] : 0.0, present ? (double)row[1] : 0.0, present ? (double)row[2] : 0.0, local, rr);
        out_state[q] = st; out_tried[q] = tk;
        for (int j = 0; j < SG_SCENE_REC; ++j) out_local[q * SG_SCENE_REC + j] = local[j];
        for (int j = 0; j < SG_SCENE_ROWREC; ++j) rowrec[q * SG_SCENE_ROWREC + j] = rr[j];
        double pose[2] = {0.0, 0.0};
        if (present) {
            double o[7];
            sg_scene_box((double)row[6], me, moved, r[5], world, o, pose);
            for (int j = 0; j < 7; ++j) out_gt[q * Cb + j] = (T)o[j];
            for (int32_t j = 7; j < Cb; ++j) out_gt[q * Cb + j] = row[j];
        } else {
            for (int32_t j = 0; j < Cb; ++j) out_gt[q * Cb + j] = row[j];
        }
        if (out_pose) { out_pose[q * 2] = pose[0]; out_pose[q * 2 + 1] = pose[1]; }
    }
}

// (rows and out_rows are the same array in the in-place form: no __restrict__ on either)
template <typename T>
__global__ __launch_bounds__(SG_SCENE_BLOCK) void k_scene_rows(const T *rows, const uint8_t *__restrict__ keep, const int64_t *__restrict__ off, int32_t blocks_per_frame,
                                                               int32_t B, int32_t local_on, const int32_t *__restrict__ box_of, const double *__restrict__ world,
                                                               const double *__restrict__ rowrec, T *out_rows, uint8_t *__restrict__ out_keep)
{
    using U = typename SceneWord<sizeof(T)>::type;
    __shared__ double rr[SG_BOX_MAX * SG_SCENE_ROWREC];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x / blocks_per_frame;
    const int64_t a = off[f], len = off[f + 1] - a, start = (int64_t)(blockIdx.x - f * blocks_per_frame) * SG_SCENE_SPAN;
    if (start >= len) return;                                              // (the workgroup's: before any barrier)
    if (local_on) {
        for (int32_t i = tid; i < B * SG_SCENE_ROWREC; i += SG_SCENE_BLOCK) rr[i] = rowrec[f * B * SG_SCENE_ROWREC + i];
        __syncthreads();
    }
    double w[6];
    for (int j = 0; j < 6; ++j) w[j] = world[f * SG_SCENE_REC + j];        // (a workgroup-uniform address: scalar loads)
    const U *in = (const U *)rows;
    U *out = (U *)out_rows;
    for (int s = 0; s < SG_SCENE_SPAN / SG_SCENE_BLOCK; ++s) {
        const int64_t i = start + (int64_t)s * SG_SCENE_BLOCK + tid;
        if (i >= len) break;
        const int64_t row = a + i;
        const bool present = !keep || keep[row] != 0;
        const U *src = in + row * 5;
        U w0 = src[0], w1 = src[1], w2 = src[2];
        const U w3 = src[3], w4 = src[4];
        if (present) {
            const T tx = __builtin_bit_cast(T, w0), ty = __builtin_bit_cast(T, w1), tz = __builtin_bit_cast(T, w2);
            if (sg_box_row_usable<T>(tx, ty, tz)) {
                double x = (double)tx, y = (double)ty, z = (double)tz;
                const double *rec = nullptr;
                if (local_on) {
                    const int32_t b = box_of[row];
                    if (b >= 0 && b < B && rr[b * SG_SCENE_ROWREC + 9] != 0.0) rec = rr + b * SG_SCENE_ROWREC;
                }
                sg_scene_row(&x, &y, &z, rec, w);
                w0 = __builtin_bit_cast(U, (T)x); w1 = __builtin_bit_cast(U, (T)y); w2 = __builtin_bit_cast(U, (T)z);
            }
        }
        U *dst = out + row * 5;
        dst[0] = w0; dst[1] = w1; dst[2] = w2; dst[3] = w3; dst[4] = w4;
        out_keep[row] = present ? 1 : 0;
    }
}

// The stage on `stream`.  cfg: host.  keep, pose_in, box_of, out_pose and out_tries may be null.  Scratch: rowrec, sg_scene_rowrecs()
// doubles; tries, sg_scene_tries() doubles, used when out_tries is null and there is a local part; box_rec, box_table (sg_box.h) and
// box_of_own (n_total int32), used when box_of is null, there is a local part and the batch has a row.
extern "C" int sg_launch_scene(const void *rows, int dtype, int64_t n_total, int64_t max_frame, const int64_t *off, int n_frames, const uint8_t *keep, int32_t B,
                               const void *gt, int32_t Cb, const double *pose_in, const SgSceneCfg *cfg, uint64_t seed, const uint64_t *d_step, const int32_t *box_of,
                               SgBoxRec *box_rec, unsigned long long *box_table, int32_t *box_of_own, double *tries, double *rowrec, void *out_rows, uint8_t *out_keep,
                               void *out_gt, double *out_world, int32_t *out_state, int32_t *out_tried, double *out_local, double *out_pose, double *out_tries,
                               void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const bool local_on = cfg->tries > 0;
    if (local_on && !box_of && n_total > 0) {
        if (int e = sg_launch_box(rows, dtype, n_total, off, n_frames, keep, B, gt, Cb, pose_in, box_rec, box_table, box_of_own, nullptr, nullptr, nullptr, stream)) return e;
        box_of = box_of_own;
    }
    const int64_t blocks_per_frame = (max_frame + SG_SCENE_SPAN - 1) / SG_SCENE_SPAN;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(k_scene_frame<T>, dim3((unsigned)n_frames), dim3(SG_SCENE_BLOCK), 0, st, *cfg, seed, d_step, B, (const T *)gt, Cb, pose_in, (T *)out_gt, out_world,
                           out_state, out_tried, out_local, out_pose, local_on ? (out_tries ? out_tries : tries) : nullptr, rowrec);
        SG_CHECK_LAUNCH();
        if (n_total > 0) {
            hipLaunchKernelGGL(k_scene_rows<T>, dim3((unsigned)((int64_t)n_frames * blocks_per_frame)), dim3(SG_SCENE_BLOCK), 0, st, (const T *)rows, keep, off,
                               (int32_t)blocks_per_frame, B, local_on ? 1 : 0, box_of, out_world, rowrec, (T *)out_rows, out_keep);
            SG_CHECK_LAUNCH();
        }
        return 0;
    });
}
