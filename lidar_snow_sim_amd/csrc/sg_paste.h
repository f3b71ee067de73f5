// sg_paste.h -- ground-truth object paste (snowgpu_paste_objects_device; the DEFINITION: include/snowgpu.h): which slot belongs to which
// class, the Philox word and the object of a slot, the records of a candidate, the sweep that decides the state of every slot of a frame
// and the sizes of the scratch.  snowgpu_paste.hip runs these functions on the device -- only the conflict words are built another way
// there, spread over a workgroup --, tests/host_harness/paste_sweep.cpp runs sg_paste_words and sg_paste_frame, the same code in one
// thread, on the host (as sg_targets.h is compiled for both), and tests/paste_reference.py restates the definition in NumPy.
//
// The slots.  Class c = 1 .. NC owns slots s_c .. s_c + n_c - 1, s_c the prefix sum of the n_c.  Slot q = s_c + j is ACTIVE iff
// j < max(n_c - cnt_c, 0) and L_c = class_offsets[c + 1] - class_offsets[c] > 0; its object is class_offsets[c] + ((r_q L_c) >> 32).
//
// The words.  r_q = word q % 4 of Philox4x32-10 under key seed at counter (step lo, step hi, frame, "PAST" + q / 4): sg_weather_block's
// rounds under another tag, as sg_targets_block has them.
//
// The conflict words.  For an active slot whose bank box is present: bit q of gt_hit is set iff AREA(candidate q, gt b) > 0 for some
// present gt b; bit p of earlier[q], p < q, iff AREA(candidate q, candidate p) > 0 with p active and present.  AREA is sg_iou_area.
//
// The states.  0 inactive; 1 pasted; 2 collides with a gt; 3 collides with an earlier PASTED candidate; 4 more points than free slots
// are left; 5 the drawn bank box is absent.  A slot that is not inactive takes the lowest-numbered of 2 .. 5 that holds, else 1.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sg_iou.h"         // the overlap: sg_iou_make, sg_iou_area
#include "sg_roipool.h"     // the enlarged box: sg_roi_make; the runs: SG_ROI_RUN, sg_roi_runs
#include "sg_weather.h"     // the Philox block: sg_weather_block

#define SG_PASTE_SLOTS_MAX 64           /* 1 <= Q <= 64: one bit per slot in a conflict word */
#define SG_PASTE_CLASSES_MAX 16         /* 1 <= NC <= 16 */
#define SG_PASTE_BOXES_MAX 256          /* B + Q <= 256: the output is a box set of points_in_boxes */
#define SG_PASTE_TAG 0x50415354u        /* "PAST" */
#define SG_PASTE_CLASS_OFFSETS (SG_PASTE_CLASSES_MAX + 2)       /* int32 of a bank's class_offsets: [c], [c + 1] for c = 1 .. 16 */
#define SG_PASTE_INACTIVE 0
#define SG_PASTE_PASTED 1
#define SG_PASTE_HIT_GT 2
#define SG_PASTE_HIT_PASTED 3
#define SG_PASTE_NO_ROOM 4
#define SG_PASTE_ABSENT 5

struct SgPasteGroups {                  // SAMPLE_GROUPS as the kernel takes it
    int32_t n_classes, Q;
    int32_t n[SG_PASTE_CLASSES_MAX];
};

// What the frame kernel leaves for the row kernel, per frame: the pasted slots in slot order.
struct SgPasteFrame {
    int32_t n_pasted, rows_pasted;
    int32_t slot[SG_PASTE_SLOTS_MAX];           // q of pasted object k
    int32_t base[SG_PASTE_SLOTS_MAX];           // its first place in the frame's free list
    int32_t points[SG_PASTE_SLOTS_MAX];         // its number of points
    int32_t first[SG_PASTE_SLOTS_MAX];          // its first row in the bank's points
    SgBoxRec rec[SG_PASTE_SLOTS_MAX];           // its box, enlarged by the extra width
};

// elements of the scratch: one int32 per (frame, run), one SgPasteFrame per frame and one 64-bit word per (frame, cell of sg_box.h's grid):
// bit k of a cell for pasted object k of the frame, marked over the footprint (sg_box_footprint) of its enlarged box
static inline size_t sg_paste_table(int n_frames, int64_t max_frame) { return (size_t)n_frames * (size_t)sg_roi_runs(max_frame); }
static inline size_t sg_paste_frames(int n_frames) { return (size_t)n_frames; }
static inline size_t sg_paste_grid(int n_frames) { return (size_t)n_frames * (size_t)SG_BOX_CELLS; }

// block b of frame f: the four words of slots 4 b .. 4 b + 3
__host__ __device__ inline void sg_paste_block(uint64_t seed, uint64_t step, uint32_t f, uint32_t b, uint32_t (&out)[4])
{
    sg_weather_block(seed, step, f, (SG_PASTE_TAG - SG_WEATHER_TAG) + b, out);         // (uint32 arithmetic: the tag becomes "PAST" + b)
}

// the class c (1 .. NC) of slot q and its number j within the class
__host__ __device__ inline void sg_paste_slot(const SgPasteGroups &g, int32_t q, int32_t *c, int32_t *j)
{
    int32_t s = 0;
    for (int32_t k = 0; k < g.n_classes; ++k) {
        if (q < s + g.n[k]) { *c = k + 1; *j = q - s; return; }
        s += g.n[k];
    }
    *c = 0; *j = 0;                                                                    // (q >= Q: no caller asks)
}

// the class of a gt whose column 7 is v: 1 .. 16 for an integral value in that range, else 0
template <typename T> __host__ __device__ inline int32_t sg_paste_class(T v)
{
    const double d = (double)v;
    if (!(d >= 1.0 && d <= (double)SG_PASTE_CLASSES_MAX)) return 0;                    // (false for NaN)
    const int32_t c = (int32_t)d;
    return (double)c == d ? c : 0;
}

// The object of slot q of frame f, -1 for an inactive slot.  cnt[c - 1]: the present gts of class c; class_offsets: the bank's.
__host__ __device__ inline int32_t sg_paste_draw(const SgPasteGroups &g, int32_t q, const int32_t *cnt, const int32_t *class_offsets, uint64_t seed,
                                                 uint64_t step, uint32_t f)
{
    int32_t c, j;
    sg_paste_slot(g, q, &c, &j);
    if (c < 1) return -1;
    const int32_t want = g.n[c - 1] - cnt[c - 1], L = class_offsets[c + 1] - class_offsets[c];
    if (j >= (want > 0 ? want : 0) || L <= 0) return -1;
    uint32_t w[4];
    sg_paste_block(seed, step, f, (uint32_t)(q >> 2), w);
    return class_offsets[c] + (int32_t)(((uint64_t)w[q & 3] * (uint64_t)(uint32_t)L) >> 32);
}

// The sweep of one frame over q ascending.  active, present, gt_hit: one bit per slot; earlier[q]: the slots before q that q overlaps;
// points[q]: the points of q's object; free_total: the frame's slots absent on input.  state[q] and base[q] (the first place of a pasted
// object in the free list, 0 otherwise) are written for every q < Q; returns the rows pasted.
__host__ __device__ inline int32_t sg_paste_frame(int32_t Q, uint64_t active, uint64_t present, uint64_t gt_hit, const uint64_t *earlier, const int32_t *points,
                                                  int32_t free_total, int32_t *state, int32_t *base)
{
    int32_t free_left = free_total;
    uint64_t pasted = 0;
    for (int32_t q = 0; q < Q; ++q) {
        const uint64_t bit = (uint64_t)1 << q;
        int32_t s = SG_PASTE_PASTED;
        if (!(active & bit)) s = SG_PASTE_INACTIVE;
        else if (gt_hit & bit) s = SG_PASTE_HIT_GT;
        else if (earlier[q] & pasted) s = SG_PASTE_HIT_PASTED;
        else if (points[q] > free_left) s = SG_PASTE_NO_ROOM;
        else if (!(present & bit)) s = SG_PASTE_ABSENT;
        state[q] = s;
        base[q] = 0;
        if (s == SG_PASTE_PASTED) {
            base[q] = free_total - free_left;
            free_left -= points[q];
            pasted |= bit;
        }
    }
    return free_total - free_left;
}

// The conflict words of one frame by plain loops (the host's route; the kernel spreads the same pairs over a workgroup).  cand[q]: the
// IoU record of slot q's bank box (ok = 0: absent or inactive); gt[b]: those of the frame's gts.
__host__ __device__ inline void sg_paste_words(int32_t Q, int32_t B, const SgIouRec *cand, const SgIouRec *gt, uint64_t *gt_hit, uint64_t *earlier)
{
    *gt_hit = 0;
    for (int32_t q = 0; q < Q; ++q) {
        earlier[q] = 0;
        if (cand[q].ok == 0.0) continue;
        for (int32_t b = 0; b < B; ++b)
            if (gt[b].ok != 0.0 && sg_iou_area(cand[q], gt[b], nullptr) > 0.0) { *gt_hit |= (uint64_t)1 << q; break; }
        for (int32_t p = 0; p < q; ++p)
            if (cand[p].ok != 0.0 && sg_iou_area(cand[q], cand[p], nullptr) > 0.0) earlier[q] |= (uint64_t)1 << p;
    }
}
