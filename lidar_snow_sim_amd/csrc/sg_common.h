// sg_common.h -- types shared by the host API (snowgpu_api.cpp, snowgpu_device.cpp, snowgpu_stages.cpp, snowgpu_batch.cpp, snowgpu_host.cpp; their own header is sg_host.h) and the gfx950 kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define SG_PI 3.141592653589793 /* np.pi (simulation.py:26) */
#define SG_TWO_PI (2 * SG_PI)
#define SG_RBINS 1230           /* M_extended (simulation.py:113) */
#define SG_NBINS 2048           /* azimuth bins per table: 3.07 mrad, one beam width at 3 mrad */
#define SG_BIN_MARGIN 1e-6      /* rad; flakes are filed under every bin their angular interval +- margin touches */
#define SG_BEAM_MARGIN 1e-9     /* rad; a beam scans every bin its wedge +- margin touches */
#define SG_TBL_STRIDE 16     /* 64-bit words between the per-table counters of the segment builder: one 128-byte line each -- the 16 384 atomics of a
                               256-sweep batch fall on 64 tables, and sixteen counters to a line queued them behind one another (k_seg_count 30 us) */
#define SG_BLKREC 8          /* int32 words per block record of the segment order (five used) */
#define SG_HITS_UNDECIDED 0x40000000   /* in a beam's flake count: a distance test of the pass over all rows was too close to call (sg_beam.h: sg_near_ray) */
#define SG_MAX_LASERS 256
#define SG_LCAP 63              /* hard cap on flakes intersecting one beam (slow path capacity) */
#define SG_TILE 1024            /* rows per sort / compaction tile */

// One filed flake, 64 bytes = one half cache line, beam-independent quantities hoisted out of
// get_occlusions' beam loop (simulation.py:351-354, :405; geometry.py:138-190, :32-80).
struct SgEntry {      // 64 bytes; the first half decides whether the flake meets a beam, the second is read of those that do (sg_beam.h: sg_flake_test)
    double phi;      // atan2(y, x) in [0, 2 pi]                simulation.py:351-352
    double x, y, r;  // table row                               simulation.py:329-330
    double t0, t1;   // tangent angles (right, left)            geometry.py:32-80
    double rho;      // sqrt(x^2 + y^2)                         simulation.py:332
    uint32_t flags;  // bit 0: this bin is the first bin of the flake's (circular) bin range
    uint32_t src;    // row in the uploaded table
};

#define SG_OV_CAP 16      /* flakes per overflow slot: a beam of the pass over all rows that meets more flakes than its LDS list holds, up to
                             this many, leaves ALL of them in the slot of its sorted position and its tier runs no second scan */
#define SG_OV_STRIDE (2 + 3 * SG_OV_CAP)   /* doubles per overflow slot: range, azimuth, then (a1, a2, rho) per flake -- the plane order of the
                                              hand-over queues, stride 1 */
#ifndef SG_QSTEPS
#define SG_QSTEPS 16     /* coarse range index of a bin: counts below 0, 8, .. 120 m (at most 64: k_table_index is one wave per bin) */
#define SG_QSTEP_M 8.0
#endif

struct SgTable {
    const SgEntry *entries;     // bins concatenated, each bin sorted by rho ascending
    const uint32_t *bin_start;  // n_bins + 1 offsets into entries
    const uint32_t *bin_q;      // n_bins x SG_QSTEPS: records of the bin nearer than SG_QSTEP_M * k metres (coarse range index)
    uint32_t n_bins;
    uint32_t n_entries;
    double inv_bin_w;           // n_bins / (2 pi)
    uint32_t n_flakes;
    uint32_t max_bin;           // longest bin (entries)
    const uint32_t *bin_qs;     // qs_steps x (n_bins + 1): counts step-major, two to a word (sg_range_index.h), or null -- bin_q alone is used
    uint32_t qs_steps;          // shape of bin_qs: steps ...
    float qs_per_m;             // ... and steps per metre (1 / step length; a power of two, so that range * qs_per_m is exact).
                                // qs_steps == 0 (a zero-initialised descriptor): SG_QSTEPS steps of SG_QSTEP_M metres, the shape of bin_q
};

struct SgLasers {
    double focal_slope[SG_MAX_LASERS];   // simulation.py:75
    double focal_offset[SG_MAX_LASERS];  // simulation.py:76
    int32_t min_i[SG_MAX_LASERS];        // simulation.py:72
    int32_t max_i[SG_MAX_LASERS];        // simulation.py:123-126
    int32_t n;
};

// Result record of one beam, one uint32 per channel-sorted position (the per-beam kernels write 4 bytes per row; the
// compaction kernels rebuild the output row from the ORIGINAL row and this record -- no un-compacted copy of the cloud):
//   bits 0..7   new intensity (simulation.py:188, an integer in [min_i, max_i] <= 255), labels 1 / 2 only
//   bits 8..9   label: 0 unchanged, 1 attenuated, 2 scattered (simulation.py:160, :174)
//   bit  10     copy-through row: its channel has no laser (Q5), column 4 keeps the channel value
//   bit  11     label 0: bits 0..7 are the row's original intensity (SG_REC_HAS_I)
//   bits 12..22 argmax bin of the power profile (simulation.py:151), label 2: the point moves to k / 10 - c tau / 2
//   bit  31     reference: the record is rec_q[bits 0..30] (written by k_power, densely, in queue order)
#define SG_REC_LABEL_SHIFT 8
#define SG_REC_COPY (1u << 10)
#define SG_REC_HAS_I (1u << 11) /* label 0 only: bits 0..7 hold the row's ORIGINAL intensity (an integer in [0, 255]), so the
                                   noise-floor pass need not read the row; set by the pass over all rows for beams it finishes itself */
#define SG_REC_SLOT (1u << 31)  /* the record proper is rec_q[low 31 bits]: the row's slot in the hand-over queue */
#define SG_REC_K_SHIFT 12
#define SG_MAX_CLASSES 4        /* later capacity tiers incl. the global-list tier */

#if defined(__HIPCC__) || defined(__HIP__)
typedef int2 int2_t;
#else
struct int2_t { int32_t x, y; };
#endif

struct SgBeamArgs {
    const void *rows;            // AoS rows, all frames
    const int64_t *frame_off;    // n_frames + 1
    int32_t n_frames;
    int64_t n_total;
    int64_t uniform_rows;        // > 0: every frame has this many rows (frame = position / uniform_rows)
    float inv_uniform_rows;
    const int32_t *perm;         // channel-sorted position (global) -> frame-local source row (written for UNSORTED frames only)
    // Rows in channel-sorted order without a gather: a frame whose input rows already are channel-sorted (frame_unsorted[f] == 0:
    // channel-major sweeps) is read in place -- sorted position g IS row g of `rows` --, any other frame (firing order: an STF .bin
    // interleaves the channels, precompute.py:78) from the sorted copy the channel sort's scatter pass makes (row g of `srows`).
    const void *srows;           // n_total rows, valid where frame_unsorted[f] != 0
    const int32_t *frame_unsorted;   // n_frames
    const SgTable *frame_tables; // n_frames x n_lasers resolved descriptors (entries == nullptr: unknown table id)
    const SgLasers *las;
    const double *rgrid;         // SG_RBINS
    double beam_div_deg;
    uint32_t *rec;               // per sorted position: result record (SG_REC_*)
    uint32_t *rec_q;             // per queue slot of the direct-mode pass: result record of the beam queued there
    void *rng;                   // per sorted position: the beam's range in the row dtype (simulation.py:89), written by the pass over
                                 // all rows for every simulated beam: the noise-floor pass reads 4 bytes instead of gathering the row
    int32_t *status;             // [0] error code, [1] first offending sorted row
    int32_t *tier_hint;          // page-locked host words the device can write (or null): beams per later tier of THIS batch, read by the host when it schedules a later one
    unsigned long long *diff2;   // per frame: sum over attenuated rows of 2 * (0.9 * max_intensity - new_i)
    int32_t exact_math;          // 1: libm sin / tan + true division (validation mode)
    // tier classes: a beam of the first pass that met more flakes than its list holds is flagged with the first later
    // tier whose capacity takes all of them (the scan keeps COUNTING after the list is full, so the count is exact)
    int32_t n_cls;               // later tiers (the last one is the global-list tier, capacity = table size)
    int32_t cls_cap[SG_MAX_CLASSES];
    // direct mode: blocks walk (table, frame, channel) segments of the sorted rows (seg_blk != null) or plain chunks of
    // q_chunk sorted positions.  Either way a block lies in ONE region, and the region is also its slice of the dict queue.
    const int32_t *seg_blk;      // n_seg: first block of segment i
    const int64_t *seg_start;    // n_seg: global sorted position of the segment's first row
    const int32_t *seg_cnt;      // n_seg: rows
    const int32_t *seg_frame;    // n_seg: frame | channel << 22
    const int32_t *seg_n;        // [0] = n_seg, [1] = blocks in all segments
    const int32_t *seg_of_blk;   // grid_blocks x SG_BLKREC: per block of the segment order {segment, its first sorted position, its rows, frame | channel << 22, its first block}
    int64_t grid_blocks;         // host: blocks of this launch (upper bound; surplus blocks leave at once)
    int32_t q_chunk;             // linear mode: sorted positions per region (a multiple of the block size)
    // The pass runs as a few launches over consecutive block ranges, so that k_power of one range runs next to the scan
    // of the next: blocks [blk_lo, blk_hi) (linear order), or chunk `chunk` of chunk_blk (segment order: device-built
    // boundaries, cut at segment starts).
    int64_t blk_lo, blk_hi;
    const int32_t *chunk_blk;
    int32_t chunk;
    // Hand-over queue of the direct-mode pass: a beam that met flakes hands its range, azimuth and flake list to k_power,
    // which builds the occlusion dict and everything after it.  Blocked SoA of 32-bit words (groups of 64 slots): range, azimuth and
    // one word per listed flake -- record index | limit-ray bits --, resolved by the reader (sg_queue.h).
    // A region's beams with ONE flake fill its slice from the front, the others from the back (waves of uniform loop
    // length in k_power); qn[region] = front count | back count << 32, bumped once per wave.
    uint32_t *dq;
    int32_t *dq_g;               // per slot: sorted position of the beam
    uint16_t *dq_sc;             // per slot: flakes in the list | channel << 8
    unsigned long long *qn;      // per region
    int2_t *pw_items;            // work items of k_power (k_power_plan): {first slot, count | (frame + 1) << 10}
    int32_t *pw_count;           // [0] items planned, [1] items of k_power_few (reset per chunk)
    int2_t *pw_items1;           // work items of k_power_few (the front of every region's slice), or null: k_power takes them too
    int32_t front_max;           // beams with up to this many flakes fill a region's slice from the front (1 .. 3 with pw_items1; else 1)
    int64_t n_regions_ub;        // host: upper bound of the regions (segments / linear chunks)
    int32_t blk_rows;            // rows per block of the direct-mode pass
    int32_t kp_lds_quarters;     // host: share of a CU's capacity k_power takes for the main queue (1..4 quarters; 0 = all)
    int64_t dq_n;                // plane stride (= n_total)
    // list mode: this launch handles entries [work_lo, min(work_hi, count)) of class `cls` of the tier lists
    // The pass over all rows puts an over-full beam on the list of the tier that holds all its flakes: into its region's slice of
    // tier_sparse (class k at k * tier_stride; tn[region][k] entries from the region's first sorted position on), which k_power_plan
    // (bases) and k_tier_gather close up into tier_list.  Any order: a tier's results do not depend on it.
    int32_t *tier_list;          // the class lists, tier_stride (= n_total) entries apart
    int32_t *tier_info;          // [0..3] entries per class
    int64_t tier_stride;
    int32_t *tier_sparse;        // the same before closing up
    int32_t *tn, *tbase;         // per region x SG_MAX_CLASSES: entries, start in the closed-up list
    int32_t cls;
    int32_t work_lo, work_hi;
    int32_t work_hint;           // host: beams this class is expected to hold (from the batches before; 0: unknown) -- sizes the grids of its kernels
    // row kernels (snowgpu_rows.hip): beams whose dict needs NumPy's pairwise sum (an owner with >= 8 slots) are deferred to a
    // second instantiation through this list (laid out like tier_list: class k at k * tier_stride) and its per-class counters
    int32_t *redo_list;
    int32_t *redo_cnt;
    // dict hand-over of a later tier's scan (k_tier_scan_direct): entry i of the class -> slot i, flakes in scan order (planes of tq_cap entries)
    double *tq;
    uint16_t *tq_sc;
    int32_t tq_cap;
    // Overflow slots of the pass over all rows, one per sorted position (SG_OV_STRIDE doubles, touched only by beams that over-fill
    // their LDS list): range, azimuth, (a1, a2, rho) of every flake met, in arrival order; ov_sc[g] = flakes | channel << 8.
    // k_power<.., LISTQ> of a class reads them instead of a hand-over buffer when ov_list is set (and sorts by range as it loads).
    double *ov;
    uint16_t *ov_sc;
    int32_t ov_cap;              // 0: no overflow slots (every over-full beam is scanned again by its tier)
    int32_t ov_list;             // k_power<.., LISTQ>: this class's flake lists are the overflow slots of its rows         // the slots hold the flakes in scan order (k_tier_scan_direct): k_power sorts them by range as it loads them
    // global-list tier: per-lane lists in global memory, h_cap entries each, h_lanes lanes
    double *h_lists;
    int32_t h_cap, h_lanes;
    // optional occlusion-dict tap (snowgpu_debug_occlusions)
    int32_t *dbg_count;
    double *dbg_rj;
    double *dbg_ratio;
    int32_t dbg_cap;
};

// Camera-FOV crop of augment() (simulation.py:39-47, :532-540) as the compaction applies it: M = V2C^T R0^T (4 x 3,
// lidar_to_rect) and P2 (3 x 4) in float64, image h x w.  enabled = 0: no crop.
struct SgFov {
    int32_t enabled;
    int32_t reserved_;           // (the pre-augment crop of precompute.py:96-99 is a context switch: snowgpu_set_fov_precrop)
    double m[12];                // lidar_to_rect: rect = [x y z 1] . m   (row-major 4 x 3)
    double p[12];                // P2 (row-major 3 x 4)
    double img_h, img_w;
};

// Launch wrappers (hipStream_t passed as void*), each implemented in the file that defines its kernels: snowgpu_sort.hip (expand_rows, sort,
// gather_rows, segments*, resolve_tables), snowgpu_kernels.hip (beams, power*, tier_*, huge, sg_beams_block), snowgpu_rows.hip (rows),
// snowgpu_compact.hip (compact, crop_*), snowgpu_mask.hip (mask_front, finish_aligned_masked, fov_mask), snowgpu_dror.hip (dror), snowgpu_voxel.hip (voxelize), snowgpu_fps.hip (fps), snowgpu_ball.hip (ball), snowgpu_range.hip (range).  Every one of these files includes this header, so a definition cannot drift from its declaration.
#ifdef __cplusplus
extern "C" {
#endif
// compact input: (x, y, z, intensity) float32 rows + channel bytes -> (x, y, z, intensity, channel) float32 rows
int sg_launch_expand_rows(const void *xyzi, const uint8_t *ch, void *rows, int64_t n, void *stream);
int sg_launch_sort(const void *rows, int dtype, const int64_t *frame_off, int n_frames, int64_t n_total,
                   int32_t *tile_hist, int32_t *tile_base, uint16_t *rank, uint8_t *ch8, int32_t *perm, int32_t *status,
                   int64_t max_tiles_per_frame, const double *lean_plane, double *lean_part, int32_t *tile_unsorted,
                   int32_t *frame_unsorted, void *srows, int identity_perm /* 1: perm also for sorted frames (debug tap) */,
                   int phase /* 1: histogram + per-frame scan; 2: second pass (sorted copy + perm of unsorted frames); 3: both */, void *stream);
// a caller-supplied permutation: the sorted copy by a plain gather, every frame flagged unsorted
int sg_launch_gather_rows(const void *rows, int dtype, const int64_t *frame_off, int n_frames, int64_t n_total, int64_t max_frame,
                          const int32_t *perm, void *srows, int32_t *frame_unsorted, int32_t *status, void *stream);
// direct == 1: the pass over all rows (dict hand-over to sg_launch_power); else list mode over class a->cls, received power in place
int sg_launch_beams(const SgBeamArgs *args, int dtype, int lmax, int direct, void *stream);
int sg_launch_power(const SgBeamArgs *args, int dtype, int lmax, void *stream, int plan_only /* 1: k_power_plan alone; 0: the kernels it feeds */,
                    void *ev_few /* hipEvent_t recorded behind k_power_few, or null */, int which /* 1: k_power_few alone, 2: k_power alone, 3: both */);
int sg_launch_tier_gather(const SgBeamArgs *args, void *stream);
int sg_launch_power_list(const SgBeamArgs *args, int dtype, int lmax, void *stream);
int sg_launch_huge(const SgBeamArgs *args, int dtype, void *stream);
// the scan of a later tier without LDS lists: hits go to the tier's hand-over buffer in scan order (its k_power sorts them as it loads)
int sg_launch_tier_scan(const SgBeamArgs *args, int dtype, int lmax, void *stream);
// class args->cls of the tier lists (capacity lmax) as a row kernel: G lanes per beam, scan + dict + received power in one pass
int sg_launch_rows(const SgBeamArgs *args, int dtype, int lmax, void *stream);
int sg_launch_segments(const int64_t *frame_off, int n_frames, const int32_t *tile_base, int64_t max_tiles, const int32_t *table_ids,
                       int n_las, int n_tables, int block, unsigned long long *tbl_cnt, unsigned long long *tbl_base, int32_t *seg_blk,
                       int64_t *seg_start, int32_t *seg_cnt, int32_t *seg_frame, int32_t *seg_n, int32_t *seg_of_blk,
                       int32_t *chunk_blk, const SgTable *tables, SgTable *resolved /* n_frames x n_las, or null */, void *stream);
int sg_launch_segments_small(const int64_t *frame_off, int n_frames, const int32_t *tile_base, int64_t max_tiles, const int32_t *table_ids,
                             int n_las, int n_tables, int block, int32_t *seg_blk, int64_t *seg_start, int32_t *seg_cnt, int32_t *seg_frame,
                             int32_t *seg_n, int32_t *seg_of_blk, int32_t *chunk_blk, const SgTable *tables, SgTable *resolved,
                             unsigned long long *zero, int64_t n_zero, void *stream);
int sg_beams_block(int lmax);
int sg_launch_resolve_tables(const SgTable *tables, int n_tables, const int32_t *table_ids, int64_t n, SgTable *out, void *stream);
// Packed result transfer (snowgpu_set_result_transfer): what the compaction writes instead of 5-column rows -- per kept row of frame f, at
// frame_off[f] + j: meta = source row (30 bits) | code << 30 (0 / 1 / 2 = label, 3 = label 0 whose column 4 keeps the input's channel value)
// and the output intensity (row dtype); the moved coordinates of the batch's label-2 rows form one list in output order (frame after
// frame: frame f's start = the sum of mv_counts of the frames before it), three values each, at mv.
struct SgPackOut {
    uint32_t *meta;
    void *inten;
    void *mv;
    int64_t *mv_counts;          // n_frames: kept label-2 rows
    int32_t *tile_mv, *tile_mv_base;   // scratch: n_frames x max_tiles
};
int sg_launch_compact(const void *rows, const void *srows, const int32_t *frame_unsorted, int dtype, const uint32_t *rec, const uint32_t *rec_q, const void *rng, const double *thr_poly, uint8_t *keep, const int32_t *perm,
                      const int64_t *frame_off, int n_frames, int64_t n_total, int32_t *tile_cnt,
                      int32_t *tile_base, void *out_rows, int32_t *out_src, int64_t *out_counts,
                      int64_t *out_stats, const unsigned long long *diff2, const SgFov *fov, int64_t max_tiles_per_frame,
                      const SgPackOut *pack /* or null: rows + out_src */, unsigned long long *tiles_done /* n_frames words, zero */, void *stream);
// the aligned finish (k_finish_aligned): every row at its input index + a keep flag; out_rows may be `rows` itself
int sg_launch_finish_aligned(const void *rows, const void *srows, const int32_t *frame_unsorted, int dtype, const uint32_t *rec, const uint32_t *rec_q, const void *rng,
                             const double *thr_poly, const int32_t *perm, const int64_t *frame_off, int n_frames, int32_t *tile_cnt, int32_t *tile_base,
                             void *out_rows, uint8_t *out_keep, int64_t *out_counts, int64_t *out_stats, const unsigned long long *diff2, const SgFov *fov,
                             int64_t max_tiles_per_frame, unsigned long long *tiles_done /* n_frames words, zero */, void *stream);
int sg_launch_crop_count(const void *rows, int dtype, const int64_t *frame_off, int n_frames, uint8_t *keep, int32_t *tile_cnt,
                         int32_t *tile_base, int64_t *out_counts, int64_t *stats_scratch, const SgFov *fov, int64_t max_tiles, void *stream);
int sg_launch_crop_scatter(const void *rows, int dtype, const uint8_t *keep, const double *gate /* or null */, const int64_t *frame_off, const int64_t *new_off,
                           int n_frames, const int32_t *tile_base, void *out_rows, int32_t *crop_src, int64_t max_tiles, void *stream);
// An input keep mask for the aligned entry.  Front end: the present rows (keep_in byte != 0) of every frame compacted, stably, into crows at
// the device-made offsets new_off[0 .. n_frames]; map = their frame-local input rows; the absent rows' keep bytes (and, out_rows != null,
// their rows) written.  Masked finish: sg_launch_finish_aligned on the compacted batch, every row written at in_off[f] + map[.] of the input.
// weather (optional, n_frames x 8 records, sg_weather.h): a frame whose snow gate is 0 contributes no row and keeps its keep bytes (keep_in may then be null).
int sg_launch_mask_front(const void *rows, int dtype, const uint8_t *keep_in, const double *weather, const int64_t *frame_off, int n_frames, void *out_rows /* null: in place */,
                         uint8_t *out_keep, int32_t *tile_cnt, int32_t *tile_base, int64_t *counts, int64_t *new_off, void *crows, int32_t *map,
                         int64_t max_tiles, void *stream);
int sg_launch_finish_aligned_masked(const void *crows, const void *srows, const int32_t *frame_unsorted, int dtype, const uint32_t *rec, const uint32_t *rec_q,
                                    const void *rng, const double *thr_poly, const int32_t *perm, const int64_t *c_off, const int64_t *in_off,
                                    const int32_t *map, int n_frames, int32_t *tile_cnt, int32_t *tile_base, void *out_rows, uint8_t *out_keep,
                                    int64_t *out_counts, int64_t *out_stats, const unsigned long long *diff2, const SgFov *fov, int64_t max_tiles_per_frame,
                                    unsigned long long *tiles_done /* n_frames words, zero */, void *stream);
// out_keep[i] = (keep_in ? keep_in[i] : 1) && the camera-FOV test of row i (out_keep may be keep_in)
int sg_launch_fov_mask(const void *rows, int dtype, int64_t n, const uint8_t *keep_in, uint8_t *out_keep, const SgFov *fov, void *stream);
// Dynamic radius outlier removal (sg_dror.h): out_keep[i] = row i is usable and has at least g->k_min neighbours, out_nb[i] (or null) = its
// neighbours, counted up to k_min.  The memset of the cell entries and four kernels.  Scratch: entry n_frames (g->cells + 1) words,
// cell_of n words, sorted 3 n values of the row dtype.  out_keep must not be keep_in: other rows' bytes are read while it is written.
struct SgDrorGrid;
int sg_launch_dror(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const struct SgDrorGrid *g,
                   uint32_t *entry, uint32_t *cell_of, void *sorted, uint8_t *out_keep, int32_t *out_nb, void *stream);
// Point-to-voxel grouping (sg_voxel.h; the definition: include/snowgpu.h): two memsets and eleven kernels.  Scratch: table n_frames g->cap
// words of 64 bits; slot_of and order n words, first n bytes; tile_cnt ceil(n / 1024) words and tile_base one more; fbase and m n_frames
// words; span n_frames g->max_voxels words.  out_voxel_of may be null.
struct SgVoxelGrid;
int sg_launch_voxelize(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const struct SgVoxelGrid *g,
                       unsigned long long *table, uint32_t *slot_of, uint8_t *first, uint32_t *order, int32_t *tile_cnt, int32_t *tile_base, int32_t *fbase,
                       int32_t *m, uint32_t *span, void *out_voxels, int32_t *out_coords, int32_t *out_num_points, int32_t *out_voxel_offsets,
                       int32_t *out_voxel_of, void *stream);
// Farthest point sampling (sg_fps.h; the definition: include/snowgpu.h): two kernels.  Scratch: sx, sy, sz, st in the rows' dtype and ssrc,
// sg_fps_scratch(n, n_frames) elements each.  out_points and out_dist may be null.
struct SgFpsRange;
int sg_launch_fps(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const struct SgFpsRange *range,
                  int32_t n_samples, int32_t n_features, void *sx, void *sy, void *sz, void *st, int32_t *ssrc, int32_t *out_index, void *out_points,
                  void *out_dist, int32_t *out_usable, void *stream);
// Sectorized, proposal-centric sampling (sg_fps_sectors.h; the definition: include/snowgpu.h): up to one memset and six kernels.  Scratch:
// sx, sy, sz, st and ssrc, sg_fpss_scratch(n, n_frames) elements each; sec n bytes; rec n_frames n_rois records of four doubles; tile
// n_frames sg_tiles(max_frame) n_sectors words; seg n_frames n_sectors words.  rois, out_points, out_dist, out_sector_of and out_reach2
// may be null.
int sg_launch_fps_sectors(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                          const struct SgFpsRange *range, int32_t n_samples, int32_t n_features, int32_t n_sectors, const void *rois, int32_t n_rois,
                          int32_t roi_features, double roi_margin, void *sx, void *sy, void *sz, void *st, int32_t *ssrc, int8_t *sec, void *rec,
                          int32_t *tile, int32_t *seg, int32_t *out_index, void *out_points, void *out_dist, int32_t *out_usable,
                          int32_t *out_offsets, int32_t *out_count, int8_t *out_sector_of, double *out_reach2, void *stream);
// Ball query around centres (sg_ball.h; the definition: include/snowgpu.h): a memset and four kernels.  Scratch: entry,
// sg_ball_entries(n_frames, g->cells) words; cell_of and ssrc, sg_ball_scratch(n) words; sx, sy, sz as many values of the rows' dtype.
// out_points may be null.
struct SgBallGrid;
int sg_launch_ball(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const struct SgFpsRange *range,
                   const struct SgBallGrid *g, int32_t n_centres, const void *centres, int32_t centre_features, int n_radii, const double *radii,
                   const int *n_samples, int32_t n_features, uint32_t *entry, uint32_t *cell_of, void *sx, void *sy, void *sz, int32_t *ssrc,
                   int32_t *out_index, int32_t *out_count, void *out_points, void *stream);
// Range-image projection (sg_range.h; the definition: include/snowgpu.h): up to three memsets and up to three kernels.  Scratch: key,
// n_frames H W 64-bit words (unused for a batch without a row).  ring is read with g->by_ring only; out_count may be null.
struct SgRangeGeom;
int sg_launch_range(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const int32_t *ring,
                    const struct SgRangeGeom *g, int32_t n_features, unsigned long long *key, void *out_image, int32_t *out_index,
                    int32_t *out_pixel_of, int32_t *out_count, void *stream);
// Nearest centres of every row (sg_nn.h; the definition: include/snowgpu.h): two kernels.  Scratch: entry, sg_nn_entries(n_frames,
// g->cells) words; box, sg_nn_boxes(n_frames) words; rec, sg_nn_records(n_frames, n_centres) records of the rows' dtype (SgNnRec).
// out_weight may be null.  Nothing is launched for a batch without a row.
struct SgNnGrid;
int sg_launch_nn(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const struct SgFpsRange *range,
                 const struct SgNnGrid *g, int32_t n_centres, const void *centres, int32_t centre_features, int k, uint32_t *entry, int32_t *box, void *rec,
                 int32_t *out_index, void *out_dist, void *out_weight, void *stream);
// Points in 3D boxes (sg_box.h; the definition: include/snowgpu.h): two kernels.  Scratch: rec, sg_box_records(n_frames, n_boxes) records;
// table, sg_box_table(n_frames, n_boxes) words.  pose_in, out_count, out_local and out_pose may be null.  A batch without a row runs the
// first kernel alone: the counts and the pose.
struct SgBoxRec;
int sg_launch_box(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, int32_t n_boxes,
                  const void *boxes, int32_t box_features, const double *pose_in, struct SgBoxRec *rec, unsigned long long *table, int32_t *out_box_of,
                  int32_t *out_count, void *out_local, double *out_pose, void *stream);
// RoI point pooling (sg_roipool.h; the definition: include/snowgpu.h): five kernels.  Scratch: rec and table as above for n_rois; run_cnt,
// sg_roi_table(n_frames, max_frame, n_rois) int32.  ew: 3 host doubles.  pose_in, out_points, out_local and out_pose may be null.  A batch
// without a row runs the first and the last kernel.
int sg_launch_roipool(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                      int32_t n_rois, const void *rois, int32_t roi_features, const double *ew, int32_t n_samples, int32_t num_features,
                      const double *pose_in, struct SgBoxRec *rec, unsigned long long *table, int32_t *run_cnt, int32_t *out_index, int32_t *out_count,
                      void *out_points, void *out_local, double *out_pose, void *stream);
// Its first four kernels alone: count (n_frames, n_rois) and the first n_slots members of every roi in row order in index (n_frames, n_rois,
// n_slots), the slots behind the count left as they were; for a batch without a row the first kernel alone, count not written.
int sg_launch_roi_members(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                          int32_t n_rois, const void *rois, int32_t roi_features, const double *ew, int32_t n_slots, const double *pose_in,
                          struct SgBoxRec *rec, unsigned long long *table, int32_t *run_cnt, int32_t *out_index, int32_t *out_count, double *out_pose,
                          void *stream);
// RoI-aware voxel pooling (sg_roiaware.h; the definition: include/snowgpu.h): sg_launch_roi_members into `list` with n_slots = cap, then
// k_roiaware_bucket and, for what was asked, k_roiaware_pool and k_roiaware_index.  Scratch of its own: rec, table and run_cnt as above;
// list and sorted, sg_roiaware_list(n_frames, n_rois, cap) int32 each (at F = 16, M = 128, P = 8192: 67 MB each); offset,
// sg_roiaware_offsets(n_frames, n_rois, G) int32.  grid: 3 host ints.  features, pose_in and every output but roi_count and count may be
// null.  A batch without a row runs the first kernel, one that writes the zero counts, and the last two.
int sg_launch_roiaware(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                       int32_t n_rois, const void *rois, int32_t roi_features, const double *ew, const int32_t *grid, int32_t max_points, int32_t cap,
                       const float *features, int32_t channels, const double *pose_in, struct SgBoxRec *rec, unsigned long long *table, int32_t *run_cnt,
                       int32_t *list, int32_t *sorted, int32_t *offset, int32_t *out_roi_count, int32_t *out_count, int32_t *out_index, float *out_max,
                       int32_t *out_argmax, float *out_avg, double *out_pose, void *stream);
// Rotated box IoU and NMS (sg_iou.h; the definition: include/snowgpu.h): three kernels each.  Scratch: rec, sg_iou_records() doubles for
// n_frames (M + B) boxes (the IoU) or n_frames B (NMS); order, n_frames B; n_cand, n_frames.  The poses and every output but the NMS
// index and count may be null (the IoU needs one output).
int sg_launch_iou(int n_frames, int32_t M, const void *boxes_a, int32_t a_features, int32_t B, const void *boxes_b, int32_t b_features, int dtype, int mode,
                  const double *pose_a, const double *pose_b, double *rec, void *out_iou, int32_t *out_best, void *out_best_iou, void *stream);
int sg_launch_nms(int n_frames, int32_t B, const void *boxes, int32_t box_features, const void *scores, int dtype, int mode, double iou_thresh,
                  double score_thresh, int32_t post_max, const double *pose_in, double *rec, int32_t *order, int32_t *n_cand, int32_t *out_index,
                  int32_t *out_count, void *out_boxes, void *out_scores, uint8_t *out_kept, void *stream);
// Proposal target sampling (sg_targets.h; the definition: include/snowgpu.h): one kernel, no scratch.  cfg: host.  pose_in, out_pose and
// out_gt_local may be null.
struct SgTargetCfg;
int sg_launch_sample_rois(const struct SgTargetCfg *cfg, int n_frames, int32_t n_rois, const void *rois, int32_t roi_features, const void *overlap,
                          const int32_t *assign, int32_t n_gt, const void *gt, int32_t gt_features, int dtype, uint64_t seed, const uint64_t *d_step,
                          const double *pose_in, int32_t *out_index, void *out_rois, void *out_roi_iou, int32_t *out_gt_index, void *out_gt_of_rois,
                          uint8_t *out_reg_valid, void *out_cls_label, int32_t *out_segments, int32_t *out_class_count, double *out_pose,
                          void *out_gt_local, void *stream);
// Anchor target assignment (sg_anchors.h; the definition: include/snowgpu.h): four kernels.  cfg: host.  recs: n_frames x n_gt records of
// 48 bytes, top: n_frames x n_gt words, blk: n_frames x sg_anchors_groups(n_anchors) x 3 int32, all scratch.  out_iou may be null.
struct SgAnchorCfg;
int sg_launch_assign_anchors(const struct SgAnchorCfg *cfg, int n_frames, int32_t n_anchors, const void *anchors, int32_t anchor_features,
                             const int32_t *anchor_class, int32_t n_gt, const void *gt, int32_t gt_features, int dtype, void *recs,
                             unsigned long long *top, int32_t *blk, int32_t *out_label, int32_t *out_gt_index, int32_t *out_count,
                             int32_t *out_gt_count, void *out_iou, void *stream);
// Centre heatmap targets (sg_centers.h; the definition: include/snowgpu.h): two kernels.  cfg: host.  recs: n_frames x n_gt records of 24 bytes,
// scratch.
struct SgCenterCfg;
int sg_launch_assign_centers(const struct SgCenterCfg *cfg, int n_frames, int32_t n_gt, const void *gt, int32_t gt_features, int dtype, void *recs,
                             float *out_heatmap, int32_t *out_gt_index, int32_t *out_ind, uint8_t *out_mask, void *out_offset, int32_t *out_radius,
                             int32_t *out_count, uint8_t *out_state, void *stream);
// Ground-truth object paste (sg_paste.h; the definition: include/snowgpu.h): three kernels, the first only with a keep mask.  groups and ew
// (3 doubles): host.  table: sg_paste_table() int32, frames: sg_paste_frames() records, grid: sg_paste_grid() words, all scratch.  keep,
// pose_in, out_source and out_pose may be null.
struct SgPasteGroups;
struct SgPasteFrame;
int sg_launch_paste(const void *rows, int dtype, int64_t n_total, int64_t max_frame, const int64_t *off, int n_frames, const uint8_t *keep, int32_t n_gt,
                    const void *gt, int32_t gt_features, const double *pose_in, const void *bank_points, const int64_t *bank_off, const void *bank_boxes,
                    const double *bank_pose, const int32_t *class_off, const struct SgPasteGroups *groups, const double *ew, uint64_t seed,
                    const uint64_t *d_step, int32_t *table, struct SgPasteFrame *frames, unsigned long long *grid, void *out_rows, uint8_t *out_keep, void *out_gt, int32_t *out_object,
                    int32_t *out_state, int32_t *out_source, int32_t *out_count, double *out_pose, void *stream);
// Scene transforms (sg_scene.h; the definition: include/snowgpu.h): two kernels, sg_launch_box in front of them when there is a local part, a
// row and no box_of.  cfg: host.  Scratch: rowrec, sg_scene_rowrecs() doubles; tries, sg_scene_tries() doubles (used without out_tries);
// box_rec, box_table and box_of_own (n_total int32) for sg_launch_box.  keep, pose_in, box_of, out_pose and out_tries may be null.
struct SgSceneCfg;
int sg_launch_scene(const void *rows, int dtype, int64_t n_total, int64_t max_frame, const int64_t *off, int n_frames, const uint8_t *keep, int32_t B,
                    const void *gt, int32_t Cb, const double *pose_in, const struct SgSceneCfg *cfg, uint64_t seed, const uint64_t *d_step, const int32_t *box_of,
                    struct SgBoxRec *box_rec, unsigned long long *box_table, int32_t *box_of_own, double *tries, double *rowrec, void *out_rows, uint8_t *out_keep,
                    void *out_gt, double *out_world, int32_t *out_state, int32_t *out_tried, double *out_local, double *out_pose, double *out_tries,
                    void *stream);
#ifdef __cplusplus
}
#endif
