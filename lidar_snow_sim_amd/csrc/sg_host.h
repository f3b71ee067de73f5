// sg_host.h -- what the five host translation units of libsnowgpu.so share: the context, the description of one batch on the
// device, the error macros, the guard of the host-pointer entries and the functions the parts call in each other.
//   snowgpu_api.cpp    context, settings, tables, sampler, profile hooks
//   snowgpu_device.cpp the *_batch_device* entries, the plane estimate, the FOV mask, the weather draw (device pointers; arguments and
//                      refusals: sg_device_args.h)
//   snowgpu_stages.cpp the stage entries on device pointers, from the outlier filter to the anchor targets (likewise sg_device_args.h)
//   snowgpu_batch.cpp  the launch sequence of one batch (run_batch)
//   snowgpu_host.cpp   every entry that takes host pointers (uploads, the chunk pipeline, downloads)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/snowgpu.h"
#include "sg_common.h"
#include "sg_prepass.h"
#include "sg_plane.h"
#include "sg_assemble.h"
#include "sg_device_args.h"

#pragma GCC visibility push(hidden)      // nothing below is part of the library's ABI

struct DeviceTable {
    SgEntry *entries = nullptr;
    uint32_t *bin_start = nullptr;
    uint32_t *bin_q = nullptr;
    uint32_t *bin_qs = nullptr;          // step-major twin of bin_q (sg_range_index.h), or null: a bin too long for its 16-bit counts
    SgTable desc{};
};

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // elements
    int ensure(size_t n)
    {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = n + n / 4 + 64;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess) return (int)e;
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// (default visibility: the type is named, opaquely, by include/snowgpu.h)
struct __attribute__((visibility("default"))) snowgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // side streams of one batch; each forks from the caller's stream and joins back before the compaction
    hipStream_t aux = nullptr;            // table resolve + segment order (next to the prepass), later k_power of the first pass
    hipStream_t aux2 = nullptr;           // noise-threshold prepass (only the compaction needs its result)
    hipStream_t aux3 = nullptr;           // later capacity tiers beyond the first of them
    int32_t *tier_hint_h = nullptr, *tier_hint_d = nullptr;   // beams per later tier of a recent batch, written by the device into page-locked host memory
    hipEvent_t ev_fork0 = nullptr, ev_join0 = nullptr;   // prepass
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;     // resolve / segments
    hipEvent_t ev_fp = nullptr, ev_join2 = nullptr;       // the pass over all rows (and its plan) done -> k_power_few / k_power
    hipEvent_t ev_few = nullptr;                          // k_power_few done -> (large batches) the tiers and the prepass
    hipEvent_t ev_lists = nullptr, ev_join3 = nullptr;   // tier lists built -> later tiers
    std::string err;
    std::vector<DeviceTable> tables;
    SgTable *d_tables = nullptr;      // device mirror of the descriptors
    size_t d_tables_cap = 0;
    bool tables_dirty = true;
    uint32_t max_flakes = 0;          // largest uploaded table (drives the capacity-tier choice)
    SgLasers h_las{};
    SgLasers *d_las = nullptr;
    double *d_rgrid = nullptr;
    int32_t *d_status = nullptr;      // 8 ints
    SgFov fov{};                      // camera-FOV crop applied by the compaction (snowgpu_set_fov)
    int fov_pre = 0;                  // also crop the INPUT rows before anything else (host entries; precompute.py:96-99)
    DevBuf<uint8_t> rows_crop;
    DevBuf<int32_t> crop_src, crop_out_src;
    DevBuf<int64_t> crop_counts, crop_off, crop_stats;
    // dynamic radius outlier removal (snowgpu_dror_mask_device): cell entries, the cell of every row, x y z sorted by cell
    DevBuf<uint32_t> dror_entry, dror_cell;
    DevBuf<uint8_t> dror_sorted;
    // point-to-voxel grouping (snowgpu_voxelize_device): the frames' tables of open cells, per row its slot (then its voxel), whether it opens
    // a cell and the row indices sorted by voxel, the opening rows per tile and per frame, the voxels' spans
    DevBuf<unsigned long long> vox_table;
    DevBuf<uint32_t> vox_slot, vox_order, vox_span;
    DevBuf<uint8_t> vox_first;
    DevBuf<int32_t> vox_tile_cnt, vox_tile_base, vox_fbase, vox_m;
    // farthest point sampling (snowgpu_fps_device): the usable rows of every frame compacted in input order -- x, y, z and the running
    // minimum t as four arrays in the rows' dtype -- and their source rows
    DevBuf<uint8_t> fps_x, fps_y, fps_z, fps_t;
    DevBuf<int32_t> fps_src;
    // sectorized sampling (snowgpu_fps_sectors_device) compacts every (frame, sector) into the same five arrays; beside them the sector
    // byte of every row, the rois' records (four doubles each), the tile counts / bases and the segments' places
    DevBuf<int8_t> fpss_sec;
    DevBuf<double> fpss_roi;
    DevBuf<int32_t> fpss_tile, fpss_seg;
    // ball query (snowgpu_ball_query_device): the cell lists of every frame -- first positions, the cell of every row -- and the usable
    // rows sorted by cell: x, y, z as three arrays in the rows' dtype and their source rows
    DevBuf<uint32_t> ball_entry, ball_cell;
    DevBuf<uint8_t> ball_x, ball_y, ball_z;
    DevBuf<int32_t> ball_src;
    // range image (snowgpu_range_image_device): one key per pixel of every frame's image
    DevBuf<unsigned long long> range_key;
    // nearest centres (snowgpu_nearest_centres_device): the cell lists of every frame's centres -- first positions and the occupied box --
    // and the usable centres sorted by cell, one record (x, y, z, centre number) each
    DevBuf<uint32_t> nn_entry;
    DevBuf<int32_t> nn_box;
    DevBuf<uint8_t> nn_rec;
    // points in boxes (snowgpu_points_in_boxes_device): one record of eight doubles per box, and per frame the bit table of its cells
    DevBuf<double> box_rec;
    DevBuf<unsigned long long> box_table;
    // RoI point pooling (snowgpu_roi_point_pool_device): the records and the bit table of the enlarged rois, as above, and one int32 per
    // (frame, run of 512 rows, roi): the roi's members in the run, then in the runs before it
    DevBuf<double> roi_rec;
    DevBuf<unsigned long long> roi_table;
    DevBuf<int32_t> roi_runs;
    // RoI-aware voxel pooling (snowgpu_roi_voxel_pool_device): the same three of its own, a roi's first roi_capacity members in row order
    // and grouped by voxel (F M P int32 each: 67 MB each at F = 16, M = 128, P = 8192), and where every voxel's rows begin (F M G int32)
    DevBuf<double> rv_rec;
    DevBuf<unsigned long long> rv_table;
    DevBuf<int32_t> rv_runs, rv_list, rv_sorted, rv_offset;
    // box IoU and NMS (snowgpu_boxes_iou_device, snowgpu_nms_device): one record of nine doubles per box; the ranking and its length
    DevBuf<double> iou_rec;
    DevBuf<int32_t> nms_order, nms_cand;
    // anchor target assignment (snowgpu_assign_anchors_device): one record of six doubles per gt, the bits of its largest overlap, and per
    // (frame, workgroup of 256 anchors) the three label counts
    DevBuf<double> anchor_rec;
    DevBuf<unsigned long long> anchor_top;
    DevBuf<int32_t> anchor_blk;
    // centre heatmap targets (snowgpu_assign_centers_device): one record of three doubles per gt
    DevBuf<double> center_rec;
    // object paste (snowgpu_paste_objects_device): one int32 per (frame, run of 512 rows) -- the run's absent rows, then those of the runs
    // before it --, one SgPasteFrame (bytes) per frame: the pasted slots' bases and enlarged boxes, and one word per (frame, grid cell):
    // the pasted boxes that can reach the cell (32 KB a frame)
    DevBuf<int32_t> paste_runs;
    DevBuf<uint8_t> paste_frames;
    DevBuf<unsigned long long> paste_grid;
    // scene transforms (snowgpu_transform_scene_device): ten doubles per box for the row kernel, eight per (box, try) when the caller takes
    // no d_out_tries, and -- when the stage makes box_of itself -- the records and the bit table of points in boxes and one int32 per row
    DevBuf<double> scene_rowrec, scene_tries, scene_box_rec;
    DevBuf<unsigned long long> scene_box_table;
    DevBuf<int32_t> scene_box_of;
    // scratch shared by every batch
    DevBuf<int32_t> tile_hist, tile_base, perm, ctile_cnt, ctile_base, table_ids, out_src;
    DevBuf<uint8_t> srows;            // channel-sorted copy of the frames whose rows did not come channel-sorted (firing order)
    DevBuf<int32_t> tile_unsorted, frame_unsorted;
    DevBuf<unsigned long long> seg_tbl_cnt, seg_tbl_base;
    DevBuf<int32_t> seg_blk, seg_cnt, seg_frame, seg_n, seg_of_blk;
    DevBuf<int64_t> seg_start;
    DevBuf<uint32_t> rec, rec_q;      // result records: one per sorted position / per queue slot
    DevBuf<uint8_t> rng;              // range of every simulated beam, per sorted position, in the row dtype
    DevBuf<uint32_t> dq;              // dict queue of the first pass (blocked SoA of 32-bit words: sg_queue.h)
    DevBuf<int32_t> dq_g;
    DevBuf<uint16_t> dq_sc;
    DevBuf<unsigned long long> qn;    // per region: front | back << 32
    DevBuf<int2_t> pw_items;          // work items of k_power
    DevBuf<double> ov;                // overflow slots of the pass over all rows (SG_OV_STRIDE doubles per sorted position)
    DevBuf<uint16_t> ov_sc;
    DevBuf<int32_t> tier_list, tier_sparse, tbase, redo_list;
    DevBuf<double> tq[SG_MAX_CLASSES];        // dict hand-over buffers of the list-mode tiers
    DevBuf<uint16_t> tq_sc[SG_MAX_CLASSES];
    DevBuf<double> h_lists;           // global-list tier: per-lane lists
    int64_t tier_cap_override = 0;    // tests: SNOWGPU_TIER_CAP=<entries> shrinks the hand-over buffers (in-place fallback runs)
    int first_tier_override = 0;      // tests: SNOWGPU_FIRST_TIER=4|8|16|63
    int few = 2;                      // SNOWGPU_FEW=0..3: beams with up to this many flakes go through k_power_few (0: all through k_power)
    int heavy_tail = -1;              // SNOWGPU_HEAVY_TAIL=0 / 1: never / always the long-tail order of the received-power phase (default: by the last batches' tier counts)
    int tier_rows = -1;               // SNOWGPU_TIER_ROWS=1 / 0: always / never the later tiers as row kernels (snowgpu_rows.hip: G lanes per beam; default: small batches only)
    hipStream_t lane_stream[3] = {nullptr, nullptr, nullptr};     // snowgpu_lane_stream: one per priority level, made on demand
    int stats_early = -1;             // SNOWGPU_STATS_EARLY=0 / 1: the prepass' per-tile statistics inside the sort's first pass / as a kernel of their own on the prepass stream (default: the latter for batches of more than 16 frames)
    int prepass_with_few = -1;        // SNOWGPU_PREPASS_WITH_FEW=0 / 1: never / always start the prepass beside k_power_few (default: long-tail batches only)
    bool serial = false;              // experiments: SNOWGPU_SERIAL=1 keeps every kernel on the caller's stream (pure kernel times)
    DevBuf<int32_t> chunk_blk;
    DevBuf<uint16_t> rank;
    DevBuf<uint8_t> keep, rows_in, rows_out;
    DevBuf<int64_t> frame_off, out_counts, out_stats;
    DevBuf<double> thr_poly, plane, dbg_rj, dbg_ratio, user_thr, out_thr;
    DevBuf<int32_t> user_perm;
    DevBuf<int32_t> dbg_count;
    DevBuf<SgTable> frame_tables;
    SgPrepassScratch prepass{};
    // ground plane estimated on the device when a batch brings neither a plane nor a polynomial (planes.py:12-50)
    SgPlaneScratch plane_scr{};
    SgPlaneParams plane_par{SG_PLANE_REFERENCE, 1024, 5, 0, -1.55};
    DevBuf<double> plane_est, wet_plane_est;
    DevBuf<int32_t> plane_info;
    int64_t resident_rows = -1;       // rows snowgpu_prepass_stats left in rows_in (and their dtype): a following snowgpu_augment_batch with
    int resident_dtype = -1;          // rows == NULL computes on them instead of uploading the same rows again ...
    std::vector<int64_t> resident_off;   // ... if it names the same frames (frame offsets compared entry by entry)
    DevBuf<int32_t> stats_hist;       // snowgpu_prepass_stats: n_frames x 50 x 2555
    DevBuf<double> stats_rec;
    // fused snow + wet (snowgpu_augment_wet_batch*): the snowfall result stays here
    DevBuf<uint8_t> snow_rows;
    DevBuf<int32_t> snow_src, wet_flags;
    DevBuf<int64_t> snow_counts, wet_counts;
    DevBuf<double> wet_rows, wet_plane;
    // measurement hooks (snowgpu_profile_begin / _end)
    std::vector<hipEvent_t> ev_start, ev_stop;
    int ev_used = 0;
    bool prof = false;
    hipStream_t prof_stream = nullptr;
    int exact_math = 0;
    // Host-pointer batches run as a pipeline of chunks (whole frames, about pipe_rows rows each); see host_batch_pipelined.
    snowgpu_ctx *root = nullptr;          // set in a lane: the context whose tables, lasers and settings it computes with
    std::vector<snowgpu_ctx *> lanes;     // further compute lanes of the host pipeline (own stream, events and scratch), made on first use
    int pipe_lanes = 2;                   // SNOWGPU_PIPE_LANES: chunks computing side by side (lane 0 is the context itself).  Downloads are the
                                          // runtime's copy, i.e. the DMA engine: a copy kernel of ours was measured (scripts/probe/chain_probe.hip) --
                                          // while ANY kernel writes host memory every kernel boundary on the device waits for its outstanding
                                          // writes (3 us per dependent launch become 17 - 41 us) -- and dropped
    // The small arrays of a host-pointer batch cross the link as ONE block each way, through page-locked mailboxes: frame
    // offsets | table ids | planes or polynomials going up, status | counts | statistics | polynomials coming back (a
    // single sweep otherwise spends a quarter of its time on seven tiny dependent copies).
    char *mail_up_h = nullptr, *mail_dn_h = nullptr;
    size_t mail_up_cap = 0, mail_dn_cap = 0;
    DevBuf<uint8_t> mail_up_d, mail_dn_d;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    std::vector<hipEvent_t> pipe_ev;      // [2 c] chunk c has been uploaded, [2 c + 1] computed
    DevBuf<int64_t> pipe_off;         // chunk-local frame offsets of every chunk, concatenated
    DevBuf<int32_t> pipe_status;      // 8 status words per chunk
    int64_t pipe_rows = (int64_t)3 << 19;   // snowgpu_set_pipeline; 0: no pipeline (one upload, one download)
    std::vector<double> wet_lines;    // snowgpu_set_wet_lines: consumed by the next snowgpu_wet_ground_batch
    DevBuf<double> d_wet_lines;
    int wet_estimation = 0;           // snowgpu_set_wet_estimation: 0 'linear', 1 'poly' (seeded RANSAC on the device)
    uint64_t wet_seed = 0;
    DevBuf<double> wet_fit;           // n_frames x 8: the curves the last wet-ground call fitted (snowgpu_wet_last_fit)
    int wet_fit_frames = 0;
    int32_t h_status[8] = {0, -1, 0, 0, 0, 0, 0, 0};   // status words of the last host-pointer batch (tier counts summed over chunks)
    // Packed result transfer of the pipelined host entry (snowgpu_set_result_transfer): per kept row 4 + 4 (8 for float64 rows) bytes come
    // down the link, the moved coordinates of scattered rows apart; host threads copy x, y, z from the caller's input rows.
    int result_mode = 0;                  // 0: whole rows (+ source indices) over the link; 1: packed
    int asm_threads = 0;                  // host threads of the packed mode (0: the CPUs this process may use, minus two, at most 8)
    DevBuf<uint32_t> pk_meta;
    DevBuf<uint8_t> pk_int, pk_mv;
    DevBuf<int64_t> pk_mvcnt;
    DevBuf<int32_t> pk_tile_mv, pk_tile_mv_base;      // per lane
    char *st_pk = nullptr;                // page-locked staging: meta | intensities | moved coordinates | counts
    size_t st_pk_cap = 0;
    std::vector<hipEvent_t> pk_ev;        // [2 c] counts of chunk c on the host, [2 c + 1] its packed data
    AsmPool *pool = nullptr;
    double pk_times[4] = {0, 0, 0, 0};    // last packed call: ms until all enqueued, all downloads landed, all rows assembled; host bytes copied
    // The caller fits the noise threshold (snowgpu_set_threshold_callback): page-locked staging for the device half of the prepass --
    // histograms | records | status words per group | the polynomials the callback writes -- and one event per group
    // compact input of the call in flight (snowgpu_augment_batch_compact): the channel bytes; `rows` then are (x, y, z, intensity) float32
    const uint8_t *in_channels = nullptr;
    DevBuf<uint8_t> rows_c4, rows_ch;     // their device staging (16 + 1 bytes per row), expanded into rows_in by k_expand_rows
    snowgpu_threshold_fn thr_fn = nullptr;
    void *thr_user = nullptr;
    char *thr_stage = nullptr;
    size_t thr_stage_cap = 0;
    std::vector<hipEvent_t> thr_ev;
};

#define HIPCHK(ctx, call)                                                                         \
    do {                                                                                          \
        hipError_t e__ = (call);                                                                  \
        if (e__ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                      \
            return SNOWGPU_E_HIP;                                                                 \
        }                                                                                         \
    } while (0)

#define ENSURE(ctx, buf, n)                                                                       \
    do {                                                                                          \
        if ((buf).ensure(n)) { (ctx)->err = "hipMalloc failed for " #buf; return SNOWGPU_E_HIP; } \
    } while (0)

static inline int fail(snowgpu_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

// the fork / join events of one launch sequence (a context or a lane): made by init_streams / ensure_pipeline, destroyed with the context
static inline std::array<hipEvent_t *, 9> lane_events(snowgpu_ctx *c)
{
    return {&c->ev_fork0, &c->ev_join0, &c->ev_fork, &c->ev_join, &c->ev_join2, &c->ev_lists, &c->ev_join3, &c->ev_few, &c->ev_fp};
}

// Declared by every host-pointer entry before its first enqueue that names caller memory or a local (locals a copy names are declared
// ahead of it: they outlive it).  No exit may leave DMA or a host thread touching such memory, so whatever path leaves the entry drains:
// the packed pool idle, then -- pipe: the chunk pipeline ran -- s_h2d and every lane's stream, ctx->stream, s_d2h synchronised; the first
// error is returned.  The success path calls drain() itself, where it needs the results; every early return drains in the destructor.
struct HostCall {
    snowgpu_ctx *ctx;
    bool pipe = false;
    bool drained = false;
    hipError_t drain()
    {
        drained = true;
        hipError_t first = hipSuccess;
        auto sync = [&first](hipStream_t s) { if (s) { hipError_t e = hipStreamSynchronize(s); if (first == hipSuccess) first = e; } };
        if (pipe) {
            if (ctx->pool) ctx->pool->wait_idle();
            sync(ctx->s_h2d);
            for (snowgpu_ctx *ln : ctx->lanes) sync(ln->stream);
        }
        sync(ctx->stream);
        if (pipe) sync(ctx->s_d2h);
        return first;
    }
    ~HostCall() { if (!drained) (void)drain(); }
};

struct BatchDev {
    int n_frames;
    int64_t n_total;
    int64_t max_frame;   // rows of the largest frame (host knowledge; n_total is a safe bound)
    int64_t uniform_rows = 0;   // > 0 when the host knows that all frames have this many rows
    const int64_t *frame_off;
    const void *rows;
    int dtype;
    const int32_t *table_ids;
    double beam_div_deg;
    const double *thr_poly;   // may be null -> prepass with plane
    const double *plane;
    double noise_floor;
    const int32_t *perm;      // may be null -> device sort
    void *out_rows;
    int32_t *out_src;
    uint8_t *out_keep = nullptr;   // non-null: the aligned finish -- every row at its input index in out_rows (which may be `rows`), its keep flag here; out_src unused
    // Masked aligned call (snowgpu_mask.hip): `rows` / `frame_off` are the COMPACTED batch in context scratch, n_total and max_frame only upper
    // bounds of it; the aligned finish writes row j of compacted frame f to out_rows / out_keep at mask_in_off[f] + mask_map[frame_off[f] + j].
    const int32_t *mask_map = nullptr;
    const int64_t *mask_in_off = nullptr;
    const double *weather = nullptr;   // per-frame weather records (snowgpu_augment_weather_batch_device_aligned): a frame gated out of the snowfall
                                       // stage arrives here empty, and the prepass reports no missing ground for it
    int64_t *out_counts;
    int64_t *out_stats;
    double *out_thr_poly;     // may be null
    int32_t *status;
    hipStream_t stream;
    // debug tap
    int32_t *dbg_count = nullptr;
    double *dbg_rj = nullptr, *dbg_ratio = nullptr;
    int dbg_cap = 0;
    int32_t *perm_out = nullptr;   // where the permutation actually used lives (device)
    bool no_fov = false;           // debug tap: never crop
    bool want_perm = false;        // the caller reads perm_out back: the sort writes the permutation of channel-sorted frames too
    SgPackOut *pack = nullptr;     // packed result transfer: the compaction writes these instead of out_rows / out_src (tile scratch filled in here)
    bool serial = false;           // every kernel on `stream`: no fork / join events (chunks of the host pipeline)
    bool defer_thr = false;        // the caller fits the noise threshold itself while the per-beam kernels run (snowgpu_set_threshold_callback):
                                   // run_batch stops ahead of the compaction, launches no prepass; run_compaction finishes with b.thr_poly
};

int run_batch(snowgpu_ctx *ctx, BatchDev &b);                 // snowgpu_batch.cpp
int run_compaction(snowgpu_ctx *ctx, BatchDev &b);
int status_to_error(snowgpu_ctx *ctx, const int32_t st[8]);
int node_of_device(int device);                               // snowgpu_host.cpp
SgFov make_fov(const double *v2c, const double *r0, const double *p2, int img_h, int img_w);      // snowgpu_api.cpp
// snowgpu_device.cpp: the SgWetParams of one wet-ground call; take_lines: consume what snowgpu_set_wet_lines left (uploaded and waited for on st)
int wet_settings(snowgpu_ctx *ctx, const SgWetScalars &w, int n_frames, bool take_lines, hipStream_t st, SgWetParams *wp);

#pragma GCC visibility pop

// snowgpu_weather.hip
struct SgWeatherDraw;
extern "C" int sg_launch_draw_weather(const SgWeatherDraw *p, int n_frames, uint64_t seed, const uint64_t *d_step, const int32_t *d_set_ids,
                                      int32_t *d_table_ids, double *d_weather, void *stream);
// flags[f] = 2 where frame f's wet gate is off, else 1: the wet flags of a batch without a row
extern "C" int sg_launch_weather_flags(const double *d_weather, int n_frames, int32_t *d_flags, void *stream);

// snowgpu_tables.hip, snowgpu_sampler.hip
extern "C" int sg_table_index(const SgEntry *entries, const uint32_t *start, uint32_t *q, uint32_t *qs /* or null */, int qs_steps, double qs_step_m, void *stream);
extern "C" int sg_file_table_stage_a(const double *d_xyr, int64_t k, SgEntry *fl, int32_t *b0, int32_t *span, uint32_t *count,
                                     uint32_t *start, uint32_t *fill, int32_t *misc, void *stream);
extern "C" int sg_file_table_stage_b(int64_t k, const SgEntry *fl, const int32_t *b0, const int32_t *span, const uint32_t *start,
                                     uint32_t *fill, SgEntry *tmp, SgEntry *entries, void *stream);
extern "C" int sg_table_dump(const SgEntry *entries, uint32_t n_entries, double *d_out, void *stream);
extern "C" int sg_sample_table(double occupancy, double scale_mm, double R0, uint64_t seed, int64_t n_cand, double *d_xyr,
                               int64_t cap, int64_t *n_rows, void *stream);
