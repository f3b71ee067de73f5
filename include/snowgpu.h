/*
 * snowgpu.h -- C ABI of libsnowgpu.so, the MI355X (gfx950) snowfall-augmentation engine.
 *
 * This is the drop-in boundary for ONE hot path of SysCV/LiDAR_snow_sim: the per-beam snow
 * scattering simulation behind
 *     tools/snowfall/simulation.py::augment                 (simulation.py:427-544)
 *       -> process_single_channel                           (simulation.py:50-194)
 *       -> get_occlusions / compute_occlusion_dict          (simulation.py:298-424, :231-295)
 *       -> tools/snowfall/geometry.py                       (geometry.py:14-223)
 *       -> received_power / xsi                             (simulation.py:547-569)
 * plus the noise-threshold prepass it shares with the wet-ground model
 *     tools/wet_ground/augmentation.py::estimate_laser_parameters (augmentation.py:195-266)
 * and the wet-ground intensity model itself
 *     tools/wet_ground/augmentation.py::ground_water_augmentation (augmentation.py:25-161).
 *
 * The reference is pure Python/NumPy and has no FFI; what a maintainer binds instead of its
 * Python loops is shown in INTEGRATION.md (a ctypes stub).  All pointers are caller-owned,
 * little-endian, C-order.  No C++ exception crosses this boundary: every entry point returns
 * an int status (0 = ok) and snowgpu_last_error() returns a message for the last failure.
 *
 * Conventions shared by every entry point
 *   rows      : (x, y, z, intensity, channel) per point, float32 (dtype 0) or float64 (dtype 1)
 *               -- the STF .bin row the reference reads (precompute.py:78) and returns
 *   frames    : a batch is n_frames frames concatenated; frame f owns rows
 *               [frame_offsets[f], frame_offsets[f+1])
 *   labels    : output column 4 is the reference's label: 0 unchanged, 1 attenuated,
 *               2 scattered (simulation.py:160, :174, :192); rows whose channel is not an
 *               integer in [0, n_lasers) are never simulated and keep their channel value there
 *               (simulation.py:480-483, quirk Q5)
 *   order     : output rows are in the reference's order -- sorted by channel
 *               (simulation.py:447), STABLY here (the reference's argsort is unstable, so its
 *               within-channel order is implementation-defined); out_src returns, per output
 *               row, the index of the input row it came from (frame-local)
 *   aligned   : snowgpu_augment_batch_device_aligned returns the same rows in the INPUT's order instead -- every input row
 *               at its own index, one keep flag per row (1: the reference returns the row) --, a result whose shape does not
 *               depend on the data and which a consumer on the same stream (or in the same HIP graph) reads without the host;
 *               snowgpu_wet_ground_batch_device_aligned / snowgpu_augment_wet_batch_device_aligned do the same for the wet-ground
 *               model and for the snowfall + wet-ground chain
 */
#ifndef SNOWGPU_H
#define SNOWGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct snowgpu_ctx snowgpu_ctx;

enum {
    SNOWGPU_OK = 0,
    SNOWGPU_E_INVALID = 1,      /* bad argument (null pointer, negative size, unknown table id) */
    SNOWGPU_E_HIP = 2,          /* a HIP runtime call failed; see snowgpu_last_error */
    SNOWGPU_E_TABLE = 3,        /* particle table the reference could not process either
                                   (disk containing the origin, non-finite row) */
    SNOWGPU_E_RANGE = 4,        /* a simulated point has range >= ~120 m: the reference raises
                                   IndexError there (simulation.py:146-149, quirk Q6) */
    SNOWGPU_E_CHANNELS = 5,     /* channel column holds values other than integers in [0, 255]
                                   and no explicit permutation was supplied */
    SNOWGPU_E_OVERFLOW = 6,     /* more than SNOWGPU_MAX_FLAKES_GLOBAL flakes intersect one beam */
    SNOWGPU_E_GROUND = 7,       /* fewer than 3 ground points: the reference raises TypeError
                                   (simulation.py:462 on None, quirk Q7) */
    SNOWGPU_E_NO_DEVICE = 8     /* no HIP device / device index out of range */
};

#define SNOWGPU_MAX_FLAKES_PER_BEAM 63   /* largest per-beam list kept in LDS; beams beyond it take the global-list tier */
#define SNOWGPU_MAX_FLAKES_GLOBAL 8192  /* capacity of that tier (or the largest uploaded table, if smaller); the
                                           reference's lists are unbounded (simulation.py:413-419) */
#define SNOWGPU_MAX_LASERS 256
#define SNOWGPU_RANGE_BINS 1230  /* M_extended, simulation.py:113 */

/* ---- context ------------------------------------------------------------------------------- */

/* One context per (device, host thread).  Owns a HIP stream, the uploaded tables and all scratch. */
int snowgpu_create(int device, snowgpu_ctx **out);
void snowgpu_destroy(snowgpu_ctx *ctx);
const char *snowgpu_last_error(const snowgpu_ctx *ctx);
/* "snowgpu <version> gfx950 ..." -- also usable without a device to check the library loads. */
const char *snowgpu_version(void);

/* Replaces yaml.safe_load(calib/20171102_64E_S3.yaml) + the per-channel constants of
 * simulation.py:72-76, :123-126.  focal_offset[c] = (1 - focal_distance[c]*100/13100)**2 is
 * computed by the caller exactly as the reference does (Python float arithmetic). */
int snowgpu_set_lasers(snowgpu_ctx *ctx, int n_lasers, const double *focal_slope,
                       const double *focal_offset, const int32_t *min_intensity,
                       const int32_t *max_intensity);

/* Replaces np.load(<prefix>_<line>.npy) (simulation.py:324-330) and hoists the per-flake,
 * beam-independent work of get_occlusions (simulation.py:351-354; geometry.py:138-190, :32-80)
 * out of the frame loop: rows are (x, y, disk radius) float64.  table_id is a small non-negative
 * integer chosen by the caller; uploading again under the same id replaces the table. */
int snowgpu_upload_table(snowgpu_ctx *ctx, int table_id, const double *xyr, int64_t n_flakes);
/* snowgpu_upload_table for rows that are already in DEVICE memory (K x 3 float64): derived, binned and sorted by kernels.
 * Per-flake quantities come from the device math library (atan / atan2 / asin may differ from glibc's in the last bit);
 * for the reference's .npy tables, whose results are pinned bit for bit, use snowgpu_upload_table. */
int snowgpu_file_table_device(snowgpu_ctx *ctx, int table_id, const double *d_xyr, int64_t n_flakes);

/* Drops a table and its device memory; the id may be uploaded again.  Batches that name a dropped id fail with
 * SNOWGPU_E_INVALID. */
int snowgpu_free_table(snowgpu_ctx *ctx, int table_id);
int snowgpu_table_count(const snowgpu_ctx *ctx);

/* dart_throwing (tools/snowfall/sampling.py:90-194) on the device: same process (uniform-area centres, Exp(scale)
 * sphere diameters truncated at 20 mm, disk = slice at uniform height, no disk over the origin, no overlaps in dart
 * order, stop when the occupied area reaches occupancy_ratio * pi * r_0^2), NOT the same random stream (Philox4x32-10
 * keyed by (seed, dart index) instead of a sequential NumPy Generator) -- statistical parity, see DESIGN.md.
 *   diameter_scale_mm  = 10 / rate_parameter with rate_parameter = gunn_marshall(rate) or sekhon_srivastava(rate)
 *                        (sampling.py:108-115, :154)
 *   table_id >= 0      file the table under that id (as snowgpu_upload_table does); -1: only return the rows
 *   xyr_out / cap      optional host buffer for the K x 3 rows; *n_out = K */
/*   The rows never visit the host unless xyr_out asks for them: with table_id >= 0 the table is filed by kernels on the
 *   sampler's output (same per-flake quantities and bin order as snowgpu_upload_table, with the device math library's
 *   atan / atan2 / asin, which may differ from glibc's in the last bit). */
int snowgpu_sample_table(snowgpu_ctx *ctx, int table_id, double occupancy_ratio, double diameter_scale_mm,
                         double r_0, uint64_t seed, double *xyr_out, int64_t cap, int64_t *n_out);

/*
 * How the results of a pipelined snowgpu_augment_batch cross the link (the reference returns a fresh N' x 5 array, simulation.py:523,
 * :540-544; here the caller's out_rows / out_src receive the same bytes either way):
 *   mode 0 (default)  output rows + source indices: 24 bytes per point down the link (20 with out_src = NULL)
 *   mode 1 "packed"   per kept row its source row | label and its intensity (8 bytes; 12 for float64 rows), the moved coordinates of
 *                     scattered rows (label 2, simulation.py:176-180) apart, every copy sized by the per-frame counts; `threads` host
 *                     threads of the library (0: the CPUs this process may use minus two, at most 8; they run on the NUMA node the caller's row
 *                     buffers live on, the device's node if that cannot be told) assemble the caller's rows --
 *                     x, y, z and the channel of rows without a laser are COPIED from the caller's input rows, nothing is computed
 *                     on the host.  A third of the download; for callers bound by the link with cores to spare.
 * rows == NULL (resident rows) and single-chunk batches always use mode 0.  Mode 1 reads `rows` while it writes `out_rows`: the two must
 * not overlap (SNOWGPU_E_INVALID; mode 0 tolerates rows == out_rows), and a frame holds fewer than 2^30 rows (30-bit source rows).
 */
int snowgpu_set_result_transfer(snowgpu_ctx *ctx, int mode, int threads);
/* NUMA node HIP device `device` hangs on (sysfs, by PCI bus id), or -1 if it cannot be told: a launcher that runs one process per GPU should
 * start it on that node's CPUs (page-locked buffers touched from the other socket cost the packed transfer a quarter of its rate). */
int snowgpu_device_numa_node(int device);
/* timeline of the last packed call, ms since its start: everything enqueued, every download landed, every row assembled; threads used */
int snowgpu_debug_transfer_times(snowgpu_ctx *ctx, double *out4);

/* Rows per chunk of the host-pointer entry's upload / compute / download pipeline (default 3 * 2^19, i.e. 12 sweeps of
 * 64 x 2048; chunks alternate between SNOWGPU_PIPE_LANES = 2 compute lanes); 0 = no pipeline: one upload, one launch sequence, one download.  The
 * reference has no counterpart (its arrays never leave the host; precompute.py:78 / :106 are its I/O boundary). */
int snowgpu_set_pipeline(snowgpu_ctx *ctx, int64_t chunk_rows);

/* Validation switch for the received-power term A * sin^2(pi (R - r) / (c tau_h)) (simulation.py:549).
 * 0 (default): the engine's own sine (one reduction step + odd polynomial, < 1 ULP) and a multiplication by
 * 1 / (c tau_h); 1: the device math library's sin and a true division, operation for operation what NumPy
 * evaluates.  Both modes give the same labels / intensities (tests/test_gpu_parity.py); mode 1 is ~3x slower.
 * The switch also covers the beam-limit distance test (geometry.py:94-106, :131-135): 0 decides it as |y cos - x sin| < r and falls
 * back on the reference's tangent / root / quotient only within 1e-12 (|x| + |y|) of equality; 1 evaluates the reference's expression,
 * with the math library's tan, for every flake. */
int snowgpu_set_exact_math(snowgpu_ctx *ctx, int on);

/* on = 1: every kernel of a device-pointer batch on the caller's stream -- no side streams, no events (the environment switch SNOWGPU_SERIAL
 * as a call).  One batch alone is slower that way (4.7 against 4.0 ms per 256 sweeps: the received-power kernels and the prepass no longer
 * run side by side), but SEVERAL batches in flight on several contexts, one stream each, overlap across batches -- the memory-bound sort and
 * compaction of one beside the latency-bound per-beam kernels of another: 3.66 ms per batch with three in flight (round 6),
 * PROVIDED every stream has a hardware queue of its own: the HIP runtime serves a process' streams of one priority from GPU_MAX_HW_QUEUES
 * (default 4) queues and hands a new stream the least-used one, so two contexts' streams may share a queue and then run one after the other.
 * Either give the contexts streams of different priorities (snowgpu_lane_stream below: two lanes 3.8 ms in an unchanged environment) or set
 * GPU_MAX_HW_QUEUES=32 in the environment before the process first touches the GPU.  (With more than four queues ONE batch on its four
 * streams is slower -- 4.85 ms: hops between streams wait for queues to be switched in --, so the variable belongs to the
 * several-batches-in-flight deployment only.)  The Python tensor boundary does all this for its compute lanes (augment_batch(..., lane=k)). */
int snowgpu_set_serial(snowgpu_ctx *ctx, int on);

/* A stream of the context's for a caller that keeps several batches in flight: level 0 / 1 / 2 = the device's highest / normal / lowest stream
 * priority (made on the first call, destroyed with the context; *stream is a hipStream_t).  The HIP runtime serves each priority from a
 * queue pool of its own, so three serial contexts on streams of three DIFFERENT levels run side by side under the runtime's default of four
 * hardware queues -- streams of one level may be handed the same queue and then run one after the other (scripts/probe/queue_map_probe.hip).
 * The level only decides whose waves the dispatcher places first when two streams have work ready. */
int snowgpu_lane_stream(snowgpu_ctx *ctx, int level, void **stream);

/* Debug / parity tap: per-flake quantities of a filed table, by table row: range (simulation.py:332), azimuth in
 * [0, 2 pi] (:351-352) and the two tangent angles ordered (right, left) (geometry.py:138-190, :32-80).  out: K x 4 doubles. */
int snowgpu_debug_table(snowgpu_ctx *ctx, int table_id, double *out, int64_t cap_rows);

/* Debug tap: the WHOLE filed table as the scan reads it, copied to host buffers (plain copies on the context's stream, no kernel):
 *   bin_start  SG_NBINS + 1 = 2049 words: bin b holds records bin_start[b] .. bin_start[b + 1]
 *   entries    n_entries + 1 records of 64 bytes (SgEntry: phi, x, y, r, t0, t1, rho as float64, then flags and src as uint32), the bins
 *              concatenated, each ordered by (rho, src); the last one is the spare record behind the last bin
 *   bin_q      2048 x 16 words, bin-major: records of the bin nearer than 8 k metres
 *   bin_qs     qs_steps x 2049 words, step-major, two 16-bit counts to a word, word 2048 of a row bin 0 again; a table whose longest bin
 *              exceeds 65 535 records has none (nothing is written, info[4] = 0)
 *   info       int64[5]: n_flakes, n_entries, max_bin, qs_steps, 1 if the table has a bin_qs else 0;  *qs_per_m: steps per metre of bin_qs
 * The capacities count words (records for entries).  info and *qs_per_m are written BEFORE the capacities are checked: a caller that
 * does not know the sizes calls once with capacities of 0 (SNOWGPU_E_INVALID, "buffer too small"), reads info and calls again.  An unknown
 * table id, a null pointer and a buffer that is too small return SNOWGPU_E_INVALID. */
int snowgpu_debug_table_bins(snowgpu_ctx *ctx, int table_id, uint32_t *bin_start, int64_t cap_start, void *entries, int64_t cap_entries,
                             uint32_t *bin_q, int64_t cap_q, uint32_t *bin_qs, int64_t cap_qs, int64_t *info, double *qs_per_m);

/* Status words (int32[8], layout under snowgpu_augment_batch_device) of the last batch that went through a host-pointer
 * entry of this context: e.g. out8[2..5] = beams each later list capacity took, out8[6] = beams the row kernels redid with the
 * pairwise sum (each summed over the chunks of a pipelined batch). */
int snowgpu_last_status(snowgpu_ctx *ctx, int32_t *out8);

/* What the status words of a DEVICE-pointer entry mean: the caller of snowgpu_augment_batch_device / snowgpu_augment_wet_batch_device
 * downloads its int32[8] `d_status` once the stream has caught up and hands the words to this function, which returns the SNOWGPU_E_*
 * code the host-pointer entries would have returned for them and leaves the message in snowgpu_last_error (0 and no message for
 * status8[0] == 0).  Same exception mapping as the host entries in the Python mirror: SNOWGPU_E_RANGE -> IndexError
 * (simulation.py:149), SNOWGPU_E_GROUND -> TypeError (simulation.py:462). */
int snowgpu_status_error(snowgpu_ctx *ctx, const int32_t *status8);

/* The 1230-entry range grid of simulation.py:106-116 as the library computes it (for tests). */
int snowgpu_range_grid(double *out /* SNOWGPU_RANGE_BINS */);

/* ---- the hot path -------------------------------------------------------------------------- */

/*
 * snowgpu_augment_batch -- augment() (simulation.py:427-544, only_camera_fov=False) for a batch of
 * frames whose rows live in HOST memory.
 *
 *   rows       the frames, concatenated -- or NULL right after snowgpu_prepass_stats on the same frames (their rows are still on the device)
 *   table_ids  n_frames x n_lasers: the table feeding channel c of frame f, i.e. the id the caller
 *              uploaded `<prefix>_<order[c]+1>.npy` under (simulation.py:70, :78, :482-486)
 *   beam_divergence_deg  as passed to augment() (degrees; simulation.py:96-97)
 *   thr_poly   n_frames x 3 quadratic (p0, p1, p2) of the per-point noise threshold over range
 *              (simulation.py:467-469), or NULL to run the prepass (simulation.py:449-467) on the
 *              device with plane (plane_w[3], plane_h) per frame: n_frames x 4 doubles (wx, wy, wz, h)
 *   plane      or NULL as well: calculate_plane (simulation.py:449, planes.py:12-50) runs on the device too, by the
 *              context's method (snowgpu_set_plane_method; default: the plane the reference returns today)
 *   noise_floor  augment()'s noise_floor (only used by the device prepass)
 *   perm       optional n_total int32 permutation (frame-local source row of each channel-sorted
 *              position); NULL = stable counting sort by channel on the device
 *   out_rows   capacity n_total rows (worst case: nothing removed); compacted per frame, frame f
 *              starts at row frame_offsets[f]
 *   out_src    n_total int32: frame-local input row of each output row; may be NULL (not downloaded: 20 instead of
 *              24 bytes per point on the way back)
 *   out_counts n_frames: rows kept per frame
 *   out_stats  n_frames x 3: num_attenuated, num_removed, avg_intensity_diff (simulation.py:525-542)
 *   out_thr_poly optional n_frames x 3: the threshold polynomial actually used
 *
 * A batch larger than ~1.5 chunks runs as a PIPELINE of chunks of whole frames (snowgpu_set_pipeline): all uploads stream
 * through one DMA queue, the chunks compute on two alternating lanes, and each chunk's results leave on a third stream while
 * the next chunks compute -- one host thread and one context keep both directions of the link and the CUs busy.
 * Page-locked rows / out_rows / out_src (snowgpu_host_alloc) make the upload asynchronous and let the download be a small
 * kernel that writes host memory directly; pageable memory works and is slower.  The call returns when everything has landed.
 */
int snowgpu_augment_batch(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets,
                          const void *rows, int dtype, const int32_t *table_ids,
                          double beam_divergence_deg, const double *thr_poly,
                          const double *plane, double noise_floor, const int32_t *perm,
                          void *out_rows, int32_t *out_src, int64_t *out_counts,
                          int64_t *out_stats, double *out_thr_poly);

/*
 * snowgpu_augment_batch for callers bound by the link (round 6): the frames cross it as (x, y, z, intensity) float32 rows plus ONE BYTE per
 * row for the channel -- 17 bytes per point instead of the 20 of the STF row, which keeps the channel as a fifth float32
 * (precompute.py:78) -- and a kernel makes the rows on the device (k_expand_rows).  float32, integer channels 0 .. 255, no caller
 * permutation, no pre-augment crop; everything else -- table ids, plane / polynomial, results, statistics, the pipeline, the packed result
 * transfer (whose host threads then copy x, y, z from `xyzi`), the threshold callback -- as snowgpu_augment_batch.  out_rows are
 * (x, y, z, intensity, label) float32 rows: byte for byte what snowgpu_augment_batch returns for the same frames.
 */
int snowgpu_augment_batch_compact(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const float *xyzi,
                                  const uint8_t *channels, const int32_t *table_ids, double beam_divergence_deg,
                                  const double *thr_poly, const double *plane, double noise_floor, float *out_rows,
                                  int32_t *out_src, int64_t *out_counts, int64_t *out_stats, double *out_thr_poly);

/*
 * Same computation with every array already in DEVICE memory (hipMalloc'ed by the caller, e.g. a
 * torch tensor's data_ptr) and launched on the caller's stream (hipStream_t passed as void*; NULL =
 * the context's stream).  Nothing is copied to the host and the call does not synchronise: this is
 * the entry point bench.py times.  max_frame_rows = rows of the largest frame (sizes the per-frame grids;
 * 0 = unknown, n_total is used; when max_frame_rows * n_frames == n_total all frames are taken to be that size).
 * d_status (device int32[8]) receives {[0] error code, [1] first offending sorted row or -1, [2] [3] [4] [5] beams handed
 * to the 2nd / 3rd / 4th / 5th list capacity (the last one in use is the global-list tier), [6] beams the row kernels redid with the pairwise sum; 0 in list mode
 * (a count like [2] .. [5]: snowgpu_status_error ignores it), [7] unused}; check it
 * after synchronising the stream.  The call forks work onto the context's side streams and joins
 * them back before the compaction kernels, so everything is ordered after earlier work and before later work on
 * `stream`; one batch at a time per context (its scratch buffers are reused).
 */
int snowgpu_augment_batch_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total,
                                 int64_t max_frame_rows, const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                 const int32_t *d_table_ids, double beam_divergence_deg,
                                 const double *d_thr_poly, const double *d_plane, double noise_floor,
                                 const int32_t *d_perm, void *d_out_rows, int32_t *d_out_src,
                                 int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly,
                                 int32_t *d_status, void *stream);

/*
 * snowgpu_augment_batch_device with the ALIGNED result layout.  The simulation never moves a point to another beam -- a beam is copied,
 * attenuated, moved along its own ray or dropped (simulation.py:160-192, :516-523) -- so the result can keep the input's size and order:
 *   d_out_rows  n_total x 5 rows (dtype of the input): row i of frame f (d_frame_offsets[f] + i) is the output row of INPUT row i.  EVERY
 *               row is written, removed ones too: those hold what aug_pc held just before simulation.py:523 (the input's coordinates --
 *               the moved ones for a scattered row only the camera crop removed --, np.round of the intensity for label 0, the
 *               attenuated intensity for label 1, column 4 as in a kept row), so the bytes are deterministic.  May be d_rows ITSELF
 *               (in place: the frames are overwritten by their augmented form); any other overlap with d_rows is SNOWGPU_E_INVALID.
 *   d_out_keep  n_total bytes: 1 where the reference returns the row (noise-floor filter, camera crop if set), else 0.
 *               d_out_rows[keep], taken in the order of snowgpu_augment_batch_device's d_out_src, are that entry's rows byte for byte.
 *   d_out_counts, d_out_stats, d_out_thr_poly, d_status   as snowgpu_augment_batch_device (counts = flags set per frame).
 * Same contract otherwise: asynchronous on `stream`, no allocation after the first call of a size, capturable into a HIP graph; on a
 * non-zero status the rows are unspecified.  The last step is one kernel instead of the compaction's three.  A context with a threshold
 * callback (snowgpu_set_threshold_callback) or the packed result transfer (snowgpu_set_result_transfer) set answers SNOWGPU_E_INVALID:
 * both finish batches through the compaction.  The host-pointer entries have no aligned form; the wet-ground model and the fused
 * snowfall + wet-ground chain have one of their own (snowgpu_wet_ground_batch_device_aligned, snowgpu_augment_wet_batch_device_aligned).
 */
int snowgpu_augment_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total,
                                         int64_t max_frame_rows, const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                         const int32_t *d_table_ids, double beam_divergence_deg,
                                         const double *d_thr_poly, const double *d_plane, double noise_floor,
                                         const int32_t *d_perm, void *d_out_rows /* n_total x 5, may be d_rows itself */,
                                         uint8_t *d_out_keep /* n_total */, int64_t *d_out_counts, int64_t *d_out_stats,
                                         double *d_out_thr_poly, int32_t *d_status, void *stream);

/*
 * Debug/parity tap: the occlusion dicts of get_occlusions (simulation.py:298-424) for the rows of
 * ONE frame, in the channel-sorted order, flattened: count[i] entries for sorted row i stored at
 * [i*cap, i*cap + count[i]) of rj / ratio, near -> far, hard target last.  Host pointers.
 */
int snowgpu_debug_occlusions(snowgpu_ctx *ctx, int64_t n_rows, const void *rows, int dtype,
                             const int32_t *table_ids, double beam_divergence_deg, int cap,
                             int32_t *count, double *rj, double *ratio, int32_t *sorted_src);

/*
 * Camera-FOV crop of augment(only_camera_fov=True) (simulation.py:39-47, :532-540; get_fov_flag(lidar_to_rect(xyz),
 * (img_h, img_w))) inside the compaction kernels of every later batch of this context: v2c = Tr_velo_to_cam (3 x 4,
 * row-major), r0 = R0_rect (3 x 3), p2 = P2 (3 x 4); (1024, 1920) is the reference's image.  Cropped rows count in
 * num_removed (:538); num_attenuated / avg_intensity_diff are taken before the crop (:525-530).  enabled = 0 switches it
 * off (the matrices may then be NULL).  The reference's projection lives in an un-vendored module: textbook KITTI,
 * float64 -- parity unpinned.
 */
int snowgpu_set_fov(snowgpu_ctx *ctx, int enabled, const double *v2c, const double *r0, const double *p2, int img_h, int img_w);
/* precompute.py:96-99 crops every frame to the camera's view BEFORE augment() is called.  on = 1 (with a crop set by
 * snowgpu_set_fov): snowgpu_augment_batch compacts the uploaded frames on the device first -- num_removed etc. then
 * count against the cropped frame, as in the reference's loop, and out_src still indexes the ORIGINAL frame's rows.
 * Host-pointer entry only (the per-frame counts of the cropped batch are read back to lay the batch out). */
int snowgpu_set_fov_precrop(snowgpu_ctx *ctx, int on);

/* ---- ground plane ------------------------------------------------------------------------------ */

/*
 * calculate_plane (tools/wet_ground/planes.py:12-50; called at simulation.py:449 and wet_ground/augmentation.py:41) on the
 * device.  The reference crops the cloud to a strip in front of the car (planes.py:21-27), returns the flat-earth plane
 * ([0, 0, 1], -1.55) for a crop of no more rows than the array has columns (:29-32) and otherwise fits z = c0 x + c1 y + b with
 * scikit-learn's RANSACRegressor (:35) -- unseeded, and with scikit-learn >= 1.2 the call raises, so the except branch (:43-48)
 * returns the flat-earth plane for every cloud.  Methods of this library (parity unpinned by construction):
 *   SNOWGPU_PLANE_REFERENCE  (default) what the reference returns today: ([0, 0, 1], standard_height), no row is read
 *   SNOWGPU_PLANE_LSQ        least squares over the crop (float64, fixed summation order); w = [c0, c1, -1] / |.|, h = b (:36-41)
 *   SNOWGPU_PLANE_RANSAC     RANSAC as scikit-learn < 1.2 ran it for the reference (3-point samples, threshold = MAD of z,
 *                            most inliers, refit on them), samples from Philox4x32-10 keyed by (seed, frame, trial)
 * Both estimators return the flat-earth plane for a crop of <= min_rows rows (the reference: 5, the column count) or when no
 * model can be fitted.  The method applies to every later batch of this context that brings neither plane nor thr_poly
 * (plane == NULL), to snowgpu_wet_ground_batch / snowgpu_augment_wet_batch with a NULL plane, and to snowgpu_estimate_planes.
 */
enum { SNOWGPU_PLANE_REFERENCE = 0, SNOWGPU_PLANE_LSQ = 1, SNOWGPU_PLANE_RANSAC = 2 };
int snowgpu_set_plane_method(snowgpu_ctx *ctx, int method, uint64_t seed, int max_trials /* 0 = 1024 */, int min_rows,
                             double standard_height);
/* The planes themselves, for frames in host memory: out_planes n_frames x 4 (wx, wy, wz, h); out_info (optional) n_frames x 4
 * int32: rows in the crop (-1: not counted, reference method), model used (0 flat earth, 1 least squares, 2 ransac), rows the
 * final fit used, valid RANSAC trials. */
int snowgpu_estimate_planes(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                            double *out_planes, int32_t *out_info);
/* ... and with every array in device memory, asynchronous on the caller's stream (semantics of snowgpu_augment_batch_device). */
int snowgpu_estimate_planes_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                   const int64_t *d_frame_offsets, const void *d_rows, int dtype, double *d_out_planes,
                                   int32_t *d_out_info, void *stream);

/*
 * First half of the noise-threshold prepass (simulation.py:449-461; wet_ground/augmentation.py:195-235) for a caller that wants the
 * reference's answer on ITS OWN machine: the reference takes the sparsest bin of every histogram row with np.argpartition(hist, 2)
 * [:, 0] (:236), whose result depends on the NumPy build (quirk Q8).  The device makes the expensive part -- ground rows, I / cos,
 * the regression line p, the 50 x 2555 histogram, the sums of the quadratic fit --, the caller takes the row minima with its own
 * NumPy, fits the noise line and the quadratic from the sums, and passes the polynomials to snowgpu_augment_batch (thr_poly).
 *   plane     n_frames x 4, or NULL (estimated on the device, snowgpu_set_plane_method)
 *   out_hist  n_frames x 50 x 2555 int32 (histogram2d of (range, I / cos) over (10, 70) x (5, max), augmentation.py:232-233)
 *   out_rec   n_frames x SNOWGPU_PREPASS_REC doubles: ground rows, mean range, np.mean of the float32 range column as NumPy
 *             computes it, mean I / cos, max I / cos, p slope, p intercept (linregress, :216-219), then the sums over the ground
 *             rows of a2 a2, a2 a1, a2, a1 a1, a1, a2 d c, a2 c, a1 d c, a1 c, d c, c  (a1 = d = range, a2 = range^2, c = cos of the
 *             incident angle): the normal equations of np.polyfit(range, nf (m0 d + m1) c, 2) are linear in the noise line (m0, m1)
 * Fewer than 3 ground rows in a frame: SNOWGPU_E_GROUND, as the batch entries report it.  Empty bins of out_hist already hold
 * the frame's ground-row count (hist[hist == 0] = len(pointcloud_planes), :234-235).  The uploaded rows stay in the context: the
 * next snowgpu_augment_batch of the SAME frames may pass rows = NULL and computes on them instead of uploading them again.
 */
#define SNOWGPU_PREPASS_REC 18
int snowgpu_prepass_stats(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                          const double *plane, int32_t *out_hist, double *out_rec);

/*
 * The same division of labour INSIDE one batch call (round 6): with a callback set, snowgpu_augment_batch calls that bring neither thr_poly
 * nor a caller permutation compute the device half above per group of frames (a chunk of the pipelined entry), start the per-beam kernels
 * of the group, and call
 *     fn(user, first_frame, n_frames, hist, rec, thr_poly_out)
 * on the CALLING thread as soon as the group's histograms (n_frames x 50 x 2555 int32) and records (n_frames x SNOWGPU_PREPASS_REC) have
 * landed in page-locked memory -- while those kernels, and the uploads / kernels / downloads of the other groups, run.  fn writes the
 * groups' polynomials (n_frames x 3, highest power first, np.polyfit's order) and returns 0 (anything else fails the call with
 * SNOWGPU_E_INVALID); the library uploads them and runs the group's compaction (simulation.py:516-540).  The rows cross the link once
 * and the host's np.argpartition (wet_ground/augmentation.py:236) hides behind the device's work; the two-call form above costs a second
 * crossing and runs the three stages in sequence.  fn = NULL switches back to the device's own fit.  Python: augment_batch(q8='numpy').
 */
typedef int (*snowgpu_threshold_fn)(void *user, int first_frame, int n_frames, const int32_t *hist, const double *rec, double *thr_poly_out);
int snowgpu_set_threshold_callback(snowgpu_ctx *ctx, snowgpu_threshold_fn fn, void *user);

/* ---- measurement hooks ------------------------------------------------------------------------ */

/* Record a HIP event pair around every launch of the per-beam kernel (the dominant kernel) on the stream
 * it is launched on, for up to max_launches launches.  snowgpu_profile_end synchronises that stream and
 * returns the summed kernel time in milliseconds and the number of launches timed. */
int snowgpu_profile_begin(snowgpu_ctx *ctx, int max_launches);
int snowgpu_profile_end(snowgpu_ctx *ctx, double *beam_kernel_ms, int *n_launches);

/* ---- page-locked host buffers ------------------------------------------------------------------ */

/*
 * The host-pointer entries (snowgpu_augment_batch, snowgpu_wet_ground_batch, snowgpu_augment_wet_batch) accept any
 * host memory, but only page-locked memory moves at PCIe speed and lets the copies of one context overlap the
 * kernels of another.  snowgpu_host_alloc returns such a buffer (hipHostMalloc); read the frames into it and hand
 * it in as `rows`, pass another one as `out_rows`.  The reference has no counterpart: its arrays never leave the host
 * (precompute.py:78 np.fromfile -> :106 tofile).
 */
int snowgpu_host_alloc(snowgpu_ctx *ctx, size_t bytes, void **ptr);
int snowgpu_host_free(snowgpu_ctx *ctx, void *ptr);

/* ---- wet ground ---------------------------------------------------------------------------- */

/*
 * ground_water_augmentation() (tools/wet_ground/augmentation.py:25-161, estimation_method
 * 'linear', debug off) for a batch of frames in host memory.  Output rows are float64 whatever
 * the input dtype (augmentation.py:150), ordered [non-ground rows ; kept ground rows]
 * (augmentation.py:151-152).  A frame with fewer than 1000 ground rows is returned unchanged
 * (augmentation.py:51-52) with out_flags[f] = 1.
 *   plane  n_frames x 4 (wx, wy, wz, h), or NULL: calculate_plane (augmentation.py:41) on the device (snowgpu_set_plane_method)
 */
int snowgpu_wet_ground_batch(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets,
                             const void *rows, int dtype, const double *plane,
                             double water_height, double pavement_depth, double noise_floor,
                             double power_factor, int flat_earth, double delta, int replace,
                             double *out_rows, int32_t *out_src, int64_t *out_counts,
                             int32_t *out_flags);

/* The two lines estimate_laser_parameters fits (augmentation.py:216-219 p = linregress(range, I / cos); :248-251 the noise
 * line through the sparsest histogram bins, quirk Q8) for the NEXT snowgpu_wet_ground_batch of this context, supplied by a
 * caller that fits them itself -- with its own NumPy, whose argpartition build decides Q8 -- instead of the device's
 * first-minimum fit: n_frames x 4 doubles (p slope, p intercept, noise-line slope, noise-line intercept).  One use; NULL clears. */
int snowgpu_set_wet_lines(snowgpu_ctx *ctx, int n_frames, const double *lines);

/* estimation_method of ground_water_augmentation (reference: tools/wet_ground/augmentation.py:25, passed through by
 * pointcloud_viewer.py:2820, :2851 as self.estimation) for every later wet-ground call of this context
 * (snowgpu_wet_ground_batch, snowgpu_augment_wet_batch[_device]):
 *   method 0  'linear' -- linregress for the laser power (:215-221) and for the noise level (:247-253); the default
 *   method 1  'poly'   -- np.polyfit of degree 2 for the laser power (:223-229) and ransac_polyfit (:171-192: n = 15, k = 100,
 *                         t = 0.1, d = 15, f = 0.8) for the noise level (:243-246).  The reference draws the RANSAC samples from
 *                         NumPy's process-global UNSEEDED generator (np.random.randint, :183), so it differs from run to run;
 *                         here trial t of frame f draws from Philox4x32-10 keyed by (seed; f, t): same cloud + same seed = same
 *                         curves on every run and GPU.  Parity unpinned by construction.
 * A frame in which NO range row of the 50 x 2555 histogram has its sparsest bin above 5 returns SNOWGPU_E_GROUND under 'poly'
 * (np.polyfit raises TypeError on an empty vector); with one or two such rows the noise curve is np.polyfit's answer to the
 * under-determined system -- the minimum-norm solution of its column-scaled Vandermonde system -- as in the reference, whose RANSAC
 * cannot replace it there (a consensus set needs more than d = 15 points).  snowgpu_set_wet_lines cannot be combined with 'poly'. */
int snowgpu_set_wet_estimation(snowgpu_ctx *ctx, int method, uint64_t seed);

/* The curves the last wet-ground call of this context fitted: per frame 8 doubles -- laser power c2, c1, c0
 * (relative_output_intensity = power_factor * polyval(c, range), :221 / :228), noise level c2, c1, c0 (adaptive_noise_threshold =
 * noise_floor * polyval(c, range), :245 / :252), ground rows, RANSAC trial whose consensus refit was kept (-1: the fit over all
 * points).  'linear' frames report their two lines with c2 = 0. */
int snowgpu_wet_last_fit(snowgpu_ctx *ctx, int n_frames, double *out);

/* Parity tap of the 'poly' noise fit: the device's ransac_polyfit(x, y, order=2) (augmentation.py:171-192) on m (3 .. 50) host points
 * with the Philox draws of (seed; frame): out4 = c2, c1, c0, trial kept (-1: the fit over all points). */
int snowgpu_debug_ransac_polyfit(snowgpu_ctx *ctx, int m, const double *x, const double *y, uint64_t seed, uint64_t frame, double *out4);

/*
 * augment() followed by ground_water_augmentation() on its output, as pointcloud_viewer.py:2807-2821 chains them
 * (snow first, then wet with replace=False), as ONE launch sequence: the intermediate cloud never leaves the device.
 * Arguments are those of snowgpu_augment_batch followed by those of snowgpu_wet_ground_batch (wet_plane: n_frames x 4, or
 * NULL: estimated on the device from the snowfall stage's result, as the chained reference calls do).
 * out_stats are the snowfall statistics; out_rows (float64) / out_counts / out_flags the wet-ground result;
 * out_src maps every final row to its row in the original input frame.
 */
int snowgpu_augment_wet_batch(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows,
                              int dtype, const int32_t *table_ids, double beam_divergence_deg,
                              const double *thr_poly, const double *plane, double noise_floor,
                              const int32_t *perm, const double *wet_plane, double water_height,
                              double pavement_depth, double wet_noise_floor, double power_factor,
                              int flat_earth, double delta, int replace, double *out_rows, int32_t *out_src,
                              int64_t *out_counts, int64_t *out_stats, int32_t *out_flags);

/*
 * The same chain with every array in DEVICE memory, asynchronous on the caller's stream (semantics of
 * snowgpu_augment_batch_device: no host copy, no synchronisation, no allocation after the first call of a given size --
 * capturable into a HIP graph).  d_out_rows: n_total x 5 float64; the snowfall stage's rows stay in context scratch.
 */
int snowgpu_augment_wet_batch_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                     const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                     const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                     const double *d_plane, double noise_floor, const int32_t *d_perm,
                                     const double *d_wet_plane, double water_height, double pavement_depth,
                                     double wet_noise_floor, double power_factor, int flat_earth, double delta, int replace,
                                     double *d_out_rows, int32_t *d_out_src, int64_t *d_out_counts, int64_t *d_out_stats,
                                     int32_t *d_out_flags, int32_t *d_status, void *stream);

/*
 * ground_water_augmentation() with the ALIGNED result, every array in DEVICE memory: the wet-ground model never moves a point -- a
 * non-ground row is copied, a ground row gets a new intensity and label 1 or is dropped (augmentation.py:145-159) -- so the result can
 * keep the input's size and order, as snowgpu_augment_batch_device_aligned's does, and the two chain: d_keep_in takes that entry's
 * d_out_keep.
 *   d_keep_in   n_total bytes or NULL (every row present): 0 = the row is not there.  The estimator skips it -- ground rows, sums,
 *               histogram and the 1000-row rule (augmentation.py:51-52) see the present rows only -- and it comes back as it came.
 *   d_plane     n_frames x 4, or NULL: calculate_plane (augmentation.py:41) by the plane method `reference`, which reads no row.  With
 *               `lsq` or `ransac` set a NULL plane is SNOWGPU_E_INVALID: both crop the rows into a list, and under a mask that list --
 *               and with it the RANSAC draws -- has another order.
 *   d_out_rows  n_total x 5 rows in the INPUT's dtype; may be d_rows itself.  For a processed frame (d_out_flags[f] = 0) and input row i:
 *                 keep-in 0            columns 0 - 4 as they came                                                               keep 0
 *                 present, not ground  columns 0 - 3 unchanged, column 4 = 0 under `replace` (:155-156), else unchanged         keep 1
 *                 ground, kept (:146)  columns 0 - 2 unchanged, the new intensity (:153), column 4 = 1 (:159)                   keep 1
 *                 ground, dropped      columns 0 - 2 unchanged, the value new_intensities held after :131 (0 whenever it was
 *                                      below the limit), column 4 = 1                                                           keep 0
 *               A frame with fewer than 1000 present ground rows (d_out_flags[f] = 1) keeps rows and keep bytes exactly as they came.
 *               Every byte is a function of the input.  Out of place every row is stored whole; in place only columns 3 and 4 of the
 *               rows that change, and the keep bytes that change.
 *               THE ONE PLACE the aligned form departs from the reference's dtype: the compact entries return float64 rows whatever came
 *               in (augmentation.py:150); here a float32 row stays float32 and its new intensity is the float64 result rounded once to
 *               float32 -- a result written in place cannot be wider than its input, and the consumer this layout is for trains in float32.
 *   d_out_keep  n_total bytes; may be d_keep_in itself.  Any overlap of d_out_rows with d_rows, or of d_out_keep with d_keep_in, other
 *               than identity is SNOWGPU_E_INVALID.
 *   d_out_counts / d_out_flags   per frame: keep bytes set / 1 where the frame came back as it was.
 *   d_status    device int32[8], cleared by the call; [0] = SNOWGPU_E_GROUND under 'poly' as snowgpu_wet_ground_batch reports it.
 * Honours snowgpu_set_wet_estimation, snowgpu_set_wet_lines (one use; the call then waits for their upload) and leaves its curves for
 * snowgpu_wet_last_fit.  The contract is the device entries': asynchronous on `stream`, no allocation after the first call of a size,
 * capturable into a HIP graph.  A context with a threshold callback or the packed result transfer set answers SNOWGPU_E_INVALID, as for
 * snowgpu_augment_batch_device_aligned.  The sums of the estimate run over the tiles of the frames as they are passed; the compact fused
 * entry sums over the tiles of the COMPACTED snowfall rows, so the fitted power line of the two chains differs in its last bits.
 */
int snowgpu_wet_ground_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                            const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                            const uint8_t *d_keep_in /* NULL: all rows present */,
                                            const double *d_plane /* n_frames x 4, or NULL */, double water_height,
                                            double pavement_depth, double noise_floor, double power_factor, int flat_earth,
                                            double delta, int replace, void *d_out_rows /* may be d_rows itself */,
                                            uint8_t *d_out_keep /* may be d_keep_in itself */, int64_t *d_out_counts,
                                            int32_t *d_out_flags, int32_t *d_status, void *stream);

/*
 * snowgpu_augment_batch_device_aligned followed by snowgpu_wet_ground_batch_device_aligned IN PLACE on its d_out_rows / d_out_keep, as one
 * launch sequence on `stream`: the chain of snowgpu_augment_wet_batch_device without its five compaction passes (count, scan, scatter of
 * the snowfall stage; scan and scatter of the wet stage) and without the snowfall stage's row scratch.  Arguments: those of
 * snowgpu_augment_batch_device_aligned, then the wet arguments of snowgpu_augment_wet_batch_device, then d_out_flags.
 *   d_out_rows / d_out_keep   the chain's result, rows in the input's dtype (see above); d_out_rows may be d_rows itself
 *   d_out_stats               the snowfall statistics;   d_out_counts / d_out_flags   the wet stage's
 *   d_wet_plane               n_frames x 4, or NULL under the plane method `reference` (SNOWGPU_E_INVALID under `lsq` / `ransac`)
 * A frame whose wet stage finds fewer than 1000 present ground rows comes back as the aligned snowfall result with d_out_flags[f] = 1.
 */
int snowgpu_augment_wet_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                             const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                             const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                             const double *d_plane, double noise_floor, const int32_t *d_perm,
                                             void *d_out_rows /* n_total x 5, may be d_rows itself */, uint8_t *d_out_keep /* n_total */,
                                             int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly, int32_t *d_status,
                                             void *stream, const double *d_wet_plane, double water_height, double pavement_depth,
                                             double wet_noise_floor, double power_factor, int flat_earth, double delta, int replace,
                                             int32_t *d_out_flags);

/*
 * snowgpu_augment_batch_device_aligned with an INPUT keep mask: a row whose d_keep_in byte is 0 is not there -- cropped away, padding of an
 * F x Nmax batch, removed by an earlier stage.  For frame f let P be the indices of its present rows in input order.  The call returns,
 * byte for byte, what snowgpu_augment_batch_device_aligned returns for the batch whose frame f holds exactly the rows P in that order
 * (same tables, planes or plane method, polynomials, noise floor, camera crop):
 *   d_out_rows[P[i]] / d_out_keep[P[i]]   that call's row i and its keep byte
 *   d_out_stats, d_out_counts, d_out_thr_poly   that call's: num_removed counts against the PRESENT rows
 *   an absent row      comes back as it came, all five columns bit for bit (out of place it is copied, in place it is not touched),
 *                      keep byte 0.  It is never looked at: NaN coordinates, a range beyond the grid or a channel that is no laser
 *                      in an absent row set no status word and change no byte of another row.
 *   d_keep_in   n_total bytes, or NULL: all rows present -- the unmasked call itself.  A frame whose bytes are all 0 behaves as an empty frame.
 *   d_out_keep  may be d_keep_in itself; any other overlap of the two, or of d_out_rows with d_rows, is SNOWGPU_E_INVALID.
 *   d_perm      must be NULL with a mask (SNOWGPU_E_INVALID): a permutation indexes the rows of the frames it was made for.
 *   d_status    as for the unmasked entry, except that [1] -- the first offending row -- indexes the sorted rows of the COMPACTED batch
 *               (the present rows of all frames back to back), not the input's.
 * How: the present rows are compacted, stably, into context scratch at offsets made on the device -- nothing is read on the host --, the
 * launch sequence of the unmasked call runs on that scratch, and its last kernel writes every row at its index in the caller's frame.
 * n_total and max_frame_rows are the INPUT's and bound the scratch (one more copy of the rows and 4 bytes per row).  The contract is the
 * device entries': asynchronous on `stream`, no allocation after the first call of a size, no host read, capturable into a HIP graph.
 * Needs at most 65536 tables and 2^22 frames (SNOWGPU_E_INVALID otherwise); refuses a threshold callback and the packed result transfer
 * as the aligned entries do.
 */
int snowgpu_augment_batch_device_aligned_masked(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                const int64_t *d_frame_offsets, const void *d_rows, int dtype, const int32_t *d_table_ids,
                                                double beam_divergence_deg, const double *d_thr_poly, const double *d_plane,
                                                double noise_floor, const int32_t *d_perm /* NULL */,
                                                const uint8_t *d_keep_in /* NULL: all present */, void *d_out_rows /* may be d_rows itself */,
                                                uint8_t *d_out_keep /* may be d_keep_in itself */, int64_t *d_out_counts, int64_t *d_out_stats,
                                                double *d_out_thr_poly, int32_t *d_status, void *stream);

/*
 * snowgpu_augment_wet_batch_device_aligned whose snowfall stage is the masked one above.  The wet stage runs in place on d_out_rows /
 * d_out_keep as in the unmasked chain: absent rows carry keep 0 there and are not there for it either.  The result equals the masked
 * snowfall call followed by snowgpu_wet_ground_batch_device_aligned on its rows and keep bytes.
 */
int snowgpu_augment_wet_batch_device_aligned_masked(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                    const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                                    const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                                    const double *d_plane, double noise_floor, const int32_t *d_perm /* NULL */,
                                                    const uint8_t *d_keep_in /* NULL: all present */, void *d_out_rows, uint8_t *d_out_keep,
                                                    int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly, int32_t *d_status,
                                                    void *stream, const double *d_wet_plane, double water_height, double pavement_depth,
                                                    double wet_noise_floor, double power_factor, int flat_earth, double delta, int replace,
                                                    int32_t *d_out_flags);

/*
 * The camera-FOV test of snowgpu_set_fov as a producer of a keep mask (precompute.py:96-99 as a mask instead of a compaction):
 *   d_out_keep[i] = (d_keep_in ? d_keep_in[i] : 1) && get_fov_flag(lidar_to_rect(row i), (img_h, img_w))
 * Matrices as snowgpu_set_fov takes them; the context's own crop setting is neither read nor changed.  A row whose keep-in byte is 0 is
 * not loaded.  d_out_keep may be d_keep_in itself (any other overlap: SNOWGPU_E_INVALID).  Asynchronous on `stream`, no allocation, capturable.
 */
int snowgpu_fov_mask_device(snowgpu_ctx *ctx, int64_t n_total, const void *d_rows, int dtype, const double *v2c, const double *r0,
                            const double *p2, int img_h, int img_w, const uint8_t *d_keep_in /* or NULL */, uint8_t *d_out_keep, void *stream);

/*
 * DYNAMIC RADIUS OUTLIER REMOVAL (DROR; Charron et al., CRV 2018 -- the de-noising filter in front of the reference's chain,
 * pointcloud_viewer.py:2756-2758, defaults :267-270) as a producer of a keep mask, frames as the batch entries take them.
 *   c = beta (alpha_deg pi / 180), c2 = c c, s2min = sr_min sr_min            (host, double, in this order)
 *   row i is USABLE iff it is present (d_keep_in NULL or its byte non-zero) and |x|, |y|, |z| <= 1e6 (false for NaN)
 *   s2_i = max(s2min, c2 (x_i x_i + y_i y_i))                                  (no square root, no fused multiply-add)
 *   usable row j != i of the same frame is a neighbour of usable row i iff (dx dx + dy dy) + dz dz <= s2_i  (closed ball, the QUERY row's
 *   radius; a duplicate point is a neighbour)
 *   d_out_keep[i] = usable_i && count_i >= k_min;  d_out_neighbours[i] (int32, or NULL) = min(count_i, k_min), 0 for an unusable row
 * An unusable row is nobody's neighbour and is never looked at beyond that test (NaN padding does no harm).  The edge conventions are this
 * library's: cadc_devkit's dror.py is not part of the reference checkout, parity with it is not pinned.
 * Domain: 0 < c <= 0.25, sr_min >= 0 and finite, 0 <= k_min <= 65535; anything else is SNOWGPU_E_INVALID.  d_out_keep must NOT overlap
 * d_keep_in, not even as the same array (SNOWGPU_E_INVALID): the query of one row reads other rows' keep-in bytes.  An empty batch returns
 * OK and launches nothing.
 * The search files every usable row in a cell of a per-frame grid (Cartesian where the radius is sr_min, log-polar beyond; sg_dror.h) and
 * counts exactly inside a conservative window of cells.  Scratch in the context, grown on first use: 4 bytes per cell -- at most
 * min(max(4 max_frame_rows, 1024), 81920) + 1 cells per frame --, 4 bytes per row and one sorted copy of x, y, z in the row dtype.
 * One memset and four kernels on `stream`; nothing is read on the host, nothing allocated after the first call of a size: capturable.
 */
int snowgpu_dror_mask_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                             const void *d_rows, int dtype, double alpha_deg, double beta, double sr_min, int64_t k_min,
                             const uint8_t *d_keep_in /* or NULL: all present */, uint8_t *d_out_keep,
                             int32_t *d_out_neighbours /* or NULL */, void *stream);

/*
 * POINT-TO-VOXEL GROUPING of an aligned batch: the static-shape hand-off to a detector's first operation (SECOND, PV-RCNN, PointPillars).
 * Frames, rows and the input keep mask as the aligned entries take them.  The reference has no voxelizer; the edge conventions are this
 * library's, restated as a sequential NumPy walk by tests/voxel_reference.py.
 *   Host constants, in double, j = x, y, z:  lo_j = range6[j], hi_j = range6[3 + j], size_j = size3[j],
 *   n_j = llround((hi_j - lo_j) / size_j).
 *   Row i of frame f is USABLE iff it is present (d_keep_in NULL or its byte non-zero), its x, y, z are finite and, for every j,
 *   c_j = floor(((double)p_j - lo_j) / size_j) satisfies 0 <= c_j < n_j.  A true double division and a floor: no reciprocal, no fused
 *   multiply-add.  A coordinate on hi_j is out (where (hi_j - lo_j) / size_j is exact; the formula decides); one on lo_j or on an inner
 *   face belongs to the upper cell.
 *   The usable rows of a frame are walked in input order, T = max_points, V = max_voxels.  The first row of a cell not seen before opens
 *   voxel v = the voxels opened so far in this frame; if V are open already the cell is DROPPED, with every later row of it.  A row of an
 *   open voxel is STORED in the voxel's next point slot while the voxel holds fewer than T rows; a later row still belongs to the voxel
 *   and is not stored.
 * Outputs, packed in frame order: m_f = min(cells of frame f, V), voxel_offsets[0] = 0, voxel_offsets[f + 1] = voxel_offsets[f] + m_f.
 *   d_out_voxels         (F V, T, C) in the rows' dtype: voxel voxel_offsets[f] + v, slot t holds columns 0 .. C - 1 of its t-th stored
 *                        row, bit for bit; unfilled slots and every voxel at or beyond voxel_offsets[F] are zero
 *   d_out_coords         (F V, 4) int32: (f, c_z, c_y, c_x); -1 at or beyond voxel_offsets[F]
 *   d_out_num_points     (F V) int32: min(rows of the voxel, T); 0 in the tail
 *   d_out_voxel_offsets  (F + 1) int32, device memory
 *   d_out_voxel_of       (N_total) int32 or NULL: the packed voxel of the row's cell, stored or not; -1 for absent, unusable and dropped rows
 * Every element of every output is written by every call: a buffer that is reused, or a graph that is replayed, needs no clearing.
 * Domain: C = n_features in 3 .. 5, T >= 1, V >= 1, every size_j > 0 and finite, every n_j >= 1 (the range finite),
 * n_x n_y n_z <= 2^31 - 2, F V <= 2^31 - 1, no frame longer than 2^30 rows, dtype float32 or float64; anything else is SNOWGPU_E_INVALID.
 * d_out_voxel_of must not overlap d_keep_in (SNOWGPU_E_INVALID).  An empty batch writes voxel_offsets = 0 and launches nothing else (its
 * other outputs may be NULL).
 * A dense counter per cell is not possible (1408 x 1600 x 40 cells for DENSE): every frame has an open-addressed table of
 * cap = the power of two >= max(2 max_frame_rows, 64) slots of 8 bytes (cell << 32 | smallest row that hit it, by atomic min; sg_voxel.h),
 * and a cell's voxel number is the rank of its first row among the frame's first rows.  Nothing in an output depends on where the hash put
 * a cell or on the order in which atomics arrived: results are identical from run to run.
 * Scratch in the context, grown on first use: 8 cap bytes per frame (16 .. 32 bytes per row of the longest frame), 9 bytes per row,
 * 8 bytes per 1024 rows, 8 bytes per frame and 4 bytes per voxel (F V).  Two memsets and eleven kernels on `stream` (snowgpu_voxel.hip);
 * nothing is read on the host, nothing allocated after the first call of a size: capturable.
 */
int snowgpu_voxelize_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                            const void *d_rows, int dtype, const double *range6 /* host: x0 y0 z0 x1 y1 z1 */,
                            const double *size3 /* host: the voxel's x, y, z edges */, int max_points, int max_voxels, int n_features,
                            const uint8_t *d_keep_in /* or NULL: all present */, void *d_out_voxels, int32_t *d_out_coords,
                            int32_t *d_out_num_points, int32_t *d_out_voxel_offsets, int32_t *d_out_voxel_of /* or NULL */, void *stream);

/*
 * FARTHEST-POINT KEYPOINTS of an aligned batch: the fixed-size point set of the point-based detectors (PV-RCNN's keypoints in front of its
 * voxel set abstraction, PointRCNN, Part-A2), with static shapes.  Frames, rows and the input keep mask as snowgpu_voxelize_device takes
 * them; K = n_samples, C = n_features.  The reference has no sampler; the edge conventions are this library's, restated as a sequential
 * NumPy program by tests/fps_reference.py.
 *   Row i of frame f is USABLE iff it is present (d_keep_in NULL or its byte non-zero), |x|, |y|, |z| <= 1e6 (false for NaN) and, when a
 *   range is given, lo_j <= (double)p_j < hi_j for j = x, y, z.  range6 may be NULL (no range test); its bounds may be infinite.
 *   u_0 < u_1 < ... < u_{m-1} are the usable rows of the frame in input order.
 *   All arithmetic is in the rows' dtype.  d(a, b) = ((dx dx) + (dy dy)) + (dz dz), dx = x_a - x_b and likewise y, z: every operation
 *   rounded on its own, no fused multiply-add, no square root, no reciprocal.
 *   The walk: t_i = +inf for every usable row; s_0 = u_0; for j = 1 .. K - 1: t_i = min(t_i, d(i, s_{j-1})) for every usable i, then
 *   s_j = the usable row with the largest t_i, the SMALLEST row index among equals.
 *   There are no special cases: a chosen row has t = 0 ever after; once every distinct position is taken all t are 0 and s_j = u_0; a
 *   frame with m < K returns its m rows (if no two coincide) and then u_0 repeated; coincident rows are never both chosen before that.
 * Outputs, every shape static, every element written by every call:
 *   d_out_index   (F, K) int32: s_j as a row index into the whole batch (rows[index] gathers); -1 everywhere for a frame with m = 0
 *   d_out_points  (F, K, C) in the rows' dtype, or NULL: columns 0 .. C - 1 of row s_j, bit for bit; zero for a frame with m = 0
 *   d_out_dist    (F, K) in the rows' dtype, or NULL: t of s_j at the moment it was chosen; element 0 is +inf; -1 for a frame with m = 0
 *   d_out_usable  (F) int32, device memory: m_f
 * Domain: K >= 1, C in 3 .. 5, F K <= 2^31 - 1, n_total < 2^31, no frame above 2^30 rows, dtype 0 (float32) or 1 (float64); with a range:
 * no NaN in it and lo_j < hi_j.  d_out_index, d_out_points and d_out_dist must not overlap d_keep_in or the rows.  Anything else is
 * SNOWGPU_E_INVALID.  An empty batch writes usable = 0, index = -1, points = 0 and dist = -1 with one fill kernel and launches no sampler
 * (d_rows may be NULL).
 * ONE workgroup of 1024 threads walks a frame (its rounds cannot run side by side; the frames of a batch can): it compacts the frame's
 * usable rows in input order into scratch and runs the K - 1 rounds without leaving the compute unit -- coordinates and running minima in
 * registers for up to 16384 usable float32 rows (8192 float64 rows), the minima in LDS and the coordinates streamed from scratch for up to
 * 39936 (19968), both streamed from scratch beyond (csrc/sg_fps.h: the tiers, chosen on the device per frame; snowgpu_fps.hip).  A
 * candidate is (bits of t, ~position), folded by an integer maximum: nothing depends on how lanes and waves are combined, and results are
 * identical from run to run.  A lone frame runs on one compute unit.
 * Scratch in the context, grown on first use: four values of the rows' dtype and 4 bytes per row, plus 8 elements per frame.  Two kernels
 * on `stream`; nothing is read on the host, nothing allocated after the first call of a size: capturable.
 */
int snowgpu_fps_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                       const void *d_rows, int dtype, const double *range6 /* host: x0 y0 z0 x1 y1 z1, or NULL */, int n_samples,
                       int n_features, const uint8_t *d_keep_in /* or NULL: all present */, int32_t *d_out_index,
                       void *d_out_points /* or NULL */, void *d_out_dist /* or NULL */, int32_t *d_out_usable, void *stream);

/*
 * SECTORIZED, PROPOSAL-CENTRIC KEYPOINTS of an aligned batch: PV-RCNN++'s replacement for the plain farthest-point walk -- keep the rows
 * near a region proposal (its sample_points_with_roi), split them by azimuth into sectors, and walk every sector on its own with a quota
 * proportional to its share of the rows (its sector_fps) --, with static shapes.  Frames, rows (N_total x 5, float32 or float64 = T),
 * frame offsets, keep mask, range6, K = n_samples and C = n_features exactly as snowgpu_fps_device takes them; S = n_sectors, 1 <= S <= 16;
 * d_rois NULL or (F, B, Cb) in T, B = n_rois in 1 .. 256, Cb = roi_features in 7 .. 10, columns 0 .. 5 cx, cy, cz, dx, dy, dz (OpenPCDet's
 * rois / gt_boxes; the heading and everything behind it are ignored); roi_margin a host double, finite and >= 0 (PV-RCNN++'s
 * SAMPLE_RADIUS_WITH_ROI is 1.6).  Without rois n_rois, roi_features and roi_margin are not read.  The definition is restated in NumPy
 * by tests/fps_sectors_reference.py.
 *   USABLE: as for snowgpu_fps_device -- present, |x|, |y|, |z| <= 1e6 (false for NaN), inside the range when there is one -- and, when
 *   d_rois is given, NEAR A PRESENT ROI OF ITS FRAME.  A roi is present by the box stage's rule on its first six values: all finite,
 *   |cx|, |cy|, |cz| <= 1e6, 0 < dx, dy, dz <= 1e6; the zero rows OpenPCDet pads with are absent.  In float64, every operation rounded on
 *   its own, no fused multiply-add:
 *     reach  = sqrt(((dx/2)(dx/2) + (dy/2)(dy/2)) + (dz/2)(dz/2)) + roi_margin        reach2 = reach reach
 *     row near roi b  iff  ((sx sx) + (sy sy)) + (sz sz) < reach2_b,  sx = x - cx and likewise y, z: STRICT
 *   Near ANY present roi counts.  pcdet tests the reach of the NEAREST roi only; ours is a superset of its rows that does not depend on
 *   the order of the rois.  A frame whose rois are all absent has no usable row.  The device's float64 sqrt is IEEE's, correctly
 *   rounded -- the range image relies on the same (sg_range_r, its pitch) --, so NumPy gives the same reach2: d_out_reach2 shows it.
 *   SECTOR of a usable row, in float64: a = atan2((double)y, (double)x) + pi, atan2 correctly rounded (csrc/sg_atan_cr.h), pi the double
 *   nearest pi; s = min((int)floor(a / ((2 pi) / S)), S - 1), the quotient as NumPy writes
 *   np.floor(np.divide(np.add(atan2, np.pi), np.divide(2 * np.pi, S))).  The origin and the +-pi seam have no special case: atan2(+-0, x < 0)
 *   = +-pi puts y = -0 into sector 0 and y = +0 into sector S - 1; the origin (atan2 = 0) falls where a = pi does.
 *   QUOTA, int64: n_s = the usable rows of the frame in sector s, m = their sum.  m >= K: q_s = floor(n_s K / m), r_s = n_s K mod m,
 *   L = K - sum q_s; the L sectors with the largest r_s get one more, among equal r_s the smaller s first (largest-remainder
 *   apportionment).  0 < m < K: q_s = n_s.  Then (m >= K):
 *     sum q_s = K      since sum n_s K = m K = m sum floor + sum r_s, sum r_s = m L with every r_s < m: 0 <= L < S, and L ones are added;
 *     winners have r_s > 0   since sum r_s = m L and every r_s <= m - 1, more than L of the r_s are positive (L > 0), and they come first;
 *     q_s <= n_s       since floor(n_s K / m) <= n_s K / m <= n_s, and for a winner n_s K / m is no integer: floor + 1 <= n_s.
 *   pcdet's min(n_s, ceil(ratio K)) gives a total that varies from frame to frame; this is its static-shape form.
 *   WALKS: sector s of frame f walks its own usable rows u_0 < u_1 < ... (input order) exactly as snowgpu_fps_device walks a frame --
 *   the same distance in T, the same tie rule -- for q_s samples: s_0 = u_0, then q_s - 1 rounds.  The frame's K slots hold the sectors'
 *   samples side by side, s = 0 .. S - 1.  With m < K the K - m trailing slots repeat the index of slot 0, with dist 0.  A frame with
 *   m = 0 is -1 / 0 / -1 as for snowgpu_fps_device.
 * Outputs, every shape static, every element written by every call:
 *   d_out_index, d_out_points (or NULL), d_out_dist (or NULL), d_out_usable (= m): as for snowgpu_fps_device; the first sample of every
 *                          sector has dist +inf
 *   d_out_sector_offsets   (F, S + 1) int32: slots [o_s, o_{s+1}) of the frame are sector s; o_S = min(m, K)
 *   d_out_sector_count     (F, S) int32: n_s
 *   d_out_sector_of        (N_total) int8, or NULL: the row's sector, -1 for an absent or unusable row
 *   d_out_reach2           (F, B) float64, or NULL (only with d_rois): reach2, 0 for an absent roi
 * With S = 1 and no rois, index, points, dist and usable are byte for byte those of snowgpu_fps_device.
 * Domain: that of snowgpu_fps_device and the bounds above; F B <= 2^31 - 1; F ceil(max_frame_rows / 1024) <= 2^27 - 1 (the tiles of the
 * classification); every output apart from the rows, the keep mask, the rois and every other output.  Anything else is SNOWGPU_E_INVALID.
 * An empty batch writes usable = 0, index = -1, points = 0, dist = -1, offsets and counts 0, and the reach.
 * One thread per row decides usable, near (the frame's rois as records in LDS, every one tried) and sector, every angle from the
 * correctly rounded atan2; the rows of a 1024-row tile are counted per sector by ballots, one workgroup per frame scans the tile counts
 * and makes the quotas, a second pass over the rows scatters x, y, z into one segment of scratch per (frame, sector) in input order, and
 * F S workgroups of 1024 threads run the walk of snowgpu_fps_device, each over its segment, in the tier its n_s asks for
 * (csrc/snowgpu_fps.hip, csrc/sg_fps_sectors.h).  Nothing depends on the arrival of atomics -- there are none --: two calls give identical
 * bytes.  Scratch in the context, grown on first use: that of snowgpu_fps_device (68 elements per frame instead of 8), one byte per row,
 * 4 S bytes per 1024-row tile, 4 S bytes per frame and 32 bytes per roi.  Up to one memset and six kernels on `stream`; nothing is read
 * on the host, nothing allocated after the first call of a size: capturable.
 */
int snowgpu_fps_sectors_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                               const void *d_rows, int dtype, const double *range6 /* host: x0 y0 z0 x1 y1 z1, or NULL */, int n_samples,
                               int n_features, const uint8_t *d_keep_in /* or NULL: all present */, int n_sectors,
                               const void *d_rois /* or NULL: no roi test */, int n_rois, int roi_features, double roi_margin,
                               int32_t *d_out_index, void *d_out_points /* or NULL */, void *d_out_dist /* or NULL */, int32_t *d_out_usable,
                               int32_t *d_out_sector_offsets, int32_t *d_out_sector_count, int8_t *d_out_sector_of /* or NULL */,
                               double *d_out_reach2 /* or NULL */, void *stream);

/*
 * BALL-QUERY NEIGHBOUR GROUPS around centres of an aligned batch: for every centre the first rows of its frame within a radius, the
 * grouping step of PV-RCNN's voxel set abstraction over the raw points and of the PointNet++ set-abstraction layers, with static shapes.
 * Frames, rows (N_total x 5, float32 or float64), frame offsets and the input keep mask as snowgpu_fps_device takes them.  F = n_frames,
 * K = n_centres per frame, R = n_radii (radius, samples) pairs, 1 <= R <= 4, S_i = n_samples[i], 1 <= S_i <= 64, S = sum of the S_i,
 * C = n_features in 3 .. 5.  The reference has no such op; the edge conventions are this library's, restated as brute-force NumPy by
 * tests/ball_reference.py, and chosen so that on ordinary data the result is what the pointnet2 ball_query op returns.
 *   A row is USABLE exactly as for snowgpu_fps_device: present, |x|, |y|, |z| <= 1e6 (false for NaN) and, with a range,
 *   lo_j <= (double)p_j < hi_j.  range6 may be NULL.
 *   CENTRES: d_centres is (F, K, Cq) in the rows' dtype, Cq = centre_features in 3 .. 5, columns 0 .. 2 x, y, z (the points of the
 *   keypoint stage go in as they are).  A centre is usable iff |x|, |y|, |z| <= 1e6; it need not lie in the range or be a row.
 *   MEMBERSHIP: all arithmetic in the rows' dtype T.  d = ((dx dx) + (dy dy)) + (dz dz), every operation rounded on its own, no fused
 *   multiply-add; r2_i = fl_T(fl_T(radius_i) fl_T(radius_i)).  Usable row j of frame f is in ball i of usable centre (f, k) iff
 *   d < r2_i: STRICT, as in the pointnet2 op.  A keypoint is in its own ball, a row at d == r2_i is out.  No square root takes part.
 *   RESULT: n = the rows in the ball.  count[f, k, i] = n, not saturated.  Slots 0 .. min(n, S_i) - 1 of the centre's segment i hold the
 *   min(n, S_i) SMALLEST batch row indices in the ball, ascending; the remaining slots repeat slot 0 (pointnet2's padding).  With n = 0,
 *   or an unusable centre, every slot is -1 and count is 0.  This is what a sequential walk in input order with an early stop returns;
 *   it depends on neither a cell order nor the arrival of atomics: two calls give identical bytes.
 * Outputs, every shape static, every element written by every call:
 *   d_out_index   (F, K, S) int32: the segments of the R pairs side by side
 *   d_out_count   (F, K, R) int32
 *   d_out_points  (F, K, S, C) in the rows' dtype, or NULL: columns 0 .. C - 1 of the indexed row, bit for bit; zero where the index is -1
 * Domain: radii finite, > 0 and <= 1e6; K >= 1 (K = 0 is refused: a call without a centre has nothing to write); F K S <= 2^31 - 1;
 * n_total < 2^31; no frame above 2^30 rows; dtype 0 or 1; the range as for snowgpu_fps_device; the outputs must not overlap the rows,
 * the keep mask or the centres.  Anything else is SNOWGPU_E_INVALID.  An empty batch writes index = -1, count = 0 and points = 0 with
 * one fill kernel (d_rows may be NULL).
 * The usable rows of every frame are filed in a uniform x-y grid (cell lists as snowgpu_dror_mask_device builds them; csrc/sg_ball.h:
 * the domain, the cell edge -- half the largest radius, wider where the cell budget asks for it -- and the window of a centre), then ONE
 * WAVE per centre walks the grid rows of its window, computes every distance once for all radii and keeps per pair its 64 smallest
 * indices in one register per lane by a bitonic sort and merge across the wave (csrc/snowgpu_ball.hip).
 * Scratch in the context, grown on first use: per frame one word per cell of the budget (1024 .. 81920) and one more, and per row two
 * words and three values of the rows' dtype.  One memset and four kernels on `stream`; nothing is read on the host, nothing allocated
 * after the first call of a size: capturable.
 */
int snowgpu_ball_query_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                              const void *d_rows, int dtype, const double *range6 /* host: x0 y0 z0 x1 y1 z1, or NULL */, int n_centres,
                              const void *d_centres, int centre_features, int n_radii, const double *radii /* host */,
                              const int *n_samples /* host */, int n_features, const uint8_t *d_keep_in /* or NULL: all present */,
                              int32_t *d_out_index, int32_t *d_out_count, void *d_out_points /* or NULL */, void *stream);

/*
 * RANGE-IMAGE PROJECTION of an aligned batch: every frame as an H x W image of its nearest returns, the first stage of the range-view
 * networks (RangeNet++, SalsaNext) and of the snow de-noisers among them (WeatherNet, 4DenoiseNet, LiSnowNet), with static shapes.
 * Frames, rows (N_total x 5, float32 or float64 = T), frame offsets and the input keep mask as snowgpu_voxelize_device takes them.
 * F = n_frames, H = height, W = width, C = n_features in 3 .. 5.  The reference has no such op; the edge conventions are this library's,
 * restated in NumPy by tests/range_reference.py, and chosen so that on ordinary data the result is what the RangeNet++ loader produces.
 *   PER ROW, in float64 on (double)x, (double)y, (double)z, every operation rounded on its own (no fused multiply-add), atan2 correctly
 *   rounded (csrc/sg_atan_cr.h), so that NumPy on glibc gives the same bits:
 *     r    = T( sqrt((x*x + y*y) + z*z) )             rounded once more to the rows' dtype: the value the image stores
 *     yaw  = -atan2(y, x)
 *     px   = (0.5 * (yaw / pi + 1.0)) * W
 *     col  = clip(floor(px), 0, W - 1)
 *   image rows by elevation (d_ring NULL; fov2 = (fov_up, fov_down) in radians):
 *     pitch = atan2(z, sqrt(x*x + y*y))               (= asin(z / r), without a function that is not correctly rounded)
 *     py    = (1.0 - (pitch - fov_down) / (fov_up - fov_down)) * H
 *     row   = clip(floor(py), 0, H - 1)               clamped as the RangeNet++ loader clamps, not dropped
 *   image rows by channel (d_ring: N_total int32, e.g. the input's column 4, which an aligned result has kept beside every row):
 *     row   = ring[i]
 *   A row is USABLE iff it is present, |x|, |y|, |z| <= 1e6 (false for NaN), T(lo) < r < T(hi) for the limits (lo, hi) -- both strict,
 *   compared in T; limits2 NULL is (0, +inf), which takes the origin out -- and, by channel, 0 <= ring < H.  x = y = 0 with z != 0 is
 *   usable: atan2(0, 0) = 0.
 *   Per pixel the WINNER is the usable row with the smallest r, compared as values of T; among equal r the smallest row index.
 *   It depends on no arrival of atomics: two calls give identical bytes.
 * Outputs, every shape static, every element written by every call:
 *   d_out_image     (F, 1 + C, H, W) in T: plane 0 the winner's r, planes 1 .. C its columns 0 .. C - 1 bit for bit; -1 in an empty pixel
 *   d_out_index     (F, H, W) int32: the winner as a row of the whole batch, -1 in an empty pixel
 *   d_out_pixel_of  (N_total) int32: every row's flat pixel f H W + row W + col, whether it won or not; -1 for absent and unusable rows
 *   d_out_count     (F, H, W) int32, or NULL: the usable rows that fell in the pixel
 * Domain: H, W >= 1; F H W <= 2^31 - 1; C in 3 .. 5; fov_down < fov_up, both within [-pi/2, pi/2] (not read by channel); 0 <= lo < hi,
 * neither NaN, hi may be +inf; n_total < 2^31; no frame above 2^30 rows; dtype 0 or 1; one of fov2 and d_ring; no output may overlap
 * the rows, the mask, the channels or another output.  Anything else is SNOWGPU_E_INVALID.  A batch without a row fills the image, the
 * index and the count and launches nothing else (d_rows and d_out_pixel_of may be NULL).
 * One 8-byte key per pixel in the context (8 F H W bytes, grown on first use), preset by a memset; one thread per row folds
 * bits(r) << 32 | row into its pixel by a 64-bit atomic min (float64 rows: bits(r), then a second pass over the rows for the smallest
 * index at that r); one thread per pixel gathers the winner (csrc/snowgpu_range.hip, csrc/sg_range.h).  An angle is evaluated by the
 * device library's atan2 where that provably decides the same pixel, by the correctly rounded one inside a guard band around every
 * pixel edge (csrc/sg_range.h derives the band): the bits are those of the definition.  Up to three memsets and three
 * kernels on `stream`; nothing is read on the host, nothing allocated after the first call of a size: capturable.
 */
int snowgpu_range_image_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                               const void *d_rows, int dtype, int height, int width,
                               const double *fov2 /* host, radians: up, down; NULL in channel mode */, const int32_t *d_ring /* or NULL */,
                               const double *limits2 /* host: lo, hi; NULL = (0, inf) */, int n_features,
                               const uint8_t *d_keep_in /* or NULL: all present */, void *d_out_image, int32_t *d_out_index,
                               int32_t *d_out_pixel_of, int32_t *d_out_count /* or NULL */, void *stream);

/*
 * NEAREST CENTRES OF EVERY ROW of an aligned batch: for every row the k nearest centres of its frame and their inverse-distance weights,
 * the way back from keypoints to rows -- pointnet2's three_nn + three_interpolate (k = 3), the feature-propagation half of PointNet++,
 * and with k = 1 the Voronoi labelling of the rows by the keypoints --, with static shapes.  Frames, rows (N_total x 5, float32 or
 * float64 = T), frame offsets and the input keep mask as snowgpu_ball_query_device takes them.  F = n_frames, K = n_centres per frame,
 * 1 <= k <= 8.  The reference has no such op; the edge conventions are this library's, restated as brute-force NumPy by
 * tests/nn_reference.py.
 *   A row is USABLE exactly as for snowgpu_fps_device: present, |x|, |y|, |z| <= 1e6 (false for NaN) and, with a range,
 *   lo_j <= (double)p_j < hi_j.  range6 may be NULL.
 *   CENTRES: d_centres is (F, K, Cq) in T, Cq = centre_features in 3 .. 5, columns 0 .. 2 x, y, z (the points of the keypoint stage go
 *   in as they are).  A centre is usable exactly as for snowgpu_ball_query_device: |x|, |y|, |z| <= 1e6; it need not lie in the range
 *   or be a row.
 *   DISTANCE: all arithmetic in T.  d = ((dx dx) + (dy dy)) + (dz dz), every operation rounded on its own, no fused multiply-add, no
 *   square root.
 *   RESULT for usable row i of frame f: order the usable centres of frame f by (d, centre number) lexicographically -- among equal
 *   distances the smaller centre number first.  With m usable centres in the frame, slots 0 .. min(k, m) - 1 of the row hold the first
 *   min(k, m) of them: index = the centre number in 0 .. K - 1 WITHIN THE FRAME, dist2 = d, bit for bit.  Slots beyond m hold index -1,
 *   dist2 +inf and weight 0, and so do all slots of a row that is absent or not usable.  Duplicate centres are distinct centres at equal
 *   d (a KeypointBatch of a short frame repeats its first): they come in centre order.
 *   WEIGHTS (d_out_weight, may be NULL), in float64, every operation rounded on its own: u_j = 1.0 / (sqrt((double)d_j) + 1e-8) for the
 *   filled slots, n = ((u_0 + u_1) + u_2) + ... in slot order, weight_j = T(u_j / n): pointnet2's 1 / (dist + 1e-8) normalisation.  A row
 *   that coincides with a centre has u = 1e8 there.
 * Outputs, every shape static, every element written by every call:
 *   d_out_index   (N_total, k) int32
 *   d_out_dist2   (N_total, k) T
 *   d_out_weight  (N_total, k) T, or NULL
 * Domain: K >= 1; 1 <= k <= 8; F K <= 2^31 - 1; n_total < 2^31; no frame above 2^30 rows; dtype 0 or 1; the range as for
 * snowgpu_fps_device; the outputs must overlap neither each other nor the rows, the keep mask or the centres.  Anything else is
 * SNOWGPU_E_INVALID.  A batch without a row has no element to write: nothing is launched (d_rows and the outputs may be NULL).
 * The result depends on neither a cell order nor the arrival of atomics: two calls give identical bytes.
 * The K centres of every frame are filed, not the rows: a uniform x-y grid of about K / 2 cells (16 .. 2048) over the range's x-y
 * rectangle (+-120 m without one), one workgroup per frame counting, scanning and scattering in LDS, one 16-byte record per centre
 * (32 for float64).  Then ONE LANE per row walks rings of growing Chebyshev radius around its cell, clipped to the occupied cells of
 * the frame, keeps its k best in registers and stops when the k-th distance is strictly below the squared gap to the nearest open side
 * of the visited block, deflated by 1e-6 (csrc/sg_nn.h: the grid rule, the bound and its derivation; csrc/snowgpu_nn.hip).
 * Scratch in the context, grown on first use: per frame one word per cell and five more, and one record per centre.  Two kernels on
 * `stream`; nothing is read on the host, nothing allocated after the first call of a size: capturable.
 */
int snowgpu_nearest_centres_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                   const void *d_rows, int dtype, const double *range6 /* host: x0 y0 z0 x1 y1 z1, or NULL */, int n_centres,
                                   const void *d_centres, int centre_features, int k, const uint8_t *d_keep_in /* or NULL: all present */,
                                   int32_t *d_out_index, void *d_out_dist2, void *d_out_weight /* or NULL */, void *stream);

/*
 * POINTS IN 3D BOXES of an aligned batch: for every row the labelled box of its frame that contains it, and for every box the number of
 * rows inside -- roiaware_pool3d.points_in_boxes_gpu (the point heads' target assignment), num_points_in_gt / filter_by_min_points and
 * the inside / outside mask of GT-sampling, recomputed after augmentation, with static shapes.  Frames, rows (N_total x 5, float32 or
 * float64 = T), frame offsets and the input keep mask as snowgpu_nearest_centres_device takes them.  F = n_frames, B = n_boxes per frame.
 * The definition is restated as brute-force NumPy by tests/box_reference.py.
 *   A row is USABLE when it is present and |x|, |y|, |z| <= 1e6 (false for NaN).  There is no range: a box is a range of its own.
 *   BOXES: d_boxes is (F, B, Cb) in T, Cb = box_features in 7 .. 10, 1 <= B <= 256; columns 0 .. 6 are cx, cy, cz, dx, dy, dz, heading
 *   (OpenPCDet's gt_boxes); further columns (class, velocity) are ignored.  A box is PRESENT when all seven values are finite,
 *   |cx|, |cy|, |cz| <= 1e6, 0 < dx, dy, dz <= 1e6, |heading| <= 1e6 and its pose passes the check below.  The zero rows that OpenPCDet
 *   pads gt_boxes with are absent by this rule.
 *   POSE: (c, s) per box, float64, (F, B, 2).  With d_pose_in NULL the device computes c = cos((double)heading), s = sin((double)heading)
 *   with the device library; otherwise the caller's values are used as they are.  A box whose pose is not finite or has
 *   |(c c + s s) - 1| > 1e-6 (float64, every operation rounded on its own) is absent.  d_out_pose, when given, receives the pose that
 *   was used, (0, 0) for an absent box.  This is the one place where the device library's rounding enters: everything below is defined
 *   from the pose, so it is exact whichever pose was used.
 *   MEMBERSHIP: all arithmetic in float64, every operation rounded on its own, no fused multiply-add.  sx = x - cx, sy = y - cy,
 *   sz = z - cz; lx = sx c + sy s, ly = sy c - sx s.  A usable row is inside a present box of its frame when |sz| <= dz / 2,
 *   |lx| < dx / 2 + 1e-5 and |ly| < dy / 2 + 1e-5: check_pt_in_box3d of pcdet's roiaware_pool3d -- z closed, x and y strict with its 1e-5
 *   margin, the box's z its CENTRE.  pcdet's op makes the same test in float32 with cosf / sinf of -heading: the two differ only for
 *   rows within float32 rounding of a face.
 * Outputs, every shape static, every element written by every call:
 *   d_out_box_of  (N_total) int32: the SMALLEST present box number of the row's frame that contains it, 0 .. B - 1 ("first box wins", as
 *                 pcdet's loop); -1 for a row in no box and for absent and unusable rows
 *   d_out_count   (F, B) int32, or NULL: the usable rows of frame f inside box b -- every containing box counts, overlaps included; 0 for
 *                 an absent box
 *   d_out_local   (N_total, 3) T, or NULL: (T)lx, (T)ly, (T)sz with respect to box_of -- Part-A2's intra-object part location before its
 *                 normalisation --, zeros where box_of is -1
 *   d_out_pose    (F, B, 2) float64, or NULL
 * Domain: 1 <= B <= 256; box_features in 7 .. 10; F B <= 2^31 - 1; n_total < 2^31; no frame above 2^30 rows; dtype 0 or 1; every output
 * apart from the rows, the keep mask, the boxes, the given pose and every other output.  Anything else is SNOWGPU_E_INVALID.  A batch
 * without a row writes zeros to the counts, writes the pose and launches nothing over rows (d_rows and d_out_box_of may be NULL).
 * The result depends on neither a cell order nor the arrival of atomics: two calls give identical bytes.
 * The B boxes of every frame are filed, not the rows: one workgroup per frame writes a record of eight doubles per box and marks every
 * present box, by atomicOr, in each cell of a 64 x 64 x-y grid over +-120 m that its footprint -- inflated for the margin, the pose
 * tolerance and the float64 rounding -- can touch; a cell is ceil(B / 64) 64-bit words, and the border cells reach to infinity.  Then
 * ONE LANE per row reads its cell's words and makes the membership test for every set bit, ascending; the counts are integer atomic
 * adds, equal boxes folded across the wave first (csrc/sg_box.h: the footprint bound and its derivation; csrc/snowgpu_box.hip).
 * Scratch in the context, grown on first use: per frame 4097 ceil(B / 64) words and B records.  Two kernels on `stream`, no memset;
 * nothing is read on the host, nothing allocated after the first call of a size: capturable as a linear graph.
 */
int snowgpu_points_in_boxes_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                   const void *d_rows, int dtype, int n_boxes, const void *d_boxes, int box_features,
                                   const double *d_pose_in /* or NULL */, const uint8_t *d_keep_in /* or NULL: all present */,
                                   int32_t *d_out_box_of, int32_t *d_out_count /* or NULL */, void *d_out_local /* or NULL */,
                                   double *d_out_pose /* or NULL */, void *stream);

/*
 * RoI POINT POOLING of an aligned batch: for every roi of a frame the first S rows inside the slightly enlarged box, in row order, and
 * each of them in the roi's own frame -- pcdet's roipoint_pool3d as PointRCNNHead.roipool3d_gpu calls it, the input of a point-based
 * second stage, with static shapes and nothing read on the host.  snowgpu_points_in_boxes_device cannot stand in for it: its box_of names
 * only the smallest containing box, and proposals overlap.  Frames, rows (N_total x 5, float32 or float64 = T), frame offsets and the input
 * keep mask as snowgpu_points_in_boxes_device takes them.  F = n_frames, M = n_rois per frame, S = n_samples, C = num_features.  The
 * definition is restated as brute-force NumPy by tests/roipool_reference.py.
 *   A row is USABLE exactly as for snowgpu_points_in_boxes_device: present and |x|, |y|, |z| <= 1e6 (false for NaN).
 *   ROIS: d_rois is (F, M, Cb) in T, Cb = roi_features in 7 .. 10, 1 <= M <= 512; columns 0 .. 6 are cx, cy, cz, dx, dy, dz, heading: the
 *   layout of gt_boxes, of the kept boxes of snowgpu_nms_device and of the rois of snowgpu_fps_sectors_device.
 *   ENLARGED BOX: centre and heading are kept; dx' = (double)dx + ew[0], dy' = (double)dy + ew[1], dz' = (double)dz + ew[2], each one
 *   float64 add -- pcdet's enlarge_box3d, where the width is added ONCE to each size.  extra_width3 NULL: zeros.
 *   A roi is PRESENT when the presence rule of snowgpu_points_in_boxes_device holds for the ENLARGED box -- all seven values finite, the
 *   1e6 bounds, 0 < dx', dy', dz' <= 1e6, the pose check -- AND its original dx, dy and dz are > 0.  Zero padding rows and the zero rows
 *   behind the count of snowgpu_nms_device are absent by the first rule when ew = 0; with ew > 0 a zero row would become a box of size ew,
 *   which the second rule forbids.
 *   POSE: as for snowgpu_points_in_boxes_device -- the caller's (F, M, 2) float64 (cos, sin) used as it is, or with NULL cos / sin of
 *   (double)heading from the device library; |(c c + s s) - 1| > 1e-6 makes the roi absent.  d_out_pose receives the pose that was used,
 *   (0, 0) for an absent roi.
 *   MEMBERSHIP: the library's one rule, on the enlarged record -- float64, every operation rounded on its own, no fused multiply-add:
 *   sx = x - cx, sy = y - cy, sz = z - cz; lx = sx c + sy s, ly = sy c - sx s; inside iff |sz| <= dz' / 2, |lx| < dx' / 2 + 1e-5 and
 *   |ly| < dy' / 2 + 1e-5.  pcdet's roipoint op makes its test in float32 with cosf / sinf of -heading: the two differ only for rows within
 *   float32 rounding of a face.  The 1e-5 margin is this library's rule as it stands (check_pt_in_box3d of roiaware_pool3d has it).  As far as
 *   recalled, roipoint_pool3d's own check_pt_in_box3d compares with dx / 2 and dy / 2 WITHOUT a margin; this was NOT CHECKED against
 *   pcdet's source.  If so, the two differ for rows within 1e-5 m of an x or y face as well.
 *   ORDER: the members of roi (f, m) are the usable rows of frame f inside it in ASCENDING ROW INDEX, cnt their number.
 * Outputs, every shape static, every element written by every call, nothing needs clearing:
 *   d_out_index   (F, M, S) int32: slot j < S holds the global row index of member j mod cnt when cnt > 0 -- pcdet's wrap-around fill,
 *                 idx[k] = idx[k % cnt]; every slot is -1 when cnt = 0, an absent roi or an empty one
 *   d_out_count   (F, M) int32: cnt, the full number of members, NOT clipped at S; 0 for an absent roi
 *   d_out_points  (F, M, S, C) T, or NULL: the first C columns of rows[index], bit copies; zeros where index is -1
 *   d_out_local   (F, M, S, 3) T, or NULL: (T)lx, (T)ly, (T)sz of that row with respect to its roi -- the head's canonical transformation,
 *                 centre subtracted and rotated by -heading, as d_out_local of snowgpu_points_in_boxes_device; zeros where index is -1
 *   d_out_pose    (F, M, 2) float64, or NULL
 *   Sizes: at F = 256, M = 128, S = 512 the index is 67 MB and the points at C = 4 float32 268 MB.
 * Domain: 1 <= M <= 512; 1 <= S <= 2048; C in 3 .. 5; Cb in 7 .. 10; every component of ew finite and in 0 .. 100; F M S max(C, 3) <=
 * 2^31 - 1; n_total < 2^31; no frame above 2^30 rows; F M (the 512-row runs of the longest frame) <= 2^31 - 1; dtype 0 or 1; every output
 * apart from the rows, the keep mask, the rois, the given pose and every other output.  Anything else is SNOWGPU_E_INVALID with a message.
 * A batch without a row writes -1, zeros and the pose and launches nothing over rows (d_rows may be NULL).  The result depends on neither
 * a cell order nor the arrival of atomics: two calls give identical bytes.
 * The enlarged rois are filed as the boxes of snowgpu_points_in_boxes_device are.  The rows of a frame are cut into runs of 512; one wave
 * owns a run, visits every roi marked in its rows' cells once per 64 rows and takes the ballot of the member lanes: lane order is row
 * order.  The walk runs twice -- the runs' counts, a scan over the runs of every (frame, roi), then the ranks -- which is the price of row
 * order without a sort; a last kernel resolves the wrap-around and writes points and local (csrc/sg_roipool.h, csrc/snowgpu_roipool.hip).
 * Scratch in the context, grown on first use: per frame 4097 ceil(M / 64) words, M records and M int32 per run.  Five kernels on `stream`,
 * no memset; nothing is read on the host, nothing allocated after the first call of a size: capturable as a linear graph.
 */
int snowgpu_roi_point_pool_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                  const void *d_rows, int dtype, int n_rois, const void *d_rois, int roi_features,
                                  const double *extra_width3 /* host, 3 doubles, or NULL = zeros */, int n_samples, int num_features,
                                  const double *d_pose_in /* or NULL */, const uint8_t *d_keep_in /* or NULL: all present */,
                                  int32_t *d_out_index, int32_t *d_out_count, void *d_out_points /* or NULL */, void *d_out_local /* or NULL */,
                                  double *d_out_pose /* or NULL */, void *stream);

/*
 * RoI-AWARE VOXEL POOLING of an aligned batch: every roi of a frame is cut into Gx Gy Gz sub-voxels along its own axes, and the features of
 * the rows inside each sub-voxel are max- and average-pooled -- pcdet's roiaware_pool3d (RoIAwarePool3d), the input of a Part-A2-style second
 * stage, with static shapes and nothing read on the host.  snowgpu_roi_point_pool_device cannot stand in for it: it keeps a roi's first S
 * rows as one list, and this op needs the members of every sub-voxel.  F = n_frames, M = n_rois per frame, G = Gx Gy Gz, T = max_points,
 * P = roi_capacity, Cf = feature_channels.  The definition is restated as brute-force NumPy by tests/roiaware_reference.py.
 *   SHARED RULES: frames, rows, frame offsets, the keep mask, USABLE rows, ROIS (1 <= M <= 512, Cb in 7 .. 10), the ENLARGED BOX
 *   (extra_width3 NULL: zeros -- Part-A2 passes none), PRESENCE, POSE and MEMBERSHIP are, word for word, those of
 *   snowgpu_roi_point_pool_device above (sg_roi_make, sg_box_inside).
 *   SUB-VOXEL OF A MEMBER: out_size3 = (Gx, Gy, Gz), each in 1 .. 16.  With lx, ly, sz the values the membership test saw and dx', dy', dz'
 *   the enlarged sizes THEMSELVES (not the test's half extents, whose x and y carry the 1e-5 margin), in float64, every operation rounded
 *   on its own, no fused multiply-add:
 *     ux = (lx + dx' / 2) / (dx' / Gx),  ix = min(max((int)floor(ux), 0), Gx - 1);   uy, iy likewise;   uz = (sz + dz' / 2) / (dz' / Gz), iz.
 *   The clamp is pcdet's: a member inside the 1e-5 margin beyond an x / y face lands in the edge voxel, a member on the closed upper z face
 *   in Gz - 1.  (The clamp is made on the floor before the conversion; a NaN quotient, which takes a dx' / Gx that underflows to 0, gives 0.)
 *   Flat voxel g = (ix Gy + iy) Gz + iz: pcdet's (out_x, out_y, out_z) layout.
 *   ORDER AND CAPS: the members of roi (f, m) are the usable rows of frame f inside it in ASCENDING ROW INDEX.  Only the FIRST P of them are
 *   distributed to voxels, 64 <= P <= 65536; within a voxel they stay in row order, and the first T of those are pooled, 1 <= T <= 128
 *   (pcdet's max_pts_each_voxel = 128 stores 127 rows beside their count: its default is T = 127).
 *   FEATURES: d_features is (N_total, Cf) float32, contiguous, one row per row of the batch, 1 <= Cf <= 256; or NULL -- then d_out_max,
 *   d_out_argmax and d_out_avg must be NULL too (but for a batch without a row, which has no feature to point to and writes them by Cf).
 * Outputs, every shape static, every element written by every call, nothing needs clearing:
 *   d_out_roi_count (F, M) int32: all members of the roi, clipped by neither cap; 0 for an absent roi
 *   d_out_count     (F, M, G) int32: the voxel's members among the roi's first P, NOT clipped at T
 *   d_out_index     (F, M, G, T) int32, or NULL: the global row numbers of the voxel's first T members, -1 behind them (no wrap-around)
 *   d_out_max       (F, M, G, Cf) float32, or NULL, and d_out_argmax (F, M, G, Cf) int32, or NULL: pcdet's loop per channel -- no winner at
 *                   the start; the pooled members are walked in order; a value wins when there is no winner and it is not NaN, or when it
 *                   is > the current maximum.  So the first of equal maxima wins, NaN never wins, -inf can win.  argmax is the winner's
 *                   global row, -1 without one; max is 0 where argmax is -1.
 *   d_out_avg       (F, M, G, Cf) float32, or NULL: the float32 sum of the pooled members' values, added one by one in row order starting
 *                   from +0, divided by (float)min(count, T), the division correctly rounded; 0 for an empty voxel.  NaN and inf propagate
 *                   as IEEE gives them.
 *   d_out_pose      (F, M, 2) float64, or NULL: as for snowgpu_roi_point_pool_device
 *   Sizes: at F = 16, M = 128, G = 12^3, Cf = 128 max, argmax and avg are 1.8 GB each; at T = 127 the index is 1.8 GB.
 * Domain: the ranges above; Cb in 7 .. 10; every component of ew finite and in 0 .. 100; F M G max(T, Cf) <= 2^31 - 1; F M P <= 2^31 - 1;
 * n_total < 2^31; no frame above 2^30 rows; F M (the 512-row runs of the longest frame) <= 2^31 - 1; dtype 0 or 1; every output apart from
 * the rows, the keep mask, the rois, the given pose, the features and every other output.  Anything else is SNOWGPU_E_INVALID with a message.
 * A batch without a row writes zeros, -1 and the pose and launches nothing over rows (d_rows may be NULL).  Nothing depends on the arrival
 * of an atomic: two calls give identical bytes.
 * The rois are filed, counted and ranked by the kernels of snowgpu_roi_point_pool_device, which leave every roi's first P members in row
 * order in scratch; one wave per roi then groups that list by voxel -- counts in LDS, a scan, and a second pass that places 64 members at
 * a time behind per-voxel cursors by ballots, lane order being row order --; one lane per (voxel, channel) pools (csrc/sg_roiaware.h,
 * csrc/snowgpu_roiaware.hip).  Scratch in the context, grown on first use: that of the pooling stage, twice F M P int32 (at F = 16, M = 128,
 * P = 8192: 67 MB each) and F M G int32.  Up to seven kernels on `stream`, no memset; nothing is read on the host, nothing allocated after
 * the first call of a size: capturable as a linear graph.
 */
int snowgpu_roi_voxel_pool_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                  const void *d_rows, int dtype, int n_rois, const void *d_rois, int roi_features,
                                  const double *extra_width3 /* host, 3 doubles, or NULL = zeros */, const int32_t *out_size3 /* host, 3 ints */,
                                  int max_points, int roi_capacity, const float *d_features /* or NULL */, int feature_channels,
                                  const double *d_pose_in /* or NULL */, const uint8_t *d_keep_in /* or NULL: all present */,
                                  int32_t *d_out_roi_count, int32_t *d_out_count, int32_t *d_out_index /* or NULL */, float *d_out_max /* or NULL */,
                                  int32_t *d_out_argmax /* or NULL */, float *d_out_avg /* or NULL */, double *d_out_pose /* or NULL */, void *stream);

/*
 * ROTATED BOX IoU AND NMS: pcdet's iou3d_nms family -- boxes_iou_bev, boxes_iou3d_gpu, nms_gpu -- with static shapes, nothing read on the
 * host.  snowgpu_boxes_iou_device gives the overlap of every box of one set with every box of another (the target layer's rois against
 * gt_boxes) and, without materialising the matrix, the best partner of every box; snowgpu_nms_device gives the keep list of scored
 * proposals in the layout the rois of snowgpu_fps_sectors_device and the boxes of snowgpu_points_in_boxes_device have.  The definition is
 * restated in NumPy by tests/iou_reference.py; csrc/sg_iou.h holds its C++, for the device and for the host.
 *   BOXES AND POSE: (F, B, Cb) in T = float32 or float64, Cb in 7 .. 10, columns 0 .. 6 cx, cy, cz, dx, dy, dz, heading; PRESENT and POSE
 *   exactly as for snowgpu_points_in_boxes_device: all seven finite, |cx|, |cy|, |cz| <= 1e6, 0 < dx, dy, dz <= 1e6, |heading| <= 1e6; the
 *   pose (c, s) the caller's (F, B, 2) float64 as it is, or with NULL cos / sin of (double)heading from the device library; a box with
 *   |(c c + s s) - 1| > 1e-6 is absent.  Zero rows are absent.  The half extents are hx = dx / 2, hy = dy / 2, hz = dz / 2 WITHOUT the
 *   1e-5 margin of the membership test (pcdet's IoU has none); the box's z is its CENTRE.
 *   Everything behind the pose is float64 with + - x /, comparisons and fabs only, every operation rounded on its own, no fused
 *   multiply-add, in the order written here.  There is no atan2 and no angular sort of intersection points.
 *   AREA(a, b), a clipped in b's frame:
 *     1. the corners of a in the order (+,+), (-,+), (-,-), (+,-): x = cxa + (lx ca - ly sa), y = cya + (lx sa + ly ca), lx = +-hxa, ly = +-hya;
 *     2. each into b's frame: sx = x - cxb, sy = y - cyb, u = sx cb + sy sb, v = sy cb - sx sb;
 *     3. the polygon is clipped against four half-planes in the order u <= hxb, -u <= hxb, v <= hyb, -v <= hyb (Sutherland-Hodgman).  For
 *        every edge (p, q) in order, q the next vertex and the first one behind the last: dp = +-p[axis], dq = +-q[axis]; a point is inside
 *        iff d <= h (the boundary is inside); p is emitted if it is inside; then, if exactly one of p and q is inside, the crossing is
 *        emitted: its clipped coordinate is exactly +-h, its other one p_o + t (q_o - p_o) with t = (h - dp) / (dq - dp) (the divisor is
 *        not 0: one of dp, dq is <= h, the other > h).  An empty polygon: the area is 0.
 *        CAPACITY: in exact arithmetic the polygon has at most 8 vertices.  In floating point it can have more (equal boxes, headings
 *        1 ulp apart: up to 10 were seen), but a pass over n vertices emits at most n + floor(n / 2) -- 4, 6, 9, 13, 19 -- and a polygon
 *        is held in 20 slots: no vertex is ever dropped, for any input (csrc/sg_iou.h; tests/host_harness/iou_clip.cpp asserts it).
 *     4. area = 0.5 |sum_i (u_i v_(i+1) - u_(i+1) v_i)|, summed sequentially from i = 0, the last term closing to vertex 0.
 *   area(a, b) and area(b, a) differ in their last bits: the IoU matrix uses area(a_m, b_b), NMS area(candidate, kept box).
 *   IoU, with A = dx dy and inter = area(a, b): BEV (mode 0) inter / max(Aa + Ab - inter, 1e-8).  3D (mode 1):
 *   h = max(min(cza + hza, czb + hzb) - max(cza - hza, czb - hzb), 0), I3 = inter h, V = (dx dy) dz, I3 / max(Va + Vb - I3, 1e-6) -- pcdet's
 *   epsilons; sums left to right.  Either box absent: exactly 0.  The value is stored as (T)iou.
 * snowgpu_boxes_iou_device, M = n_a boxes a and B = n_b boxes b per frame:
 *   d_out_iou       (F, M, B) T, or NULL: iou(a_m, b_b)
 *   d_out_best      (F, M) int32, or NULL: the smallest b with the largest IoU of a_m (compared in float64), provided that IoU is > 0;
 *                   otherwise -1 -- the target layer's gt_assignment
 *   d_out_best_iou  (F, M) T, or NULL: (T) of that IoU, 0 where best is -1 -- max_overlaps
 *   Domain: 1 <= M, B <= 9216; both feature counts in 7 .. 10; F M B <= 2^31 - 1; dtype 0 or 1; mode 0 or 1; at least one output; every
 *   output apart from the boxes, the given poses and every other output (the two box sets may be one).
 * snowgpu_nms_device, class-agnostic rotated NMS as nms_gpu, B = n_boxes per frame, d_scores (F, B) T:
 *   The CANDIDATES of a frame are its present boxes whose score is not NaN and has (double)score >= score_thresh.  They are RANKED by score
 *   descending (compared in T; -0 and +0 are equal), the smallest box number first among equals.  Walking the ranking, candidate j is
 *   suppressed iff some already KEPT box i has iou(j, i) > iou_thresh -- strict, compared in float64 before any rounding to T, with
 *   area(j, i), in the mode asked for; otherwise it is kept.  The walk stops after post_max kept.  There is no pre_max: callers take
 *   top-k first, as pcdet does in front of nms_gpu.
 *   d_out_index   (F, post_max) int32: the kept box numbers in rank order, -1 behind the count
 *   d_out_count   (F) int32: the kept boxes of the frame
 *   d_out_boxes   (F, post_max, Cb) T, or NULL: the kept boxes with all their columns, ZERO rows behind the count: a valid rois / gt_boxes
 *                 tensor as it stands
 *   d_out_scores  (F, post_max) T, or NULL: their scores, 0 behind the count
 *   d_out_kept    (F, B) uint8, or NULL: 1 for a kept box
 *   Domain: 1 <= post_max <= B <= 9216; box_features in 7 .. 10; F B <= 2^31 - 1; neither threshold NaN (score_thresh -inf: every score
 *   but NaN); dtype and mode as above; every output apart from the boxes, the scores, the given pose and every other output.
 * Anything outside a domain is SNOWGPU_E_INVALID.  Every element of every output is written by every call; two calls give identical bytes;
 * no atomic is used.  One lane per pair: the IoU runs one wave per box a over tiles of 64 records of b in LDS and folds best across the
 * wave; NMS ranks by counting and then sweeps LAZILY, one workgroup per frame: blocks of 64 ranked candidates are tested against the
 * boxes kept so far, then the block's own triangle is resolved in order -- candidates x kept pairs, no mask in memory
 * (csrc/snowgpu_iou.hip).  Scratch in the context, grown on first use: nine doubles per box, and for NMS an int32 per box.  Both entries
 * use the SAME record scratch: two calls on one context, of either entry, must be ordered on their streams; calls on streams that run
 * concurrently need a context each.  Three kernels
 * each on `stream`, no memset; nothing is read on the host, nothing allocated after the first call of a size: capturable as a linear graph.
 */
int snowgpu_boxes_iou_device(snowgpu_ctx *ctx, int n_frames, int n_a, const void *d_boxes_a, int a_features, int n_b, const void *d_boxes_b,
                             int b_features, int dtype, int mode, const double *d_pose_a /* or NULL */, const double *d_pose_b /* or NULL */,
                             void *d_out_iou /* or NULL */, int32_t *d_out_best /* or NULL */, void *d_out_best_iou /* or NULL */, void *stream);
int snowgpu_nms_device(snowgpu_ctx *ctx, int n_frames, int n_boxes, const void *d_boxes, int box_features, const void *d_scores, int dtype, int mode,
                       double iou_thresh, double score_thresh, int post_max, const double *d_pose_in /* or NULL */, int32_t *d_out_index,
                       int32_t *d_out_count, void *d_out_boxes /* or NULL */, void *d_out_scores /* or NULL */, uint8_t *d_out_kept /* or NULL */,
                       void *stream);

/*
 * PER-FRAME WEATHER in one aligned call.  snowgpu_augment_wet_batch_device_aligned_masked applies one weather to every frame, its wet
 * settings host scalars that a captured graph bakes in.  Here every frame brings a record of 8 doubles in DEVICE memory,
 *     d_weather[f] = [snow, wet, water_height, pavement_depth, wet_noise_floor, power_factor, delta, 0]
 * snow and wet are the frame's gates, 0.0 or 1.0 -- anything else is UNDEFINED (the kernels only promise that +-0.0 is off); the five
 * values after them replace the wet scalars of the masked chain.  flat_earth, replace, the beam divergence and the snowfall stage's
 * noise_floor stay per call.  Arguments: those of snowgpu_augment_wet_batch_device_aligned_masked with d_weather (n_frames x 8) in place
 * of the five wet doubles.  d_keep_in may be NULL (all rows present); d_weather NULL is SNOWGPU_E_INVALID; d_perm must be NULL.
 *
 * Frame f comes back, byte for byte -- rows, keep bytes, counts, statistics, d_out_thr_poly row and flag -- as an existing entry called
 * on the same batch (same d_keep_in, tables, planes, polynomials, camera crop) with frame f's values as its scalars returns it:
 *   snow wet   frame f equals                                                                              d_out_flags[f]
 *    1    1    snowgpu_augment_wet_batch_device_aligned_masked                                             its flag (0 or 1)
 *    1    0    snowgpu_augment_batch_device_aligned_masked; d_out_counts[f] = keep bytes set               2
 *    0    1    snowgpu_wet_ground_batch_device_aligned on the input rows and d_keep_in; statistics (0, 0, 0)
 *              and polynomial row as the masked entry returns them for a frame with no present row          its flag
 *    0    0    every row bit for bit, keep = d_keep_in (1 if NULL), counts = present rows, statistics (0, 0, 0)   2
 * Flag 2 is "wet stage not asked"; flag 1 keeps its meaning (asked, fewer than 1000 present ground rows).
 * A frame with snow = 0 and wet = 0 is never looked at, as an absent row is not: NaN, a range beyond the grid or a channel that is no
 * laser set no status word there.  A frame with snow = 0 is never looked at by the snowfall stage: SNOWGPU_E_GROUND of the device
 * prepass can only come from snow = 1 frames.  Out of place (d_out_rows != d_rows) the rows of a gated frame are copied; in place with
 * d_out_keep == d_keep_in nothing of it is touched.
 *
 * How: the snow gate joins the input mask in the masked front end -- a frame left out reaches the per-beam kernels as an empty frame and
 * costs them nothing, its keep bytes are written as they came --, the wet kernels read their settings from the frame's record, and a
 * frame whose wet gate is off takes the path of a frame with too few ground rows, without its rows being read.  Because the gates are
 * device data the host cannot know that every frame is on: an all-on batch without a mask pays the masked front end too (one more copy
 * of the rows and three small kernels) that snowgpu_augment_wet_batch_device_aligned does not.
 * The wet stage honours snowgpu_set_wet_estimation ('poly' draws are keyed by the frame's index in the batch, which a gate does not
 * change) and snowgpu_set_wet_lines, and keeps the NULL-wet-plane rule of the chain.  The contract is the device entries': asynchronous
 * on `stream`, no allocation after the first call of a size, no host read, capturable into a HIP graph.  It refuses what the aligned
 * entries refuse.
 */
int snowgpu_augment_weather_batch_device_aligned(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows,
                                                 const int64_t *d_frame_offsets, const void *d_rows, int dtype,
                                                 const int32_t *d_table_ids, double beam_divergence_deg, const double *d_thr_poly,
                                                 const double *d_plane, double noise_floor, const int32_t *d_perm /* NULL */,
                                                 const uint8_t *d_keep_in /* NULL: all present */, void *d_out_rows, uint8_t *d_out_keep,
                                                 int64_t *d_out_counts, int64_t *d_out_stats, double *d_out_thr_poly, int32_t *d_status,
                                                 void *stream, const double *d_wet_plane, const double *d_weather /* n_frames x 8 */,
                                                 int flat_earth, int replace, int32_t *d_out_flags);

/*
 * The draw of those records -- and of every frame's table ids -- on the device: what a training loader does per sample (the reference's
 * production loop runs five (rate, velocity) pairs times two modes, precompute.py:20-21, :70-104; its viewer varies the wet settings,
 * pointcloud_viewer.py:2814-2821) as one small kernel, one wave per frame.  Asynchronous on `stream` and capturable; the step is read
 * from DEVICE memory, so a replayed graph that also holds a `step += 1` draws anew on every replay.
 *   d_set_ids    n_sets x n_lasers table ids (snowgpu_upload_table): set s is one snowfall setting, one table per laser
 *   plan         HOST memory, read during the call: the gates' probabilities, the choices of water height and pavement depth, the three
 *                wet settings every frame shares, and whether the tables of the set are shuffled over the lasers (simulation.py:78, :482-486)
 *   d_table_ids  n_frames x n_lasers;   d_weather  n_frames x 8 (see above)
 * Limits: n_sets <= 64, n_lasers <= 128, n_frames <= 2^22, 1 <= n_water, n_pave <= 16, probabilities in [0, 1]; else SNOWGPU_E_INVALID.
 * With W(b) the four words of Philox4x32-10 under key `seed` at counter (step, frame f, 0x57544852 + b):
 *   block 0       snow = w0 < T(p_snow), wet = w1 < T(p_wet) with T(p) = min(2^32, floor(p 2^32)): 0 is never, 1 is always;
 *                 set = (w2 n_sets) >> 32; water index = (w3 n_water) >> 32
 *   block 1       pavement index = (w0 n_pave) >> 32
 *   permutation   order = 0 .. L-1; for i = L-1 down to 1, k = L-1-i: r = word k % 4 of block 2 + k / 4, j = (r (i + 1)) >> 32, swap
 *                 order[i], order[j]; shuffle = 0: the identity.  d_table_ids[f][c] = d_set_ids[set][order[c]]
 * Every draw is made whether or not its gate is on: a gate never shifts another frame's or another field's draw.  The stream is Philox,
 * not Python's random: parity with the reference's own shuffle is distributional.
 */
typedef struct snowgpu_weather_plan {
    double p_snow, p_wet;
    int32_t n_water, n_pave;
    double water_heights[16], pavement_depths[16];
    double wet_noise_floor, power_factor, delta;
    int32_t shuffle;
} snowgpu_weather_plan;
int snowgpu_draw_weather_device(snowgpu_ctx *ctx, int n_frames, int n_lasers, int n_sets, const int32_t *d_set_ids /* n_sets x n_lasers */,
                                const snowgpu_weather_plan *plan /* host */, uint64_t seed, const uint64_t *d_step,
                                int32_t *d_table_ids /* n_frames x n_lasers */, double *d_weather /* n_frames x 8 */, void *stream);

/*
 * PROPOSAL TARGET SAMPLING: which S = roi_per_image of a frame's M rois the second stage trains on, and their targets -- the step of
 * OpenPCDet's ProposalTargetLayer (sample_rois_for_rcnn, subsample_rois, sample_bg_inds) between the best overlaps of
 * snowgpu_boxes_iou_device and the two pooling stages, with static shapes, nothing read on the host and a seeded draw.  pcdet is not part
 * of the reference checkout: the definition below is THIS LIBRARY'S, modelled on pcdet's layer as recalled, and was NOT CHECKED against
 * pcdet's source.  pcdet draws from torch's global generator (randperm / randint); here the draws are Philox words, so parity with
 * pcdet's random stream is distributional, as for the weather draw.  The definition is restated in NumPy and Python integers by
 * tests/targets_reference.py; csrc/sg_targets.h holds its C++, for the device and for the host.
 *   INPUTS, F = n_frames, M = n_rois, B = n_gt, T = float32 or float64: d_rois (F, M, Cb) T and d_gt_boxes (F, B, Cg) T, Cb and Cg in 7 .. 10,
 *   columns 0 .. 6 cx, cy, cz, dx, dy, dz, heading; d_overlap (F, M) T and d_assignment (F, M) int32 -- d_out_best_iou and d_out_best of
 *   snowgpu_boxes_iou_device as they stand (max_overlaps, gt_assignment); d_pose (F, M, 2) float64 (cos, sin) or NULL; cfg in HOST memory,
 *   read during the call; seed; d_step, a uint64 in DEVICE memory read by the kernel.
 *   CANDIDATES: roi m is a candidate iff it is PRESENT by the rule of snowgpu_points_in_boxes_device (all seven finite, the 1e6 bounds,
 *   0 < dx, dy, dz <= 1e6, the pose check -- under the given pose or cos / sin of (double)heading from the device library) and its overlap
 *   is not NaN.  The zero rows behind the count of snowgpu_nms_device are therefore NEVER sampled; pcdet samples its zero padding as easy
 *   background.  An assignment outside 0 .. B - 1 counts as -1.
 *   CLASSES, ov = (double)overlap, fg_thresh = min(reg_fg_thresh, cls_fg_thresh): FG ov >= fg_thresh; HARD ov < reg_fg_thresh and
 *   ov >= cls_bg_thresh_lo; EASY ov < cls_bg_thresh_lo.  Each class is the list of its candidates in ASCENDING roi number, n_fg, n_hard,
 *   n_easy their lengths, n_bg = n_hard + n_easy.  FG and HARD overlap when reg_fg_thresh > cls_fg_thresh, as in pcdet.
 *   DRAWS: r_k = word k % 4 of Philox4x32-10 under key `seed` at counter (step, frame f, 0x524F4953 + k / 4), the argument positions of
 *   the weather draw above.  Slot k always uses r_k, whatever the other slots do.  A pick WITH REPLACEMENT from a list of n is
 *   list[(r_k n) >> 32].
 *   SLOTS hold fg picks, then hard picks, then easy picks:
 *     (a) n_fg > 0 and n_bg > 0: fg_this = min(fg_per_image, n_fg) picks WITHOUT replacement by a forward Fisher-Yates walk -- for
 *         i = 0 .. fg_this - 1: j = i + ((r_i (n_fg - i)) >> 32), swap list[i] and list[j], the pick is list[i] --; bg_this = S - fg_this;
 *     (b) n_fg > 0, n_bg = 0: S fg picks with replacement;
 *     (c) n_fg = 0, n_bg > 0: bg_this = S;
 *     (d) no candidate: every slot is empty.
 *   BACKGROUND PICKS of count n, all with replacement: with both lists non-empty hard_this = min((int)((double)n hard_bg_ratio), n_hard)
 *   -- one float64 product, truncated -- and the rest easy picks; with one list non-empty all n from it.
 * Outputs, every shape static, every element written by every call; an empty slot gives -1 / 0:
 *   d_out_index       (F, S) int32: the roi number
 *   d_out_rois        (F, S, Cb) T: bit copies of the picked rois, zero rows in empty slots: a rois tensor as it stands
 *   d_out_roi_iou     (F, S) T: the pick's overlap
 *   d_out_gt_index    (F, S) int32: its assignment
 *   d_out_gt_of_rois  (F, S, Cg) T: a bit copy of gt_boxes[f, gt_index], a ZERO row where gt_index is -1 (pcdet hands back gt 0 there;
 *                     only reg_valid slots use the gt, and those have one when the overlaps are the IoU stage's)
 *   d_out_reg_valid   (F, S) uint8: ov > reg_fg_thresh
 *   d_out_cls_label   (F, S) T, -1 in an empty slot.  cls_mode 0 ('roi_iou'): 1 if ov > cls_fg_thresh; 0 if ov < cls_bg_thresh; otherwise
 *                     (ov - cls_bg_thresh) / (cls_fg_thresh - cls_bg_thresh) in float64, each operation rounded on its own, then (T).
 *                     cls_mode 1 ('cls'): 1 if ov > cls_fg_thresh; -1 if cls_bg_thresh < ov < cls_fg_thresh; otherwise 0
 *   d_out_segments    (F, 3) int32: (fg_this, hard_this, easy_this);   d_out_class_count (F, 3) int32: (n_fg, n_hard, n_easy)
 *   d_out_pose        (F, S, 2) float64, or NULL: the pose used for the pick, (0, 0) in an empty slot
 *   d_out_gt_local    (F, S, 7) T, or NULL: the head's canonical transformation of the gt into the roi's frame, [lx, ly, lz, dx, dy, dz,
 *                     heading_label]; zeros where the slot is empty, gt_index is -1 or one of the gt's seven values is not within 1e6 (NaN
 *                     and inf included).  sx = gx - cx, sy = gy - cy, lz = gz - cz; lx = sx c + sy s, ly = sy c - sx s -- float64, every
 *                     operation rounded on its own, no fused multiply-add; dx, dy, dz the gt's, bit copies.  With pmod(x) = fmod(x, 2 pi),
 *                     plus 2 pi when that is negative, +0 when it is zero: ry = pmod(h_roi); hl = pmod(h_gt - ry); if pi / 2 < hl < 3 pi / 2
 *                     then hl = pmod(hl + pi); if hl > pi then hl -= 2 pi; hl clamped to [-pi / 2, pi / 2]; stored as (T)hl.  The constants
 *                     are the doubles nearest pi, 2 pi, pi / 2 and 3 pi / 2 (NumPy's np.pi, 2 * np.pi, 0.5 * np.pi, 1.5 * np.pi).
 * Domain: 1 <= M, B <= 9216; Cb, Cg in 7 .. 10; 1 <= S <= 1024; 0 <= fg_per_image <= S; the five thresholds finite;
 * cls_fg_thresh > cls_bg_thresh; hard_bg_ratio in [0, 1]; cls_mode 0 or 1; F S max(Cb, Cg) <= 2^31 - 1; dtype 0 or 1; every output apart
 * from every input and every other output.  Anything else is SNOWGPU_E_INVALID with a message.
 * One kernel on `stream`, one workgroup per frame: the classes of every roi, the three ordered lists by wave ballots and prefix sums in
 * LDS (uint16 entries), the Philox blocks one per lane, the walk without replacement on one lane in LDS (at most S dependent steps),
 * then one lane per slot (csrc/snowgpu_targets.hip).  No atomics, no memset, no scratch, nothing read on the host, nothing allocated:
 * capturable as a linear graph; a replayed graph that also holds a `step += 1` draws anew on every replay.  Two calls with one step give
 * identical bytes.  The frame's position in the batch is part of the counter: frame f of a batch equals a one-frame call only at f = 0.
 */
typedef struct snowgpu_roi_sampler {
    int32_t roi_per_image, fg_per_image;
    double reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo, hard_bg_ratio;
    int32_t cls_mode;
} snowgpu_roi_sampler;
int snowgpu_sample_rois_device(snowgpu_ctx *ctx, int n_frames, int n_rois, const void *d_rois, int roi_features, const void *d_overlap,
                               const int32_t *d_assignment, int n_gt, const void *d_gt_boxes, int gt_features, int dtype,
                               const snowgpu_roi_sampler *cfg /* host */, uint64_t seed, const uint64_t *d_step, const double *d_pose /* or NULL */,
                               int32_t *d_out_index, void *d_out_rois, void *d_out_roi_iou, int32_t *d_out_gt_index, void *d_out_gt_of_rois,
                               uint8_t *d_out_reg_valid, void *d_out_cls_label, int32_t *d_out_segments, int32_t *d_out_class_count,
                               double *d_out_pose /* or NULL */, void *d_out_gt_local /* or NULL */, void *stream);

/*
 * ANCHOR TARGET ASSIGNMENT: which anchors of a first stage are positive, background or ignored in every frame, and which gt a positive
 * regresses to -- the step of OpenPCDet's AxisAlignedTargetAssigner (assign_targets, assign_targets_single) between the augmentation and
 * the anchor head's loss, with static shapes and nothing read on the host.  pcdet is not part of the reference checkout: the definition
 * below is THIS LIBRARY'S, modelled on pcdet's assigner as recalled, and was NOT CHECKED against pcdet's source.  It is restated as
 * brute-force NumPy by tests/anchors_reference.py; csrc/sg_anchors.h holds its C++, for the device and for the host.
 *   INPUTS, F = n_frames, A = n_anchors, B = n_gt, NC = n_classes, T = float32 or float64: d_anchors (A, Ca) T, Ca in 7 .. 10, SHARED by all
 *   frames, columns 0 .. 6 cx, cy, cz, dx, dy, dz, heading; d_anchor_class (A) int32, the class number of each anchor; d_gt_boxes
 *   (F, B, Cg) T, Cg in 8 .. 10, column 7 the class; matched and unmatched, NC doubles each in HOST memory, read during the call, class c at
 *   [c - 1].
 *   ARITHMETIC: float64 computed from (double) of the inputs, every operation rounded on its own, no fused multiply-add, no transcendental
 *   function: NumPy gives the same bytes.
 *   PRESENCE: an anchor is present iff the presence rule of snowgpu_points_in_boxes_device holds for its seven columns (all finite, the
 *   1e6 bounds, 0 < dx, dy, dz <= 1e6; no pose is involved) and 1 <= anchor_class <= NC.  A gt is present iff the same rule holds and its
 *   column 7 is integral with a value in 1 .. NC; zero rows are padding.  An absent anchor has label -1, gt_index -1 and iou 0 and takes
 *   part in nothing; an absent gt takes part in nothing, its gt_count is 0.
 *   NEAREST AXIS-ALIGNED BEV BOX of a box (cx, cy, ., dx, dy, ., h), PI the double nearest pi: r = |h - floor(h / PI + 0.5) PI|;
 *   (ex, ey) = (dx, dy) if r < PI / 4 (the double 0.7853981633974483), else (dy, dx); x0 = cx - ex / 2, x1 = cx + ex / 2, y0 and y1 likewise.
 *   OVERLAP of anchor a and gt g: ix = max(min(ax1, gx1) - max(ax0, gx0), 0), iy likewise, inter = ix iy; area = (x1 - x0) (y1 - y0);
 *   iou = inter / max((area_a + area_g) - inter, 1e-6).
 *   PER PRESENT ANCHOR of class c: over the frame's present gts of class c in ascending g, best is the largest iou (0 without such a gt),
 *   arg the SMALLEST g that reaches it; arg = -1 if best is not > 0.
 *   PER PRESENT GT of class c: top is the largest iou over the present anchors of class c; if top > 0, every such anchor with
 *   iou(a, g) == top is FORCED.
 *   LABEL: positive (label c, gt_index arg) iff forced or best >= matched[c]; a forced anchor is assigned ITS OWN arg, not the gt that
 *   forced it (pcdet's behaviour).  Otherwise background iff best < unmatched[c]; otherwise ignored.  A class without a present gt in the
 *   frame is all background.
 * Outputs, every shape static, every element written by every call:
 *   d_out_label     (F, A) int32: the class for a positive, 0 for background, -1 for ignored or absent
 *   d_out_gt_index  (F, A) int32: the gt number for a positive, -1 otherwise
 *   d_out_count     (F, 3) int32: positives, backgrounds, ignored; absent anchors are in none of them
 *   d_out_gt_count  (F, B) int32: the positives assigned to each gt
 *   d_out_iou       (F, A) T, or NULL: best, rounded once to T; 0 for an absent anchor
 * Domain: 1 <= A; 1 <= B <= 256; Ca in 7 .. 10; Cg in 8 .. 10; 1 <= NC <= 16; 0 < unmatched[c] <= matched[c] <= 1; F A <= 2^31 - 1; dtype 0
 * or 1; every output apart from every input and every other output.  Anything else is SNOWGPU_E_INVALID with a message.
 * Departures from pcdet: float64 instead of float32; the smallest gt among equal maxima, where torch's argmax is unspecified; absent
 * anchors and gts; no pos_fraction sampling and no match_height (3D IoU); the box coder and the direction targets stay the caller's
 * arithmetic on the matched gts.
 * Four kernels on `stream` (csrc/snowgpu_anchors.hip): the gt records (48 bytes each) into context scratch with the frame's top words and
 * gt_count zeroed -- no memset --; one lane per (frame, anchor) walking, in LDS, the frame's gts near the box around its workgroup's 256
 * anchors (every other gt meets them at exactly 0), the wave's maximum per gt by a cross-lane reduction and one 64-bit integer atomicMax
 * on the bits of the non-negative double per (wave, gt), which does not depend on the order of arrival; the same walk again by the same
 * function, compared with top, gt_count by integer atomic adds, the workgroup's three label counts stored to scratch; their sums per
 * frame.  No sort, nothing read on the host, nothing allocated after the first call of a size, no floating-point atomic: capturable as
 * a linear graph, and two calls give identical bytes.  The records are scratch of the context: calls on streams that are not ordered
 * against each other need a context each.
 */
int snowgpu_assign_anchors_device(snowgpu_ctx *ctx, int n_frames, int n_anchors, const void *d_anchors, int anchor_features,
                                  const int32_t *d_anchor_class, int n_gt, const void *d_gt_boxes, int gt_features, int dtype, int n_classes,
                                  const double *matched /* host */, const double *unmatched /* host */, int32_t *d_out_label, int32_t *d_out_gt_index,
                                  int32_t *d_out_count, int32_t *d_out_gt_count, void *d_out_iou /* or NULL */, void *stream);

/*
 * CENTRE HEATMAP TARGETS: the class heatmaps, the centre pixels with their fractional offsets and the slots of the gts of every frame --
 * the step of OpenPCDet's CenterHead (assign_targets, assign_target_of_single_head, with centernet_utils' gaussian_radius and
 * draw_gaussian_to_heatmap) between the augmentation and a centre head's loss, with static shapes and nothing read on the host.  pcdet is
 * not part of the reference checkout: the definition below is THIS LIBRARY'S, modelled on pcdet's CenterHead and centernet_utils as
 * recalled, and was NOT CHECKED against pcdet's source.  It is restated as sequential NumPy by tests/centers_reference.py;
 * csrc/sg_centers.h holds its C++, for the device and for the host.
 *   INPUTS, F = n_frames, B = n_gt, T = float32 or float64: d_gt_boxes (F, B, Cg) T, Cg in 8 .. 10, columns 0 .. 6 cx, cy, cz, dx, dy, dz,
 *   heading, column 7 the class; cfg in HOST memory, read during the call: (x0, y0) the origin of the point-cloud range, (vx, vy) the
 *   voxel's edges, stride the feature map's stride, (W, H) = (width, height) the feature map, NC = n_classes, NH = n_heads,
 *   class_head[c - 1] the head of class c, M = max_objs, o = gaussian_overlap, min_radius, outside (0 clamp, 1 drop).
 *   ARITHMETIC: float64 computed from (double) of the inputs, every operation rounded on its own, no fused multiply-add, in exactly the
 *   parenthesisation written here (a b c is (a b) c, as C and Python read it).
 *   PRESENCE: a gt is present iff the presence rule of snowgpu_points_in_boxes_device holds for its seven columns (all finite, the 1e6
 *   bounds, 0 < dx, dy, dz <= 1e6; no pose is involved) and its column 7 is integral with a value in 1 .. NC -- the rule of
 *   snowgpu_assign_anchors_device; zero rows are padding.  An absent gt has state 0 and takes part in nothing.  The head of a present gt
 *   of class c is class_head[c - 1].
 *   CENTRE: coord_x = ((x - x0) / vx) / stride, coord_y = ((y - y0) / vy) / stride.  With outside = drop, a gt that is not in
 *   0 <= coord_x < W and 0 <= coord_y < H has state 2 and takes part in nothing.  Otherwise, and always with outside = clamp,
 *   c = min(max(coord, 0), size - 0.5) on either axis (size = W or H); ci = trunc(c); offset = c - ci, which is exact, rounded once to T.
 *   RADIUS: h = (dx / vx) / stride, w = (dy / vy) / stride and
 *     b1 = h + w;            c1 = w * h * (1 - o) / (1 + o);   r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2
 *     b2 = 2 * (h + w);      c2 = (1 - o) * w * h;             r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2
 *     b3 = -2 * o * (h + w); c3 = (o - 1) * w * h;             r3 = (b3 + sqrt(b3 * b3 - 16 * o * c3)) / 2
 *   (r3 keeps pcdet's division by 2, not by 2 a); m = r1, then r2 if r2 < m, then r3 if r3 < m; radius = min_radius unless m >= min_radius
 *   (so also for a NaN), else 512 if m >= 512, else trunc(m): radius = min(max(trunc(min(r1, r2, r3)), min_radius), 512).  For 0 < o < 1,
 *   r3 <= 2 sqrt(o (1 - o) w h) <= sqrt(w h) <= (h + w) / 2 <= r1 <= r2: in exact arithmetic r3 is always the minimum.
 *   SLOTS: per frame and head, the present gts of that head that were not dropped take the slots 0, 1, ... in ascending g; those beyond M
 *   have state 3 and are not drawn (pcdet does not draw them either); the others have state 1.
 *   HEAT: for a drawn gt of class c with d = 2 radius + 1, sigma = d / 6, den = 2 * sigma * sigma: at every pixel (px, py) of the map with
 *   |px - cix| <= radius and |py - ciy| <= radius, ex = px - cix, ey = py - ciy, v = float32(exp(-(ex * ex + ey * ey) / den)).
 *   heatmap[f, c - 1, py, px] is the maximum of v over the frame's drawn gts of class c, 0 where there is none.
 *   WHY THE BYTES AGREE WITH AN exp IN IT: the argument of exp is the same double on the device and in NumPy; both exps are faithful, not
 *   correctly rounded, so the float32 agree as long as the float64 value stays away from the float32 rounding midpoints.  For every radius
 *   0 .. 512 and every distinct ex ex + ey ey of its patch (14.6 million values) the nearest value lies 15.0 float64 ulp from a midpoint
 *   (radius 473, ex ex + ey ey = 147293); tests/test_centers_reference.py repeats the walk and asks for more than 4 ulp: one for NumPy's
 *   exp, one for the device library's, two spare.  The 1 ulp of the device library's double exp is SUPPOSED: the figure is recalled from
 *   the table of ROCm's HIP math API documentation, not read from a copy of it.  The cap of 512 is what makes the walk exhaustive: it is
 *   not to be raised without walking again.
 * Outputs, every shape static, every element written by every call:
 *   d_out_heatmap   (F, NC, H, W) float32 whatever T: channel c - 1 is class c; a head's map is the channels of its classes
 *   d_out_gt_index  (F, NH, M) int32: the gt of the slot, -1 when empty
 *   d_out_ind       (F, NH, M) int32: ciy W + cix, 0 when empty
 *   d_out_mask      (F, NH, M) uint8: 1 in a filled slot
 *   d_out_offset    (F, NH, M, 2) T: the fractional part of the centre, x then y; 0 when empty
 *   d_out_radius    (F, NH, M) int32: the Gaussian radius, 0 when empty
 *   d_out_count     (F, NH) int32: the filled slots
 *   d_out_state     (F, B) uint8: 0 absent, 1 drawn, 2 outside and dropped, 3 no slot left
 * The regression targets of a slot -- offset, z, the logarithms of the sizes, cos and sin of the heading, the extra columns -- are the
 * caller's arithmetic on d_out_gt_index: log, cos and sin stay out of the kernels and out of the byte-for-byte claim.
 * Domain: 1 <= B <= 256; Cg in 8 .. 10; 1 <= NC <= 16; 1 <= NH <= 16; 0 <= class_head[c - 1] < NH; 1 <= M <= 512; 1 <= W, H and
 * F NC H W <= 2^31 - 1; x0, y0 finite; vx, vy positive and finite; stride >= 1; 0 < o < 1; 0 <= min_radius <= 512; outside 0 or 1; dtype 0
 * or 1; every output apart from the gt boxes and from every other output.  Anything else is SNOWGPU_E_INVALID with a message.
 * Departures from pcdet: float64 where pcdet computes in float32, so a radius can differ by one where pcdet's float32 truncates on the
 * other side; the cap of 512 on the radius; absent gts (pcdet stops at the first zero row of a frame's padding); the `outside` option
 * (pcdet always clamps the centre and, separately, skips a gt whose clamped pixel leaves the map, which cannot happen after the clamp);
 * the heat channels by global class, not re-labelled per head; gaussian2D's rule "h < eps max -> 0" is omitted because it is vacuous: the
 * smallest value over all radii up to 512 is about 1.26e-4, far above 2^-52 (the no-GPU test asserts it).
 * Two kernels on `stream` (csrc/snowgpu_centers.hip): one workgroup of 256 per frame, lane = gt -- presence, centre, radius, head, the
 * rank within the head by wave ballots and a prefix over the four waves in LDS, the frame's slot table cleared and filled in LDS and then
 * written out one store per element, state, count and a record of 24 bytes per gt into context scratch --; then one workgroup per
 * (tile of 64 x 16 pixels, class, frame): the frame's records in LDS, the ascending list of the class's drawn gts whose patch meets the
 * tile by a ballot and a prefix sum, every lane the maximum over that list for its four pixels, 0 included.  No memset, no atomics, no
 * sort, nothing read on the host, nothing allocated after the first call of a size: capturable as a linear graph, and two calls give
 * identical bytes.  The records are scratch of the context: calls on streams that are not ordered against each other need a context each.
 */
typedef struct snowgpu_center_cfg {
    double x0, y0, vx, vy, gaussian_overlap;
    int32_t stride, width, height, n_classes, n_heads, max_objs, min_radius, outside;
    int32_t class_head[16];
} snowgpu_center_cfg;
int snowgpu_assign_centers_device(snowgpu_ctx *ctx, int n_frames, int n_gt, const void *d_gt_boxes, int gt_features, int dtype,
                                  const snowgpu_center_cfg *cfg /* host */, float *d_out_heatmap, int32_t *d_out_gt_index, int32_t *d_out_ind,
                                  uint8_t *d_out_mask, void *d_out_offset, int32_t *d_out_radius, int32_t *d_out_count, uint8_t *d_out_state,
                                  void *stream);

/*
 * GROUND-TRUTH OBJECT PASTE: database objects written into the absent slots of an aligned batch, with their boxes appended to the gt
 * boxes and the scene rows in their place cleared -- the step of OpenPCDet's DataBaseSampler (the gt_sampling augmentor) in front of the
 * snowfall stage, with static shapes, nothing read on the host and a seeded draw.  pcdet is not part of the reference checkout: the
 * definition below is THIS LIBRARY'S, modelled on pcdet's sampler as recalled, and was NOT CHECKED against pcdet's source.  It is restated
 * in NumPy and Python integers by tests/paste_reference.py; csrc/sg_paste.h holds its C++, for the device and for the host.
 *   INPUTS, F = n_frames, B = n_gt, T = float32 or float64: the aligned batch (d_rows (N, 5) T, d_frame_offsets, d_keep_in (N) bytes or NULL:
 *   every row present); d_gt_boxes (F, B, Cb) T, Cb in 8 .. 10, columns 0 .. 6 cx, cy, cz, dx, dy, dz, heading, column 7 the class; d_pose_in
 *   (F, B, 2) float64 (cos, sin) or NULL; THE BANK, O objects of P points: d_bank_points (P, 5) T -- x, y, z, intensity, channel as cropped
 *   from real sweeps, positions kept --, d_bank_offsets (O + 1) int64, d_bank_boxes (O, 8) T with the class in column 7, classes ascending
 *   over the objects, d_bank_pose (O, 2) float64, d_class_offsets 18 int32: the objects of class c = 1 .. 16 are
 *   [class_offsets[c], class_offsets[c + 1]), L_c their number; sample_groups, NC = n_classes int32 in HOST memory, n_c = sample_groups[c - 1]
 *   the number of objects of class c a frame should hold (pcdet's SAMPLE_GROUPS), Q = sum n_c; extra_width3 in HOST memory or NULL (zeros);
 *   seed; d_step, a uint64 in DEVICE memory read by the kernel.
 *   ARITHMETIC: float64 from (double) of the inputs, every operation rounded on its own, no fused multiply-add.
 *   PRESENT: a gt or a bank box is present by the rule of snowgpu_points_in_boxes_device under its pose -- for a gt the given pose, or
 *   cos / sin of (double)heading from the device library when d_pose_in is NULL; for a bank box the bank's.  cnt_c = the present gts of the
 *   frame whose column 7 is integral and equals c.
 *   SLOTS: class c owns slots s_c .. s_c + n_c - 1 in ascending class order, s_c the prefix sum of the n_c.  Slot q = s_c + j is ACTIVE
 *   iff j < max(n_c - cnt_c, 0) and L_c > 0.  Its object is class_offsets[c] + ((r_q L_c) >> 32), r_q = word q % 4 of Philox4x32-10 under
 *   key `seed` at counter (step, frame f, 0x50415354 + q / 4), the argument positions of the weather draw above.  Objects are drawn WITH
 *   replacement; duplicates collide and are settled by the sweep.
 *   COLLISION: candidate a collides with box b iff AREA(a, b) > 0, AREA the BEV clip of a in b's frame of snowgpu_boxes_iou_device (half
 *   extents, no margin); both boxes present.
 *   SWEEP over q ascending, free_left starting as the number of rows of the frame that are absent on input.  A slot that is not inactive
 *   takes the LOWEST-NUMBERED of the states 2 .. 5 whose condition holds, else 1:
 *     0  the slot is inactive (its object is -1);
 *     5  the drawn bank box is not present (it collides with nothing);
 *     2  the candidate collides with a present gt of the frame;
 *     3  the candidate collides with an earlier PASTED candidate;
 *     4  the object's point count exceeds free_left;
 *     1  otherwise: the object is pasted and free_left decreases by its point count.
 *   This is greedy in slot order.  It is NOT pcdet's all-pairs rejection, which also rejects a candidate for a neighbour that is itself
 *   rejected.
 *   REMOVAL: a row that is present on input and usable (|x|, |y|, |z| <= 1e6) is tested against every pasted box, enlarged ONCE by the
 *   extra width as snowgpu_roi_point_pool_device enlarges a roi (pcdet's REMOVE_EXTRA_WIDTH; a box the enlargement makes absent removes
 *   nothing), by the membership rule of snowgpu_points_in_boxes_device.  A row inside any such box gets keep 0; its row bytes stay.  Pasted
 *   rows are never tested.
 *   PLACEMENT: the frame's rows that are absent on input, in ascending row index, are its free list.  The pasted objects take it front to
 *   back in slot order, each object's points in bank order as bit copies of all five columns, keep 1, source B + q.  Unused free slots keep
 *   their input bytes and keep 0.  Absent rows are never read as numbers.
 * Outputs, every shape static, every element written by every call:
 *   d_out_rows      (N, 5) T and d_out_keep (N) bytes: the batch after the paste, same offsets
 *   d_out_gt_boxes  (F, B + Q, Cb) T: rows 0 .. B - 1 bit copies of the input; row B + q the 8 bank columns of slot q's object when it was
 *                   pasted, zeros in columns 8 and 9; otherwise a zero row
 *   d_out_object    (F, Q) int32: the bank object slot q drew, -1 for an inactive slot
 *   d_out_state     (F, Q) int32: as numbered above
 *   d_out_source    (N) int32, or NULL: B + q for a pasted row, -1 for every other row
 *   d_out_count     (F, 4) int32: objects pasted, rows pasted, scene rows removed, free slots on input
 *   d_out_pose      (F, B + Q, 2) float64, or NULL: the pose used, (0, 0) for absent boxes and unpasted slots
 * Domain: 1 <= Q <= 64; 1 <= NC <= 16; 1 <= B, B + Q <= 256; Cb in 8 .. 10; n_c >= 0; the extra width finite, in 0 .. 100;
 * F (B + Q) Cb <= 2^31 - 1; N, P, O < 2^31; a frame of at most 2^30 rows; d_step not NULL; dtype 0 or 1; every output apart from every input
 * and every other output -- there is no in-place form.  Anything else is SNOWGPU_E_INVALID with a message.  The bank's offsets and class
 * offsets are device data and are trusted: they must ascend and end at P and O.
 * Three kernels on `stream` (csrc/snowgpu_paste.hip): one wave per 512-row run counts the absent rows (only with a mask); one workgroup
 * per frame scans the counts, counts the gt classes, draws, clips the Q x B and Q x Q pairs into one 64-bit word per side by LDS
 * atomicOr, sweeps on one lane and writes the per-slot outputs and the frame's scratch record; one lane per row copies, tests or fills.
 * The removed count is an integer add per workgroup.  No memset, no floating-point atomic, nothing read on the host, nothing allocated
 * after the first call of a size: capturable as a linear graph, and two calls give identical bytes.  The scratch is the context's: calls on
 * streams that are not ordered against each other need a context each.  The frame's position in the batch is part of the counter.
 */
int snowgpu_paste_objects_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                 const void *d_rows, int dtype, int n_gt, const void *d_gt_boxes, int gt_features, const double *d_pose_in /* or NULL */,
                                 int64_t n_bank_points, int64_t n_bank_objects, const void *d_bank_points, const int64_t *d_bank_offsets,
                                 const void *d_bank_boxes, const double *d_bank_pose, const int32_t *d_class_offsets, int n_classes,
                                 const int32_t *sample_groups /* host */, const double *extra_width3 /* host, or NULL */, uint64_t seed,
                                 const uint64_t *d_step, const uint8_t *d_keep_in /* or NULL */, void *d_out_rows, uint8_t *d_out_keep,
                                 void *d_out_gt_boxes, int32_t *d_out_object, int32_t *d_out_state, int32_t *d_out_source /* or NULL */,
                                 int32_t *d_out_count, double *d_out_pose /* or NULL */, void *stream);

/*
 * SCENE TRANSFORMS: the geometric augmentation behind gt_sampling -- OpenPCDet's random_world_flip, random_world_rotation and
 * random_world_scaling and, per object, the noise of random_local_translation / rotation / scaling and of SECOND's noise_per_object -- on
 * an aligned batch and its gt boxes, with static shapes, nothing read on the host and a seeded draw.  pcdet and SECOND are not part of the
 * reference checkout: the definition below is THIS LIBRARY'S, modelled on pcdet's augmentor_utils and SECOND's per-object noise as
 * recalled, and was NOT CHECKED against their source.  It is restated in NumPy and Python integers by tests/scene_reference.py;
 * csrc/sg_scene.h holds its C++, for the device and for the host.
 *   PLACE IN THE CHAIN: BEHIND the weather stages and range_image(ring=), which need rows in the sensor frame (range, beam and channel),
 *   and IN FRONT of everything that groups or labels: voxelize, the keypoint stages, ball_query, points_in_boxes for labels, assign_anchors.
 *   INPUTS, F = n_frames, B = n_boxes, T = float32 or float64: the aligned batch (d_rows (N, 5) T, d_frame_offsets, d_keep_in (N) bytes or
 *   NULL: every row present); d_gt_boxes (F, B, Cb) T, Cb in 7 .. 10, columns 0 .. 6 cx, cy, cz, dx, dy, dz, heading; d_pose_in (F, B, 2)
 *   float64 (cos, sin) or NULL; in HOST memory: flip (bit 0: the x axis is asked for, bit 1: the y axis), rotation2 and scaling2 (lo, hi;
 *   NULL: the part is off), tries (the tries per box, 0: NO LOCAL PART, the next three are not read), local_translation3 (ax, ay, az: a
 *   component is uniform in -a .. a), local_rotation2 and local_scaling2 (lo, hi), NULL each: off; seed; d_step, a uint64 in DEVICE
 *   memory read by the kernel; d_box_of (N) int32 or NULL: the box of every row as snowgpu_points_in_boxes_device gives it for THESE
 *   boxes under THIS pose -- with NULL and a local part the stage runs that stage's kernels itself, into scratch.
 *   ARITHMETIC: float64 from (double) of the inputs, every operation rounded on its own, no fused multiply-add; one rounding to T at the
 *   store.  A part that is off has the identity's values -- 0, (cos, sin) = (1, 0), 1 -- and goes through the same arithmetic, so it changes
 *   no value (a -0 may become +0).
 *   DRAWS: Philox4x32-10 under key `seed` at counter (step, frame f, 0x5846524D + b), the argument positions of the weather draw above.
 *   Block 0 is the world block: flip_x iff the x axis is asked for and w0 < 2^31, flip_y likewise with w1, theta from w2, sigma from w3.
 *   Blocks 1 + 2 (i T + t) and the next hold the five words of try t of box i: tx, ty, tz, delta from the first, s from w0 of the second.
 *   A uniform value is lo + ((double)w 2^-32) (hi - lo), the difference, the product and the sum rounded each.  A part that is off draws
 *   nothing but keeps its word positions.  cos / sin of theta and of every delta come from the device library; they are the only
 *   transcendental calls, and what they returned is in d_out_world and d_out_tries.
 *   PRESENT: a gt is present by the rule of snowgpu_points_in_boxes_device under its pose -- the given pose, or cos / sin of
 *   (double)heading from the device library when d_pose_in is NULL.
 *   OBJECT SWEEP, per frame, i ascending over the present gts: candidate (i, t) is box i with centre + (tx, ty, tz), dims s and the pose
 *   (c cos delta - s sin delta, s cos delta + c sin delta), all float64, nothing rounded to T.  It COLLIDES iff AREA(candidate, current_j)
 *   > 0 for some present j != i, AREA the BEV clip of snowgpu_boxes_iou_device (half extents, no margin, no test in z); current_j is the
 *   settled float64 record of box j for j < i -- moved or not -- and its original record for j > i.  The smallest t that does not collide
 *   is taken: state 1, and the candidate becomes the settled record.  If every try collides the box stays: state 2.  Every try of a
 *   present box is tested, also those behind the one taken.  This is greedy in box order, as SECOND's loop is; it is NOT a joint search,
 *   and a box is never tested against its own original place.
 *   ROWS: a row that is absent (keep 0) or unusable (not |x|, |y|, |z| <= 1e6) is a bit copy; an absent row is never read as a number.
 *   Any other row: (1) if box_of[row] = i >= 0 and box i has state 1, subtract the ORIGINAL centre, rotate by delta (x' = x cos - y sin,
 *   y' = x sin + y cos), multiply x, y, z by s, add the centre, then the translation; (2) the world part in pcdet's order: flip x
 *   (y = -y), flip y (x = -x), rotate by theta, multiply x, y, z by sigma.  Columns 3 and 4 are bit copies.
 *   BOXES: a present box: the local part where the state is 1 -- centre + t, dims s, heading + delta --, then flip x: cy = -cy, heading =
 *   -heading; flip y: cx = -cx, heading = -(heading + pi), pi the float64 nearest; the centre rotated by theta and heading + theta; columns
 *   0 .. 5 multiplied by sigma.  The heading is NOT wrapped.  Columns 7 and up are bit copies: the class is in column 7 here; VELOCITY
 *   COLUMNS ARE OUT OF SCOPE and are not rotated.  An absent box is a bit copy with state 0.  The output pose is composed from the pose
 *   used: the angle-addition formulas for delta and theta, exact sign changes for the flips ((c, s) -> (c, -s) about x, (-c, s) about y);
 *   no new transcendental call.
 * Outputs, every shape static, every element written by every call:
 *   d_out_rows      (N, 5) T; may BE d_rows, the in-place form: a row is read and written by its own lane only
 *   d_out_keep      (N) bytes: 1 for a row present on input, else 0 -- the input mask, carried for the next stage
 *   d_out_gt_boxes  (F, B, Cb) T
 *   d_out_world     (F, 8) float64: flip_x, flip_y (0 or 1), cos theta, sin theta, theta, sigma, 0, 0
 *   d_out_state     (F, B) int32: 0 absent, or no local part; 1 moved; 2 every try collided
 *   d_out_tried     (F, B) int32: the try taken, -1 otherwise
 *   d_out_local     (F, B, 8) float64: tx, ty, tz, cos delta, sin delta, delta, s, 0 of the try taken; the identity otherwise
 *   d_out_pose      (F, B, 2) float64, or NULL: the pose of the OUTPUT boxes, (0, 0) for an absent box
 *   d_out_tries     (F, B, tries, 8) float64, or NULL: per try tx, ty, tz, cos delta, sin delta, delta, s, collided (0 or 1); the
 *                   identity for an absent box
 * Domain: 1 <= B <= 256; Cb in 7 .. 10; flip in 0 .. 3; tries in 0 .. 16; every range finite with lo <= hi; scaling ranges above 0; the
 * local translation finite, in 0 .. 100; F B max(tries, 1) 10 <= 2^31 - 1; N < 2^31; a frame of at most 2^30 rows; d_step not NULL; dtype 0
 * or 1; every output apart from every input and every other output, but d_out_rows, which may be d_rows itself (not a part of it).
 * Anything else is SNOWGPU_E_INVALID with a message.  d_box_of is device data and is trusted to be this batch's; a value outside
 * 0 .. B - 1 is a row in no box.
 * Kernels on `stream` (csrc/snowgpu_scene.hip): with a local part, a row and no d_box_of, the two of snowgpu_points_in_boxes_device; one
 * workgroup per frame for the records, the draws and the sweep (the (t, j) pairs of a box spread over the lanes, an LDS OR per try); one
 * lane per row.  No memset, no atomic whose arrival shows, nothing read on the host, nothing allocated after the first call of a size:
 * capturable as a linear graph, and two calls give identical bytes.  The scratch is the context's: calls on streams that are not ordered
 * against each other need a context each.  The frame's position in the batch is part of the counter.
 */
int snowgpu_transform_scene_device(snowgpu_ctx *ctx, int n_frames, int64_t n_total, int64_t max_frame_rows, const int64_t *d_frame_offsets,
                                   const void *d_rows, int dtype, int n_boxes, const void *d_gt_boxes, int box_features, const double *d_pose_in /* or NULL */,
                                   int flip, const double *rotation2 /* host, or NULL */, const double *scaling2 /* host, or NULL */, int tries,
                                   const double *local_translation3 /* host, or NULL */, const double *local_rotation2 /* host, or NULL */,
                                   const double *local_scaling2 /* host, or NULL */, uint64_t seed, const uint64_t *d_step,
                                   const int32_t *d_box_of /* or NULL */, const uint8_t *d_keep_in /* or NULL */, void *d_out_rows, uint8_t *d_out_keep,
                                   void *d_out_gt_boxes, double *d_out_world, int32_t *d_out_state, int32_t *d_out_tried, double *d_out_local,
                                   double *d_out_pose /* or NULL */, double *d_out_tries /* or NULL */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNOWGPU_H */
