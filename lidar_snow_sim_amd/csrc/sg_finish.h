// sg_finish.h -- what the kernels that finish a batch share (snowgpu_compact.hip: compaction, aligned finish, camera crop;
// snowgpu_mask.hip: the masked aligned finish and the FOV mask): the camera-FOV test, the keep decision about one sorted position, the
// tile counts of a block and the per-frame scan over them.  Device code only; include after sg_common.h, sg_kutil.h and sg_row.h.
#pragma once

// get_fov_flag(calib.lidar_to_rect(xyz), (h, w), calib) (simulation.py:39-47, :535-536) in float64, fixed operation order.
// The projection is OpenPCDet's (pcdet/utils/calibration_kitti.py, the reference's un-vendored submodule lib/OpenPCDet:
// parity unpinned, SURVEY 8 c): rect_to_img divides the image coordinates by the RECTIFIED point's z, not by the third
// homogeneous coordinate -- the two differ by P2[2][3], which real KITTI files carry (~ 3e-3) --, and the depth is that
// coordinate minus P2[2][3].
__device__ __forceinline__ bool sg_in_fov(const SgFov &v, double x, double y, double z)
{
    double r[3];
    for (int j = 0; j < 3; ++j) r[j] = ((x * v.m[j] + y * v.m[3 + j]) + z * v.m[6 + j]) + v.m[9 + j];
    double h[3];
    for (int j = 0; j < 3; ++j) h[j] = ((r[0] * v.p[4 * j] + r[1] * v.p[4 * j + 1]) + r[2] * v.p[4 * j + 2]) + v.p[4 * j + 3];
    const double u = h[0] / r[2], w = h[1] / r[2];
    const double depth = h[2] - v.p[11];
    return u >= 0 && u < v.img_w && w >= 0 && w < v.img_h && depth >= 0;
}

// per frame: tile offsets of the kept rows and the statistics (simulation.py:522-530).  diff2 (per frame: twice the intensity-
// difference sum of the attenuated beams, final once the per-beam kernels are through) may be null: the pre-augment crop has none.
// One WAVE (all 64 lanes call it): lane l takes tiles l, l + 64, .. -- the counts come in one round of loads per 64 tiles and are summed by
// shuffles (one thread walking the tiles waited for every load in turn: 21 us for a sweep's 47 tiles, a tenth of a single sweep's chain).
// tile_cnt / tile_mv may have been written by other blocks of the running launch (k_compact_count's last block): read past the L1.
__device__ __forceinline__ void sg_compact_scan_frame(int f, int64_t n, const int32_t *tile_cnt, int32_t *__restrict__ tile_base, int64_t *__restrict__ out_counts,
                                                      int64_t *__restrict__ out_stats, const unsigned long long *diff2, int64_t max_tiles,
                                                      const int32_t *tile_mv, int32_t *__restrict__ tile_mv_base, int64_t *__restrict__ out_mv_counts)
{
    const int lane = threadIdx.x & 63;
    const int64_t tiles = (n + SG_TILE - 1) / SG_TILE;
    const volatile int32_t *vc = tile_cnt + (int64_t)f * max_tiles, *vm = tile_mv ? tile_mv + (int64_t)f * max_tiles : nullptr;
    int run = 0, mrun = 0;
    int64_t att = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += 64) {
        const int64_t t = t0 + lane;
        const int c = t < tiles ? vc[t] : 0;
        const int m = (vm && t < tiles) ? vm[t] : 0;
        const int kc = c & 0xffff;
        int ik = kc, im = m, ia = c >> 16;       // inclusive prefix of the kept / moved counts, total of the attenuated
        for (int o = 1; o < 64; o <<= 1) {
            const int a = __shfl_up(ik, o), b = __shfl_up(im, o);
            if (lane >= o) { ik += a; im += b; }
            ia += __shfl_xor(ia, o);
        }
        if (t < tiles) {
            tile_base[(int64_t)f * max_tiles + t] = run + ik - kc;
            if (vm) tile_mv_base[(int64_t)f * max_tiles + t] = mrun + im - m;
        }
        run += __shfl(ik, 63); mrun += __shfl(im, 63); att += ia;
    }
    if (lane != 0) return;
    if (out_mv_counts) out_mv_counts[f] = mrun;
    out_counts[f] = run;
    out_stats[f * 3 + 0] = att;              // num_attenuated (:525)
    out_stats[f * 3 + 1] = n - run;          // num_removed (simulation.py:522, + the camera crop :538)
    const double diff_sum = diff2 ? (double)(long long)((const volatile unsigned long long *)diff2)[f] / 2.0 : 0.0;
    out_stats[f * 3 + 2] = att > 0 ? (int64_t)(diff_sum / (double)att) : 0;   // :527-530 int()
}

// The decision about one sorted position (simulation.py:518-520, :532-540), shared by k_compact_count and k_finish_aligned: the one place it
// is written down.  keep = (label == 2) | (intensity > p0 d^2 + p1 d + p2), d the ORIGINAL range, d^2 in the row dtype (simulation.py:465,
// :469).  `row` is the original row (global memory, or the caller's registers), rc the record (slot references resolved), dd_rng the range
// the pass over all rows left (have_rng).
struct SgDecision { bool keep, noise_ok, is_att; };

template <typename T>
__device__ __forceinline__ SgDecision sg_row_decision(const T *row, uint32_t rc, T dd_rng, bool have_rng, const SgFov &fov, double p0, double p1, double p2)
{
    const int lab_i = (int)((rc >> SG_REC_LABEL_SHIFT) & 3u);
    // Without the camera crop the decision needs the label, the (new or original) intensity and the original range only: a
    // beam the pass over all rows simulated left its range in rng, and the record holds the intensity unless the beam came
    // back unchanged from a later kernel -- those, and rows without a laser, read the row as before.
    const bool from_rec = have_rng && !fov.enabled && !(rc & SG_REC_COPY) && (lab_i != 0 || (rc & SG_REC_HAS_I));
    SgDecision d;
    if (from_rec) {
        const T dd = dd_rng;
        const T dd2 = dd * dd;
        const double thr = (p0 * (double)dd2 + p1 * (double)dd) + p2;
        d.noise_ok = (lab_i == 2) || ((double)(T)(int)(rc & 255u) > thr);
        d.is_att = lab_i == 1;
        d.keep = d.noise_ok;
    } else {
        const SgRow<T> o = sg_rebuild_row<T>(row, rc);
        const T dd2 = o.dd * o.dd;
        const double thr = (p0 * (double)dd2 + p1 * (double)o.dd) + p2;
        d.noise_ok = (o.lab == (T)2) || ((double)o.i > thr);
        d.is_att = o.lab == (T)1;
        d.keep = d.noise_ok;
        if (fov.enabled && d.keep) d.keep = sg_in_fov(fov, (double)o.x, (double)o.y, (double)o.z);   // :532-540
    }
    return d;
}

// What a block of k_compact_count / k_finish_aligned does once its threads have decided their rows: c = kept | attenuated << 16 and mv
// (kept label-2 rows) summed over the block into the tile's words; for small batches the frame's scan by the block that completes it.
__device__ __forceinline__ void sg_tile_counts_done(int f, int64_t n, int c, int mv, int32_t *__restrict__ tile_cnt, int64_t max_tiles, int32_t *__restrict__ tile_mv,
                                                    unsigned long long *__restrict__ tiles_done, int32_t *__restrict__ tile_base, int64_t *__restrict__ out_counts,
                                                    int64_t *__restrict__ out_stats, const unsigned long long *__restrict__ diff2,
                                                    int32_t *__restrict__ tile_mv_base, int64_t *__restrict__ out_mv_counts)
{
    __shared__ int s[4], s2[4], s_last;
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_down(c, o); mv += __shfl_down(mv, o); }
    if ((threadIdx.x & 63) == 0) { s[threadIdx.x >> 6] = c; s2[threadIdx.x >> 6] = mv; }
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_cnt[(int64_t)f * max_tiles + blockIdx.x] = s[0] + s[1] + s[2] + s[3];   // kept | attenuated << 16 (a tile has 1024 rows)
        if (tile_mv) tile_mv[(int64_t)f * max_tiles + blockIdx.x] = s2[0] + s2[1] + s2[2] + s2[3];
        // Small batches (tiles_done != null): the block that completes a frame scans its tiles -- what k_compact_scan does as a launch of its
        // own: one link less on the chain.  Not for large batches: the device-scope fence this needs writes back the L2 of the block's XCD
        // (eight XCDs, eight L2s), and 32 768 of them made this kernel 1.37 ms long on 256 sweeps instead of 0.15.
        if (tiles_done) {
            __threadfence();
            const unsigned long long tiles = (unsigned long long)((n + SG_TILE - 1) / SG_TILE);
            s_last = atomicAdd(&tiles_done[f], 1ull) == tiles - 1;
            if (s_last) __threadfence();
        }
    }
    if (tiles_done) {                                 // (kernel argument: uniform)
        __syncthreads();
        if (s_last && threadIdx.x < 64)
            sg_compact_scan_frame(f, n, tile_cnt, tile_base, out_counts, out_stats, diff2, max_tiles, tile_mv, tile_mv_base, out_mv_counts);
    }
}
