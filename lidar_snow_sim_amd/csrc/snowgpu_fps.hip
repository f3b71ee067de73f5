// snowgpu_fps.hip -- farthest-point keypoints of aligned batches (snowgpu_fps_device; definition: include/snowgpu.h, the usable test, the
// distance, the candidate key and the tier capacities: sg_fps.h).  Two kernels on one stream:
//   k_fps          ONE workgroup of 1024 threads per frame -- the rounds of a frame cannot run side by side, the frames of a batch can.
//                  (a) the usable rows of the frame, compacted in input order into scratch (x, y, z apart, the source row, t = +inf): a
//                      ballot per wave and sixteen wave counts through LDS per 1024 rows; m = their number, chosen on the device;
//                  (b) the K - 1 rounds.  m within a resident tier: x, y, z and t of every row stay in registers (P rows per lane, row
//                      k 1024 + thread in slot k), two barriers a round -- the sixteen wave candidates through LDS, then the winner's
//                      coordinates from the lane that holds them.  Beyond: the coordinates stream from scratch in 16-byte pieces, t is
//                      read and written in LDS (tier 2: t of the frame fits 156 KiB) or in scratch alike, one barrier a round, the
//                      winner's coordinates read back from scratch.
//                  It writes the winner's POSITION among the usable rows into d_out_index, and its t into d_out_dist; -1 for m = 0.
//   k_fps_finish   every (frame, sample): position -> row of the batch, and the row's first C columns into d_out_points.
// A workgroup never waits for another one; nothing spins, nothing is launched per round.  The candidate fold is a maximum of integers:
// results are identical from run to run.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see lidar_snow_sim_amd/build.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sg_common.h"
#include "sg_fps.h"
#include "sg_launch.h"

// ---- the wave's largest key, in lane 63: DPP row shifts, then the last lane of a row to the rows after it (as sg_beam.h scans) -------------
template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint32_t fps_dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);      // a lane without a source reads 0: "no candidate"
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ SgFpsKey<float> fps_step(SgFpsKey<float> k)
{
    const uint32_t lo = fps_dpp<CTRL, ROW_MASK>((uint32_t)k.w), hi = fps_dpp<CTRL, ROW_MASK>((uint32_t)(k.w >> 32));
    return sg_fps_fold(k, SgFpsKey<float>{((uint64_t)hi << 32) | lo});
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ SgFpsKey<double> fps_step(SgFpsKey<double> k)
{
    const uint32_t lo = fps_dpp<CTRL, ROW_MASK>((uint32_t)k.t), hi = fps_dpp<CTRL, ROW_MASK>((uint32_t)(k.t >> 32)), np = fps_dpp<CTRL, ROW_MASK>(k.np);
    return sg_fps_fold(k, SgFpsKey<double>{((uint64_t)hi << 32) | lo, np});
}
template <typename T> __device__ __forceinline__ SgFpsKey<T> fps_wave_fold(SgFpsKey<T> k)
{
    k = fps_step<0x111, 0xf>(k); k = fps_step<0x112, 0xf>(k); k = fps_step<0x114, 0xf>(k); k = fps_step<0x118, 0xf>(k);      // row_shr:1, 2, 4, 8
    k = fps_step<0x142, 0xa>(k);                                     // row_bcast:15 into rows 1 and 3
    k = fps_step<0x143, 0xc>(k);                                     // row_bcast:31 into rows 2 and 3
    return k;
}

template <typename T> struct FpsShared {
    SgFpsKey<T> key[2][SG_FPS_WAVES];      // the waves' candidates, by the round's parity
    T centre[3];
    int cnt[SG_FPS_WAVES];
};

// the workgroup's best key of round j from the lanes' keys: ONE barrier
template <typename T> __device__ __forceinline__ SgFpsKey<T> fps_block_fold(FpsShared<T> &s, SgFpsKey<T> k, int j, int tid)
{
    k = fps_wave_fold<T>(k);
    if ((tid & 63) == 63) s.key[j & 1][tid >> 6] = k;
    __syncthreads();
    SgFpsKey<T> best = s.key[j & 1][0];
#pragma unroll
    for (int w = 1; w < SG_FPS_WAVES; ++w) best = sg_fps_fold(best, s.key[j & 1][w]);
    return best;
}

// Rounds 1 .. K - 1 with the frame in registers: m <= 1024 P.  Slot k of thread `tid` is position k 1024 + tid; a slot beyond m holds t = 0,
// which never beats position 0.
template <typename T, int P>
__device__ __forceinline__ void fps_walk_resident(FpsShared<T> &s, const T *__restrict__ cx, const T *__restrict__ cy, const T *__restrict__ cz, int32_t m,
                                                  int32_t K, int32_t *__restrict__ out_index, T *__restrict__ out_dist, int tid)
{
    T x[P], y[P], z[P], t[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int32_t p = k * SG_FPS_BLOCK + tid;
        const bool in = p < m;
        x[k] = in ? cx[p] : (T)0; y[k] = in ? cy[p] : (T)0; z[k] = in ? cz[p] : (T)0;
        t[k] = in ? (T)INFINITY : (T)0;
    }
    T ax = cx[0], ay = cy[0], az = cz[0];
    for (int32_t j = 1; j < K; ++j) {
        T bt = (T)0;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) {
            t[k] = sg_fps_min(t[k], sg_fps_dist(x[k], y[k], z[k], ax, ay, az));
            if (k == 0 || t[k] > bt) { bt = t[k]; bk = k; }            // (positions grow with k: the first of equals stays)
        }
        const SgFpsKey<T> best = fps_block_fold<T>(s, sg_fps_key(bt, (uint32_t)(bk * SG_FPS_BLOCK + tid)), j, tid);
        const uint32_t w = sg_fps_key_pos(best);
        if ((int)(w & (SG_FPS_BLOCK - 1)) == tid) {
            const int kw = (int)(w >> 10);
#pragma unroll
            for (int k = 0; k < P; ++k)
                if (k == kw) { s.centre[0] = x[k]; s.centre[1] = y[k]; s.centre[2] = z[k]; }
        }
        if (tid == 0) {
            out_index[j] = (int32_t)w;
            if (out_dist) out_dist[j] = sg_fps_key_t(best);
        }
        __syncthreads();
        ax = s.centre[0]; ay = s.centre[1]; az = s.centre[2];
    }
}

template <typename T> struct alignas(4 * sizeof(T)) FpsVec4 { T v[4]; };

// Rounds 1 .. K - 1 for any m: four consecutive positions per thread and step, x, y, z read and t read and written as whole 16-byte pieces
// (the frame's scratch begins on a multiple of four elements and is padded to one, the padding with t = 0).
template <typename T>
__device__ __forceinline__ void fps_walk_general(FpsShared<T> &s, const T *__restrict__ cx, const T *__restrict__ cy, const T *__restrict__ cz, T *__restrict__ ct,
                                                 int32_t m, int32_t K, int32_t *__restrict__ out_index, T *__restrict__ out_dist, int tid)
{
    const int32_t m4 = (m + 3) & ~3;
    T ax = cx[0], ay = cy[0], az = cz[0];
    for (int32_t j = 1; j < K; ++j) {
        T bt = (T)0;
        int32_t bp = m4;                                               // (no position yet)
        for (int32_t p = tid * 4; p < m4; p += SG_FPS_BLOCK * 4) {
            const FpsVec4<T> x = *(const FpsVec4<T> *)(cx + p), y = *(const FpsVec4<T> *)(cy + p), z = *(const FpsVec4<T> *)(cz + p);
            FpsVec4<T> t = *(const FpsVec4<T> *)(ct + p);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                t.v[q] = sg_fps_min(t.v[q], sg_fps_dist(x.v[q], y.v[q], z.v[q], ax, ay, az));
                if (bp == m4 || t.v[q] > bt) { bt = t.v[q]; bp = p + q; }
            }
            *(FpsVec4<T> *)(ct + p) = t;
        }
        const SgFpsKey<T> mine = bp == m4 ? sg_fps_no_key<T>() : sg_fps_key(bt, (uint32_t)bp);
        const SgFpsKey<T> best = fps_block_fold<T>(s, mine, j, tid);
        const uint32_t w = sg_fps_key_pos(best);
        if (tid == 0) {
            out_index[j] = (int32_t)w;
            if (out_dist) out_dist[j] = sg_fps_key_t(best);
        }
        ax = cx[w]; ay = cy[w]; az = cz[w];
    }
}

extern __shared__ __align__(32) unsigned char fps_lds_t[];            // SG_FPS_TIER2_BYTES: the running minima of a frame of tier 2

template <typename T>
__global__ __launch_bounds__(SG_FPS_BLOCK) void k_fps(const T *__restrict__ rows, int64_t n, const int64_t *__restrict__ frame_off,
                                                     const uint8_t *__restrict__ keep_in, SgFpsRange range, int32_t K, T *__restrict__ sx, T *__restrict__ sy,
                                                     T *__restrict__ sz, T *__restrict__ st, int32_t *__restrict__ ssrc, int32_t *__restrict__ out_index,
                                                     T *__restrict__ out_dist, int32_t *__restrict__ out_usable)
{
    __shared__ FpsShared<T> s;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t a = std::min<int64_t>(std::max<int64_t>(frame_off[f], 0), n), b = std::min<int64_t>(std::max<int64_t>(frame_off[f + 1], a), n);
    const int64_t base = sg_fps_base(a, f);
    T *cx = sx + base, *cy = sy + base, *cz = sz + base, *ct = st + base;
    int32_t *csrc = ssrc + base;
    out_index += (int64_t)f * K;
    if (out_dist) out_dist += (int64_t)f * K;

    // (a) the usable rows in input order
    int32_t m = 0;
    for (int64_t i0 = a; i0 < b; i0 += SG_FPS_BLOCK) {
        const int64_t i = i0 + tid;
        T x = (T)0, y = (T)0, z = (T)0;
        bool u = false;
        if (i < b && (!keep_in || keep_in[i] != 0)) {
            const T *row = rows + i * 5;
            x = row[0]; y = row[1]; z = row[2];
            u = sg_fps_usable<T>(range, x, y, z);
        }
        const unsigned long long bal = __ballot(u);
        if (lane == 0) s.cnt[wave] = __popcll(bal);
        __syncthreads();
        int32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SG_FPS_WAVES; ++w) {
            const int c = s.cnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (u) {
            const int32_t p = m + before + __popcll(bal & ((1ull << lane) - 1ull));
            cx[p] = x; cy[p] = y; cz[p] = z; ct[p] = (T)INFINITY;
            csrc[p] = (int32_t)i;
        }
        m += total;
        __syncthreads();
    }
    const int32_t m4 = (m + 3) & ~3;
    if (tid < m4 - m) {                                                // the padding of the last 16-byte piece
        const int32_t p = m + tid;
        cx[p] = (T)0; cy[p] = (T)0; cz[p] = (T)0; ct[p] = (T)0;
    }
    if (tid == 0) out_usable[f] = m;
    if (m == 0) {
        for (int32_t j = tid; j < K; j += SG_FPS_BLOCK) {
            out_index[j] = -1;
            if (out_dist) out_dist[j] = (T)-1;
        }
        return;
    }
    if (tid == 0) {
        out_index[0] = 0;
        if (out_dist) out_dist[0] = (T)INFINITY;
    }
    __syncthreads();                                                   // the compacted rows are the whole workgroup's

    // (b) the rounds
    constexpr int P0 = SgFpsTier<T>::P0, P1 = SgFpsTier<T>::P1;
    if (m <= P0 * SG_FPS_BLOCK) fps_walk_resident<T, P0>(s, cx, cy, cz, m, K, out_index, out_dist, tid);
    else if (m <= P1 * SG_FPS_BLOCK) fps_walk_resident<T, P1>(s, cx, cy, cz, m, K, out_index, out_dist, tid);
    else if (m <= SgFpsTier<T>::ROWS2) {
        T *lt = (T *)fps_lds_t;                                        // t of the whole frame in LDS, padded like the scratch
        for (int32_t p = tid; p < m4; p += SG_FPS_BLOCK) lt[p] = p < m ? (T)INFINITY : (T)0;
        __syncthreads();
        fps_walk_general<T>(s, cx, cy, cz, lt, m, K, out_index, out_dist, tid);
    } else fps_walk_general<T>(s, cx, cy, cz, ct, m, K, out_index, out_dist, tid);
}

// index: the position among the frame's usable rows -> the row of the batch; points: its first C columns
template <typename T>
__global__ __launch_bounds__(256) void k_fps_finish(const T *__restrict__ rows, const int64_t *__restrict__ frame_off, int64_t n, int n_frames, int32_t K, int32_t C,
                                                   const int32_t *__restrict__ ssrc, int32_t *__restrict__ out_index, T *__restrict__ out_points)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n_frames * K) return;
    const int f = (int)(e / K);
    const int32_t p = out_index[e];
    int32_t row = -1;
    if (p >= 0) {
        const int64_t a = std::min<int64_t>(std::max<int64_t>(frame_off[f], 0), n);
        row = ssrc[sg_fps_base(a, f) + p];
        out_index[e] = row;
    }
    if (!out_points) return;
    T *dst = out_points + e * C;
    for (int c = 0; c < C; ++c) dst[c] = row >= 0 ? rows[(int64_t)row * 5 + c] : (T)0;
}

// a batch without a row: every frame has m = 0
template <typename T>
__global__ __launch_bounds__(256) void k_fps_empty(int n_frames, int32_t K, int32_t C, int32_t *__restrict__ out_index, T *__restrict__ out_points,
                                                  T *__restrict__ out_dist, int32_t *__restrict__ out_usable)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n_frames) out_usable[e] = 0;
    if (e >= (int64_t)n_frames * K) return;
    out_index[e] = -1;
    if (out_dist) out_dist[e] = (T)-1;
    if (out_points)
        for (int c = 0; c < C; ++c) out_points[e * C + c] = (T)0;
}

// The whole sequence on `stream`.  Scratch: sx, sy, sz, st (the rows' dtype) and ssrc, sg_fps_scratch(n, n_frames) elements each (unused,
// and no sampling kernel launched, for a batch without a row).
extern "C" int sg_launch_fps(const void *rows, int dtype, int64_t n, const int64_t *frame_off, int n_frames, const uint8_t *keep_in, const SgFpsRange *range,
                             int32_t n_samples, int32_t n_features, void *sx, void *sy, void *sz, void *st, int32_t *ssrc, int32_t *out_index, void *out_points,
                             void *out_dist, int32_t *out_usable, void *stream)
{
    hipStream_t q = (hipStream_t)stream;
    const int64_t elems = (int64_t)n_frames * n_samples;
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (n <= 0) {
            hipLaunchKernelGGL(k_fps_empty<T>, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, q, n_frames, n_samples, n_features, out_index, (T *)out_points,
                               (T *)out_dist, out_usable);
            SG_CHECK_LAUNCH();
            return 0;
        }
        static bool lds_set[64];                                       // (one per row type: the lambda is instantiated twice)
        if (int e = sg_set_lds(k_fps<T>, SG_FPS_TIER2_BYTES, lds_set)) return e;
        hipLaunchKernelGGL(k_fps<T>, dim3(n_frames), dim3(SG_FPS_BLOCK), SG_FPS_TIER2_BYTES, q, (const T *)rows, n, frame_off, keep_in, *range, n_samples, (T *)sx, (T *)sy,
                           (T *)sz, (T *)st, ssrc, out_index, (T *)out_dist, out_usable);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_fps_finish<T>, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, q, (const T *)rows, frame_off, n, n_frames, n_samples,
                           n_features, (const int32_t *)ssrc, out_index, (T *)out_points);
        SG_CHECK_LAUNCH();
        return 0;
    });
}

// ==== sectorized, proposal-centric sampling (snowgpu_fps_sectors_device; definition: include/snowgpu.h; sg_fps_sectors.h) =====================
// F S independent walks instead of F: the usable rows of a frame -- near a present roi of the frame when rois are given -- are split by
// azimuth into S sectors, every (frame, sector) is compacted into a segment of the scratch and walked by a workgroup of its own for its quota.
//   k_fpss_rois      one thread per roi: its record (centre, reach2), and d_out_reach2
//   k_fpss_classify  grid F x tiles of 1024 rows: usable, near and sector of every row, one byte per row; per tile the S counts, by a ballot
//                    per wave and sector (no atomics)
//   k_fpss_plan      one workgroup per frame, wave s scans the tile counts of sector s into tile bases; then n_s, m, the quotas, the slot
//                    offsets and the segments' places; the padding of every segment
//   k_fpss_scatter   grid as k_fpss_classify: x, y, z, t = +inf and the source row into the sector's segment, in input order (rank = tile
//                    base + the waves before + the ballot's lanes before)
//   k_fps_sectors    grid F S, 1024 threads: the walk of k_fps over one segment for q_s samples, positions into the frame's slots from o_s
//   k_fpss_finish    every (frame, slot): position -> row of the batch, the C columns, the trailing repeats, the m = 0 fill
// Nothing waits for another workgroup, nothing spins, no result depends on the arrival of an atomic.
#include "sg_fps_sectors.h"

struct SgFpssShape {
    int32_t F, S, K, C, B, Cb;      // frames, sectors, samples, features, rois per frame (0: none), roi features
    int64_t n, tpf;                 // rows of the batch, tiles per frame (of the longest)
};

template <typename T>
__global__ __launch_bounds__(256) void k_fpss_rois(int64_t n_rois, int32_t Cb, const T *__restrict__ rois, double margin, SgFpsRoi *__restrict__ rec,
                                                   double *__restrict__ out_reach2)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_rois) return;
    SgFpsRoi r;
    sg_fpss_roi<T>(rois + e * Cb, margin, &r);
    rec[e] = r;
    if (out_reach2) out_reach2[e] = r.reach2;
}

__device__ __forceinline__ void fpss_frame(const int64_t *__restrict__ frame_off, int f, int64_t n, int64_t &a, int64_t &b)
{
    a = std::min<int64_t>(std::max<int64_t>(frame_off[f], 0), n);
    b = std::min<int64_t>(std::max<int64_t>(frame_off[f + 1], a), n);
}

template <typename T>
__global__ __launch_bounds__(SG_FPS_BLOCK) void k_fpss_classify(const T *__restrict__ rows, SgFpssShape h, const int64_t *__restrict__ frame_off,
                                                               const uint8_t *__restrict__ keep_in, SgFpsRange range, const SgFpsRoi *__restrict__ rec,
                                                               int8_t *__restrict__ sec, int32_t *__restrict__ tile_cnt)
{
    __shared__ SgFpsRoi roi[SG_FPSS_MAX_ROIS];
    __shared__ int32_t cnt[SG_FPS_WAVES][SG_FPSS_MAX_SECTORS];
    const int f = (int)(blockIdx.x / h.tpf), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x % h.tpf;
    int64_t a, b;
    fpss_frame(frame_off, f, h.n, a, b);
    const int64_t i0 = a + tile * SG_FPS_BLOCK;
    if (i0 >= b) return;                                               // (the whole workgroup: a tile beyond the frame has no count to write)
    if (tid < h.B) roi[tid] = rec[(int64_t)f * h.B + tid];
    __syncthreads();
    const int64_t i = i0 + tid;
    int s = -1;
    if (i < b && (!keep_in || keep_in[i] != 0)) {
        const T *row = rows + i * 5;
        const T x = row[0], y = row[1], z = row[2];
        bool u = sg_fps_usable<T>(range, x, y, z);
        if (u && h.B > 0) {
            u = false;
            for (int k = 0; k < h.B && !u; ++k) u = sg_fpss_near(roi[k], (double)x, (double)y, (double)z);
        }
        if (u) s = sg_fpss_sector((double)x, (double)y, h.S);
    }
    if (i < b) sec[i] = (int8_t)s;
    for (int k = 0; k < h.S; ++k) {
        const unsigned long long bal = __ballot(s == k);
        if (lane == 0) cnt[wave][k] = __popcll(bal);
    }
    __syncthreads();
    if (tid < h.S) {
        int32_t c = 0;
#pragma unroll
        for (int w = 0; w < SG_FPS_WAVES; ++w) c += cnt[w][tid];
        tile_cnt[((int64_t)f * h.tpf + tile) * h.S + tid] = c;
    }
}

// tile counts -> tile bases (in place), the frame's counts, quotas, slot offsets and segment places; the padding of the segments
template <typename T>
__global__ __launch_bounds__(SG_FPS_BLOCK) void k_fpss_plan(SgFpssShape h, const int64_t *__restrict__ frame_off, int32_t *__restrict__ tile, int32_t *__restrict__ seg,
                                                           T *__restrict__ sx, T *__restrict__ sy, T *__restrict__ sz, T *__restrict__ st,
                                                           int32_t *__restrict__ out_usable, int32_t *__restrict__ out_offsets, int32_t *__restrict__ out_count)
{
    __shared__ int64_t ns[SG_FPSS_MAX_SECTORS];
    __shared__ int32_t place[SG_FPSS_MAX_SECTORS];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t a, b;
    fpss_frame(frame_off, f, h.n, a, b);
    const int64_t nt = (b - a + SG_FPS_BLOCK - 1) / SG_FPS_BLOCK;
    if (wave < h.S) {
        int32_t carry = 0;
        for (int64_t t0 = 0; t0 < nt; t0 += 64) {
            const int64_t t = t0 + lane;
            int32_t *p = tile + ((int64_t)f * h.tpf + t) * h.S + wave;
            const int32_t c = t < nt ? *p : 0;
            int32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int32_t v = __shfl_up(incl, d);
                if (lane >= d) incl += v;
            }
            if (t < nt) *p = carry + incl - c;
            carry += __shfl(incl, 63);
        }
        if (lane == 0) ns[wave] = carry;
    }
    __syncthreads();
    if (tid == 0) {
        int64_t n_s[SG_FPSS_MAX_SECTORS];
        int32_t q[SG_FPSS_MAX_SECTORS];
        for (int s = 0; s < h.S; ++s) n_s[s] = ns[s];
        const int64_t m = sg_fpss_quota(n_s, h.S, h.K, q);
        int32_t o = 0, at = 0;
        for (int s = 0; s < h.S; ++s) {
            out_offsets[(int64_t)f * (h.S + 1) + s] = o;
            out_count[(int64_t)f * h.S + s] = (int32_t)n_s[s];
            seg[(int64_t)f * h.S + s] = at;
            place[s] = at;
            o += q[s];
            at += ((int32_t)n_s[s] + 3) & ~3;
        }
        out_offsets[(int64_t)f * (h.S + 1) + h.S] = o;
        out_usable[f] = (int32_t)m;
    }
    __syncthreads();
    if (tid < 4 * h.S) {                                               // the padding of every segment's last 16-byte piece
        const int s = tid >> 2;
        const int32_t m = (int32_t)ns[s], p = m + (tid & 3);
        if (p < ((m + 3) & ~3)) {
            const int64_t at = sg_fpss_base(a, f) + place[s] + p;
            sx[at] = (T)0; sy[at] = (T)0; sz[at] = (T)0; st[at] = (T)0;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(SG_FPS_BLOCK) void k_fpss_scatter(const T *__restrict__ rows, SgFpssShape h, const int64_t *__restrict__ frame_off,
                                                              const int8_t *__restrict__ sec, const int32_t *__restrict__ tile_base, const int32_t *__restrict__ seg,
                                                              T *__restrict__ sx, T *__restrict__ sy, T *__restrict__ sz, T *__restrict__ st, int32_t *__restrict__ ssrc)
{
    __shared__ int32_t cnt[SG_FPS_WAVES][SG_FPSS_MAX_SECTORS];
    const int f = (int)(blockIdx.x / h.tpf), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tile = blockIdx.x % h.tpf;
    int64_t a, b;
    fpss_frame(frame_off, f, h.n, a, b);
    const int64_t i0 = a + tile * SG_FPS_BLOCK;
    if (i0 >= b) return;
    const int64_t i = i0 + tid;
    const int s = i < b ? (int)sec[i] : -1;
    int rank = 0;
    for (int k = 0; k < h.S; ++k) {
        const unsigned long long bal = __ballot(s == k);
        if (lane == 0) cnt[wave][k] = __popcll(bal);
        if (s == k) rank = sg_fpss_rank(bal, lane);
    }
    __syncthreads();
    if (s < 0) return;
    int32_t before = 0;
#pragma unroll
    for (int w = 0; w < SG_FPS_WAVES; ++w) before += w < wave ? cnt[w][s] : 0;
    const int64_t at = sg_fpss_base(a, f) + seg[(int64_t)f * h.S + s] + tile_base[((int64_t)f * h.tpf + tile) * h.S + s] + before + rank;
    const T *row = rows + i * 5;
    sx[at] = row[0]; sy[at] = row[1]; sz[at] = row[2]; st[at] = (T)INFINITY;
    ssrc[at] = (int32_t)i;
}

template <typename T>
__global__ __launch_bounds__(SG_FPS_BLOCK) void k_fps_sectors(SgFpssShape h, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ seg,
                                                             const int32_t *__restrict__ offsets, const int32_t *__restrict__ count, T *__restrict__ sx,
                                                             T *__restrict__ sy, T *__restrict__ sz, T *__restrict__ st, int32_t *__restrict__ out_index,
                                                             T *__restrict__ out_dist)
{
    __shared__ FpsShared<T> s;
    // Which (frame, sector) a workgroup walks -- a bijection, so no result depends on it (DESIGN.md section 9 has the three measured).
    // Consecutive workgroups are dealt to the XCDs in turn.  Frame-major (f S + k), sector k of every frame met the same XCDs whenever S
    // shares a factor with their number.  Sector-major (k F + f) spreads every sector over all XCDs, and neighbours in the grid are walks
    // alike in length and tier; it was the fastest of the three in five of six settings.  Rotating the sector by the frame on top of it
    // ((j + f) mod S) mixes the lengths again and lost to it everywhere but at S = 6 on all rows.
    const int f = blockIdx.x % h.F, k = blockIdx.x / h.F, tid = threadIdx.x;
    const int32_t o = offsets[(int64_t)f * (h.S + 1) + k], q = offsets[(int64_t)f * (h.S + 1) + k + 1] - o, m = count[(int64_t)f * h.S + k];
    if (q <= 0) return;                                                // (q <= m: a sector with a quota has rows)
    const int64_t a = std::min<int64_t>(std::max<int64_t>(frame_off[f], 0), h.n);
    const int64_t base = sg_fpss_base(a, f) + seg[(int64_t)f * h.S + k];
    T *cx = sx + base, *cy = sy + base, *cz = sz + base, *ct = st + base;
    out_index += (int64_t)f * h.K + o;
    if (out_dist) out_dist += (int64_t)f * h.K + o;
    if (tid == 0) {
        out_index[0] = 0;
        if (out_dist) out_dist[0] = (T)INFINITY;
    }
    constexpr int P0 = SgFpsTier<T>::P0, P1 = SgFpsTier<T>::P1;
    if (m <= P0 * SG_FPS_BLOCK) fps_walk_resident<T, P0>(s, cx, cy, cz, m, q, out_index, out_dist, tid);
    else if (m <= P1 * SG_FPS_BLOCK) fps_walk_resident<T, P1>(s, cx, cy, cz, m, q, out_index, out_dist, tid);
    else if (m <= SgFpsTier<T>::ROWS2) {
        const int32_t m4 = (m + 3) & ~3;
        T *lt = (T *)fps_lds_t;
        for (int32_t p = tid; p < m4; p += SG_FPS_BLOCK) lt[p] = p < m ? (T)INFINITY : (T)0;
        __syncthreads();
        fps_walk_general<T>(s, cx, cy, cz, lt, m, q, out_index, out_dist, tid);
    } else fps_walk_general<T>(s, cx, cy, cz, ct, m, q, out_index, out_dist, tid);
}

template <typename T>
__global__ __launch_bounds__(256) void k_fpss_finish(const T *__restrict__ rows, SgFpssShape h, const int64_t *__restrict__ frame_off, const int32_t *__restrict__ seg,
                                                    const int32_t *__restrict__ offsets, const int32_t *__restrict__ ssrc, int32_t *__restrict__ out_index,
                                                    T *__restrict__ out_points, T *__restrict__ out_dist)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)h.F * h.K) return;
    const int f = (int)(e / h.K);
    const int32_t j = (int32_t)(e % h.K);
    const int32_t *o = offsets + (int64_t)f * (h.S + 1);
    const int32_t filled = o[h.S];                                     // min(m, K)
    int32_t row = -1;
    if (filled > 0) {
        const int64_t a = std::min<int64_t>(std::max<int64_t>(frame_off[f], 0), h.n);
        int k = 0, p = 0;
        if (j < filled) {
            while (o[k + 1] <= j) ++k;
            p = out_index[e];
        } else {                                                       // a trailing slot repeats slot 0: the first row of the first sector with a sample
            while (o[k + 1] <= 0) ++k;
            if (out_dist) out_dist[e] = (T)0;
        }
        row = ssrc[sg_fpss_base(a, f) + seg[(int64_t)f * h.S + k] + p];
    } else if (out_dist) out_dist[e] = (T)-1;
    out_index[e] = row;
    if (!out_points) return;
    T *dst = out_points + e * h.C;
    for (int c = 0; c < h.C; ++c) dst[c] = row >= 0 ? rows[(int64_t)row * 5 + c] : (T)0;
}

// a batch without a row: every frame has m = 0
__global__ __launch_bounds__(256) void k_fpss_empty(int n_frames, int32_t S, int32_t *__restrict__ out_offsets, int32_t *__restrict__ out_count)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (int64_t)n_frames * (S + 1)) out_offsets[e] = 0;
    if (e < (int64_t)n_frames * S) out_count[e] = 0;
}

// The whole sequence on `stream`.  Scratch: sx, sy, sz, st (the rows' dtype) and ssrc, sg_fpss_scratch(n, n_frames) elements each; sec, n
// bytes (unused when out_sector_of is given); rec, n_frames n_rois records; tile, n_frames tiles-per-frame S words; seg, n_frames S words.
extern "C" int sg_launch_fps_sectors(const void *rows, int dtype, int64_t n, int64_t max_frame, const int64_t *frame_off, int n_frames, const uint8_t *keep_in,
                                     const SgFpsRange *range, int32_t n_samples, int32_t n_features, int32_t n_sectors, const void *rois, int32_t n_rois,
                                     int32_t roi_features, double roi_margin, void *sx, void *sy, void *sz, void *st, int32_t *ssrc, int8_t *sec, void *rec,
                                     int32_t *tile, int32_t *seg, int32_t *out_index, void *out_points, void *out_dist, int32_t *out_usable,
                                     int32_t *out_offsets, int32_t *out_count, int8_t *out_sector_of, double *out_reach2, void *stream)
{
    hipStream_t q = (hipStream_t)stream;
    const int64_t elems = (int64_t)n_frames * n_samples;
    const SgFpssShape h{n_frames, n_sectors, n_samples, n_features, rois ? n_rois : 0, roi_features, n, sg_tiles(max_frame)};
    return sg_by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (rois) {
            const int64_t nr = (int64_t)n_frames * n_rois;
            hipLaunchKernelGGL(k_fpss_rois<T>, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, q, nr, roi_features, (const T *)rois, roi_margin, (SgFpsRoi *)rec,
                               out_reach2);
            SG_CHECK_LAUNCH();
        }
        if (n <= 0) {
            hipLaunchKernelGGL(k_fps_empty<T>, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, q, n_frames, n_samples, n_features, out_index, (T *)out_points,
                               (T *)out_dist, out_usable);
            SG_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_fpss_empty, dim3((unsigned)(((int64_t)n_frames * (n_sectors + 1) + 255) / 256)), dim3(256), 0, q, n_frames, n_sectors, out_offsets,
                               out_count);
            SG_CHECK_LAUNCH();
            return 0;
        }
        if (out_sector_of) {                                           // (a row outside every frame is absent: -1)
            hipError_t e = hipMemsetAsync(out_sector_of, 0xff, (size_t)n, q);
            if (e != hipSuccess) return (int)e;
        }
        int8_t *sector = out_sector_of ? out_sector_of : sec;
        const unsigned tiles = (unsigned)((int64_t)n_frames * h.tpf);
        static bool lds_set[64];                                       // (one per row type: the lambda is instantiated twice)
        if (int e = sg_set_lds(k_fps_sectors<T>, SG_FPS_TIER2_BYTES, lds_set)) return e;
        hipLaunchKernelGGL(k_fpss_classify<T>, dim3(tiles), dim3(SG_FPS_BLOCK), 0, q, (const T *)rows, h, frame_off, keep_in, *range, (const SgFpsRoi *)rec, sector, tile);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_fpss_plan<T>, dim3(n_frames), dim3(SG_FPS_BLOCK), 0, q, h, frame_off, tile, seg, (T *)sx, (T *)sy, (T *)sz, (T *)st, out_usable, out_offsets,
                           out_count);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_fpss_scatter<T>, dim3(tiles), dim3(SG_FPS_BLOCK), 0, q, (const T *)rows, h, frame_off, (const int8_t *)sector, (const int32_t *)tile,
                           (const int32_t *)seg, (T *)sx, (T *)sy, (T *)sz, (T *)st, ssrc);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_fps_sectors<T>, dim3((unsigned)((int64_t)n_frames * n_sectors)), dim3(SG_FPS_BLOCK), SG_FPS_TIER2_BYTES, q, h, frame_off, (const int32_t *)seg,
                           (const int32_t *)out_offsets, (const int32_t *)out_count, (T *)sx, (T *)sy, (T *)sz, (T *)st, out_index, (T *)out_dist);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_fpss_finish<T>, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, q, (const T *)rows, h, frame_off, (const int32_t *)seg,
                           (const int32_t *)out_offsets, (const int32_t *)ssrc, out_index, (T *)out_points, (T *)out_dist);
        SG_CHECK_LAUNCH();
        return 0;
    });
}
