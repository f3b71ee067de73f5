// snowgpu_host.cpp -- the entries of the C ABI that take HOST pointers: uploads, the launch sequence (run_batch, snowgpu_batch.cpp),
// downloads; large batches as a pipeline of chunks, their results optionally packed and put together by host threads (sg_assemble.h).
#include <cctype>
#include <chrono>

#include "sg_host.h"
#include "sg_launch.h"      // sg_tiles

constexpr size_t SG_THR_HIST = (size_t)50 * 2555;      // words of one frame's histogram of (range, I / cos) (snowgpu_prepass_stats)

int node_of_device(int device)
{
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
    char path[256];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *fh = std::fopen(path, "r");
    if (!fh) return -1;
    int node = -1;
    const int got = std::fscanf(fh, "%d", &node);
    std::fclose(fh);
    return got == 1 ? node : -1;
}

// a page-locked staging block of at least `need` bytes (contents are not kept)
static int grow_pinned(snowgpu_ctx *ctx, char *&p, size_t &cap, size_t need, size_t slack)
{
    if (need <= cap) return SNOWGPU_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    HIPCHK(ctx, hipHostMalloc((void **)&p, need + slack, hipHostMallocDefault));
    cap = need + slack;
    return SNOWGPU_OK;
}

static int grow_events(snowgpu_ctx *ctx, std::vector<hipEvent_t> &ev, size_t n)
{
    while (ev.size() < n) {
        hipEvent_t e;
        HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev.push_back(e);
    }
    return SNOWGPU_OK;
}

// rows of the largest frame; uniform: every frame has that many (and it is not zero)
static void frame_extent(int n_frames, const int64_t *offsets, int64_t *max_frame, bool *uniform)
{
    int64_t mx = 0;
    for (int f = 0; f < n_frames; ++f) mx = std::max(mx, offsets[f + 1] - offsets[f]);
    bool uni = mx > 0;
    for (int f = 0; f < n_frames && uni; ++f) uni = (offsets[f + 1] - offsets[f]) == mx;
    *max_frame = mx; *uniform = uni;
}

// The frame offsets of a host-pointer entry: n_frames + 1 of them, from 0, non-decreasing, below 2^31 rows in all.
static int check_frames(snowgpu_ctx *ctx, int n_frames, const int64_t *offsets, int64_t *max_frame, bool *uniform, int64_t *n_total)
{
    if (offsets[0] != 0) return fail(ctx, SNOWGPU_E_INVALID, "frame_offsets[0] must be 0");
    for (int f = 0; f < n_frames; ++f)
        if (offsets[f + 1] < offsets[f]) return fail(ctx, SNOWGPU_E_INVALID, "frame_offsets must be non-decreasing");
    if (offsets[n_frames] >= ((int64_t)1 << 31)) return fail(ctx, SNOWGPU_E_INVALID, "batch too large: split it below 2^31 rows");
    frame_extent(n_frames, offsets, max_frame, uniform);
    *n_total = offsets[n_frames];
    return SNOWGPU_OK;
}

// The device half of the noise-threshold prepass (simulation.py:449-461) on a launch sequence's own scratch (lc: the context or a lane of
// R): the plane, estimated by R's method unless the caller brought one, then the 50 x 2555 histograms and the per-frame records into
// lc->stats_hist / stats_rec and the status words into lc->d_status.  Errors are left in R.
static int device_prepass_half(snowgpu_ctx *lc, snowgpu_ctx *R, const void *rows, int dtype, const int64_t *off, int n_frames, int64_t n_total,
                               int64_t max_frame, const double *plane, hipStream_t st)
{
    const size_t nf = (size_t)n_frames;
    if (!plane) {
        if (lc->plane_est.ensure(nf * 4) || lc->plane_info.ensure(nf * 4)) return fail(R, SNOWGPU_E_HIP, "hipMalloc failed for the plane estimate");
        int pe = sg_plane_run(&lc->plane_scr, &R->plane_par, rows, dtype, off, nullptr, n_frames, n_total, max_frame, lc->plane_est.p, lc->plane_info.p, st);
        if (pe) return fail(R, SNOWGPU_E_HIP, std::string("plane estimate: ") + (pe > 0 ? hipGetErrorString((hipError_t)pe) : "allocation"));
        plane = lc->plane_est.p;
    }
    if (lc->stats_hist.ensure(nf * SG_THR_HIST) || lc->stats_rec.ensure(nf * SG_PRE_REC) || (!lc->d_status && hipMalloc((void **)&lc->d_status, 32) != hipSuccess))
        return fail(R, SNOWGPU_E_HIP, "hipMalloc failed for the prepass statistics");
    HIPCHK(R, hipMemsetAsync(lc->d_status, 0, 32, st));
    int se = sg_prepass_stats_run(&lc->prepass, rows, dtype, off, n_frames, n_total, max_frame, plane, lc->stats_hist.p, lc->stats_rec.p, lc->d_status, st);
    if (se) return fail(R, SNOWGPU_E_HIP, std::string("prepass: ") + (se > 0 ? hipGetErrorString((hipError_t)se) : "allocation"));
    return SNOWGPU_OK;
}

// The caller fits the noise threshold (snowgpu_set_threshold_callback): page-locked staging for the device half of the prepass --
// histograms | records | the polynomials the callback writes | 8 status words per group -- two events per group, and the device copy of
// the polynomials.
struct ThrStage {
    int32_t *hist, *stat;
    double *rec, *thr;
};
static int ensure_thr_stage(snowgpu_ctx *ctx, size_t nf, size_t n_status_groups, ThrStage *s)
{
    const size_t o_rec = nf * SG_THR_HIST * 4, o_thr = o_rec + nf * SG_PRE_REC * 8, o_stat = o_thr + nf * 3 * 8, need = o_stat + n_status_groups * 32 + 64;
    if (int rc = grow_pinned(ctx, ctx->thr_stage, ctx->thr_stage_cap, need, need / 8)) return rc;
    if (int rc = grow_events(ctx, ctx->thr_ev, 2 * n_status_groups)) return rc;
    ENSURE(ctx, ctx->user_thr, nf * 3);
    *s = ThrStage{(int32_t *)ctx->thr_stage, (int32_t *)(ctx->thr_stage + o_stat), (double *)(ctx->thr_stage + o_rec), (double *)(ctx->thr_stage + o_thr)};
    return SNOWGPU_OK;
}

// Upload / download streams and chunk events of the host pipeline: made on the first pipelined batch, so that a context that
// only ever sees device-resident batches keeps the normal-priority queue pool to its own streams (see host_batch_pipelined).
static int ensure_pipeline(snowgpu_ctx *ctx, int n_chunks, int n_lanes)
{
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (!ctx->s_h2d) HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->s_h2d, hipStreamNonBlocking, greatest));
    if (!ctx->s_d2h) HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->s_d2h, hipStreamNonBlocking, least));
    if (int rc = grow_events(ctx, ctx->pipe_ev, 2 * (size_t)n_chunks)) return rc;
    while ((int)ctx->lanes.size() < n_lanes - 1) {       // lane 0 is the context itself; the others: ONE stream each (low-priority pool)
        snowgpu_ctx *ln = new snowgpu_ctx();
        ln->device = ctx->device;
        ln->root = ctx;
        ctx->lanes.push_back(ln);
        if (hipStreamCreateWithPriority(&ln->stream, hipStreamNonBlocking, least) != hipSuccess) return fail(ctx, SNOWGPU_E_HIP, "lane stream");
        for (hipEvent_t *ep : lane_events(ln)) HIPCHK(ctx, hipEventCreateWithFlags(ep, hipEventDisableTiming));
    }
    return SNOWGPU_OK;
}

// A host-pointer batch as a pipeline of chunks of whole frames.  What the traces of the first versions taught:
// the runtime keeps a pool of (by default four) hardware queues PER stream priority, and streams beyond that share a queue
// with another stream -- whose packets they then wait behind, events and copies included; its device-to-host copy is a
// full-grid blit kernel in a process that has initialised PyTorch and stalls every kernel beside it; a chunk's launch
// sequence is a third faster with its side streams than on one stream.  So:
//   * the upload of ALL chunks is one stream of DMA copies (high-priority pool) into a batch-sized buffer -- it never waits
//     for anything -- with one event per chunk;
//   * the chunks compute into a batch-sized result buffer, each as ONE chain of launches on one stream, alternating between
//     two lanes (the context itself and a sub-context with its own stream, events and scratch in the low-priority pool): a
//     chunk starts the moment its upload lands, and the launch latency of one chain hides behind the other;
//   * the downloads run on one more stream (low-priority pool: a hardware queue of its own), each after its chunk's event: the
//     runtime's copy, i.e. the DMA engine (a small-grid kernel of ours writing page-locked memory directly was measured slower:
//     every kernel boundary on the device then waits for the outstanding host writes).
// The host enqueues everything and waits once at the end.  Small per-frame arrays (table ids, planes / polynomials, counts,
// statistics) cross once for the whole batch; a chunk sees its slice of them.
static int host_batch_pipelined(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                                const int32_t *table_ids, double beam_div_deg, const double *thr_poly, const double *plane,
                                double noise_floor, const int32_t *perm, void *out_rows, int32_t *out_src, int64_t *out_counts,
                                int64_t *out_stats, double *out_thr_poly)
{
    const size_t esz = dtype == 0 ? 4 : 8, rb = 5 * esz, nf = (size_t)n_frames, nl = (size_t)ctx->h_las.n;
    const int64_t n_total = frame_offsets[n_frames];
    hipStream_t st = ctx->stream;
    // chunks of whole frames, about pipe_rows rows each
    std::vector<int> c_first;
    std::vector<int64_t> h_off;                  // chunk-local offsets: chunk c owns h_off[c_pos[c] .. c_pos[c] + frames + 1)
    std::vector<size_t> c_pos;
    // (the caller fits the threshold -- snowgpu_set_threshold_callback, below --: groups of 40 sweeps; the callback's cost per frame
    // falls with the group's size -- its selection runs on a thread pool, every call pays the pool's round trip -- and the calling thread
    // enqueues nothing while it is inside it: 256 sweeps, 24 / 32 / 40 / 48 / 56 sweeps per group: 1.36 / 1.32 / 1.42 / 1.44 / 1.40 G
    // points/s with the rows transfer, 1.39 / 1.42 / 1.57 / 1.63 / 1.66 with the packed one, scripts/probe/q8_group_probe.py)
    const int64_t pipe_rows = (ctx->thr_fn != nullptr && !thr_poly && !perm) ? std::max<int64_t>(ctx->pipe_rows, (int64_t)5 << 20) : ctx->pipe_rows;
    for (int f = 0; f < n_frames;) {
        int g = f;
        const int64_t base = frame_offsets[f];
        // (the last chunks are half size: what remains to be done after the last upload has landed -- the last chunk's kernels, its
        // download, the assembly of its rows -- is the part of the call nothing overlaps)
        const int64_t target = (n_total - base <= 2 * pipe_rows) ? std::max<int64_t>(pipe_rows / 2, 1) : pipe_rows;
        while (g < n_frames && (g == f || frame_offsets[g + 1] - base <= target)) ++g;
        c_first.push_back(f);
        c_pos.push_back(h_off.size());
        for (int k = f; k <= g; ++k) h_off.push_back(frame_offsets[k] - base);
        f = g;
    }
    c_first.push_back(n_frames);
    const int n_chunks = (int)c_first.size() - 1;
    const int L = std::max(1, std::min(ctx->pipe_lanes, n_chunks));
    {
        int prc = ensure_pipeline(ctx, n_chunks, L);
        if (prc) return prc;
    }
    static const bool trace = std::getenv("SNOWGPU_PIPE_TRACE") != nullptr;
    ENSURE(ctx, ctx->pipe_off, h_off.size());
    ENSURE(ctx, ctx->pipe_status, (size_t)n_chunks * 8);
    ENSURE(ctx, ctx->out_counts, nf);
    ENSURE(ctx, ctx->out_stats, nf * 3);
    ENSURE(ctx, ctx->table_ids, nf * nl);
    ENSURE(ctx, ctx->plane, nf * 4);
    ENSURE(ctx, ctx->rows_in, std::max<size_t>((size_t)n_total * rb, 8));
    const uint8_t *chn = (rows && dtype == 0) ? ctx->in_channels : nullptr;          // compact input (snowgpu_augment_batch_compact)
    if (chn) {
        ENSURE(ctx, ctx->rows_c4, std::max<size_t>((size_t)n_total * 16, 16));
        ENSURE(ctx, ctx->rows_ch, std::max<size_t>((size_t)n_total, 16));
    }
    // Packed result transfer: the compaction leaves, per kept row, its source row | label code and its intensity, and the moved
    // coordinates of the label-2 rows apart (SgPackOut); those cross the link in exact sizes once a chunk's counts have landed, and host
    // threads put the caller's rows together -- x, y, z (and the channel of rows without a laser) copied from the caller's INPUT rows.
    const bool packed = ctx->result_mode == 1 && rows != nullptr && n_total > 0;
    const size_t nt = (size_t)n_total;
    if (packed) {
        // the host threads read the caller's INPUT rows while they write out_rows: the two must not overlap (the rows transfer tolerates
        // rows == out_rows, this one would corrupt frames whose rows do not come channel-sorted); a word holds a 30-bit source row
        const char *r0 = (const char *)rows, *r1 = r0 + nt * (ctx->in_channels ? 4 : 5) * esz, *o0 = (const char *)out_rows, *o1 = o0 + nt * 5 * esz;
        if (r0 < o1 && o0 < r1) return fail(ctx, SNOWGPU_E_INVALID, "packed result transfer: out_rows overlaps rows (the rows are assembled from the input rows)");
        for (int f = 0; f < n_frames; ++f)
            if (frame_offsets[f + 1] - frame_offsets[f] >= ((int64_t)1 << 30))
                return fail(ctx, SNOWGPU_E_INVALID, "packed result transfer: a frame of 2^30 rows or more (30-bit source rows); use the rows transfer");
    }
    char *st_meta = nullptr, *st_int = nullptr, *st_mv = nullptr;
    int64_t *st_cnt = nullptr, *st_mvcnt = nullptr;
    if (packed) {
        ENSURE(ctx, ctx->pk_meta, nt);
        ENSURE(ctx, ctx->pk_int, nt * esz);
        ENSURE(ctx, ctx->pk_mv, nt * 3 * esz);
        ENSURE(ctx, ctx->pk_mvcnt, nf);
        const size_t o_int = (nt * 4 + 63) / 64 * 64, o_mv = o_int + (nt * esz + 63) / 64 * 64, o_cnt = o_mv + (nt * 3 * esz + 63) / 64 * 64;
        const size_t need = o_cnt + 16 * nf + 64;
        if (int grc = grow_pinned(ctx, ctx->st_pk, ctx->st_pk_cap, need, need / 8)) return grc;
        st_meta = ctx->st_pk; st_int = ctx->st_pk + o_int; st_mv = ctx->st_pk + o_mv;
        st_cnt = (int64_t *)(ctx->st_pk + o_cnt); st_mvcnt = st_cnt + nf;
        if (int grc = grow_events(ctx, ctx->pk_ev, 2 * (size_t)n_chunks)) return grc;
        if (!ctx->pool) {
            int n_thr = ctx->asm_threads;
            if (n_thr <= 0) {
                cpu_set_t cs;
                CPU_ZERO(&cs);
                int avail = (sched_getaffinity(0, sizeof cs, &cs) == 0) ? CPU_COUNT(&cs) : (int)std::thread::hardware_concurrency();
                if (FILE *fh = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {      // a container's CPU quota, if any
                    long long q = 0, per = 0;
                    if (std::fscanf(fh, "%lld %lld", &q, &per) == 2 && q > 0 && per > 0) avail = std::min<int>(avail, (int)((q + per - 1) / per));
                    std::fclose(fh);
                }
                n_thr = std::max(1, std::min(8, avail - 2));      // (eight copy at the pace of the link: measured 6 .. 14 threads, 2.25 - 2.31 G points/s)
            }
            ctx->pool = new AsmPool();
            ctx->pool->start(n_thr);
        }
        {   // the threads go where the rows they copy live (see node_of_address); the device's node if that cannot be told
            const int n_in = node_of_address(rows), n_out = node_of_address(out_rows);
            int nd = (n_out >= 0) ? n_out : n_in;
            if (nd < 0) nd = node_of_device(ctx->device);
            ctx->pool->set_node(nd);
        }
    } else {
        ENSURE(ctx, ctx->rows_out, std::max<size_t>((size_t)n_total * rb, 8));
        ENSURE(ctx, ctx->out_src, std::max<size_t>((size_t)n_total, 1));
    }
    // The small arrays lead the upload stream (chunk 0's event covers them).  On the compute stream they would leave it
    // "after a DMA copy" for the whole batch: 28 instead of 20 ms for 256 sweeps (measured).
    hipStream_t up = ctx->s_h2d;
    HostCall hc{ctx, true};
    HIPCHK(ctx, hipMemcpyAsync(ctx->pipe_off.p, h_off.data(), sizeof(int64_t) * h_off.size(), hipMemcpyHostToDevice, up));
    HIPCHK(ctx, hipMemcpyAsync(ctx->table_ids.p, table_ids, sizeof(int32_t) * nf * nl, hipMemcpyHostToDevice, up));
    const double *d_thr = nullptr;
    if (thr_poly) {
        ENSURE(ctx, ctx->user_thr, nf * 3);
        HIPCHK(ctx, hipMemcpyAsync(ctx->user_thr.p, thr_poly, sizeof(double) * 3 * nf, hipMemcpyHostToDevice, up));
        d_thr = ctx->user_thr.p;
    } else if (plane) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->plane.p, plane, sizeof(double) * 4 * nf, hipMemcpyHostToDevice, up));
    }
    if (perm) {
        ENSURE(ctx, ctx->user_perm, (size_t)n_total);
        HIPCHK(ctx, hipMemcpyAsync(ctx->user_perm.p, perm, sizeof(int32_t) * (size_t)n_total, hipMemcpyHostToDevice, up));
    }
    if (out_thr_poly) ENSURE(ctx, ctx->out_thr, nf * 3);
    auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    std::vector<hipEvent_t> tev;                  // SNOWGPU_PIPE_TRACE: timed events -- base, then per chunk: uploaded, compute begins, computed, downloaded
    if (trace) {
        tev.resize(1 + 4 * (size_t)n_chunks);
        for (auto &e : tev) HIPCHK(ctx, hipEventCreate(&e));
        HIPCHK(ctx, hipStreamSynchronize(st));
        HIPCHK(ctx, hipEventRecord(tev[0], ctx->s_h2d));
    }
    // uploads: all of them, back to back (the scratch of an earlier batch on this context has been drained: every host entry
    // ends with a synchronisation)
    for (int c = 0; c < n_chunks; ++c) {
        const int64_t r0 = frame_offsets[c_first[(size_t)c]], cn = frame_offsets[c_first[(size_t)c + 1]] - r0;
        if (cn && rows && chn) {                       // compact input: 16 + 1 bytes per row up the link (k_expand_rows on the chunk's lane makes the rows)
            HIPCHK(ctx, hipMemcpyAsync(ctx->rows_c4.p + (size_t)r0 * 16, (const char *)rows + (size_t)r0 * 16, (size_t)cn * 16, hipMemcpyHostToDevice, ctx->s_h2d));
            HIPCHK(ctx, hipMemcpyAsync(ctx->rows_ch.p + (size_t)r0, chn + r0, (size_t)cn, hipMemcpyHostToDevice, ctx->s_h2d));
        } else if (cn && rows) HIPCHK(ctx, hipMemcpyAsync(ctx->rows_in.p + (size_t)r0 * rb, (const char *)rows + (size_t)r0 * rb, (size_t)cn * rb, hipMemcpyHostToDevice, ctx->s_h2d));
        HIPCHK(ctx, hipEventRecord(ctx->pipe_ev[2 * (size_t)c], ctx->s_h2d));
        if (trace) HIPCHK(ctx, hipEventRecord(tev[1 + 4 * (size_t)c], ctx->s_h2d));
    }
    const double t_up = now();
    int rc = SNOWGPU_OK;
    // ---- packed result transfer: downloads sized by the counts, and the host threads that put the rows together ----------------------
    int pk_enq = 0, pk_asm = 0;                      // chunks whose compute and download are enqueued / whose rows are with the pool
    // chunks that stopped at their prepass status (finish(): no compaction, no downloads): never assembled -- their pk_ev and staging
    // words are an earlier call's
    std::vector<char> pk_skip((size_t)n_chunks, 0);
    const size_t in_w = chn ? 4 : 5;               // columns of the caller's input rows
    void (*const assemble)(const SgAsmFrame &) = esz == 8 ? sg_assemble_frame<double, false> : (chn ? sg_assemble_frame<float, true> : sg_assemble_frame<float, false>);
    // Enqueue what has become possible: the downloads of chunks whose counts have landed; the assembly of chunks whose downloads have.
    // wait = false: only what is ready now (called between the launches of later chunks); true: everything, blocking.
    auto pk_progress = [&](bool wait) -> hipError_t {
        while (pk_asm < pk_enq) {
            const int c = pk_asm;
            if (pk_skip[(size_t)c]) { ++pk_asm; continue; }
            hipEvent_t ev = ctx->pk_ev[2 * (size_t)c];
            hipError_t q = wait ? hipEventSynchronize(ev) : hipEventQuery(ev);
            if (q == hipErrorNotReady) { (void)hipGetLastError(); return hipSuccess; }     // ("not ready" must not be what the next launch check finds)
            if (q != hipSuccess) return q;
            // the chunk's words, intensities, the head of its moved-coordinates list and its counts are here
            const int f0 = c_first[(size_t)c], f1 = c_first[(size_t)c + 1];
            const size_t o = (size_t)frame_offsets[f0], head = pk_mv_head((size_t)(frame_offsets[f1] - frame_offsets[f0]));
            auto mv_rows = [&](int f) { return sg_moved_rows(st_mvcnt[f], frame_offsets[f + 1] - frame_offsets[f]); };
            size_t n_mv = 0;
            for (int f = f0; f < f1; ++f) n_mv += (size_t)mv_rows(f);
            if (n_mv > head) {                        // a list longer than its head (more than one row in eight scattered): the rest now, waited for
                hipError_t e = hipMemcpyAsync(st_mv + (o + head) * 3 * esz, ctx->pk_mv.p + (o + head) * 3 * esz, (n_mv - head) * 3 * esz, hipMemcpyDeviceToHost, ctx->s_d2h);
                if (e == hipSuccess) e = hipEventRecord(ctx->pk_ev[2 * (size_t)c + 1], ctx->s_d2h);
                if (e == hipSuccess) e = hipEventSynchronize(ctx->pk_ev[2 * (size_t)c + 1]);
                if (e != hipSuccess) return e;
            }
            if (trace) (void)hipEventRecord(tev[4 + 4 * (size_t)c], ctx->s_d2h);
            int64_t mv_at = frame_offsets[f0];     // where the frame's part of the batch's list of moved coordinates starts, in rows
            for (int f = f0; f < f1; ++f) {
                const size_t fo = (size_t)frame_offsets[f];
                const SgAsmFrame a{(const char *)rows + fo * in_w * esz, chn ? chn + fo : nullptr, (const uint32_t *)st_meta + fo, st_int + fo * esz,
                                   st_mv + (size_t)mv_at * 3 * esz, (char *)out_rows + fo * 5 * esz, out_src ? out_src + fo : nullptr,
                                   (uint32_t)(frame_offsets[f + 1] - frame_offsets[f]), st_cnt[f]};
                if (a.kept_dev > 0) ctx->pool->push([=]() { assemble(a); });
                mv_at += mv_rows(f);
            }
            ++pk_asm;
        }
        return hipSuccess;
    };
    // The caller fits the noise threshold (snowgpu_set_threshold_callback): per chunk the device half of the prepass leads the chunk's
    // kernels, its histograms come down while they run, and the chunk is FINISHED -- callback, polynomials up, compaction, downloads --
    // when its lane is needed again (L chunks later) or at the end; the host's selection of chunk c thus runs beside the kernels of
    // chunks c + 1 .. c + L - 1 and beside the link's traffic.
    const bool cb = ctx->thr_fn != nullptr && !thr_poly && !perm && n_total > 0;
    ThrStage ts{};
    if (cb) { if (int trc = ensure_thr_stage(ctx, nf, (size_t)n_chunks, &ts)) return trc; }
    struct Chunk { BatchDev b; SgPackOut po; snowgpu_ctx *lc; };
    std::vector<Chunk> chunks((size_t)n_chunks);
    // chunk c: its kernels (all of them, or everything ahead of the compaction when the caller fits the threshold)
    auto compute = [&](int c) -> int {
        const int f0 = c_first[(size_t)c], f1 = c_first[(size_t)c + 1], cf = f1 - f0;
        const int64_t r0 = frame_offsets[f0], cn = frame_offsets[f1] - r0;
        const int64_t *lo = &h_off[c_pos[(size_t)c]];
        Chunk &k = chunks[(size_t)c];
        snowgpu_ctx *lc = (c % L) == 0 ? ctx : ctx->lanes[(size_t)(c % L) - 1];     // chunk c computes on lane c mod L
        k.lc = lc;
        hipStream_t cs = lc->stream;
        HIPCHK(ctx, hipStreamWaitEvent(cs, ctx->pipe_ev[2 * (size_t)c], 0));
        if (trace) HIPCHK(ctx, hipEventRecord(tev[2 + 4 * (size_t)c], cs));
        if (chn && cn) {
            int xe = sg_launch_expand_rows(ctx->rows_c4.p + (size_t)r0 * 16, ctx->rows_ch.p + (size_t)r0, ctx->rows_in.p + (size_t)r0 * rb, cn, cs);
            if (xe) return fail(ctx, SNOWGPU_E_HIP, std::string("expand launch: ") + hipGetErrorString((hipError_t)xe));
        }
        BatchDev &b = k.b;
        b = BatchDev{};
        b.n_frames = cf; b.n_total = cn; b.frame_off = ctx->pipe_off.p + c_pos[(size_t)c]; b.rows = ctx->rows_in.p + (size_t)r0 * rb;
        int64_t mx = 0;
        bool uni = false;
        frame_extent(cf, lo, &mx, &uni);
        b.max_frame = mx; b.uniform_rows = uni ? mx : 0;
        b.dtype = dtype; b.table_ids = ctx->table_ids.p + (size_t)f0 * nl; b.beam_div_deg = beam_div_deg;
        b.thr_poly = d_thr ? d_thr + 3 * (size_t)f0 : nullptr;
        b.plane = (!d_thr && plane) ? ctx->plane.p + 4 * (size_t)f0 : nullptr;
        b.noise_floor = noise_floor; b.perm = perm ? ctx->user_perm.p + r0 : nullptr;
        k.po = SgPackOut{};
        if (packed) {
            k.po.meta = ctx->pk_meta.p + r0; k.po.inten = ctx->pk_int.p + (size_t)r0 * esz; k.po.mv = ctx->pk_mv.p + (size_t)r0 * 3 * esz;
            k.po.mv_counts = ctx->pk_mvcnt.p + f0;
            b.pack = &k.po;
        } else {
            b.out_rows = ctx->rows_out.p + (size_t)r0 * rb; b.out_src = ctx->out_src.p + r0;
        }
        b.out_counts = ctx->out_counts.p + f0; b.out_stats = ctx->out_stats.p + 3 * (size_t)f0;
        b.out_thr_poly = out_thr_poly ? ctx->out_thr.p + 3 * (size_t)f0 : nullptr;
        b.status = ctx->pipe_status.p + 8 * (size_t)c; b.stream = cs;
        // Beside a saturated link every cross-stream event costs more (the queues' completion signals live in host memory), so a
        // chunk keeps its kernels on one stream: 1.80 instead of 1.76 G points/s (2.09 / 1.96 without source indices), although
        // the same chunk alone is faster with its side streams.
        b.serial = true;
        if (cb && cn > 0) {
            // the device half of the prepass first (snowgpu_prepass_stats' kernels on the chunk), its results on their way down at once
            if (int hrc = device_prepass_half(lc, ctx, b.rows, dtype, b.frame_off, cf, cn, mx, b.plane, cs)) return hrc;
            HIPCHK(ctx, hipEventRecord(ctx->thr_ev[2 * (size_t)c], cs));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->s_d2h, ctx->thr_ev[2 * (size_t)c], 0));
            HIPCHK(ctx, hipMemcpyAsync(ts.hist + (size_t)f0 * SG_THR_HIST, lc->stats_hist.p, (size_t)cf * SG_THR_HIST * 4, hipMemcpyDeviceToHost, ctx->s_d2h));
            HIPCHK(ctx, hipMemcpyAsync(ts.rec + (size_t)f0 * SG_PRE_REC, lc->stats_rec.p, (size_t)cf * SG_PRE_REC * 8, hipMemcpyDeviceToHost, ctx->s_d2h));
            HIPCHK(ctx, hipMemcpyAsync(ts.stat + 8 * (size_t)c, lc->d_status, 32, hipMemcpyDeviceToHost, ctx->s_d2h));
            HIPCHK(ctx, hipEventRecord(ctx->thr_ev[2 * (size_t)c + 1], ctx->s_d2h));
            b.defer_thr = true;
        }
        int brc = run_batch(lc, b);
        if (brc != SNOWGPU_OK && lc != ctx) ctx->err = lc->err;
        return brc;
    };
    // chunk c: (the caller's threshold fit and the compaction, then) its downloads
    auto finish = [&](int c) -> int {
        const int f0 = c_first[(size_t)c], f1 = c_first[(size_t)c + 1], cf = f1 - f0;
        const int64_t r0 = frame_offsets[f0], cn = frame_offsets[f1] - r0;
        Chunk &k = chunks[(size_t)c];
        BatchDev &b = k.b;
        hipStream_t cs = k.lc->stream;
        if (b.defer_thr) {
            HIPCHK(ctx, hipEventSynchronize(ctx->thr_ev[2 * (size_t)c + 1]));
            const int32_t *s8 = ts.stat + 8 * (size_t)c;
            if (s8[0] != 0) {                                  // (fewer than 3 ground rows in a frame: reported as the device prepass reports it)
                HIPCHK(ctx, hipMemcpyAsync(b.status, k.lc->d_status, 32, hipMemcpyDeviceToDevice, cs));
                pk_skip[(size_t)c] = 1;                        // (a later chunk's finish moves pk_enq past this one: nothing of it to assemble)
                return SNOWGPU_OK;                             // the chunk's status words carry the error to the end of the call
            }
            const int crc = ctx->thr_fn(ctx->thr_user, f0, cf, ts.hist + (size_t)f0 * SG_THR_HIST, ts.rec + (size_t)f0 * SG_PRE_REC, ts.thr + 3 * (size_t)f0);
            if (crc != 0) return fail(ctx, SNOWGPU_E_INVALID, "the threshold callback reported an error");
            HIPCHK(ctx, hipMemcpyAsync(ctx->user_thr.p + 3 * (size_t)f0, ts.thr + 3 * (size_t)f0, sizeof(double) * 3 * (size_t)cf, hipMemcpyHostToDevice, cs));
            b.thr_poly = ctx->user_thr.p + 3 * (size_t)f0;
            int crc2 = run_compaction(k.lc, b);
            if (crc2 != SNOWGPU_OK) { if (k.lc != ctx) ctx->err = k.lc->err; return crc2; }
        }
        if (packed) {
            // The chunk's words and intensities come down as two copies of its whole row range (the rows of a frame are compacted at the
            // frame's offset: what lies behind a frame's kept rows travels unused -- a copy per frame instead cost ~20 us each, 17 ms per
            // batch), then the head of its list of moved coordinates -- room for one row in eight: the list's length is only known on the
            // device, and a copy sized by it would have to queue behind the copies of every later chunk --, then its counts.  A chunk with
            // more scattered rows than that gets the rest of its list by one more copy (pk_progress).
            SgPackOut &po = k.po;
            HIPCHK(ctx, hipEventRecord(ctx->pipe_ev[2 * (size_t)c + 1], cs));
            if (trace) HIPCHK(ctx, hipEventRecord(tev[3 + 4 * (size_t)c], cs));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->s_d2h, ctx->pipe_ev[2 * (size_t)c + 1], 0));
            if (cn) {
                HIPCHK(ctx, hipMemcpyAsync(st_meta + (size_t)r0 * 4, po.meta, (size_t)cn * 4, hipMemcpyDeviceToHost, ctx->s_d2h));
                HIPCHK(ctx, hipMemcpyAsync(st_int + (size_t)r0 * esz, po.inten, (size_t)cn * esz, hipMemcpyDeviceToHost, ctx->s_d2h));
                HIPCHK(ctx, hipMemcpyAsync(st_mv + (size_t)r0 * 3 * esz, po.mv, pk_mv_head((size_t)cn) * 3 * esz, hipMemcpyDeviceToHost, ctx->s_d2h));
            }
            HIPCHK(ctx, hipMemcpyAsync(st_cnt + f0, b.out_counts, sizeof(int64_t) * (size_t)cf, hipMemcpyDeviceToHost, ctx->s_d2h));
            HIPCHK(ctx, hipMemcpyAsync(st_mvcnt + f0, po.mv_counts, sizeof(int64_t) * (size_t)cf, hipMemcpyDeviceToHost, ctx->s_d2h));
            HIPCHK(ctx, hipEventRecord(ctx->pk_ev[2 * (size_t)c], ctx->s_d2h));
            pk_enq = c + 1;
            if (hipError_t pe = pk_progress(false); pe != hipSuccess) return fail(ctx, SNOWGPU_E_HIP, std::string("packed download: ") + hipGetErrorString(pe));
            return SNOWGPU_OK;
        }
        HIPCHK(ctx, hipEventRecord(ctx->pipe_ev[2 * (size_t)c + 1], cs));
        if (trace) HIPCHK(ctx, hipEventRecord(tev[3 + 4 * (size_t)c], cs));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->s_d2h, ctx->pipe_ev[2 * (size_t)c + 1], 0));
        if (cn) {
            HIPCHK(ctx, hipMemcpyAsync((char *)out_rows + (size_t)r0 * rb, b.out_rows, (size_t)cn * rb, hipMemcpyDeviceToHost, ctx->s_d2h));
            if (out_src) HIPCHK(ctx, hipMemcpyAsync(out_src + r0, b.out_src, sizeof(int32_t) * (size_t)cn, hipMemcpyDeviceToHost, ctx->s_d2h));
        }
        if (trace) HIPCHK(ctx, hipEventRecord(tev[4 + 4 * (size_t)c], ctx->s_d2h));
        return SNOWGPU_OK;
    };
    for (int c = 0; c < n_chunks && rc == SNOWGPU_OK; ++c) {
        if (cb && c >= L) rc = finish(c - L);                  // (frees the lane chunk c computes on)
        if (rc == SNOWGPU_OK) rc = compute(c);
        if (rc == SNOWGPU_OK && !cb) rc = finish(c);
    }
    for (int c = std::max(0, n_chunks - L); cb && c < n_chunks && rc == SNOWGPU_OK; ++c) rc = finish(c);
    if (packed) {
        ctx->pk_times[0] = now() - t_begin;
        if (rc == SNOWGPU_OK) { if (hipError_t pe = pk_progress(true); pe != hipSuccess) rc = fail(ctx, SNOWGPU_E_HIP, std::string("packed download (drain): ") + hipGetErrorString(pe)); }
        ctx->pk_times[1] = now() - t_begin;
        ctx->pool->wait_idle();                       // (drain() waits for the pool too; here for the time stamp)
        ctx->pk_times[2] = now() - t_begin;
    }
    if (trace) fprintf(stderr, "pipe: %d chunks; uploads enqueued in %.3f ms, everything in %.3f ms\n", n_chunks, t_up - t_begin, now() - t_begin);
    const hipError_t se = hc.drain();
    if (trace) {
        fprintf(stderr, "pipe: drained at %.3f ms\n", now() - t_begin);
        for (int c = 0; c < n_chunks; ++c) {
            float t[4] = {0, 0, 0, 0};
            for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&t[k], tev[0], tev[1 + 4 * (size_t)c + k]);
            fprintf(stderr, "pipe chunk %2d: uploaded %7.3f  compute %7.3f .. %7.3f  downloaded %7.3f ms\n", c, t[0], t[1], t[2], t[3]);
        }
        for (auto &e : tev) (void)hipEventDestroy(e);
    }
    if (rc != SNOWGPU_OK) return rc;
    if (se != hipSuccess) return fail(ctx, SNOWGPU_E_HIP, std::string("stream synchronize: ") + hipGetErrorString(se));
    std::vector<int32_t> h_st((size_t)n_chunks * 8, 0);
    HIPCHK(ctx, hipMemcpy(h_st.data(), ctx->pipe_status.p, sizeof(int32_t) * h_st.size(), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(out_counts, ctx->out_counts.p, sizeof(int64_t) * nf, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(out_stats, ctx->out_stats.p, sizeof(int64_t) * 3 * nf, hipMemcpyDeviceToHost));
    if (out_thr_poly) HIPCHK(ctx, hipMemcpy(out_thr_poly, ctx->out_thr.p, sizeof(double) * 3 * nf, hipMemcpyDeviceToHost));
    int32_t agg[8] = {0, -1, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < n_chunks; ++c) {
        const int32_t *s8 = &h_st[(size_t)c * 8];
        if (agg[0] == 0 && s8[0] != 0) {           // the offending row is chunk-local on the device: report it as a row of the batch
            agg[0] = s8[0];
            agg[1] = s8[1] >= 0 ? (int32_t)std::min<int64_t>(s8[1] + frame_offsets[c_first[(size_t)c]], INT32_MAX) : -1;
        }
        for (int k = 2; k < 7; ++k) agg[k] += s8[k];        // tier populations and the row kernels' redone beams
    }
    std::memcpy(ctx->h_status, agg, sizeof agg);
    return status_to_error(ctx, agg);
}

static int ensure_mail(snowgpu_ctx *ctx, size_t up, size_t dn)
{
    if (int rc = grow_pinned(ctx, ctx->mail_up_h, ctx->mail_up_cap, up, up / 2 + 4096)) return rc;
    if (int rc = grow_pinned(ctx, ctx->mail_dn_h, ctx->mail_dn_cap, dn, dn / 2 + 4096)) return rc;
    ENSURE(ctx, ctx->mail_up_d, ctx->mail_up_cap);
    ENSURE(ctx, ctx->mail_dn_d, ctx->mail_dn_cap);
    return SNOWGPU_OK;
}

static int host_batch(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                      const int32_t *table_ids, double beam_div_deg, const double *thr_poly, const double *plane,
                      double noise_floor, const int32_t *perm, void *out_rows, int32_t *out_src, int64_t *out_counts,
                      int64_t *out_stats, double *out_thr_poly, int dbg_cap, int32_t *dbg_count, double *dbg_rj,
                      double *dbg_ratio, int32_t *perm_out)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || !frame_offsets || !table_ids || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_augment_batch: null pointer or bad dtype");
    int64_t max_frame = 0, n_total = 0;
    bool uniform = false;
    if (int frc = check_frames(ctx, n_frames, frame_offsets, &max_frame, &uniform, &n_total)) return frc;
    if (n_total > 0 && !out_rows) return fail(ctx, SNOWGPU_E_INVALID, "null row buffers");
    if (n_total > 0 && !rows && (ctx->resident_rows != n_total || ctx->resident_dtype != dtype || (int)ctx->resident_off.size() != n_frames + 1 ||
                                 !std::equal(ctx->resident_off.begin(), ctx->resident_off.end(), frame_offsets)))
        return fail(ctx, SNOWGPU_E_INVALID, "rows == NULL needs the rows of the last snowgpu_prepass_stats call (same frame offsets and dtype)");
    if (rows) ctx->resident_rows = -1;                 // (a fresh upload replaces whatever was resident)
    if (!out_counts || !out_stats) return fail(ctx, SNOWGPU_E_INVALID, "null count/stat buffers");
    if (ctx->h_las.n <= 0) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_lasers has not been called");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool wants_precrop = ctx->fov.enabled && ctx->fov_pre && !dbg_count && n_total > 0;
    if (wants_precrop && !rows) return fail(ctx, SNOWGPU_E_INVALID, "rows == NULL cannot be combined with the pre-augment crop");
    if (wants_precrop && perm) return fail(ctx, SNOWGPU_E_INVALID, "a caller-supplied permutation cannot be combined with the pre-augment crop");
    if (!dbg_count && !perm_out && !wants_precrop && ctx->pipe_rows > 0 && n_frames > 1 && n_total > ctx->pipe_rows + ctx->pipe_rows / 2)
        return host_batch_pipelined(ctx, n_frames, frame_offsets, rows, dtype, table_ids, beam_div_deg, thr_poly, plane, noise_floor, perm,
                                    out_rows, out_src, out_counts, out_stats, out_thr_poly);
    const size_t esz = dtype == 0 ? 4 : 8, n = (size_t)n_total;
    const size_t row_bytes = n * 5 * esz;
    hipStream_t st = ctx->stream;
    ENSURE(ctx, ctx->rows_in, std::max<size_t>(row_bytes, 8));
    ENSURE(ctx, ctx->rows_out, std::max<size_t>(row_bytes, 8));
    ENSURE(ctx, ctx->out_src, std::max<size_t>(n, 1));
    ENSURE(ctx, ctx->thr_poly, (size_t)n_frames * 3);
    // the small arrays: one block up (offsets | polynomials or planes | table ids), one block down (status | counts | stats | polynomials)
    const size_t nfz = (size_t)n_frames, nlz = (size_t)ctx->h_las.n;
    const size_t up_off = 0, up_par = up_off + 8 * (nfz + 1), up_ids = up_par + 8 * 4 * nfz, up_bytes = up_ids + 4 * nfz * nlz;
    const size_t dn_st = 0, dn_cnt = 32, dn_stats = dn_cnt + 8 * nfz, dn_thr = dn_stats + 24 * nfz, dn_bytes = dn_thr + 24 * nfz;
    {
        int mrc = ensure_mail(ctx, up_bytes, dn_bytes);
        if (mrc) return mrc;
    }
    std::memcpy(ctx->mail_up_h + up_off, frame_offsets, 8 * (nfz + 1));
    if (thr_poly) std::memcpy(ctx->mail_up_h + up_par, thr_poly, 24 * nfz);
    else if (plane) std::memcpy(ctx->mail_up_h + up_par, plane, 32 * nfz);          // neither: the plane is estimated on the device
    std::memcpy(ctx->mail_up_h + up_ids, table_ids, 4 * nfz * nlz);
    std::vector<int64_t> crop_off, crop_cnt;           // (the pre-augment crop copies from / into them: declared ahead of the guard)
    HostCall hc{ctx};
    HIPCHK(ctx, hipMemcpyAsync(ctx->mail_up_d.p, ctx->mail_up_h, up_bytes, hipMemcpyHostToDevice, st));
    if (row_bytes && rows && ctx->in_channels) {       // compact input (snowgpu_augment_batch_compact)
        ENSURE(ctx, ctx->rows_c4, n * 16);
        ENSURE(ctx, ctx->rows_ch, n);
        HIPCHK(ctx, hipMemcpyAsync(ctx->rows_c4.p, rows, n * 16, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->rows_ch.p, ctx->in_channels, n, hipMemcpyHostToDevice, st));
        int xe = sg_launch_expand_rows(ctx->rows_c4.p, ctx->rows_ch.p, ctx->rows_in.p, n_total, st);
        if (xe) return fail(ctx, SNOWGPU_E_HIP, std::string("expand launch: ") + hipGetErrorString((hipError_t)xe));
    } else if (row_bytes && rows) HIPCHK(ctx, hipMemcpyAsync(ctx->rows_in.p, rows, row_bytes, hipMemcpyHostToDevice, st));
    const int64_t *d_frame_off = (const int64_t *)(ctx->mail_up_d.p + up_off);
    const int32_t *d_table_ids = (const int32_t *)(ctx->mail_up_d.p + up_ids);
    const double *d_thr = thr_poly ? (const double *)(ctx->mail_up_d.p + up_par) : nullptr;
    const double *d_plane = (thr_poly || !plane) ? nullptr : (const double *)(ctx->mail_up_d.p + up_par);
    int32_t *d_status = (int32_t *)(ctx->mail_dn_d.p + dn_st);
    int64_t *d_counts = (int64_t *)(ctx->mail_dn_d.p + dn_cnt), *d_stats = (int64_t *)(ctx->mail_dn_d.p + dn_stats);
    double *d_thr_out = (double *)(ctx->mail_dn_d.p + dn_thr);
    DevBuf<int32_t> &user_perm = ctx->user_perm;
    if (perm) {
        if (user_perm.ensure(std::max<size_t>(n, 1))) return fail(ctx, SNOWGPU_E_HIP, "hipMalloc failed for perm");
        if (n) HIPCHK(ctx, hipMemcpyAsync(user_perm.p, perm, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    }
    // Pre-augment camera crop (precompute.py:96-99): the frames are compacted on the device before anything else sees
    // them; only the per-frame counts visit the host (the frame offsets of the cropped batch are made there).
    const bool precrop = wants_precrop;
    const void *d_rows_used = ctx->rows_in.p;
    const int64_t *d_off_used = d_frame_off;
    int64_t n_used = n_total, max_frame_used = max_frame;
    if (precrop) {
        const int64_t max_tiles = sg_tiles(max_frame);
        ENSURE(ctx, ctx->keep, n);
        ENSURE(ctx, ctx->ctile_cnt, (size_t)n_frames * (size_t)max_tiles + 1);
        ENSURE(ctx, ctx->ctile_base, (size_t)n_frames * (size_t)max_tiles + 1);
        ENSURE(ctx, ctx->crop_counts, (size_t)n_frames);
        ENSURE(ctx, ctx->crop_stats, (size_t)n_frames * 3);
        ENSURE(ctx, ctx->crop_off, (size_t)n_frames + 1);
        ENSURE(ctx, ctx->rows_crop, row_bytes);
        ENSURE(ctx, ctx->crop_src, n);
        ENSURE(ctx, ctx->crop_out_src, n);
        int e = sg_launch_crop_count(ctx->rows_in.p, dtype, d_frame_off, n_frames, ctx->keep.p, ctx->ctile_cnt.p, ctx->ctile_base.p,
                                     ctx->crop_counts.p, ctx->crop_stats.p, &ctx->fov, max_tiles, st);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("crop launch: ") + hipGetErrorString((hipError_t)e));
        crop_cnt = std::vector<int64_t>((size_t)n_frames);
        HIPCHK(ctx, hipMemcpyAsync(crop_cnt.data(), ctx->crop_counts.p, sizeof(int64_t) * (size_t)n_frames, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        crop_off.assign((size_t)n_frames + 1, 0);
        for (int f = 0; f < n_frames; ++f) crop_off[(size_t)f + 1] = crop_off[(size_t)f] + crop_cnt[(size_t)f];
        frame_extent(n_frames, crop_off.data(), &max_frame_used, &uniform);
        n_used = crop_off[(size_t)n_frames];
        HIPCHK(ctx, hipMemcpyAsync(ctx->crop_off.p, crop_off.data(), sizeof(int64_t) * ((size_t)n_frames + 1), hipMemcpyHostToDevice, st));
        e = sg_launch_crop_scatter(ctx->rows_in.p, dtype, ctx->keep.p, nullptr, d_frame_off, ctx->crop_off.p, n_frames, ctx->ctile_base.p,
                                   ctx->rows_crop.p, ctx->crop_src.p, max_tiles, st);
        if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("crop launch: ") + hipGetErrorString((hipError_t)e));
        d_rows_used = ctx->rows_crop.p; d_off_used = ctx->crop_off.p;
    }
    BatchDev b{};
    b.n_frames = n_frames; b.n_total = n_used; b.max_frame = max_frame_used; b.frame_off = d_off_used; b.rows = d_rows_used;
    b.uniform_rows = uniform ? max_frame_used : 0;
    b.dtype = dtype; b.table_ids = d_table_ids; b.beam_div_deg = beam_div_deg; b.thr_poly = d_thr;
    b.plane = d_plane; b.noise_floor = noise_floor; b.perm = perm ? user_perm.p : nullptr;
    b.out_rows = ctx->rows_out.p; b.out_src = ctx->out_src.p; b.out_counts = d_counts; b.out_stats = d_stats;
    b.out_thr_poly = out_thr_poly ? d_thr_out : nullptr; b.status = d_status; b.stream = st;
    b.no_fov = dbg_count != nullptr;
    b.want_perm = perm_out != nullptr;
    if (dbg_count) {
        ENSURE(ctx, ctx->dbg_count, std::max<size_t>(n, 1));
        ENSURE(ctx, ctx->dbg_rj, std::max<size_t>(n * (size_t)dbg_cap, 1));
        ENSURE(ctx, ctx->dbg_ratio, std::max<size_t>(n * (size_t)dbg_cap, 1));
        HIPCHK(ctx, hipMemsetAsync(ctx->dbg_count.p, 0, sizeof(int32_t) * std::max<size_t>(n, 1), st));
        b.dbg_count = ctx->dbg_count.p; b.dbg_rj = ctx->dbg_rj.p; b.dbg_ratio = ctx->dbg_ratio.p; b.dbg_cap = dbg_cap;
    }
    int rc = SNOWGPU_OK;
    if (ctx->thr_fn && !thr_poly && !perm && !dbg_count && !precrop && n_used > 0) {
        // The caller fits the noise threshold (snowgpu_set_threshold_callback), one group = the whole (small) batch: device half of the
        // prepass, its results down, the per-beam kernels meanwhile, callback, polynomials up, compaction.
        ThrStage ts{};
        if (int trc = ensure_thr_stage(ctx, nfz, 1, &ts)) return trc;
        if (int hrc = device_prepass_half(ctx, ctx, d_rows_used, dtype, d_off_used, n_frames, n_used, max_frame_used, d_plane, st)) return hrc;
        HIPCHK(ctx, hipMemcpyAsync(ts.hist, ctx->stats_hist.p, nfz * SG_THR_HIST * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(ts.rec, ctx->stats_rec.p, nfz * SG_PRE_REC * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(ts.stat, ctx->d_status, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipEventRecord(ctx->thr_ev[1], st));
        b.defer_thr = true;
        rc = run_batch(ctx, b);
        if (rc == SNOWGPU_OK) {
            HIPCHK(ctx, hipEventSynchronize(ctx->thr_ev[1]));
            if (ts.stat[0] != 0) {
                std::memcpy(ctx->h_status, ts.stat, 32);
                return status_to_error(ctx, ts.stat);
            }
            if (ctx->thr_fn(ctx->thr_user, 0, n_frames, ts.hist, ts.rec, ts.thr) != 0) return fail(ctx, SNOWGPU_E_INVALID, "the threshold callback reported an error");
            HIPCHK(ctx, hipMemcpyAsync(ctx->user_thr.p, ts.thr, 24 * nfz, hipMemcpyHostToDevice, st));
            b.thr_poly = ctx->user_thr.p;
            rc = run_compaction(ctx, b);
        }
    } else {
        rc = run_batch(ctx, b);
    }
    int32_t status[8] = {0, -1, 0, 0, 0, 0, 0, 0};
    if (rc == SNOWGPU_OK) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->mail_dn_h, ctx->mail_dn_d.p, out_thr_poly ? dn_bytes : dn_thr, hipMemcpyDeviceToHost, st));
        if (row_bytes && !precrop) {
            HIPCHK(ctx, hipMemcpyAsync(out_rows, ctx->rows_out.p, row_bytes, hipMemcpyDeviceToHost, st));
            if (out_src) HIPCHK(ctx, hipMemcpyAsync(out_src, ctx->out_src.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        } else if (precrop && n_used > 0) {
            // source rows in the ORIGINAL frame: output row -> cropped row -> original row; every frame goes back to its own slot
            int e = sg_launch_compose_src(ctx->crop_off.p, d_counts, n_frames, max_frame_used, ctx->out_src.p, ctx->crop_src.p,
                                          ctx->crop_out_src.p, st);
            if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("compose launch: ") + hipGetErrorString((hipError_t)e));
            for (int f = 0; f < n_frames; ++f) {
                const size_t m = (size_t)(crop_off[(size_t)f + 1] - crop_off[(size_t)f]);
                if (!m) continue;
                HIPCHK(ctx, hipMemcpyAsync((char *)out_rows + (size_t)frame_offsets[f] * 5 * esz, (const char *)ctx->rows_out.p + (size_t)crop_off[(size_t)f] * 5 * esz,
                                           m * 5 * esz, hipMemcpyDeviceToHost, st));
                if (out_src) HIPCHK(ctx, hipMemcpyAsync(out_src + frame_offsets[f], ctx->crop_out_src.p + crop_off[(size_t)f], sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
            }
        }
        if (dbg_count && n) {
            HIPCHK(ctx, hipMemcpyAsync(dbg_count, ctx->dbg_count.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipMemcpyAsync(dbg_rj, ctx->dbg_rj.p, sizeof(double) * n * (size_t)dbg_cap, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipMemcpyAsync(dbg_ratio, ctx->dbg_ratio.p, sizeof(double) * n * (size_t)dbg_cap, hipMemcpyDeviceToHost, st));
        }
        if (perm_out && n && b.perm_out) HIPCHK(ctx, hipMemcpyAsync(perm_out, b.perm_out, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    }
    const hipError_t se = hc.drain();
    if (rc != SNOWGPU_OK) return rc;
    if (se != hipSuccess) return fail(ctx, SNOWGPU_E_HIP, std::string("stream synchronize: ") + hipGetErrorString(se));
    std::memcpy(status, ctx->mail_dn_h + dn_st, sizeof status);
    std::memcpy(out_counts, ctx->mail_dn_h + dn_cnt, 8 * nfz);
    std::memcpy(out_stats, ctx->mail_dn_h + dn_stats, 24 * nfz);
    if (out_thr_poly) std::memcpy(out_thr_poly, ctx->mail_dn_h + dn_thr, 24 * nfz);
    std::memcpy(ctx->h_status, status, sizeof status);
    return status_to_error(ctx, status);
}

extern "C" int snowgpu_augment_batch(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                                     const int32_t *table_ids, double beam_divergence_deg, const double *thr_poly,
                                     const double *plane, double noise_floor, const int32_t *perm, void *out_rows,
                                     int32_t *out_src, int64_t *out_counts, int64_t *out_stats, double *out_thr_poly)
{
    return host_batch(ctx, n_frames, frame_offsets, rows, dtype, table_ids, beam_divergence_deg, thr_poly, plane, noise_floor,
                      perm, out_rows, out_src, out_counts, out_stats, out_thr_poly, 0, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int snowgpu_augment_batch_compact(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const float *xyzi, const uint8_t *channels,
                                             const int32_t *table_ids, double beam_divergence_deg, const double *thr_poly, const double *plane,
                                             double noise_floor, float *out_rows, int32_t *out_src, int64_t *out_counts, int64_t *out_stats,
                                             double *out_thr_poly)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (!xyzi || !channels) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_augment_batch_compact: null input");
    if (ctx->fov.enabled && ctx->fov_pre) return fail(ctx, SNOWGPU_E_INVALID, "the pre-augment crop takes (x, y, z, intensity, channel) rows: snowgpu_augment_batch");
    ctx->in_channels = channels;
    const int rc = host_batch(ctx, n_frames, frame_offsets, xyzi, 0, table_ids, beam_divergence_deg, thr_poly, plane, noise_floor, nullptr, out_rows,
                              out_src, out_counts, out_stats, out_thr_poly, 0, nullptr, nullptr, nullptr, nullptr);
    ctx->in_channels = nullptr;
    return rc;
}

extern "C" int snowgpu_debug_occlusions(snowgpu_ctx *ctx, int64_t n_rows, const void *rows, int dtype, const int32_t *table_ids,
                                        double beam_divergence_deg, int cap, int32_t *count, double *rj, double *ratio,
                                        int32_t *sorted_src)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_rows < 0 || cap <= 0 || !count || !rj || !ratio || !sorted_src) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_debug_occlusions: bad arguments");
    const int64_t off[2] = {0, n_rows};
    const double thr[3] = {0.0, 0.0, -1.0};   // keep everything
    const size_t esz = dtype == 0 ? 4 : 8;
    std::vector<unsigned char> out_rows((size_t)n_rows * 5 * esz + 8);
    std::vector<int32_t> out_src((size_t)n_rows + 1);
    int64_t cnt = 0, stats[3];
    return host_batch(ctx, 1, off, rows, dtype, table_ids, beam_divergence_deg, thr, nullptr, 0.7, nullptr, out_rows.data(),
                      out_src.data(), &cnt, stats, nullptr, cap, count, rj, ratio, sorted_src);
}

// The same chain for frames in HOST memory: copies in, the device entry above, copies out -- one synchronisation.
extern "C" int snowgpu_augment_wet_batch(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                                         const int32_t *table_ids, double beam_divergence_deg, const double *thr_poly,
                                         const double *plane, double noise_floor, const int32_t *perm, const double *wet_plane,
                                         double water_height, double pavement_depth, double wet_noise_floor, double power_factor,
                                         int flat_earth, double delta, int replace, double *out_rows, int32_t *out_src,
                                         int64_t *out_counts, int64_t *out_stats, int32_t *out_flags)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || !frame_offsets || !table_ids || !out_counts || !out_stats || !out_flags || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_augment_wet_batch: null pointer or bad dtype");
    if (ctx->h_las.n <= 0) return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_set_lasers has not been called");
    int64_t max_frame = 0, n_total = 0;
    bool uni = false;
    if (int frc = check_frames(ctx, n_frames, frame_offsets, &max_frame, &uni, &n_total)) return frc;
    if (n_total > 0 && (!rows || !out_rows || !out_src)) return fail(ctx, SNOWGPU_E_INVALID, "null row buffers");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t esz = dtype == 0 ? 4 : 8, n = (size_t)n_total, nf = (size_t)n_frames, nl = (size_t)ctx->h_las.n;
    hipStream_t st = ctx->stream;
    ENSURE(ctx, ctx->rows_in, std::max<size_t>(n * 5 * esz, 8));
    ENSURE(ctx, ctx->wet_rows, std::max<size_t>(n * 5, 1));
    ENSURE(ctx, ctx->out_src, std::max<size_t>(n, 1));
    ENSURE(ctx, ctx->frame_off, nf + 1);
    ENSURE(ctx, ctx->wet_counts, nf);
    ENSURE(ctx, ctx->wet_flags, nf);
    ENSURE(ctx, ctx->out_stats, nf * 3);
    ENSURE(ctx, ctx->table_ids, nf * nl);
    ENSURE(ctx, ctx->plane, nf * 4);
    ENSURE(ctx, ctx->wet_plane, nf * 4);
    ctx->resident_rows = -1;
    int32_t status[8] = {0, -1, 0, 0, 0, 0, 0, 0};
    HostCall hc{ctx};
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->rows_in.p, rows, n * 5 * esz, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->frame_off.p, frame_offsets, sizeof(int64_t) * (nf + 1), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->table_ids.p, table_ids, sizeof(int32_t) * nf * nl, hipMemcpyHostToDevice, st));
    if (wet_plane) HIPCHK(ctx, hipMemcpyAsync(ctx->wet_plane.p, wet_plane, sizeof(double) * 4 * nf, hipMemcpyHostToDevice, st));
    const double *d_thr = nullptr;
    if (thr_poly) {
        ENSURE(ctx, ctx->user_thr, nf * 3);
        HIPCHK(ctx, hipMemcpyAsync(ctx->user_thr.p, thr_poly, sizeof(double) * 3 * nf, hipMemcpyHostToDevice, st));
        d_thr = ctx->user_thr.p;
    } else if (plane) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->plane.p, plane, sizeof(double) * 4 * nf, hipMemcpyHostToDevice, st));
    }
    if (perm) {
        ENSURE(ctx, ctx->user_perm, std::max<size_t>(n, 1));
        if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->user_perm.p, perm, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    }
    int rc = snowgpu_augment_wet_batch_device(ctx, n_frames, n_total, uni ? max_frame : std::max<int64_t>(max_frame, 1) , ctx->frame_off.p,
                                              ctx->rows_in.p, dtype, ctx->table_ids.p, beam_divergence_deg, d_thr, (d_thr || !plane) ? nullptr : ctx->plane.p,
                                              noise_floor, perm ? ctx->user_perm.p : nullptr, wet_plane ? ctx->wet_plane.p : nullptr, water_height,
                                              pavement_depth, wet_noise_floor, power_factor, flat_earth, delta, replace, ctx->wet_rows.p,
                                              ctx->out_src.p, ctx->wet_counts.p, ctx->out_stats.p, ctx->wet_flags.p, ctx->d_status, st);
    if (rc == SNOWGPU_OK) {
        HIPCHK(ctx, hipMemcpyAsync(status, ctx->d_status, sizeof status, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(out_counts, ctx->wet_counts.p, sizeof(int64_t) * nf, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(out_flags, ctx->wet_flags.p, sizeof(int32_t) * nf, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(out_stats, ctx->out_stats.p, sizeof(int64_t) * 3 * nf, hipMemcpyDeviceToHost, st));
        if (n) {
            HIPCHK(ctx, hipMemcpyAsync(out_rows, ctx->wet_rows.p, n * 5 * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipMemcpyAsync(out_src, ctx->out_src.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        }
    }
    const hipError_t se = hc.drain();
    if (rc != SNOWGPU_OK) return rc;
    if (se != hipSuccess) return fail(ctx, SNOWGPU_E_HIP, std::string("stream synchronize: ") + hipGetErrorString(se));
    std::memcpy(ctx->h_status, status, sizeof status);
    return status_to_error(ctx, status);
}

extern "C" int snowgpu_wet_ground_batch(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                                        const double *plane, double water_height, double pavement_depth, double noise_floor,
                                        double power_factor, int flat_earth, double delta, int replace, double *out_rows,
                                        int32_t *out_src, int64_t *out_counts, int32_t *out_flags)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || !frame_offsets || !out_counts || !out_flags || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_wet_ground_batch: null pointer or bad dtype");
    int64_t max_frame = 0, n_total = 0;
    bool uniform = false;
    if (int frc = check_frames(ctx, n_frames, frame_offsets, &max_frame, &uniform, &n_total)) return frc;
    if (n_total > 0 && (!rows || !out_rows || !out_src)) return fail(ctx, SNOWGPU_E_INVALID, "null row buffers");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t esz = dtype == 0 ? 4 : 8, n = (size_t)n_total;
    hipStream_t st = ctx->stream;
    ENSURE(ctx, ctx->rows_in, std::max<size_t>(n * 5 * esz, 8));
    ENSURE(ctx, ctx->rows_out, std::max<size_t>(n * 5 * 8, 8));
    ENSURE(ctx, ctx->out_src, std::max<size_t>(n, 1));
    ENSURE(ctx, ctx->frame_off, (size_t)n_frames + 1);
    ENSURE(ctx, ctx->out_counts, (size_t)n_frames);
    ENSURE(ctx, ctx->plane, (size_t)n_frames * 4);
    ENSURE(ctx, ctx->dbg_count, (size_t)n_frames);   // reused as the per-frame "returned unchanged" flags
    ctx->resident_rows = -1;
    int32_t status[8] = {0, -1, 0, 0, 0, 0, 0, 0};
    HostCall hc{ctx};
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->rows_in.p, rows, n * 5 * esz, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->frame_off.p, frame_offsets, sizeof(int64_t) * ((size_t)n_frames + 1), hipMemcpyHostToDevice, st));
    if (plane) HIPCHK(ctx, hipMemcpyAsync(ctx->plane.p, plane, sizeof(double) * 4 * (size_t)n_frames, hipMemcpyHostToDevice, st));
    else {                   // wet_ground/augmentation.py:41 calculate_plane(pointcloud) on the device
        int pe = sg_plane_run(&ctx->plane_scr, &ctx->plane_par, ctx->rows_in.p, dtype, ctx->frame_off.p, nullptr, n_frames, n_total, max_frame,
                              ctx->plane.p, nullptr, st);
        if (pe) return fail(ctx, SNOWGPU_E_HIP, std::string("plane estimate: ") + (pe > 0 ? hipGetErrorString((hipError_t)pe) : "allocation"));
    }
    HIPCHK(ctx, hipMemsetAsync(ctx->d_status, 0, sizeof(int32_t) * 8, st));
    SgWetParams wp;
    if (int rc = wet_settings(ctx, SgWetScalars{water_height, pavement_depth, noise_floor, power_factor, delta, flat_earth, replace}, n_frames, true, st, &wp)) return rc;
    int e = sg_wet_run(&ctx->prepass, ctx->rows_in.p, dtype, ctx->frame_off.p, nullptr, n_frames, n_total, max_frame, ctx->plane.p, &wp,
                       (double *)ctx->rows_out.p, ctx->out_src.p, ctx->out_counts.p, ctx->dbg_count.p, ctx->d_status, st);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("wet ground: ") + (e > 0 ? hipGetErrorString((hipError_t)e) : "allocation"));
    HIPCHK(ctx, hipMemcpyAsync(out_counts, ctx->out_counts.p, sizeof(int64_t) * (size_t)n_frames, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(out_flags, ctx->dbg_count.p, sizeof(int32_t) * (size_t)n_frames, hipMemcpyDeviceToHost, st));
    if (n) {
        HIPCHK(ctx, hipMemcpyAsync(out_rows, ctx->rows_out.p, n * 5 * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(out_src, ctx->out_src.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(status, ctx->d_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hc.drain());
    if (status[0] == SNOWGPU_E_GROUND)     // only 'poly' reports here: np.polyfit of degree 2 over fewer than 3 points (augmentation.py:243)
        return fail(ctx, SNOWGPU_E_GROUND, "estimation method 'poly': fewer than 3 range rows of the histogram have a sparsest bin above 5");
    return status_to_error(ctx, status);
}

extern "C" int snowgpu_estimate_planes(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                                       double *out_planes, int32_t *out_info)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || !frame_offsets || !out_planes || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_estimate_planes: null pointer or bad dtype");
    int64_t max_frame = 0, n_total = 0;
    bool uniform = false;
    if (int frc = check_frames(ctx, n_frames, frame_offsets, &max_frame, &uniform, &n_total)) return frc;
    if (n_total > 0 && !rows) return fail(ctx, SNOWGPU_E_INVALID, "null row buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t esz = dtype == 0 ? 4 : 8, nf = (size_t)n_frames;
    hipStream_t st = ctx->stream;
    ENSURE(ctx, ctx->frame_off, nf + 1);
    ENSURE(ctx, ctx->plane_est, nf * 4);
    ENSURE(ctx, ctx->plane_info, nf * 4);
    HostCall hc{ctx};
    HIPCHK(ctx, hipMemcpyAsync(ctx->frame_off.p, frame_offsets, sizeof(int64_t) * (nf + 1), hipMemcpyHostToDevice, st));
    if (ctx->plane_par.method != SG_PLANE_REFERENCE && n_total > 0) {       // (the reference-today plane reads no row)
        ctx->resident_rows = -1;
        ENSURE(ctx, ctx->rows_in, (size_t)n_total * 5 * esz);
        HIPCHK(ctx, hipMemcpyAsync(ctx->rows_in.p, rows, (size_t)n_total * 5 * esz, hipMemcpyHostToDevice, st));
    }
    int e = sg_plane_run(&ctx->plane_scr, &ctx->plane_par, ctx->rows_in.p, dtype, ctx->frame_off.p, nullptr, n_frames, n_total, max_frame,
                         ctx->plane_est.p, ctx->plane_info.p, st);
    if (e) return fail(ctx, SNOWGPU_E_HIP, std::string("plane estimate: ") + (e > 0 ? hipGetErrorString((hipError_t)e) : "allocation"));
    HIPCHK(ctx, hipMemcpyAsync(out_planes, ctx->plane_est.p, sizeof(double) * 4 * nf, hipMemcpyDeviceToHost, st));
    if (out_info) HIPCHK(ctx, hipMemcpyAsync(out_info, ctx->plane_info.p, sizeof(int32_t) * 4 * nf, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hc.drain());
    return SNOWGPU_OK;
}

// ---- noise-threshold prepass, first half (simulation.py:449-461; wet_ground/augmentation.py:195-235) -------------------------
// For a caller that wants the reference's answer on ITS machine (quirk Q8): the 50 x 2555 histogram of (range, I / cos) over the
// ground rows and the per-frame sums, from the device; the caller takes np.argpartition(hist, 2)[:, 0] itself, fits the noise
// line and the quadratic from the sums, and hands the polynomials to snowgpu_augment_batch (thr_poly).
extern "C" int snowgpu_prepass_stats(snowgpu_ctx *ctx, int n_frames, const int64_t *frame_offsets, const void *rows, int dtype,
                                     const double *plane, int32_t *out_hist, double *out_rec)
{
    if (!ctx) return SNOWGPU_E_INVALID;
    if (n_frames <= 0 || !frame_offsets || !out_hist || !out_rec || (dtype != 0 && dtype != 1))
        return fail(ctx, SNOWGPU_E_INVALID, "snowgpu_prepass_stats: null pointer or bad dtype");
    int64_t max_frame = 0, n_total = 0;
    bool uniform = false;
    if (int frc = check_frames(ctx, n_frames, frame_offsets, &max_frame, &uniform, &n_total)) return frc;
    if (n_total > 0 && !rows) return fail(ctx, SNOWGPU_E_INVALID, "null row buffer");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t esz = dtype == 0 ? 4 : 8, nf = (size_t)n_frames, hist_n = nf * SG_THR_HIST;
    hipStream_t st = ctx->stream;
    ENSURE(ctx, ctx->frame_off, nf + 1);
    ENSURE(ctx, ctx->plane, nf * 4);
    ENSURE(ctx, ctx->rows_in, std::max<size_t>((size_t)n_total * 5 * esz, 8));
    int32_t status[8] = {0, -1, 0, 0, 0, 0, 0, 0};
    HostCall hc{ctx};
    HIPCHK(ctx, hipMemcpyAsync(ctx->frame_off.p, frame_offsets, sizeof(int64_t) * (nf + 1), hipMemcpyHostToDevice, st));
    if (n_total) HIPCHK(ctx, hipMemcpyAsync(ctx->rows_in.p, rows, (size_t)n_total * 5 * esz, hipMemcpyHostToDevice, st));
    if (plane) HIPCHK(ctx, hipMemcpyAsync(ctx->plane.p, plane, sizeof(double) * 4 * nf, hipMemcpyHostToDevice, st));
    if (int hrc = device_prepass_half(ctx, ctx, ctx->rows_in.p, dtype, ctx->frame_off.p, n_frames, n_total, max_frame, plane ? ctx->plane.p : nullptr, st)) return hrc;
    HIPCHK(ctx, hipMemcpyAsync(out_hist, ctx->stats_hist.p, sizeof(int32_t) * hist_n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(out_rec, ctx->stats_rec.p, sizeof(double) * nf * SG_PRE_REC, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(status, ctx->d_status, sizeof status, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hc.drain());
    ctx->resident_rows = n_total; ctx->resident_dtype = dtype;
    ctx->resident_off.assign(frame_offsets, frame_offsets + n_frames + 1);
    return status_to_error(ctx, status);
}
