// sg_assemble.h -- the host-thread side of the packed result transfer (snowgpu_set_result_transfer): where the threads run, the pool
// they form and the loop that puts one frame's output rows together.  Plain C++17, no HIP: tests/host_harness/assemble_frames.cpp
// compiles it with g++ and runs it under the sanitizers.
#pragma once
#include <pthread.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#pragma GCC visibility push(hidden)

// NUMA placement of the host threads that copy rows (packed result transfer).  On a two-socket host a core reaches the other socket's
// memory at a fraction of the speed: with free-roaming threads the same call gave 1.4 - 2.2 G points/s from run to run, with the threads
// on the wrong node 1.3, on the right one 2.3.  The right one is where the caller's row buffers live (asked of the kernel per call:
// get_mempolicy on their first pages); if that cannot be told -- a container may forbid the call -- the node the device hangs on.
inline bool cpus_of_node(int node, cpu_set_t *out)
{
    char path[128];
    std::snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *fh = std::fopen(path, "r");
    if (!fh) return false;
    char list[4096] = {0};
    const bool ok = std::fgets(list, (int)sizeof list, fh) != nullptr;
    std::fclose(fh);
    if (!ok) return false;
    cpu_set_t allowed, node_set;
    CPU_ZERO(&allowed); CPU_ZERO(&node_set);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return false;
    for (char *p = list; *p;) {                       // "0-63,128-191"
        char *end = nullptr;
        long a = std::strtol(p, &end, 10), b = a;
        if (end == p) break;
        if (*end == '-') { p = end + 1; b = std::strtol(p, &end, 10); }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) if (CPU_ISSET((int)c, &allowed)) CPU_SET((int)c, &node_set);
        if (*end != ',') break;
        p = end + 1;
    }
    if (CPU_COUNT(&node_set) == 0) return false;
    *out = node_set;
    return true;
}

inline int node_of_address(const void *p)
{
    if (!p) return -1;
    int node = -1;
    // get_mempolicy(&node, NULL, 0, addr, MPOL_F_NODE | MPOL_F_ADDR): the node of the page that holds addr
    const long rc = syscall(SYS_get_mempolicy, &node, nullptr, 0UL, const_cast<void *>(p), 1UL /* MPOL_F_NODE */ | 2UL /* MPOL_F_ADDR */);
    return rc == 0 ? node : -1;
}

// Host threads that put output rows together in the packed result transfer (snowgpu_set_result_transfer): plain copies, no arithmetic.
struct AsmPool {
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv, cv_done;
    std::deque<std::function<void()>> q;
    size_t pending = 0;
    bool stop = false;
    cpu_set_t want{};                 // where the threads should run (set_node), applied by each thread before its next job
    std::atomic<int> want_gen{0};
    int node = -2;
    void set_node(int nd)
    {
        if (nd == node) return;
        cpu_set_t c;
        if (nd < 0 || !cpus_of_node(nd, &c)) return;
        { std::lock_guard<std::mutex> lk(mu); want = c; node = nd; }
        want_gen.fetch_add(1);
    }
    void start(int n)
    {
        for (int i = 0; i < n; ++i)
            threads.emplace_back([this]() {
                int seen = 0;
                for (;;) {
                    std::function<void()> job;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [this]() { return stop || !q.empty(); });
                        if (q.empty()) return;
                        job = std::move(q.front());
                        q.pop_front();
                        if (seen != want_gen.load()) {      // (best effort: a forbidden call leaves the thread where it is)
                            seen = want_gen.load();
                            (void)pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), &want);
                        }
                    }
                    job();
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (--pending == 0) cv_done.notify_all();
                    }
                }
            });
    }
    void push(std::function<void()> job)
    {
        { std::lock_guard<std::mutex> lk(mu); q.push_back(std::move(job)); ++pending; }
        cv.notify_one();
    }
    void wait_idle()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [this]() { return pending == 0; });
    }
    ~AsmPool()
    {
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        for (auto &t : threads) t.join();
    }
};

// Rows of a chunk's list of moved coordinates that come down with the chunk's words (room for one row in eight; host_batch_pipelined says why).
inline size_t pk_mv_head(size_t chunk_rows) { return std::min(chunk_rows, std::max<size_t>(4096, chunk_rows / 8)); }

// A frame's moved rows as the device counted them, clamped to its row count (as sg_assemble_frame clamps kept): no copy or read past the frame's rows.
inline int64_t sg_moved_rows(int64_t mvcnt, int64_t n_rows) { return std::min<int64_t>(std::max<int64_t>(mvcnt, 0), n_rows); }

// One frame of a packed result: every pointer at the FRAME's first element.
struct SgAsmFrame {
    const void *in;             // the caller's input rows: (x, y, z, intensity, channel), or (x, y, z, intensity) for compact input
    const uint8_t *chn;         // compact input: the channel bytes
    const uint32_t *meta;       // per kept row: label code << 30 | source row
    const void *inten, *mv;     // per kept row its intensity; the moved coordinates of the label-2 rows, in their order
    void *out_rows;
    int32_t *out_src;           // may be null
    uint32_t n_rows;            // rows of the input frame
    int64_t kept_dev;           // kept rows as the device counted them
};

// out row j of the frame = the caller's input row src_j with the device's intensity and label; label-2 rows take their moved coordinates;
// rows without a laser (label 3) keep their channel.  What came back from the device bounds no host loop or index unchecked: kept is
// clamped to n_rows, src to n_rows - 1.
template <typename T, bool Compact> void sg_assemble_frame(const SgAsmFrame &a)
{
    constexpr size_t W = Compact ? 4 : 5;
    const int64_t kept = std::min<int64_t>(a.kept_dev, (int64_t)a.n_rows);
    const T *in = (const T *)a.in, *it = (const T *)a.inten, *mv = (const T *)a.mv;
    T *out = (T *)a.out_rows;
    for (int64_t j = 0; j < kept; ++j) {
        const uint32_t m = a.meta[j], code = m >> 30;
        uint32_t src = m & 0x3fffffffu;
        if (src >= a.n_rows) src = a.n_rows - 1;
        const T *ip = in + (size_t)src * W;
        T *q = out + (size_t)j * 5;
        if (code == 2) { q[0] = mv[0]; q[1] = mv[1]; q[2] = mv[2]; mv += 3; }
        else { q[0] = ip[0]; q[1] = ip[1]; q[2] = ip[2]; }
        q[3] = it[j];
        if constexpr (Compact) q[4] = code == 3 ? (T)a.chn[src] : (T)code;
        else q[4] = code == 3 ? ip[4] : (T)code;
        if (a.out_src) a.out_src[j] = (int32_t)src;
    }
}

#pragma GCC visibility pop
