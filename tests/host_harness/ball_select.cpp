// The selection network of the ball query (csrc/sg_ball.h: sg_ball_cx, the step schedule, sg_ball_sort_lanes, sg_ball_merge_lanes,
// sg_ball_wanted) compiled for the host and walked over 64 "lanes" as k_ball_query walks it across a wave, against std::sort.
//   ball_select            runs every case below; prints "ok <cases>" and returns 0, or prints the first difference and returns 1.
// Cases: candidate streams of 0 .. 5000 distinct indices arriving ascending, descending and scrambled, cut into batches of 64 whose
// lanes outside the ball hold SG_BALL_EMPTY; S = 1, 2, 16, 63, 64; fewer than S candidates in total; batches the threshold rejects.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "sg_ball.h"

static int fail(const char *what, int a, int b, int c)
{
    std::printf("FAILED %s %d %d %d\n", what, a, b, c);
    return 1;
}

// the schedule: 21 steps, blocks 2, 4, 4, 8, 8, 8, ..., distances k / 2 .. 1
static int check_schedule()
{
    int s = 0;
    for (int k = 2; k <= 64; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1, ++s)
            if (sg_ball_step_k(s) != k || sg_ball_step_j(s) != j) return fail("schedule", s, sg_ball_step_k(s), sg_ball_step_j(s));
    return s == SG_BALL_SORT_STEPS ? 0 : fail("steps", s, SG_BALL_SORT_STEPS, 0);
}

// one stream of candidates through the wave's loop; in_ball[i] == 0: the lane is outside the ball
static int run_stream(const std::vector<int32_t> &idx, const std::vector<uint8_t> &in_ball, int S, int tag, long *taken, long *rejected)
{
    int32_t kept[64];
    for (int l = 0; l < 64; ++l) kept[l] = SG_BALL_EMPTY;
    long count = 0;
    for (size_t p0 = 0; p0 < idx.size(); p0 += 64) {
        int32_t batch[64];
        bool any = false;
        for (int l = 0; l < 64; ++l) {
            const size_t p = p0 + (size_t)l;
            const bool in = p < idx.size() && in_ball[p] != 0;
            count += in ? 1 : 0;
            any = any || sg_ball_wanted(in, in ? idx[p] : SG_BALL_EMPTY, kept[S - 1]);
            batch[l] = in ? idx[p] : SG_BALL_EMPTY;
        }
        if (!any) { ++*rejected; continue; }
        ++*taken;
        sg_ball_sort_lanes(batch);
        for (int l = 1; l < 64; ++l)
            if (batch[l - 1] > batch[l]) return fail("sort", tag, l, batch[l]);
        sg_ball_merge_lanes(kept, batch);
    }
    std::vector<int32_t> want;
    for (size_t p = 0; p < idx.size(); ++p)
        if (in_ball[p]) want.push_back(idx[p]);
    std::sort(want.begin(), want.end());
    if ((long)want.size() != count) return fail("count", tag, (int)want.size(), (int)count);
    for (int l = 0; l < S; ++l) {
        const int32_t w = (size_t)l < want.size() ? want[(size_t)l] : SG_BALL_EMPTY;
        if (kept[l] != w) return fail("kept", tag, l, kept[l]);
    }
    return 0;
}

int main()
{
    if (check_schedule()) return 1;
    std::mt19937_64 rng(7);
    const int samples[5] = {1, 2, 16, 63, 64};
    const int sizes[12] = {0, 1, 15, 16, 17, 63, 64, 65, 128, 200, 1000, 5000};
    long cases = 0, taken = 0, rejected = 0;
    for (int S : samples)
        for (int n : sizes)
            for (int order = 0; order < 3; ++order)
                for (int sparse = 0; sparse < 2; ++sparse) {
                    // n distinct indices out of a range eight times as wide
                    std::vector<int32_t> idx;
                    int32_t v = (int32_t)(rng() % 1000);
                    for (int i = 0; i < n; ++i) { v += 1 + (int32_t)(rng() % 15); idx.push_back(v); }
                    if (order == 1) std::reverse(idx.begin(), idx.end());
                    if (order == 2) std::shuffle(idx.begin(), idx.end(), rng);
                    std::vector<uint8_t> in_ball(idx.size(), 1);
                    if (sparse)
                        for (auto &b : in_ball) b = rng() % 3 == 0;
                    if (run_stream(idx, in_ball, S, (int)cases, &taken, &rejected)) return 1;
                    ++cases;
                }
    if (taken == 0 || rejected == 0) return fail("vacuous", (int)taken, (int)rejected, 0);
    std::printf("ok %ld taken %ld rejected %ld\n", cases, taken, rejected);
    return 0;
}
