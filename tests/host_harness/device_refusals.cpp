// device_refusals.cpp -- every shape of a *_batch_device* entry through every refusal of sg_device_args.h, one defect at a time, and
// through clean calls at the edges.  Plain C++ (g++ -std=c++17 -I lidar_snow_sim_amd/csrc), no device: prints entry|case|code|message,
// then the derived values.  tests/test_device_refusals.py compares the lines with a table.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "sg_device_args.h"

struct Entry {
    const char *key, *who;
    SgEntryShape shape;
    bool takes_keep_in;      // the entry has a d_keep_in of its own to hand to the overlap check
};

static const Entry ENTRIES[] = {
    {"compact", "snowgpu_augment_batch_device", SG_SHAPE_COMPACT, false},
    {"compact_wet", "snowgpu_augment_wet_batch_device", SG_SHAPE_COMPACT_WET, false},
    {"aligned", "snowgpu_augment_batch_device_aligned", SG_SHAPE_ALIGNED, false},
    {"wet_only", "snowgpu_wet_ground_batch_device_aligned", SG_SHAPE_WET_ONLY, true},
    {"aligned_wet", "snowgpu_augment_wet_batch_device_aligned", SG_SHAPE_ALIGNED_WET, false},
    {"masked", "snowgpu_augment_batch_device_aligned_masked", SG_SHAPE_MASKED, true},
    {"masked_wet", "snowgpu_augment_wet_batch_device_aligned_masked", SG_SHAPE_MASKED_WET, true},
    {"weather", "snowgpu_augment_weather_batch_device_aligned", SG_SHAPE_WEATHER, true},
};

// host arrays of the sizes the arguments stand for: 8 rows of 5 float64 (float32 rows use the first half) and room for an adjacent output
static double g_rows[2 * 8 * 5], g_out_rows[8 * 5], g_plane[8], g_weather[16], g_thr[6];
static uint8_t g_keep[2 * 8], g_out_keep[8];
static int64_t g_off[3] = {0, 4, 8}, g_counts[2], g_stats[6];
static int32_t g_tids[128], g_src[8], g_flags[2], g_status[8], g_perm[8];

struct Call {
    SgDeviceArgs a;
    SgCtxView c;
};

// what the entry itself passes on a call that is in order: two frames of four float32 rows, every buffer apart from every other
static Call clean_call(const Entry &e)
{
    Call k{};
    SgDeviceArgs &a = k.a;
    a.who = e.who; a.n_frames = 2; a.n_total = 8; a.max_frame_rows = 4; a.dtype = 0;
    a.frame_off = g_off; a.rows = g_rows; a.out_rows = g_out_rows; a.out_counts = g_counts; a.status = g_status;
    if (e.shape.tables) { a.table_ids = g_tids; a.out_stats = g_stats; a.out_thr_poly = g_thr; }
    if (e.shape.aligned) a.out_keep = g_out_keep; else a.out_src = g_src;
    if (e.takes_keep_in) a.keep_in = g_keep;
    if (e.shape.wet) a.out_flags = g_flags;
    if (e.shape.weather) a.weather = g_weather;
    k.c = SgCtxView{false, 0, 0, 4};
    return k;
}

static void report(const Entry &e, const char *name, const Call &k)
{
    std::string msg;
    const int rc = sg_check_device_args(k.a, k.c, e.shape, &msg);
    std::printf("%s|%s|%d|%s\n", e.key, name, rc, rc ? msg.c_str() : "OK");
}

int main()
{
    using Edit = std::function<void(Call &)>;
    const int64_t two31 = (int64_t)1 << 31;
    auto in_place = [](Call &k) { k.a.out_rows = (void *)k.a.rows; if (k.a.keep_in) k.a.out_keep = (uint8_t *)k.a.keep_in; };
    const std::vector<std::pair<const char *, Edit>> cases = {
        {"clean", [](Call &) {}},
        {"null_frame_offsets", [](Call &k) { k.a.frame_off = nullptr; }},
        {"null_rows", [](Call &k) { k.a.rows = nullptr; }},
        {"null_table_ids", [](Call &k) { k.a.table_ids = nullptr; }},
        {"null_out_rows", [](Call &k) { k.a.out_rows = nullptr; }},
        {"null_out_src_or_keep", [](Call &k) { k.a.out_src = nullptr; k.a.out_keep = nullptr; }},
        {"null_out_counts", [](Call &k) { k.a.out_counts = nullptr; }},
        {"null_out_stats", [](Call &k) { k.a.out_stats = nullptr; }},
        {"null_out_flags", [](Call &k) { k.a.out_flags = nullptr; }},
        {"null_out_thr_poly", [](Call &k) { k.a.out_thr_poly = nullptr; }},
        {"null_status", [](Call &k) { k.a.status = nullptr; }},
        {"null_weather", [](Call &k) { k.a.weather = nullptr; }},
        {"null_keep_in", [](Call &k) { k.a.keep_in = nullptr; }},
        {"bad_dtype", [](Call &k) { k.a.dtype = 2; }},
        {"no_frames", [](Call &k) { k.a.n_frames = 0; }},
        {"negative_rows", [](Call &k) { k.a.n_total = -1; }},
        {"empty_null_rows", [](Call &k) { k.a.n_total = 0; k.a.rows = nullptr; }},
        {"empty_null_buffers", [](Call &k) { k.a.n_total = 0; k.a.rows = nullptr; k.a.out_rows = nullptr; k.a.out_src = nullptr; k.a.out_keep = nullptr; }},
        {"empty_tables_65537", [](Call &k) { k.a.n_total = 0; k.c.n_tables = 65537; }},
        {"rows_2p31_minus_1", [&](Call &k) { in_place(k); k.a.n_total = two31 - 1; }},
        {"rows_2p31", [&](Call &k) { in_place(k); k.a.n_total = two31; }},
        {"threshold_callback", [](Call &k) { k.c.thr_fn = true; }},
        {"packed_transfer", [](Call &k) { k.c.result_mode = 1; }},
        {"out_rows_overlap_f32", [](Call &k) { k.a.out_rows = (char *)g_rows + 5 * 4; }},
        {"out_rows_in_place_f32", [](Call &k) { k.a.out_rows = g_rows; }},
        {"out_rows_adjacent_f32", [](Call &k) { k.a.out_rows = (char *)g_rows + 8 * 5 * 4; }},
        {"out_rows_overlap_f64", [](Call &k) { k.a.dtype = 1; k.a.out_rows = (char *)g_rows + 5 * 8; }},
        {"out_rows_in_place_f64", [](Call &k) { k.a.dtype = 1; k.a.out_rows = g_rows; }},
        {"out_rows_adjacent_f64", [](Call &k) { k.a.dtype = 1; k.a.out_rows = (char *)g_rows + 8 * 5 * 8; }},
        {"out_keep_overlap", [](Call &k) { if (k.a.keep_in) k.a.out_keep = g_keep + 3; }},
        {"out_keep_in_place", [](Call &k) { if (k.a.keep_in) k.a.out_keep = g_keep; }},
        {"out_keep_adjacent", [](Call &k) { if (k.a.keep_in) k.a.out_keep = g_keep + 8; }},
        {"null_wet_plane_lsq", [](Call &k) { k.c.plane_method = 1; }},
        {"null_wet_plane_ransac", [](Call &k) { k.c.plane_method = 2; }},
        {"wet_plane_lsq", [](Call &k) { k.c.plane_method = 1; k.a.wet_plane = g_plane; }},
        {"perm", [](Call &k) { k.a.perm = g_perm; }},
        {"tables_65536", [](Call &k) { k.c.n_tables = 65536; }},
        {"tables_65537", [](Call &k) { k.c.n_tables = 65537; }},
        {"frames_2p22", [](Call &k) { k.a.n_frames = 1 << 22; }},
        {"frames_2p22_plus_1", [](Call &k) { k.a.n_frames = (1 << 22) + 1; }},
    };
    for (const Entry &e : ENTRIES)
        for (const auto &cs : cases) {
            // the two _masked entries hand a batch without a mask or without rows to the unmasked entry before any check: no such call reaches their shape
            if (e.shape.masked && !e.shape.weather && (!std::strncmp(cs.first, "empty_", 6) || !std::strcmp(cs.first, "null_keep_in"))) continue;
            Call k = clean_call(e);
            cs.second(k);
            report(e, cs.first, k);
        }
    // the wet stage asks for the plane again where it needs it: the first time for the wet model on its own
    for (int method = 0; method < 3; ++method)
        for (const double *plane : {(const double *)nullptr, (const double *)g_plane}) {
            std::string msg;
            const int rc = sg_check_wet_plane(ENTRIES[3].who, plane, method, &msg);
            std::printf("wet_only_stage|%s_method_%d|%d|%s\n", plane ? "plane" : "null_plane", method, rc, rc ? msg.c_str() : "OK");
        }
    for (int64_t mfr : {(int64_t)0, (int64_t)3, (int64_t)8, (int64_t)9, (int64_t)-1})
        std::printf("max_frame|%lld|%lld|%lld\n", (long long)mfr, 8LL, (long long)sg_max_frame(mfr, 8));
    std::printf("max_frame|%lld|%lld|%lld\n", 0LL, 0LL, (long long)sg_max_frame(0, 0));
    for (int64_t mfr : {(int64_t)0, (int64_t)4, (int64_t)3, (int64_t)5, (int64_t)8})
        for (int nf : {2, 1})
            std::printf("uniform_rows|%lld|%d|%lld|%lld\n", (long long)mfr, nf, 8LL, (long long)sg_uniform_rows(mfr, nf, 8));
    std::printf("uniform_rows|%lld|%d|%lld|%lld\n", 4LL, 2, 9LL, (long long)sg_uniform_rows(4, 2, 9));
    std::printf("uniform_rows|%lld|%d|%lld|%lld\n", 4LL, 2, 7LL, (long long)sg_uniform_rows(4, 2, 7));
    std::printf("uniform_rows|%lld|%d|%lld|%lld\n", 3LL, 2, 0LL, (long long)sg_uniform_rows(3, 2, 0));
    return 0;
}
