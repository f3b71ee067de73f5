// range_pixels.cpp -- csrc/sg_range.h on the host: the usable test, the range, the column, the image row and the key that
// snowgpu_range.hip runs on the device, walked over a batch from files in the kernels' sequence (project, the float64 tie pass, the
// decoding of the finish).  hipcc --cuda-host-only -x hip -I lidar_snow_sim_amd/csrc; tests/test_range_reference.py compares what it writes
// with the NumPy restatement, and runs it once more as a stand-alone program under the address and undefined-behaviour sanitizers.
//   range_pixels walk <dtype 0|1> <by_ring 0|1> <H> <W> <fov_up> <fov_down> <lo> <hi> <n_frames> <offsets.i64> <rows.f64 N x 3> <keep.u8> <ring.i32> <out.i32>
// The rows come as float64 (exact for float32 values) and are rounded back to the rows' dtype.  Writes pixel_of (N), index (F H W) and
// count (F H W) as int32, in this order.
//   range_pixels guard <points per setting>
// The guarded angles against the definition: for every W in {1, 96, 2048} and H in {1, 64}, points within a few ulps of column edges, of
// image-row edges, on the seam and the axis, and uniform ones; sg_range_col / sg_range_row must give what their sg_atan2_cr forms give.
// Prints "guard <settings> <points> <different> <share of angles decided by sg_atan2_cr>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sg_range.h"

template <typename V> static bool read_file(const char *path, std::vector<V> &v, size_t n)
{
    v.resize(n);
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = n ? std::fread(v.data(), sizeof(V), n, f) : 0;
    std::fclose(f);
    return got == n;
}

template <typename T>
static int walk(const SgRangeGeom &g, int n_frames, const std::vector<int64_t> &off, const std::vector<double> &xyz, const std::vector<uint8_t> &keep,
                const std::vector<int32_t> &ring, const char *out_path)
{
    const int64_t n = off[n_frames], pixels = (int64_t)n_frames * g.H * g.W;
    std::vector<unsigned long long> key((size_t)pixels, SG_RANGE_EMPTY);
    std::vector<int32_t> pixel_of((size_t)n, -1), index((size_t)pixels, -1), count((size_t)pixels, 0);
    std::vector<uint32_t> tie((size_t)pixels, 0xffffffffu);
    // k_range_project
    for (int64_t i = 0; i < n; ++i) {
        if (!keep[i]) continue;
        int f = 0;
        while (off[f + 1] <= i) ++f;
        T r;
        const int32_t q = sg_range_pixel<T>(g, (T)xyz[3 * i], (T)xyz[3 * i + 1], (T)xyz[3 * i + 2], g.by_ring ? ring[i] : 0, &r);
        if (q < 0) continue;
        if (q >= g.H * g.W) return 3;                          // a pixel outside the image: never
        const int32_t p = f * (g.H * g.W) + q;
        pixel_of[i] = p;
        sg_range_lower(&key[p], sg_range_key(r, (uint32_t)i));
        ++count[p];
    }
    // k_range_tie (float64 rows)
    if (sizeof(T) == 8)
        for (int64_t i = 0; i < n; ++i) {
            const int32_t p = pixel_of[i];
            if (p < 0) continue;
            if (sg_range_bits(sg_range_r<double>(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) == key[p]) sg_range_lower(&tie[p], (uint32_t)i);
        }
    // k_range_finish: the winner
    for (int64_t p = 0; p < pixels; ++p) {
        if (key[p] == SG_RANGE_EMPTY) continue;
        index[p] = sizeof(T) == 8 ? (int32_t)tie[p] : (int32_t)(uint32_t)key[p];
    }
    FILE *f = std::fopen(out_path, "wb");
    if (!f) return 4;
    if (n) std::fwrite(pixel_of.data(), 4, (size_t)n, f);
    std::fwrite(index.data(), 4, (size_t)pixels, f);
    std::fwrite(count.data(), 4, (size_t)pixels, f);
    std::fclose(f);
    std::printf("walk %lld %lld\n", (long long)n, (long long)pixels);
    return 0;
}

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64()                                     // splitmix64
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double uniform(double a, double b) { return a + (b - a) * ((double)(next_u64() >> 11) * 0x1p-53); }
static double ulps_away(double v, int k)
{
    for (; k > 0; --k) v = nextafter(v, INFINITY);
    for (; k < 0; ++k) v = nextafter(v, -INFINITY);
    return v;
}

static int guard(long long per_setting)
{
    const int Ws[3] = {1, 96, 2048}, Hs[2] = {1, 64};
    long long points = 0, different = 0, angles = 0, slow = 0;
    int settings = 0;
    for (int W : Ws)
        for (int H : Hs) {
            ++settings;
            SgRangeGeom fast{};
            fast.H = H; fast.W = W; fast.fov_up = 3.0 * (SG_RANGE_PI / 180.0); fast.fov_down = -25.0 * (SG_RANGE_PI / 180.0);
            const double D = fast.fov_up - fast.fov_down;
            for (long long i = 0; i < per_setting; ++i) {
                double x, y, z;
                const int kind = (int)(next_u64() % 8), k = (int)(next_u64() % 9) - 4;
                const double rho = uniform(0.5, 120.0);
                if (kind < 3) {                                // a column edge, y a few ulps beside it
                    const double th = SG_RANGE_PI * (1.0 - 2.0 * (double)(next_u64() % (uint64_t)(W + 1)) / W);
                    x = rho * cos(th); y = ulps_away(rho * sin(th), k); z = uniform(-3.0, 1.0);
                } else if (kind < 6) {                         // an image-row edge, z a few ulps beside it
                    const double pitch = fast.fov_up - D * (double)(next_u64() % (uint64_t)(H + 1)) / H, az = uniform(-SG_RANGE_PI, SG_RANGE_PI);
                    x = rho * cos(az); y = rho * sin(az); z = ulps_away(sqrt(x * x + y * y) * tan(pitch), k);
                } else if (kind == 6) {                        // the seam, the axes and the quadrant lines
                    const double v[4] = {0.0, -0.0, rho, -rho};
                    x = v[next_u64() % 4]; y = v[next_u64() % 4]; z = v[next_u64() % 4] * 0.01;
                } else {
                    x = uniform(-120.0, 120.0); y = uniform(-120.0, 120.0); z = uniform(-30.0, 10.0);
                }
                ++points;
                if (sg_range_col(fast, x, y) != sg_range_clip(sg_range_px_exact(x, y, W), W) || sg_range_row(fast, x, y, z) != sg_range_clip(sg_range_py_exact(fast, x, y, z), H)) {
                    if (++different <= 5) std::fprintf(stderr, "W %d H %d: %a %a %a\n", W, H, x, y, z);
                }
                angles += 2;
                slow += !sg_range_decided(sg_range_px_at(-atan2(y, x), W), SG_RANGE_BAND_X * (double)W);
                const double pitch = atan2(z, sqrt(x * x + y * y));
                slow += !sg_range_decided(sg_range_py_at(fast, pitch), SG_RANGE_BAND_Y * (double)H * ((1.0 / D + fabs((pitch - fast.fov_down) / D)) + 1.0));
            }
        }
    std::printf("guard %d %lld %lld %.6f\n", settings, points, different, (double)slow / (double)angles);
    return different ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "guard") return guard(std::atoll(argv[2]));
    if (argc != 16 || std::string(argv[1]) != "walk") {
        std::fprintf(stderr, "usage: range_pixels walk dtype by_ring H W fov_up fov_down lo hi n_frames offsets rows keep ring out\n");
        return 2;
    }
    const int dtype = std::atoi(argv[2]);
    SgRangeGeom g{};
    g.by_ring = std::atoi(argv[3]);
    g.H = std::atoi(argv[4]);
    g.W = std::atoi(argv[5]);
    g.fov_up = std::strtod(argv[6], nullptr);
    g.fov_down = std::strtod(argv[7], nullptr);
    const double limits[2] = {std::strtod(argv[8], nullptr), std::strtod(argv[9], nullptr)};
    sg_range_limits(dtype, limits, &g.lo, &g.hi);
    const int n_frames = std::atoi(argv[10]);
    std::vector<int64_t> off;
    if (n_frames < 1 || !read_file(argv[11], off, (size_t)n_frames + 1)) return 2;
    const size_t n = (size_t)off[n_frames];
    std::vector<double> xyz;
    std::vector<uint8_t> keep;
    std::vector<int32_t> ring;
    if (!read_file(argv[12], xyz, 3 * n) || !read_file(argv[13], keep, n) || !read_file(argv[14], ring, n)) return 2;
    return dtype == 0 ? walk<float>(g, n_frames, off, xyz, keep, ring, argv[15]) : walk<double>(g, n_frames, off, xyz, keep, ring, argv[15]);
}
