// roiaware_voxel.cpp -- csrc/sg_roiaware.h on the host (hipcc --cuda-host-only -x hip, as box_cells.cpp is compiled): the sub-voxel of a
// member.  tests/test_roiaware_reference.py writes triples, runs this and holds the answers equal to the NumPy rule -- once more under the
// address and undefined-behaviour sanitizers.
//   roiaware_voxel <n> <values.f64 n x 6: lx, ly, sz, dx', dy', dz'> <grids.i32 n x 3: Gx, Gy, Gz> <out.i32 n>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_roiaware.h"

template <typename T> static std::vector<T> slurp(const char *path, size_t count)
{
    std::vector<T> v(count);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(T), count, f) != count) { std::fprintf(stderr, "cannot read %zu elements of %s\n", count, path); std::exit(2); }
    std::fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: roiaware_voxel n values grids out\n"); return 2; }
    const size_t n = (size_t)std::atol(argv[1]);
    const std::vector<double> v = slurp<double>(argv[2], n * 6);
    const std::vector<int32_t> g = slurp<int32_t>(argv[3], n * 3);
    std::vector<int32_t> out(n);
    for (size_t i = 0; i < n; ++i)
        out[i] = sg_roiaware_voxel(v[i * 6], v[i * 6 + 1], v[i * 6 + 2], v[i * 6 + 3], v[i * 6 + 4], v[i * 6 + 5], g[i * 3], g[i * 3 + 1], g[i * 3 + 2]);
    FILE *f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(out.data(), sizeof(int32_t), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
    std::fclose(f);
    std::printf("voxel %zu\n", n);
    return 0;
}
