// The cell arithmetic and the table of open cells of the voxel stage (csrc/sg_voxel.h) compiled for the host; the grid's dimensions
// come from the argument check (csrc/sg_device_args.h), as in the entry.
//   voxel_cells cells <x0> <y0> <z0> <x1> <y1> <z1> <sx> <sy> <sz> <in: n x 3 float64> <out: n int32>
//       the key of every row (sg_voxel_key), -1 for a row that is not usable.  Prints "dims n_x n_y n_z".
//   voxel_cells table <x0> ... <sz> <in> <out> <seed>
//       every usable row into ONE frame's table (sg_voxel_insert) in an order scrambled by <seed>, then per row the low word of its
//       cell's slot: the smallest row of the cell (-1 for a row that is not usable).  Prints "cap <slots> used <slots in use>".
// Leaves with status 3 for a grid outside the domain.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sg_device_args.h"
#include "sg_voxel.h"

int main(int argc, char **argv)
{
    if (argc < 13) return 2;
    double range6[6], size3[3];
    for (int k = 0; k < 6; ++k) range6[k] = atof(argv[2 + k]);
    for (int k = 0; k < 3; ++k) size3[k] = atof(argv[8 + k]);
    SgVoxelGrid g{};
    if (sg_voxel_dims(range6, size3, g.n)) { fprintf(stderr, "outside the domain\n"); return 3; }
    for (int j = 0; j < 3; ++j) { g.lo[j] = range6[j]; g.size[j] = size3[j]; }
    FILE *fi = fopen(argv[11], "rb");
    if (!fi) return 4;
    std::vector<double> p;
    double t[3];
    while (fread(t, sizeof(double), 3, fi) == 3) p.insert(p.end(), t, t + 3);
    fclose(fi);
    const size_t n = p.size() / 3;
    std::vector<uint32_t> key(n);
    for (size_t i = 0; i < n; ++i) key[i] = sg_voxel_key(g, p[3 * i], p[3 * i + 1], p[3 * i + 2]);
    std::vector<int32_t> out(n, -1);
    if (!strcmp(argv[1], "cells")) {
        printf("dims %d %d %d\n", g.n[0], g.n[1], g.n[2]);
        for (size_t i = 0; i < n; ++i) out[i] = (int32_t)key[i];
    } else if (!strcmp(argv[1], "table") && argc >= 14) {
        g.cap = sg_voxel_capacity((int64_t)n);
        g.shift = sg_voxel_shift(g.cap);
        std::vector<unsigned long long> table(g.cap, SG_VOXEL_EMPTY);
        std::vector<uint32_t> order(n), slot(n, SG_VOXEL_NONE);
        for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
        std::mt19937_64 rng((uint64_t)atoll(argv[13]));
        std::shuffle(order.begin(), order.end(), rng);
        for (uint32_t i : order)
            if (key[i] != SG_VOXEL_NONE) {
                slot[i] = sg_voxel_insert(table.data(), g.cap, g.shift, key[i], i);
                if (slot[i] == SG_VOXEL_NONE || slot[i] >= g.cap) return 6;
            }
        size_t used = 0;
        for (unsigned long long w : table) used += w != SG_VOXEL_EMPTY;
        for (size_t i = 0; i < n; ++i)
            if (slot[i] != SG_VOXEL_NONE) {
                if ((uint32_t)(table[slot[i]] >> 32) != key[i]) return 7;
                out[i] = (int32_t)(uint32_t)table[slot[i]];
            }
        printf("cap %u used %zu\n", g.cap, used);
    } else
        return 2;
    FILE *fo = fopen(argv[12], "wb");
    if (!fo) return 5;
    fwrite(out.data(), sizeof(int32_t), n, fo);
    fclose(fo);
    return 0;
}
