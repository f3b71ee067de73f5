// sg_voxel.h -- point-to-voxel grouping (snowgpu_voxelize_device): the cell of a row and the per-frame table of open cells.
// snowgpu_voxel.hip runs these functions on the device, tests/host_harness/voxel_cells.cpp the same code on the host (as sg_dror.h is
// compiled for both), and tests/voxel_reference.py restates the DEFINITION of include/snowgpu.h as a sequential NumPy walk.
//
// The cell.  c_j = floor(((double)p_j - lo_j) / size_j) for j = x, y, z: a subtraction, a true division and a floor in double, each
// rounded on its own -- no reciprocal, no fused multiply-add.  The row is usable iff every p_j is finite and 0 <= c_j < n_j; its KEY is
// (c_z n_y + c_y) n_x + c_x, below 2^31 - 2 by the entry's domain.  n_j = llround((hi_j - lo_j) / size_j) is made by the argument check
// (sg_device_args.h: sg_voxel_dims).
//
// The table.  One open-addressed table per frame, `cap` slots (a power of two, at least twice the rows of the longest frame, so at most
// half full), linear probing from a multiplicative hash of the key.  A slot is ONE 64-bit word, key << 32 | row: the first insert of a key
// claims an empty slot by compare-and-swap, every other insert of it lowers the word by an atomic min -- the key bits are equal, so the
// min is the min of the row indices.  When every row has been inserted each slot holds the SMALLEST row index of its cell: the row that
// opens the voxel in the definition's walk.  Where the hash put a cell, and in which order the atomics arrived, decides nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SG_VOXEL_NONE 0xffffffffu                 /* no cell / no slot / no voxel (as int32: -1) */
#define SG_VOXEL_EMPTY 0xffffffffffffffffull      /* an empty slot: what the memset in front of the inserts leaves */
#define SG_VOXEL_MIN_CAP 64u
#define SG_VOXEL_MAX_FRAME ((int64_t)1 << 30)     /* rows of the longest frame: the table's capacity stays below 2^32 */

struct SgVoxelGrid {
    double lo[3], size[3];         // x, y, z
    int32_t n[3];                  // cells per axis
    int32_t max_points, max_voxels, n_features;      // T, V, C
    uint32_t cap;                  // slots per frame
    int32_t shift;                 // 32 - log2(cap)
};

// slots per frame for a batch whose longest frame has max_frame rows (at most SG_VOXEL_MAX_FRAME)
static inline uint32_t sg_voxel_capacity(int64_t max_frame)
{
    uint64_t cap = SG_VOXEL_MIN_CAP;
    while (cap < 2 * (uint64_t)max_frame) cap <<= 1;
    return (uint32_t)cap;
}

static inline int32_t sg_voxel_shift(uint32_t cap)
{
    int32_t log2cap = 0;
    while (((uint32_t)1 << log2cap) < cap) ++log2cap;
    return 32 - log2cap;
}

// c = the cell of coordinate p on one axis; false: not finite, or outside [0, n)
__host__ __device__ inline bool sg_voxel_axis(double p, double lo, double size, int32_t n, int32_t *c)
{
    if (!(fabs(p) <= 1.7976931348623157e308)) return false;      // (false for NaN)
    const double t = floor((p - lo) / size);
    if (!(t >= 0.0 && t < (double)n)) return false;
    *c = (int32_t)t;
    return true;
}

// the key of a row, or SG_VOXEL_NONE for a row that is not usable
__host__ __device__ inline uint32_t sg_voxel_key(const SgVoxelGrid &g, double x, double y, double z)
{
    int32_t cx, cy, cz;
    if (!sg_voxel_axis(x, g.lo[0], g.size[0], g.n[0], &cx) || !sg_voxel_axis(y, g.lo[1], g.size[1], g.n[1], &cy) ||
        !sg_voxel_axis(z, g.lo[2], g.size[2], g.n[2], &cz))
        return SG_VOXEL_NONE;
    return ((uint32_t)cz * (uint32_t)g.n[1] + (uint32_t)cy) * (uint32_t)g.n[0] + (uint32_t)cx;
}

__host__ __device__ inline void sg_voxel_unkey(const SgVoxelGrid &g, uint32_t key, int32_t *cx, int32_t *cy, int32_t *cz)
{
    const uint32_t nx = (uint32_t)g.n[0], ny = (uint32_t)g.n[1], zy = key / nx;
    *cx = (int32_t)(key - zy * nx);
    *cz = (int32_t)(zy / ny);
    *cy = (int32_t)(zy - (uint32_t)*cz * ny);
}

__host__ __device__ inline uint32_t sg_voxel_hash(uint32_t key, int32_t shift) { return (key * 2654435761u) >> shift; }

// `word` into *p if *p is empty; returns what *p held
__host__ __device__ inline unsigned long long sg_voxel_claim(unsigned long long *p, unsigned long long word)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, SG_VOXEL_EMPTY, word);
#else
    const unsigned long long old = *p;
    if (old == SG_VOXEL_EMPTY) *p = word;
    return old;
#endif
}

__host__ __device__ inline void sg_voxel_lower(unsigned long long *p, unsigned long long word)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, word);
#else
    if (word < *p) *p = word;
#endif
}

// Row `row` of cell `key` into the frame's table: the slot of the cell.  SG_VOXEL_NONE if `cap` slots were probed without finding the key or
// room for it -- which a table of the promised size never answers (the walk is bounded so that a caller who understated max_frame_rows
// gets rows without a voxel, not a kernel that never ends).
__host__ __device__ inline uint32_t sg_voxel_insert(unsigned long long *table, uint32_t cap, int32_t shift, uint32_t key, uint32_t row)
{
    const unsigned long long word = ((unsigned long long)key << 32) | row;
    uint32_t s = sg_voxel_hash(key, shift);
    for (uint32_t probes = 0; probes < cap; ++probes) {
        const unsigned long long old = sg_voxel_claim(&table[s], word);
        if (old == SG_VOXEL_EMPTY) return s;
        if ((uint32_t)(old >> 32) == key) {
            if ((uint32_t)old > row) sg_voxel_lower(&table[s], word);
            return s;
        }
        s = (s + 1) & (cap - 1);
    }
    return SG_VOXEL_NONE;
}
