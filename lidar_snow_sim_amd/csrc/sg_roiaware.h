// sg_roiaware.h -- RoI-aware voxel pooling (snowgpu_roi_voxel_pool_device; the DEFINITION: include/snowgpu.h): the sub-voxel of a member
// and the sizes of the scratch.  Everything before it -- the enlarged roi, presence, the record, the membership test, the runs in which a
// roi's members are counted and ranked in row order -- is sg_roipool.h and sg_box.h as they stand.  snowgpu_roiaware.hip runs
// sg_roiaware_voxel on the device, tests/host_harness/roiaware_voxel.cpp the same code on the host, and tests/roiaware_reference.py restates
// it in NumPy.
//
// The sub-voxel.  A roi is cut into G = (Gx, Gy, Gz) voxels along its own axes.  A member has the local coordinates (lx, ly, sz) that
// sg_box_inside gave the membership test; with the ENLARGED sizes (dx', dy', dz') themselves -- not the record's half extents, whose x and
// y carry the 1e-5 margin --
//     ux = (lx + dx' / 2) / (dx' / Gx),   ix = min(max((int)floor(ux), 0), Gx - 1),       y likewise, z from sz, dz' and Gz;
// float64, every operation rounded on its own.  The clamp is pcdet's: a member inside the margin beyond an x / y face lands in the edge
// voxel, a member on the closed upper z face in Gz - 1.  The clamp is made on the double, before the conversion, and a NaN quotient (0 / 0,
// which takes a dx' / Gx that underflows to 0) counts as below 0: the index is defined for every record.  The flat voxel is
// g = (ix Gy + iy) Gz + iz, pcdet's (out_x, out_y, out_z) layout.
//
// The scratch, beside that of the pooling stage (rec, table, run_cnt for n_rois): list and sorted, n_frames M P int32 each, P =
// roi_capacity -- a roi's first P members in row order, and the same rows grouped by voxel, row order kept within a voxel --; offset,
// n_frames M G int32: where a voxel's rows begin in its roi's part of `sorted`.  At F = 16, M = 128, P = 8192 list and sorted are 67 MB each.
#pragma once
#include "sg_roipool.h"

#define SG_ROIAWARE_GRID_MAX 16         /* voxels per axis: 1 <= Gx, Gy, Gz <= 16 */
#define SG_ROIAWARE_POINTS_MAX 128      /* 1 <= T <= 128: the members of a voxel that are pooled */
#define SG_ROIAWARE_CHANNELS_MAX 256    /* 1 <= Cf <= 256 */
#define SG_ROIAWARE_CAP_MIN 64          /* 64 <= P <= 65536: the members of a roi that are distributed to voxels */
#define SG_ROIAWARE_CAP_MAX 65536

static inline size_t sg_roiaware_list(int n_frames, int32_t M, int32_t P) { return (size_t)n_frames * (size_t)M * (size_t)P; }
static inline size_t sg_roiaware_offsets(int n_frames, int32_t M, int32_t G) { return (size_t)n_frames * (size_t)M * (size_t)G; }

// the voxel index along one axis: l the local coordinate, d the enlarged size, n the voxels of the axis
__host__ __device__ inline int32_t sg_roiaware_axis(double l, double d, int32_t n)
{
    const double u = floor((l + d * 0.5) / (d / (double)n));
    if (!(u >= 0.0)) return 0;                                             // (also NaN)
    return u >= (double)n ? n - 1 : (int32_t)u;
}

// the flat voxel of a member with local coordinates (lx, ly, sz) in a roi of enlarged sizes (dx, dy, dz) cut into gx gy gz voxels
__host__ __device__ inline int32_t sg_roiaware_voxel(double lx, double ly, double sz, double dx, double dy, double dz, int32_t gx, int32_t gy, int32_t gz)
{
    return (sg_roiaware_axis(lx, dx, gx) * gy + sg_roiaware_axis(ly, dy, gy)) * gz + sg_roiaware_axis(sz, dz, gz);
}

// the enlarged sizes of the roi b[0 .. 6]: sg_roi_make's own adds
template <typename T> __host__ __device__ inline void sg_roiaware_sizes(const T *b, double ewx, double ewy, double ewz, double *dx, double *dy, double *dz)
{
    *dx = (double)b[3] + ewx; *dy = (double)b[4] + ewy; *dz = (double)b[5] + ewz;
}
