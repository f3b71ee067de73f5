// sg_roipool.h -- RoI point pooling (snowgpu_roi_point_pool_device; the DEFINITION: include/snowgpu.h): the enlarged roi, the runs of rows
// in which members are counted and ranked, and the sizes of the scratch.  Everything else -- presence, the record, the membership test,
// the grid and the footprint -- is sg_box.h as it stands: a roi is a box whose sizes have grown by the extra width, and there is ONE
// membership function, sg_box_inside.
//
// The enlarged roi.  dx' = (double)dx + ew[0], dy' and dz' likewise, each one float64 add (pcdet's enlarge_box3d: the width is added once
// to each size); centre and heading are kept.  sg_box_make judges presence on the enlarged sizes and builds the record from them, so
// hx = dx' / 2 + 1e-5, hy likewise, hz = dz' / 2.  Beside that rule a roi whose ORIGINAL dx, dy or dz is not > 0 is absent: with ew > 0
// the zero rows behind an NmsBatch's count would otherwise become boxes of the extra width.
//
// The footprint.  The bound of sg_box.h is derived for half extents of boxes with 0 < sizes <= 1e6; presence is judged on the ENLARGED
// sizes, so a present roi's record meets exactly that premise and sg_box_footprint holds as it is: no member row lies outside the marked
// cells.
//
// The runs.  The rows of frame f are cut into runs of SG_ROI_RUN consecutive rows, run r = rows [off[f] + r RUN, off[f] + (r + 1) RUN)
// within the frame: a run never crosses a frame boundary.  ONE WAVE owns a run and walks it in row order, 64 rows a step.  The scratch
// table holds one int32 per (frame, run, roi): first the members of the roi in the run, after the scan the members in all earlier runs of
// the frame.  Its rows are runs_per_frame = ceil(max_frame_rows / RUN) per frame, whatever the frame's own length (empty runs count 0).
#pragma once
#include "sg_box.h"

#define SG_ROI_MAX 512             /* rois per frame: 1 <= M <= 512 */
#define SG_ROI_SAMPLES_MAX 2048    /* 1 <= S <= 2048 */
#define SG_ROI_EW_MAX 100.0        /* every component of the extra width in 0 .. 100 m */
#define SG_ROI_RUN 512             /* rows of a run: eight steps of a wave */

// runs per frame for a longest frame of max_frame rows (at least one), and the elements of the (frames, runs, rois) table
static inline int64_t sg_roi_runs(int64_t max_frame) { const int64_t r = (max_frame + SG_ROI_RUN - 1) / SG_ROI_RUN; return r > 0 ? r : 1; }
static inline size_t sg_roi_table(int n_frames, int64_t max_frame, int32_t M) { return (size_t)n_frames * (size_t)sg_roi_runs(max_frame) * (size_t)M; }

// The record of the roi b[0 .. 6] enlarged by ew[0 .. 2], under the caller's pose or (NULL) cos / sin of the heading.  True: the roi is
// present.  An absent roi leaves a record of zeros.
template <typename T> __host__ __device__ inline bool sg_roi_make(const T *b, double ewx, double ewy, double ewz, const double *pose_in, SgBoxRec *r)
{
    const double dx = (double)b[3], dy = (double)b[4], dz = (double)b[5];
    const double e[7] = {(double)b[0], (double)b[1], (double)b[2], dx + ewx, dy + ewy, dz + ewz, (double)b[6]};
    const bool present = sg_box_make<double>(e, pose_in, r);
    if (present && dx > 0.0 && dy > 0.0 && dz > 0.0) return true;                      // (false for NaN)
    *r = SgBoxRec{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    return false;
}
