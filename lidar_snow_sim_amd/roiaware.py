"""RoI-aware voxel pooling for host arrays, in the call shape of pcdet's roiaware_pool3d_utils.RoIAwarePool3d for one frame: rois, points
and their features in, the pooled features (M, out_x, out_y, out_z, C) out.

The arrays are uploaded, pooled by the HIP kernels (include/snowgpu.h, snowgpu_roi_voxel_pool_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.roi_voxel_pool, which
stays on the device and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from .boxes import box_pose


def roiaware_pool3d(rois, pts, pts_feature, out_size, max_pts_each_voxel=128, pool_method='max', device=None):
    """(M, out_x, out_y, out_z, C) float32: `pts_feature` (N x C, 1 <= C <= 256, computed in float32) of the points `pts` (N x 3: x, y, z;
    float32 stays float32, everything else is computed in float64) pooled over the sub-voxels of `rois` (M x 7 .. 10, 1 <= M <= 512: cx,
    cy, cz, dx, dy, dz, heading first), `out_size` a whole number or three.  As pcdet's op a voxel pools its first max_pts_each_voxel - 1
    points in input order -- the op keeps their number in the slot that is missing; pool_method is 'max' or 'avg'.  All of a roi's first
    65536 points are distributed to its voxels.  The pose is NumPy's cos / sin of the heading in float64, given to the device as it is:
    the result is that of the definition under NumPy's own trigonometry, byte for byte."""
    import torch
    from .tensors import roi_voxel_pool as on_device
    rois, pts, feats = np.asarray(rois), np.asarray(pts), np.asarray(pts_feature)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("pts must be N x 3 (x, y, z)")
    if feats.ndim != 2 or feats.shape[0] != pts.shape[0] or not 1 <= feats.shape[1] <= 256:
        raise ValueError("pts_feature must be N x C with 1 <= C <= 256, one row per point")
    if rois.ndim != 2 or not 7 <= rois.shape[1] <= 10 or not 1 <= rois.shape[0] <= 512:
        raise ValueError("rois must be M x 7 .. 10 with 1 <= M <= 512 (cx, cy, cz, dx, dy, dz, heading, ...)")
    if pool_method not in ('max', 'avg'):
        raise ValueError("pool_method must be 'max' or 'avg'")
    if int(max_pts_each_voxel) != max_pts_each_voxel or not 2 <= int(max_pts_each_voxel) <= 129:
        raise ValueError("max_pts_each_voxel must be a whole number in 2 .. 129: one slot holds the count")
    if not torch.cuda.is_available():
        raise RuntimeError("roiaware_pool3d runs on the GPU: no device is visible (there is no CPU fallback)")
    dt = np.float32 if pts.dtype == np.float32 else np.float64
    rows = np.zeros((pts.shape[0], 5), dt)
    rows[:, :3] = pts[:, :3]
    b = np.array(rois[None], dt, order="C")
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    got = on_device(torch.from_numpy(rows).to(dev), torch.from_numpy(b).to(dev), out_size, int(max_pts_each_voxel) - 1,
                    torch.from_numpy(np.array(feats, np.float32, order="C")).to(dev), roi_capacity=65536,
                    pose=torch.from_numpy(np.ascontiguousarray(box_pose(b))).to(dev), pool=(pool_method,))
    return got.as_grid(got.max if pool_method == 'max' else got.avg)[0].cpu().numpy()
