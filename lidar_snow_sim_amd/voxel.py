"""Point-to-voxel grouping for host arrays, in the call shape of the common CPU voxel generators (spconv's VoxelGenerator.generate,
mmdetection3d's points_to_voxel): one cloud in, (voxels, coordinates, num_points_per_voxel) out, voxels in the order their first points
appear.

The array is uploaded, grouped by the HIP kernels (include/snowgpu.h, snowgpu_voxelize_device: the definition and its edge conventions)
and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.voxelize, which stays on the device
and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np


def points_to_voxels(pc, point_cloud_range, voxel_size, max_points=5, max_voxels=40000, num_features=None, device=None):
    """(voxels M x max_points x C, coordinates M x 3 int32 as (z, y, x) cells, num_points_per_voxel M int32) of `pc` (N x K, K >= 3: x, y,
    z first; float32 stays float32, everything else is computed from float64).  C = num_features, by default min(K, 5) columns."""
    import torch
    from .tensors import voxelize
    pc = np.asarray(pc)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x K with K >= 3 (x, y, z, ...)")
    c = min(pc.shape[1], 5) if num_features is None else int(num_features)
    if not 3 <= c <= min(pc.shape[1], 5):
        raise ValueError("num_features must lie in 3 .. min(K, 5): the leading columns of pc that a voxel stores")
    if not torch.cuda.is_available():
        raise RuntimeError("points_to_voxels runs on the GPU: no device is visible (there is no CPU fallback)")
    k = min(pc.shape[1], 5)
    rows = np.zeros((pc.shape[0], 5), np.float32 if pc.dtype == np.float32 else np.float64)
    rows[:, :k] = pc[:, :k]
    index = torch.cuda.current_device() if device is None else int(device)
    t = torch.from_numpy(rows).to(torch.device("cuda", index))
    (voxels, coords, num), = voxelize(t, point_cloud_range, voxel_size, max_points, max_voxels, num_features=c).frames()
    return voxels.cpu().numpy(), np.ascontiguousarray(coords.cpu().numpy()[:, 1:]), num.cpu().numpy()
