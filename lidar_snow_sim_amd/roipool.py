"""RoI point pooling for host arrays, in the call shape of pcdet's roipoint_pool3d for one frame: a cloud and its rois in,
(pooled, empty_flag) out.

The arrays are uploaded, pooled by the HIP kernels (include/snowgpu.h, snowgpu_roi_point_pool_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.roi_point_pool, which
stays on the device and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from .boxes import box_pose


def roipoint_pool3d(pc, boxes, n_samples=512, extra_width=0.0, device=None):
    """(pooled M x S x C, empty_flag M int32) of `pc` (N x C', C' >= 3: x, y, z first; float32 stays float32, everything else is computed
    in float64; C = min(C', 5) columns are pooled) against `boxes` (M x 7 .. 10, 1 <= M <= 512: cx, cy, cz, dx, dy, dz, heading first),
    each enlarged once by `extra_width` (a number, or three for x, y, z): per roi its first n_samples member rows in row order, repeated
    from the start when it has fewer, zeros when it has none -- then empty_flag is 1.  The pose is NumPy's cos / sin of the heading in
    float64, given to the device as it is: the result is that of the definition under NumPy's own trigonometry, byte for byte."""
    import torch
    from .tensors import roi_point_pool as on_device
    pc, boxes = np.asarray(pc), np.asarray(boxes)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x M with M >= 3 (x, y, z, ...)")
    if boxes.ndim != 2 or not 7 <= boxes.shape[1] <= 10 or not 1 <= boxes.shape[0] <= 512:
        raise ValueError("boxes must be M x 7 .. 10 with 1 <= M <= 512 (cx, cy, cz, dx, dy, dz, heading, ...)")
    if not torch.cuda.is_available():
        raise RuntimeError("roipoint_pool3d runs on the GPU: no device is visible (there is no CPU fallback)")
    m = min(pc.shape[1], 5)
    dt = np.float32 if pc.dtype == np.float32 else np.float64
    rows = np.zeros((pc.shape[0], 5), dt)
    rows[:, :m] = pc[:, :m]
    b = np.array(boxes[None], dt, order="C")
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    got = on_device(torch.from_numpy(rows).to(dev), torch.from_numpy(b).to(dev), n_samples, extra_width=extra_width,
                    pose=torch.from_numpy(np.ascontiguousarray(box_pose(b))).to(dev), num_features=m)
    return got.points[0].cpu().numpy(), got.empty_flag[0].to(torch.int32).cpu().numpy()
