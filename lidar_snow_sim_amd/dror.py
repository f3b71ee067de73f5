"""Dynamic radius outlier removal (DROR; Charron, Phillips and Waslander, "De-noising of Lidar Point Clouds Corrupted by Snowfall", CRV 2018)
for host arrays, in the call shape of the reference's viewer (pointcloud_viewer.py:2266-2270; defaults :267-270).

The reference takes the filter from its cadc_devkit submodule, which is not part of the checkout; this is the published algorithm with
this library's edge conventions (include/snowgpu.h, snowgpu_dror_mask_device): a point is kept iff at least k_min OTHER points lie within
max(sr_min, beta * radians(alpha) * r_xy) of it, the ball closed.  The array is uploaded, filtered by the HIP kernels and the mask
downloaded; torch CUDA tensors go to lidar_snow_sim_amd.tensors.dror_keep, which stays on the device.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np


def dynamic_radius_outlier_filter(pc, alpha=0.45, beta=3, k_min=3, sr_min=0.04, device=None) -> np.ndarray:
    """The keep mask of `pc` (N x C, C >= 3: x, y, z first; any real dtype -- float32 stays float32, everything else is computed from
    float64): True for the points DROR keeps.  `pc[mask]` is the de-noised cloud."""
    import torch
    from .tensors import dror_keep
    pc = np.asarray(pc)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x C with C >= 3 (x, y, z, ...)")
    if not torch.cuda.is_available():
        raise RuntimeError("dynamic_radius_outlier_filter runs on the GPU: no device is visible (there is no CPU fallback)")
    rows = np.zeros((pc.shape[0], 5), np.float32 if pc.dtype == np.float32 else np.float64)
    rows[:, :3] = pc[:, :3]
    index = torch.cuda.current_device() if device is None else int(device)
    t = torch.from_numpy(rows).to(torch.device("cuda", index))
    return dror_keep(t, alpha, beta, k_min, sr_min).cpu().numpy()
