"""Nearest centres for host arrays, in the call shape of pointnet2's three_nn: one cloud and its centres in, (dist2, index[, weight]) out.

The arrays are uploaded, searched by the HIP kernels (include/snowgpu.h, snowgpu_nearest_centres_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.nearest_keypoints, which
stays on the device and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np


def three_nn(pc, centres, k=3, point_cloud_range=None, return_weights=True, device=None):
    """(dist2 N x k, index N x k int32[, weight N x k]) of `pc` (N x M, M >= 3: x, y, z first; float32 stays float32, everything else is
    computed in float64) against `centres` (K x 3 .. 5): per row the k nearest usable centres by (squared distance, centre number), -1 /
    +inf / 0 in the slots beyond them and for a row that is not usable, and pointnet2's normalised 1 / (dist + 1e-8) weights."""
    import torch
    from .tensors import nearest_keypoints
    pc, centres = np.asarray(pc), np.asarray(centres)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x M with M >= 3 (x, y, z, ...)")
    if centres.ndim != 2 or not 3 <= centres.shape[1] <= 5 or centres.shape[0] < 1:
        raise ValueError("centres must be K x 3 .. 5 with K >= 1 (x, y, z, ...)")
    if not torch.cuda.is_available():
        raise RuntimeError("three_nn runs on the GPU: no device is visible (there is no CPU fallback)")
    m = min(pc.shape[1], 5)
    dt = np.float32 if pc.dtype == np.float32 else np.float64
    rows = np.zeros((pc.shape[0], 5), dt)
    rows[:, :m] = pc[:, :m]
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    got = nearest_keypoints(torch.from_numpy(rows).to(dev), torch.from_numpy(np.array(centres[None], dt, order="C")).to(dev), k,
                            point_cloud_range=point_cloud_range, return_weights=return_weights)
    res = (got.dist2.cpu().numpy(), got.index.cpu().numpy())
    return res + (got.weight.cpu().numpy(),) if return_weights else res
