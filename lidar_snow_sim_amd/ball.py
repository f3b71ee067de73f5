"""Ball query for host arrays, in the call shape of the common point-cloud libraries' ball_query: one cloud and its centres in,
(index, count) out.

The arrays are uploaded, grouped by the HIP kernels (include/snowgpu.h, snowgpu_ball_query_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.ball_query, which stays
on the device and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np


def ball_query(pc, centres, radius, n_neighbours, point_cloud_range=None, num_features=None, return_points=False, device=None):
    """(index K x S int32, count K x R int32[, points K x S x C]) of `pc` (N x M, M >= 3: x, y, z first; float32 stays float32, everything
    else is computed in float64) around `centres` (K x 3 .. 5): per (radius, n_neighbours) pair the n_neighbours smallest indices of the
    rows strictly within the radius, ascending, padded with the first (-1 for an empty ball), the pairs side by side, and the rows in
    every ball.  C = num_features, by default min(M, 5) columns."""
    import torch
    from .tensors import ball_query as on_device
    pc, centres = np.asarray(pc), np.asarray(centres)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x M with M >= 3 (x, y, z, ...)")
    if centres.ndim != 2 or not 3 <= centres.shape[1] <= 5 or centres.shape[0] < 1:
        raise ValueError("centres must be K x 3 .. 5 with K >= 1 (x, y, z, ...)")
    c = min(pc.shape[1], 5) if num_features is None else int(num_features)
    if not 3 <= c <= min(pc.shape[1], 5):
        raise ValueError("num_features must lie in 3 .. min(M, 5): the leading columns of pc that a neighbour carries")
    if not torch.cuda.is_available():
        raise RuntimeError("ball_query runs on the GPU: no device is visible (there is no CPU fallback)")
    m = min(pc.shape[1], 5)
    dt = np.float32 if pc.dtype == np.float32 else np.float64
    rows = np.zeros((pc.shape[0], 5), dt)
    rows[:, :m] = pc[:, :m]
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    got = on_device(torch.from_numpy(rows).to(dev), torch.from_numpy(np.array(centres[None], dt, order="C")).to(dev), radius, n_neighbours,
                    point_cloud_range=point_cloud_range, num_features=c, return_points=return_points)
    res = (got.index[0].cpu().numpy(), got.count[0].cpu().numpy())
    return res + (got.points[0].cpu().numpy(),) if return_points else res
