"""Farthest point sampling for host arrays, in the call shape of the common point-cloud libraries' furthest_point_sample followed by a
gather: one cloud in, (index, points) out.

The array is uploaded, sampled by the HIP kernels (include/snowgpu.h, snowgpu_fps_device: the definition and its edge conventions) and
the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.sample_keypoints, which stays on the
device and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

# Usable rows of a frame up to which the sampler keeps the frame in registers (the first two entries) or its running minima in LDS (the
# third), per row dtype (csrc/sg_fps.h: SG_FPS_TIER0_ROWS_*, SG_FPS_TIER1_ROWS_*, SG_FPS_TIER2_ROWS_*); a frame of more usable rows
# streams from scratch.  Every entry is a size at which the kernel takes another path.
TIER_ROWS = {"float32": (8192, 16384, 39936), "float64": (4096, 8192, 19968)}


def farthest_point_sample(pc, n_samples, point_cloud_range=None, num_features=None, device=None):
    """(index n_samples int32, points n_samples x C) of `pc` (N x K, K >= 3: x, y, z first; float32 stays float32, everything else is
    computed in float64): row 0 -- the first usable row -- then n_samples - 1 times the row farthest from every row taken so far.
    C = num_features, by default min(K, 5) columns.  A cloud without a usable row returns index -1 and points 0."""
    import torch
    from .tensors import sample_keypoints
    pc = np.asarray(pc)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x K with K >= 3 (x, y, z, ...)")
    c = min(pc.shape[1], 5) if num_features is None else int(num_features)
    if not 3 <= c <= min(pc.shape[1], 5):
        raise ValueError("num_features must lie in 3 .. min(K, 5): the leading columns of pc that a keypoint carries")
    if not torch.cuda.is_available():
        raise RuntimeError("farthest_point_sample runs on the GPU: no device is visible (there is no CPU fallback)")
    k = min(pc.shape[1], 5)
    rows = np.zeros((pc.shape[0], 5), np.float32 if pc.dtype == np.float32 else np.float64)
    rows[:, :k] = pc[:, :k]
    index = torch.cuda.current_device() if device is None else int(device)
    t = torch.from_numpy(rows).to(torch.device("cuda", index))
    got = sample_keypoints(t, n_samples, point_cloud_range=point_cloud_range, num_features=c)
    return got.index[0].cpu().numpy(), got.points[0].cpu().numpy()


def sectorized_sample(pc, n_samples, n_sectors=6, rois=None, roi_margin=1.6, point_cloud_range=None, num_features=None, device=None):
    """PV-RCNN++'s sectorized, proposal-centric sampling of one cloud (include/snowgpu.h, snowgpu_fps_sectors_device): (index n_samples
    int32, points n_samples x C, sector_offsets n_sectors + 1 int32).  `pc` as farthest_point_sample takes it; rois: B x 7 .. 10 boxes
    (cx, cy, cz, dx, dy, dz, heading, ...; zero rows are padding) or None -- with rois only the rows within a box's half diagonal +
    roi_margin of its centre are sampled.  The usable rows are split by azimuth into n_sectors sectors, and sector s fills the slots
    sector_offsets[s] .. sector_offsets[s + 1] - 1 by a farthest-point walk of its own; slots from sector_offsets[-1] on repeat slot 0."""
    import torch
    from .tensors import sample_keypoints
    pc = np.asarray(pc)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x K with K >= 3 (x, y, z, ...)")
    c = min(pc.shape[1], 5) if num_features is None else int(num_features)
    if not 3 <= c <= min(pc.shape[1], 5):
        raise ValueError("num_features must lie in 3 .. min(K, 5): the leading columns of pc that a keypoint carries")
    if not torch.cuda.is_available():
        raise RuntimeError("sectorized_sample runs on the GPU: no device is visible (there is no CPU fallback)")
    k = min(pc.shape[1], 5)
    rows = np.zeros((pc.shape[0], 5), np.float32 if pc.dtype == np.float32 else np.float64)
    rows[:, :k] = pc[:, :k]
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    d_rois = None
    if rois is not None:
        rois = np.asarray(rois)
        if rois.ndim != 2 or not 7 <= rois.shape[1] <= 10 or not 1 <= rois.shape[0] <= 256:
            raise ValueError("rois must be B x 7 .. 10 with 1 <= B <= 256 (cx, cy, cz, dx, dy, dz, heading, ...)")
        d_rois = torch.from_numpy(np.array(rois[None], rows.dtype, order="C")).to(dev)          # (a copy: from_numpy wants a writable array)
    got = sample_keypoints(torch.from_numpy(rows).to(dev), n_samples, point_cloud_range=point_cloud_range, num_features=c, sectors=n_sectors, rois=d_rois,
                           roi_margin=roi_margin)
    return got.index[0].cpu().numpy(), got.points[0].cpu().numpy(), got.sector_offsets[0].cpu().numpy()
