"""Range-image projection for host arrays, in the call shape of the range-view loaders' projection: one cloud in, (image, index,
pixel_of) out.

The array is uploaded, projected by the HIP kernels (include/snowgpu.h, snowgpu_range_image_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.range_image, which stays
on the device and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np


def project(pc, height, width, fov_up=3.0, fov_down=-25.0, ring=None, range_limits=(0.0, float("inf")), num_features=None, return_count=False,
            device=None):
    """(image (1 + C) x H x W, index H x W int32, pixel_of N int32[, count H x W int32]) of `pc` (N x M, M >= 3: x, y, z first; float32
    stays float32, everything else is computed in float64): per pixel the range and the first C = num_features columns (by default
    min(M, 5)) of its nearest row, -1 where no row fell.  fov_up, fov_down in degrees; ring: N integers, the image row of every row of
    pc instead of its elevation."""
    import torch
    from .tensors import range_image as on_device
    pc = np.asarray(pc)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x M with M >= 3 (x, y, z, ...)")
    c = min(pc.shape[1], 5) if num_features is None else int(num_features)
    if not 3 <= c <= min(pc.shape[1], 5):
        raise ValueError("num_features must lie in 3 .. min(M, 5): the leading columns of pc that a pixel stores")
    if ring is not None:
        ring = np.asarray(ring)
        if ring.shape != (pc.shape[0],) or ring.dtype.kind not in "iu":
            raise ValueError("ring must hold one integer per row of pc")
    if not torch.cuda.is_available():
        raise RuntimeError("project runs on the GPU: no device is visible (there is no CPU fallback)")
    m = min(pc.shape[1], 5)
    dt = np.float32 if pc.dtype == np.float32 else np.float64
    rows = np.zeros((pc.shape[0], 5), dt)
    rows[:, :m] = pc[:, :m]
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    d_ring = None if ring is None else torch.from_numpy(np.clip(ring, -1, 2 ** 31 - 1).astype(np.int32)).to(dev)
    got = on_device(torch.from_numpy(rows).to(dev), height, width, fov_up=fov_up, fov_down=fov_down, ring=d_ring, range_limits=range_limits,
                    num_features=c, return_count=return_count)
    res = (got.image[0].cpu().numpy(), got.index[0].cpu().numpy(), got.pixel_of.cpu().numpy())
    return res + (got.count[0].cpu().numpy(),) if return_count else res
