"""Points in 3D boxes for host arrays, in the call shape of roiaware_pool3d's points_in_boxes: one cloud and its boxes in, (box_of, count) out.

The arrays are uploaded, labelled by the HIP kernels (include/snowgpu.h, snowgpu_points_in_boxes_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.points_in_boxes, which
stays on the device and keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np


def box_pose(boxes):
    """(..., 2) float64: (cos, sin) of the heading column in float64, with NumPy -- the pose points_in_boxes() passes to the device."""
    h = np.asarray(boxes)[..., 6].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack((np.cos(h), np.sin(h)), axis=-1)


def points_in_boxes(pc, boxes, return_local=False, device=None):
    """(box_of N int32, count B int32[, local N x 3]) of `pc` (N x M, M >= 3: x, y, z first; float32 stays float32, everything else is
    computed in float64) against `boxes` (B x 7 .. 10, 1 <= B <= 256: cx, cy, cz, dx, dy, dz, heading first): per row the smallest
    number of a box that contains it or -1, per box the rows inside.  The pose is NumPy's cos / sin of the heading in float64, given to
    the device as it is: the result is that of the definition under NumPy's own trigonometry, byte for byte."""
    import torch
    from .tensors import points_in_boxes as on_device
    pc, boxes = np.asarray(pc), np.asarray(boxes)
    if pc.ndim != 2 or pc.shape[1] < 3:
        raise ValueError("pc must be N x M with M >= 3 (x, y, z, ...)")
    if boxes.ndim != 2 or not 7 <= boxes.shape[1] <= 10 or not 1 <= boxes.shape[0] <= 256:
        raise ValueError("boxes must be B x 7 .. 10 with 1 <= B <= 256 (cx, cy, cz, dx, dy, dz, heading, ...)")
    if not torch.cuda.is_available():
        raise RuntimeError("points_in_boxes runs on the GPU: no device is visible (there is no CPU fallback)")
    m = min(pc.shape[1], 5)
    dt = np.float32 if pc.dtype == np.float32 else np.float64
    rows = np.zeros((pc.shape[0], 5), dt)
    rows[:, :m] = pc[:, :m]
    b = np.array(boxes[None], dt, order="C")
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    got = on_device(torch.from_numpy(rows).to(dev), torch.from_numpy(b).to(dev), pose=torch.from_numpy(np.ascontiguousarray(box_pose(b))).to(dev),
                    return_local=return_local)
    res = (got.box_of.cpu().numpy(), got.count[0].cpu().numpy())
    return res + (got.local.cpu().numpy(),) if return_local else res
