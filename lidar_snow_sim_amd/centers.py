"""Centre heatmap targets for host arrays, one frame: the gt boxes in, the heatmap, the regression targets, the pixel indices and the mask of
a centre head out -- the call shape of pcdet's CenterHead.assign_target_of_single_head.

The array is uploaded, assigned by the HIP kernels (include/snowgpu.h, snowgpu_assign_centers_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors go to lidar_snow_sim_amd.tensors.assign_centers, which stays on the device and
keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("heatmap", "gt_index", "ind", "mask", "offset", "radius", "count", "state")


def assign_targets(gt_boxes, point_cloud_range, voxel_size, stride, feature_map_size, n_classes=3, class_head=None, max_objs=500, gaussian_overlap=0.1,
                   min_radius=2, outside="clamp", device=None, return_batch=False):
    """(heatmap, ret_boxes, inds, mask) for `gt_boxes` (B x 8 .. 10, 1 <= B <= 256: cx, cy, cz, dx, dy, dz, heading, class first; float32
    stays float32, everything else is computed in float64): heatmap (NC, H, W) float32, ret_boxes (NH, M, Cg), inds (NH, M) int64 and mask
    (NH, M) bool, the head axis kept whatever NH.  With return_batch a fifth value: a dict of NumPy arrays, one per field of
    CenterTargetBatch without the frame axis."""
    import torch
    from .tensors import assign_centers as on_device
    gt_boxes = np.asarray(gt_boxes)
    if gt_boxes.ndim != 2 or not 8 <= gt_boxes.shape[1] <= 10 or not 1 <= gt_boxes.shape[0] <= 256:
        raise ValueError("gt_boxes must be B x 8 .. 10 with 1 <= B <= 256 (cx, cy, cz, dx, dy, dz, heading, class, ...)")
    if not torch.cuda.is_available():
        raise RuntimeError("assign_targets runs on the GPU: no device is visible (there is no CPU fallback)")
    dt = np.float32 if gt_boxes.dtype == np.float32 else np.float64
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    gt = torch.from_numpy(np.array(gt_boxes[None], dt, order="C")).to(dev)
    got = on_device(gt, point_cloud_range, voxel_size, stride, feature_map_size, n_classes, class_head, max_objs, gaussian_overlap, min_radius, outside)
    res = (got.heatmap[0].cpu().numpy(), got.target_boxes(gt)[0].cpu().numpy(), got.ind[0].cpu().numpy().astype(np.int64), got.mask[0].cpu().numpy())
    return res + ({name: getattr(got, name)[0].cpu().numpy() for name in FIELDS},) if return_batch else res
