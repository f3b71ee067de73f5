"""Anchor target assignment for host arrays, one frame: anchors, their classes and the gt boxes in, the label and the gt of every anchor out.

The arrays are uploaded, assigned by the HIP kernels (include/snowgpu.h, snowgpu_assign_anchors_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors go to lidar_snow_sim_amd.tensors.assign_anchors, which stays on the device and
keeps static shapes.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("label", "gt_index", "count", "gt_count", "iou")


def assign_targets(anchors, anchor_class, gt_boxes, matched=(0.6, 0.5, 0.5), unmatched=(0.45, 0.35, 0.35), device=None):
    """A dict of NumPy arrays, one per field of AnchorTargetBatch without the frame axis (`iou` included), for `anchors` (A x 7 .. 10: cx,
    cy, cz, dx, dy, dz, heading first; float32 stays float32, everything else is computed in float64), `anchor_class` (A: the class number
    of each anchor) and `gt_boxes` (B x 8 .. 10, 1 <= B <= 256: column 7 is the class) under the thresholds `matched` and `unmatched`, one
    number per class each."""
    import torch
    from .tensors import assign_anchors as on_device
    anchors, gt_boxes, anchor_class = np.asarray(anchors), np.asarray(gt_boxes), np.asarray(anchor_class)
    if anchors.ndim != 2 or not 7 <= anchors.shape[1] <= 10 or anchors.shape[0] < 1:
        raise ValueError("anchors must be A x 7 .. 10 with 1 <= A (cx, cy, cz, dx, dy, dz, heading, ...)")
    if gt_boxes.ndim != 2 or not 8 <= gt_boxes.shape[1] <= 10 or not 1 <= gt_boxes.shape[0] <= 256:
        raise ValueError("gt_boxes must be B x 8 .. 10 with 1 <= B <= 256 (cx, cy, cz, dx, dy, dz, heading, class, ...)")
    if anchor_class.shape != anchors.shape[:1]:
        raise ValueError("anchor_class holds one class number per anchor")
    if not torch.cuda.is_available():
        raise RuntimeError("assign_targets runs on the GPU: no device is visible (there is no CPU fallback)")
    dt = np.float32 if anchors.dtype == np.float32 else np.float64
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))

    def up(a, kind):
        return torch.from_numpy(np.array(a, kind, order="C")).to(dev)
    got = on_device(up(anchors, dt), up(anchor_class, np.int32), up(gt_boxes[None], dt), matched, unmatched, return_iou=True)
    return {name: getattr(got, name)[0].cpu().numpy() for name in FIELDS}
