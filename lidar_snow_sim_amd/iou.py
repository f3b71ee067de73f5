"""Rotated box IoU and NMS for host arrays of one frame, in the call shapes of pcdet's iou3d_nms_utils: boxes_iou_bev(a, b),
boxes_iou3d(a, b) and nms(boxes, scores, thresh).

The arrays are uploaded, computed by the HIP kernels (include/snowgpu.h, snowgpu_boxes_iou_device and snowgpu_nms_device: the definition
and its edge conventions) and the result downloaded; torch CUDA tensors go to lidar_snow_sim_amd.tensors.boxes_iou and .nms, which stay
on the device and keep static shapes.  The pose is NumPy's cos / sin of the heading in float64, given to the device as it is: the result
is that of the definition under NumPy's own trigonometry, byte for byte.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from .boxes import box_pose


def _checked(who, boxes, name):
    """`boxes` as an array after the shape check; RuntimeError when no device is visible."""
    import torch
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or not 7 <= boxes.shape[1] <= 10 or not 1 <= boxes.shape[0] <= 9216:
        raise ValueError(f"{who}: {name} must be B x 7 .. 10 with 1 <= B <= 9216 (cx, cy, cz, dx, dy, dz, heading, ...)")
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} runs on the GPU: no device is visible (there is no CPU fallback)")
    return boxes


def _uploader(device):
    """A function that puts a host array on the device `device` names (None: torch's current one)."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    return lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _iou(who, a, b, mode, device):
    from .tensors import boxes_iou as on_device
    a, b = _checked(who, a, "boxes_a"), _checked(who, b, "boxes_b")
    dt = np.float32 if a.dtype == np.float32 and b.dtype == np.float32 else np.float64
    a, b = np.array(a[None], dt, order="C"), np.array(b[None], dt, order="C")
    up = _uploader(device)
    return on_device(up(a), up(b), mode=mode, pose_a=up(box_pose(a)), pose_b=up(box_pose(b))).iou[0].cpu().numpy()


def boxes_iou_bev(boxes_a, boxes_b, device=None):
    """(M, B) bird's-eye-view IoU of `boxes_a` (M x 7 .. 10) with `boxes_b` (B x 7 .. 10); float32 in, float32 out, everything else float64."""
    return _iou("boxes_iou_bev", boxes_a, boxes_b, "bev", device)


def boxes_iou3d(boxes_a, boxes_b, device=None):
    """(M, B) 3D IoU of `boxes_a` with `boxes_b`."""
    return _iou("boxes_iou3d", boxes_a, boxes_b, "3d", device)


def nms(boxes, scores, thresh, post_max=None, device=None):
    """The kept box numbers (int32, rank order) of rotated BEV NMS over `boxes` (B x 7 .. 10) with `scores` (B): pcdet's nms_gpu.  post_max:
    keep at most so many (None: B)."""
    from .tensors import nms as on_device
    boxes = _checked("nms", boxes, "boxes")
    scores = np.asarray(scores)
    if scores.shape != boxes.shape[:1]:
        raise ValueError("nms: scores must hold one value per box")
    dt = np.float32 if boxes.dtype == np.float32 and scores.dtype == np.float32 else np.float64
    b, s = np.array(boxes[None], dt, order="C"), np.array(scores[None], dt, order="C")
    up = _uploader(device)
    got = on_device(up(b), up(s), float(thresh), post_max=len(boxes) if post_max is None else post_max, pose=up(box_pose(b)), return_boxes=False)
    return got.index[0, :int(got.count[0])].cpu().numpy()
