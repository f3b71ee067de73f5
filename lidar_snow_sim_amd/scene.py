"""Scene transforms for host arrays: the one-frame call shape of the geometric augmentation behind gt_sampling.

The arrays are uploaded, transformed by the HIP kernels (include/snowgpu.h, snowgpu_transform_scene_device: the definition, its edge
conventions and its place in the chain -- behind the weather stages, in front of everything that groups or labels) and the result
downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.transform_scene, which stays on the device, keeps
static shapes and reads the step from device memory.  There is no CPU fallback.
"""
from __future__ import annotations

import math

import numpy as np

from .boxes import box_pose

FIELDS = ("rows", "keep", "gt_boxes", "world", "state", "tried", "local", "pose", "tries")


def transform_scene(pc, gt_boxes, keep=None, seed=0, step=0, flip=('x',), rotation=(-math.pi / 4, math.pi / 4), scaling=(0.95, 1.05), local=None, device=None):
    """A dict of NumPy arrays, one per field of SceneBatch without the frame axis (`pose` included, `tries` with a local part), for one
    frame `pc` (N x 5; float32 stays float32, everything else is computed in float64) with its keep mask (N bool; None: every row
    present) and `gt_boxes` (B x 7 .. 10), at draw `step` under `seed`; flip, rotation, scaling and local as
    tensors.transform_scene takes them.  The gts' pose is NumPy's cos / sin of the heading in float64, given to the device as it is;
    box_of is made on the device.  A one-frame call is frame 0 of the draw."""
    import torch
    from .tensors import transform_scene as on_device
    pc, gt_boxes = np.asarray(pc), np.asarray(gt_boxes)
    if pc.ndim != 2 or pc.shape[1] != 5:
        raise ValueError("pc must be N x 5 (x, y, z, intensity, channel)")
    if gt_boxes.ndim != 2 or not 7 <= gt_boxes.shape[1] <= 10 or gt_boxes.shape[0] < 1:
        raise ValueError("gt_boxes must be B x 7 .. 10 with B >= 1 (cx, cy, cz, dx, dy, dz, heading, ...)")
    if keep is not None and np.shape(keep) != pc.shape[:1]:
        raise ValueError("keep holds one value per row")
    if not torch.cuda.is_available():
        raise RuntimeError("transform_scene runs on the GPU: no device is visible (there is no CPU fallback)")
    dt = np.float32 if pc.dtype == np.float32 else np.float64
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    g = np.array(gt_boxes[None], dt, order="C")
    got = on_device(torch.from_numpy(np.array(pc, dt, order="C")).to(dev), torch.from_numpy(g).to(dev),
                    step=torch.tensor([int(step)], dtype=torch.int64, device=dev), seed=seed, flip=flip, rotation=rotation, scaling=scaling, local=local,
                    keep=None if keep is None else torch.from_numpy(np.ascontiguousarray(np.asarray(keep).astype(bool))).to(dev),
                    pose=torch.from_numpy(np.ascontiguousarray(box_pose(g))).to(dev), return_pose=True, return_tried=local is not None)
    per_frame = ("gt_boxes", "world", "state", "tried", "local", "pose", "tries")
    return {name: (getattr(got, name)[0] if name in per_frame else getattr(got, name)).cpu().numpy() for name in FIELDS if getattr(got, name) is not None}
