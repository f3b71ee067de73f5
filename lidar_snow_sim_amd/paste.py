"""Ground-truth object paste for host arrays: a bank built from NumPy frames and labels, and the one-frame call shape of the paste.

The arrays are uploaded, pasted by the HIP kernels (include/snowgpu.h, snowgpu_paste_objects_device: the definition and its edge
conventions) and the result downloaded; torch CUDA tensors and aligned results go to lidar_snow_sim_amd.tensors.paste_objects, which
stays on the device, keeps static shapes and reads the step from device memory.  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from .boxes import box_pose, points_in_boxes

FIELDS = ("rows", "keep", "gt_boxes", "object", "state", "source", "count", "pose")


def build_bank(frames, gt_boxes, min_points=5, device=None):
    """An ObjectBank from NumPy frames (N_f x 5 each: x, y, z, intensity, channel) and their labels (B_f x 8 .. 10 each, the class in
    column 7): the rows of every box are cropped with boxes.points_in_boxes -- a row inside several boxes goes to the first --, positions
    kept; objects of fewer than min_points rows and boxes whose class is not a whole number in 1 .. 16 are dropped; the objects are sorted
    by class, frame and box order kept within a class.  float32 frames stay float32, everything else becomes float64.  No other filter of
    pcdet's database PREPARE step is applied."""
    import torch
    from .tensors import ObjectBank
    frames, gt_boxes = [np.asarray(p) for p in frames], [np.asarray(b) for b in gt_boxes]
    if len(frames) != len(gt_boxes) or not frames:
        raise ValueError("build_bank: one array of labels per frame, and at least one frame")
    if isinstance(min_points, bool) or int(min_points) != min_points or int(min_points) < 0:
        raise ValueError("build_bank: min_points must be a whole number >= 0")
    dt = np.float32 if all(p.dtype == np.float32 for p in frames) else np.float64
    objects = []                                     # (class, points, box)
    for pc, boxes in zip(frames, gt_boxes):
        if pc.ndim != 2 or pc.shape[1] != 5 or boxes.ndim != 2 or not 8 <= boxes.shape[1] <= 10:
            raise ValueError("build_bank: a frame is N x 5, its labels B x 8 .. 10 with the class in column 7")
        pc, boxes = pc.astype(dt), boxes.astype(dt)
        for lo in range(0, len(boxes), 256):         # (points_in_boxes takes 256 boxes a call)
            part = boxes[lo:lo + 256]
            box_of, _ = points_in_boxes(pc, part, device=device)
            for b, box in enumerate(part):
                cls = float(box[7])
                if not (cls == np.floor(cls) and 1 <= cls <= 16):
                    continue
                rows = pc[box_of == b]
                if len(rows) >= int(min_points):
                    objects.append((int(cls), rows, box[:8]))
    if not objects:
        raise ValueError("build_bank: no object of at least min_points rows")
    objects.sort(key=lambda o: o[0])                 # (stable)
    points = np.ascontiguousarray(np.concatenate([o[1] for o in objects]).reshape(-1, 5), dt)
    offsets = np.concatenate(([0], np.cumsum([len(o[1]) for o in objects]))).astype(np.int64)
    boxes = np.ascontiguousarray(np.stack([o[2] for o in objects]), dt)
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    return ObjectBank(torch.from_numpy(points).to(dev), offsets, torch.from_numpy(boxes).to(dev), torch.from_numpy(np.ascontiguousarray(box_pose(boxes))).to(dev))


def paste_objects(pc, keep, gt_boxes, bank, sample_groups, seed=0, step=0, remove_extra_width=(0., 0., 0.), device=None):
    """A dict of NumPy arrays, one per field of PasteBatch without the frame axis (`source` and `pose` included), for one frame `pc`
    (N x 5; float32 stays float32, everything else is computed in float64) with its keep mask (N bool; None: every row present),
    `gt_boxes` (B x 8 .. 10) and an ObjectBank of the same dtype, at draw `step` under `seed`.  The gts' pose is NumPy's cos / sin of the
    heading in float64, given to the device as it is.  A one-frame call is frame 0 of the draw."""
    import torch
    from .tensors import paste_objects as on_device
    pc, gt_boxes = np.asarray(pc), np.asarray(gt_boxes)
    if pc.ndim != 2 or pc.shape[1] != 5:
        raise ValueError("pc must be N x 5 (x, y, z, intensity, channel)")
    if gt_boxes.ndim != 2 or not 8 <= gt_boxes.shape[1] <= 10 or gt_boxes.shape[0] < 1:
        raise ValueError("gt_boxes must be B x 8 .. 10 with B >= 1 (cx, cy, cz, dx, dy, dz, heading, class, ...)")
    if keep is not None and np.shape(keep) != pc.shape[:1]:
        raise ValueError("keep holds one value per row")
    if not torch.cuda.is_available():
        raise RuntimeError("paste_objects runs on the GPU: no device is visible (there is no CPU fallback)")
    dt = np.float32 if pc.dtype == np.float32 else np.float64
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    g = np.array(gt_boxes[None], dt, order="C")
    got = on_device(torch.from_numpy(np.array(pc, dt, order="C")).to(dev), torch.from_numpy(g).to(dev), bank, sample_groups,
                    step=torch.tensor([int(step)], dtype=torch.int64, device=dev), seed=seed,
                    keep=None if keep is None else torch.from_numpy(np.ascontiguousarray(np.asarray(keep).astype(bool))).to(dev),
                    remove_extra_width=remove_extra_width, pose=torch.from_numpy(np.ascontiguousarray(box_pose(g))).to(dev), return_source=True, return_pose=True)
    per_frame = ("gt_boxes", "object", "state", "count", "pose")
    return {name: (getattr(got, name)[0] if name in per_frame else getattr(got, name)).cpu().numpy() for name in FIELDS}
