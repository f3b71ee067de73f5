#!/usr/bin/env python3
"""What a call of each device stage of the torch-tensor boundary costs the HOST: the Python prologue (input checks, out= check, the
offsets' cached upload) and the enqueue through the C entry.  Two float32 frames of 256 rows, two boxes and eight centres per frame, a
preallocated out=, on a stream of the caller's -- the kernels are over in microseconds, so the wall clock around back-to-back calls is
the host's time per call.  Per stage: five warm-up calls, then the wall clock around `--calls` back-to-back calls and the synchronise
after them.

    fov_keep dror_keep voxelize sample_keypoints sample_keypoints_sectors ball_query range_image nearest_keypoints points_in_boxes
    boxes_iou nms roi_point_pool roi_voxel_pool sample_rois assign_anchors

`--tree DIR` imports the package of another checkout (an A/B of two trees: one process per run, the trees alternating).  Prints one JSON
line: milliseconds per call by stage.

    python scripts/probe/stage_enqueue_ab.py [--calls 200] [--tree DIR]
"""
import argparse
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
WARMUP = 5


def stages(torch, T):
    """{name: a call without arguments} on two float32 frames of 256 rows."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    rows = torch.rand((512, 5), generator=g, device=dev) * torch.tensor([40.0, 40.0, 4.0, 1.0, 63.0], device=dev)
    offsets = np.array([0, 256, 512], np.int64)
    fr = T.DeviceBatch(rows.contiguous(), offsets)
    cen = rows[:512:32, :3].reshape(2, 8, 3).contiguous()
    boxes = torch.tensor([[[10.0, 10.0, 2.0, 8.0, 6.0, 4.0, 0.3], [30.0, 20.0, 2.0, 9.0, 5.0, 4.0, 1.2]]] * 2, device=dev)
    scores = torch.tensor([[0.9, 0.4]] * 2, device=dev)
    calib = SimpleNamespace(V2C=np.eye(3, 4), R0=np.eye(3), P2=np.array([[700.0, 0, 600, 0], [0, 700.0, 180, 0], [0, 0, 1.0, 0]]))
    rng = (0.0, 0.0, 0.0, 40.0, 40.0, 4.0)
    mask = torch.empty(512, dtype=torch.bool, device=dev)
    vox = T.VoxelBatch.empty(2, 8, 64)
    key = T.KeypointBatch.empty(2, 32)
    sec = T.KeypointBatch.empty(2, 32, sectors=4)
    nb = T.NeighbourBatch.empty(2, 8, 16)
    img = T.RangeImageBatch.empty(2, 16, 64, 512)
    nn = T.NearestBatch.empty(offsets, 8, 3)
    lab = T.BoxLabelBatch.empty(offsets, 2)
    iou = T.IouBatch.empty(2, 2, 2)
    kept = T.NmsBatch.empty(2, 2, 2)
    pooled = T.RoiPointBatch.empty(2, 2, 16)
    voxels = T.RoiVoxelBatch.empty(2, 2, 2, 8)
    best = (torch.tensor([[0.9, 0.2]] * 2, device=dev), torch.tensor([[0, 1]] * 2, dtype=torch.int32, device=dev))
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    targets = T.RoiTargetBatch.empty(2, 8, 7, 7)
    anchors, anchor_class = boxes[0].contiguous(), torch.tensor([1, 2], dtype=torch.int32, device=dev)
    gt = torch.cat([boxes, torch.tensor([[[1.0], [2.0]]] * 2, device=dev)], dim=2).contiguous()
    labels = T.AnchorTargetBatch.empty(2, 2, 2)
    return {
        "fov_keep": lambda: T.fov_keep(fr, calib),
        "dror_keep": lambda: T.dror_keep(fr, out=mask),
        "voxelize": lambda: T.voxelize(fr, rng, (1.0, 1.0, 1.0), 8, 64, out=vox),
        "sample_keypoints": lambda: T.sample_keypoints(fr, 32, out=key),
        "sample_keypoints_sectors": lambda: T.sample_keypoints(fr, 32, sectors=4, out=sec),
        "ball_query": lambda: T.ball_query(fr, cen, 2.0, 16, out=nb),
        "range_image": lambda: T.range_image(fr, 16, 64, out=img),
        "nearest_keypoints": lambda: T.nearest_keypoints(fr, cen, 3, out=nn),
        "points_in_boxes": lambda: T.points_in_boxes(fr, boxes, out=lab),
        "boxes_iou": lambda: T.boxes_iou(boxes, boxes, out=iou),
        "nms": lambda: T.nms(boxes, scores, 0.5, post_max=2, out=kept),
        "roi_point_pool": lambda: T.roi_point_pool(fr, boxes, 16, out=pooled),
        "roi_voxel_pool": lambda: T.roi_voxel_pool(fr, boxes, 2, 8, out=voxels),
        "sample_rois": lambda: T.sample_rois(boxes, boxes, best, step=step, roi_per_image=8, out=targets),
        "assign_anchors": lambda: T.assign_anchors(anchors, anchor_class, gt, out=labels),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--tree", default=str(ROOT), help="the checkout whose lidar_snow_sim_amd is imported (default: this one)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.tree).resolve()))
    import torch
    from lidar_snow_sim_amd import tensors as T
    stream = torch.cuda.Stream(device=0)
    ms = {}
    with torch.cuda.stream(stream):
        for name, call in stages(torch, T).items():
            for _ in range(WARMUP):
                call()
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            stream.synchronize()
            ms[name] = round((time.perf_counter() - t0) * 1e3 / args.calls, 5)
    print(json.dumps({"probe": "stage_enqueue", "tree": str(Path(T.__file__).resolve().parent.parent), "calls": args.calls, "ms_per_call": ms}))


if __name__ == "__main__":
    main()
