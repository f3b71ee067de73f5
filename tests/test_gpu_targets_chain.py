"""-m gpu: the documented second stage as one chain of device stages on a small aligned batch -- nms -> boxes_iou(return_best=True) ->
sample_rois -> roi_point_pool on the sampled rois -- with every link held to its restatement: the sampled rois are the restatement's
picks from the NMS boxes under the IoU stage's own best overlaps, and pooling them gives what pooling the same rois picked by hand gives.
RoiTargetBatch.rois is also taken as it stands by roi_voxel_pool, points_in_boxes and boxes_iou."""
import numpy as np
import pytest
import torch

import iou_reference as ir
import targets_reference as tr
from lidar_snow_sim_amd.tensors import sample_rois  # noqa: F401  (the stage under test: without it nothing here runs)

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def test_nms_iou_sample_pool():
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import AlignedResult, boxes_iou, nms, points_in_boxes, roi_point_pool, roi_voxel_pool, sample_rois
    F, n, B, P, G, S, NS, C = 3, 2000, 96, 32, 6, 16, 32, 4
    rng = np.random.default_rng(5700)
    boxes = np.stack([ir.clustered(rng, B, 10) for _ in range(F)]).astype(np.float32)
    scores = rng.uniform(0.05, 1.0, (F, B)).astype(np.float32)
    gt = np.zeros((F, G, 8), np.float32)
    for f in range(F):
        gt[f, :, :7] = boxes[f, rng.choice(B, G, replace=False), :7] + rng.normal(0, 0.15, (G, 7)).astype(np.float32) * np.array([1, 1, 0.3, 0.3, 0.2, 0.2, 0.3], np.float32)
        gt[f, :, 7] = rng.integers(1, 4, G)
    gt[2] = 0                                                               # a frame without a gt box: background only
    gt[2, :, 0] = 500
    gt[2, :, 3:6] = 1
    frames = []
    for f in range(F):
        at = boxes[f, rng.integers(0, B, n), :3]
        frames.append(np.column_stack((at + rng.normal(0, 1.5, (n, 3)) * np.array([1, 1, 0.4]), rng.integers(1, 255, n), rng.integers(0, 64, n))))
    cloud = np.concatenate(frames).astype(np.float32)
    own = rng.uniform(0, 1, F * n) < 0.85
    offsets = np.arange(F + 1, dtype=np.int64) * n
    eng = engine.get_engine(torch.cuda.current_device(), 0)
    z = torch.zeros(1, dtype=torch.int64).cuda()
    res = AlignedResult(eng.ctx, _t(cloud), _t(own), z, z, z, offsets, torch.cuda.current_stream())
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    cfg = tr.settings(roi_per_image=S, fg_ratio=0.5)

    nb = nms(_t(boxes), _t(scores), 0.45, post_max=P, score_thresh=0.1)
    ib = boxes_iou(nb.boxes, _t(gt), return_iou=False, return_best=True)
    rt = sample_rois(nb, _t(gt), ib, step=step, seed=77, return_pose=True, return_local=True, **cfg)
    pooled = roi_point_pool(res, rt.rois, NS, extra_width=0.2, pose=rt.pose, num_features=C, return_pose=True)
    torch.cuda.synchronize()

    # the sampled rois are the restatement's picks from the kept boxes under the overlaps the IoU stage gave
    kept, count = nb.boxes.cpu().numpy(), nb.count.cpu().numpy()
    assert (count > 4).all() and (count < P).any()
    index, used = rt.index.cpu().numpy(), rt.pose.cpu().numpy()
    pose = ir.numpy_pose(kept)
    for f, k in zip(*np.nonzero(index >= 0)):
        pose[f, index[f, k]] = used[f, k]
    want = tr.sample_rois(kept, gt, ib.best_iou.cpu().numpy(), ib.best.cpu().numpy(), pose, cfg, 77, 5)
    for name in tr.FIELDS:
        assert getattr(rt, name).cpu().numpy().tobytes() == want[name].tobytes(), name
    assert want["branch"] == ["a", "a", "c"] and (index >= 0).all() and (index < count[:, None]).all()      # the zero rows behind the count are never sampled
    assert rt.reg_valid.cpu().numpy()[:2].any() and not rt.reg_valid.cpu().numpy()[2].any() and (rt.gt_index.cpu().numpy()[2] == -1).all()

    # pooling the sampled rois = pooling the same rois picked by hand
    by_hand = torch.gather(nb.boxes, 1, rt.index.long()[..., None].expand(-1, -1, nb.boxes.shape[2])).contiguous()
    assert torch.equal(by_hand.view(torch.uint8), rt.rois.view(torch.uint8))
    hand = roi_point_pool(res, by_hand, NS, extra_width=0.2, pose=rt.pose, num_features=C, return_pose=True)
    torch.cuda.synchronize()
    for name in ("count", "index", "points", "pose"):
        assert torch.equal(getattr(pooled, name).view(torch.uint8), getattr(hand, name).view(torch.uint8)), name
    full = roi_point_pool(res, nb, NS, extra_width=0.2, num_features=C)
    assert torch.equal(pooled.count, torch.gather(full.count, 1, rt.index.long())) and (pooled.count > 0).any()

    # the sampled rois as the other box stages take them
    voxels = roi_voxel_pool(res, rt.rois, out_size=4, max_points=8)
    labels = points_in_boxes(res, rt.rois)
    again = boxes_iou(rt.rois, _t(gt), return_iou=False, return_best=True)
    torch.cuda.synchronize()
    assert (voxels.roi_count <= pooled.count).all() and (voxels.roi_count > 0).any()          # (no extra width there: no more members than the pooled rois have)
    assert labels.count.shape == (F, S) and torch.equal(again.best, rt.gt_index) and torch.equal(again.best_iou, rt.roi_iou)
