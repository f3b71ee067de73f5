#!/usr/bin/env python3
"""What proposal target sampling (snowgpu_sample_rois_device) costs beside the torch formulation it replaces, in one process:

    sample_rois[_local]   the stage on F frames of M rois against B gt boxes, S slots, float32 (_local: with gt_local and pose)
    torch_nonzero         pcdet's subsample_rois / sample_bg_inds frame by frame in torch ops: nonzero() on the three overlap classes,
                          their sizes read on the host, randperm / randint from torch's generator, the gathers and the labels

Synthetic inputs: clustered proposals as scripts/probe/iou_ab.py makes them, gt boxes near some of them, the overlaps from boxes_iou.
The two forms draw from different random streams, so their outputs are compared in distribution only: the segment sizes must agree
frame by frame, and every pick must come from its class.  The device form is timed with device events around `--steps` back-to-back calls,
the torch form by the wall clock around synchronized calls (it reads on the host anyway); `--repeats` windows each, the forms alternating,
two warm-up calls first.

    python scripts/probe/targets_ab.py [--frames 16] [--rois 512] [--gt 64] [--slots 128] [--steps 200] [--repeats 5]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

CFG = dict(reg_fg_thresh=0.55, cls_fg_thresh=0.75, cls_bg_thresh=0.25, cls_bg_thresh_lo=0.1, hard_bg_ratio=0.8)


def torch_sample(torch, rois, gt, ov, assign, S, fg_per_image):
    """(index, rois, roi_iou, gt_of_rois, reg_valid, cls_label, segments) frame by frame, as pcdet's layer does it."""
    fg_thresh = min(CFG["reg_fg_thresh"], CFG["cls_fg_thresh"])
    picked, segments = [], []
    for f in range(rois.shape[0]):
        o = ov[f]
        fg = (o >= fg_thresh).nonzero().view(-1)
        easy = (o < CFG["cls_bg_thresh_lo"]).nonzero().view(-1)
        hard = ((o < CFG["reg_fg_thresh"]) & (o >= CFG["cls_bg_thresh_lo"])).nonzero().view(-1)
        n_fg, n_bg = fg.numel(), hard.numel() + easy.numel()                      # host reads

        def bg(n):
            if hard.numel() > 0 and easy.numel() > 0:
                h = min(int(n * CFG["hard_bg_ratio"]), hard.numel())
                return torch.cat((hard[torch.randint(0, hard.numel(), (h,), device=o.device)], easy[torch.randint(0, easy.numel(), (n - h,), device=o.device)])), h
            src = hard if hard.numel() > 0 else easy
            return src[torch.randint(0, src.numel(), (n,), device=o.device)], (n if hard.numel() > 0 else 0)
        if n_fg > 0 and n_bg > 0:
            k = min(fg_per_image, n_fg)
            head = fg[torch.randperm(n_fg, device=o.device)[:k]]
            tail, h = bg(S - k)
            picked.append(torch.cat((head, tail)))
            segments.append((k, h, S - k - h))
        elif n_fg > 0:
            picked.append(fg[torch.randint(0, n_fg, (S,), device=o.device)])
            segments.append((S, 0, 0))
        else:
            tail, h = bg(S)
            picked.append(tail)
            segments.append((0, h, S - h))
    index = torch.stack(picked)
    got_rois = torch.gather(rois, 1, index[..., None].expand(-1, -1, rois.shape[2]))
    iou = torch.gather(ov, 1, index)
    got_gt = torch.gather(gt, 1, torch.gather(assign, 1, index).clamp(min=0).long()[..., None].expand(-1, -1, gt.shape[2]))
    reg_valid = iou > CFG["reg_fg_thresh"]
    label = torch.where(iou > CFG["cls_fg_thresh"], 1.0, torch.where(iou < CFG["cls_bg_thresh"], 0.0, (iou - CFG["cls_bg_thresh"]) / (CFG["cls_fg_thresh"] - CFG["cls_bg_thresh"])))
    return index, got_rois, iou, got_gt, reg_valid, label, segments


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rois", type=int, default=512)
    ap.add_argument("--gt", type=int, default=64)
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from lidar_snow_sim_amd.tensors import RoiTargetBatch, boxes_iou, sample_rois
    dev = torch.device("cuda:0")
    F, M, B, S = args.frames, args.rois, args.gt, args.slots
    fg_per_image = int(np.round(0.5 * S))
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    Cn = max(M // 8, B)                                                    # clustered proposals (iou_ab.py): Cn centres, M proposals about them
    u = torch.rand((F, Cn, 4), device=dev, generator=g)
    cen = torch.zeros((F, Cn, 7), device=dev)
    cen[:, :, :2] = (torch.rand((F, Cn, 2), device=dev, generator=g) - 0.5) * 140
    cen[:, :, 2] = -1.0
    cen[:, :, 3], cen[:, :, 4], cen[:, :, 5] = 3.5 + 1.5 * u[:, :, 0], 1.6 + 0.5 * u[:, :, 1], 1.4 + 0.6 * u[:, :, 2]
    cen[:, :, 6] = (2 * u[:, :, 3] - 1) * np.pi
    of = torch.randint(0, Cn, (F, M), device=dev, generator=g)
    rois = torch.gather(cen, 1, of[:, :, None].expand(F, M, 7)).clone()
    rois[:, :, :2] += 0.4 * torch.randn((F, M, 2), device=dev, generator=g)
    rois[:, :, 3:6] *= 0.92 + 0.16 * torch.rand((F, M, 3), device=dev, generator=g)
    rois[:, :, 6] += 0.1 * torch.randn((F, M), device=dev, generator=g)
    rois = rois.contiguous()
    gt = torch.cat((cen[:, :B], torch.ones((F, B, 1), device=dev)), -1).contiguous()
    s = torch.cuda.Stream()
    out_json = {"frames": F, "rois": M, "gt": B, "slots": S, "steps": args.steps, "device": torch.cuda.get_device_name(0), "dtype": "float32"}
    with torch.cuda.stream(s):
        ib = boxes_iou(rois, gt, return_iou=False, return_best=True)
        ov, assign = ib.best_iou, ib.best
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        bare = RoiTargetBatch.empty(F, S, 7, 8, torch.float32, dev)
        full = RoiTargetBatch.empty(F, S, 7, 8, torch.float32, dev, with_pose=True, with_local=True)
        forms = {"sample_rois": lambda: sample_rois(rois, gt, (ov, assign), step=step, seed=1, roi_per_image=S, out=bare, **CFG),
                 "sample_rois_local": lambda: sample_rois(rois, gt, (ov, assign), step=step, seed=1, roi_per_image=S, out=full, return_local=True, return_pose=True, **CFG)}
        for form in forms.values():
            for _ in range(2):
                form()
        for _ in range(2):
            ref = torch_sample(torch, rois, gt, ov, assign, S, fg_per_image)
        s.synchronize()
        # in distribution: the same segments, and every pick from its class
        seg = bare.segments.cpu().numpy()
        assert seg.tolist() == [list(x) for x in ref[6]], (seg.tolist(), ref[6])
        count = bare.class_count.cpu().numpy()
        out_json["class_count_mean"] = [round(float(v), 1) for v in count.mean(0)]
        out_json["segments_mean"] = [round(float(v), 1) for v in seg.mean(0)]
        iou = bare.roi_iou.cpu().numpy()
        for f in range(F):
            a, b = seg[f, 0], seg[f, 0] + seg[f, 1]
            assert (iou[f, :a] >= 0.55).all() and ((iou[f, a:b] < 0.55) & (iou[f, a:b] >= 0.1)).all() and (iou[f, b:] < 0.1).all()
            assert len(set(bare.index[f, :a].tolist())) == a

        def timed(form):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(args.steps):
                form()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b) / args.steps

        def wall():
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                torch_sample(torch, rois, gt, ov, assign, S, fg_per_image)
            s.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.steps

        runs = {k: [] for k in list(forms) + ["torch_nonzero"]}
        for _ in range(args.repeats):
            for k, form in forms.items():
                runs[k].append(timed(form))
            runs["torch_nonzero"].append(wall())
        out_json["ms_per_call"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        out_json["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(out_json), flush=True)


if __name__ == "__main__":
    main()
