#!/usr/bin/env python3
"""What anchor target assignment (snowgpu_assign_anchors_device) costs beside the torch formulation it replaces and beside the aligned
snowfall call, in one process:

    snowfall_aligned      the aligned snowfall call on F C2 sweeps (bench.py's synthetic 64 x 2048 sweeps), for scale
    assign_anchors[_iou]  the stage on SECOND's KITTI head -- 176 x 200 positions, 3 classes x 2 rotations, A = 211 200 anchors -- against
                          B gt boxes in each of F frames, float32, into out= (_iou: with the best overlap)
    torch_assigner        the formulation of pcdet's AxisAlignedTargetAssigner run the way pcdet runs it: per frame and class the gts of the
                          class by a mask (their number read on the host), the anchors x gts nearest-BEV IoU matrix, two argmax / max, and
                          nonzero() for the forced, the positive and the background anchors

Synthetic gts: per frame B boxes of a random class around grid positions, sizes within 15 % of the class's anchor, any heading.  The torch
form is run once more in float64 on (double) of the same inputs, operation by operation in the definition's order; its labels must equal
the stage's wherever the torch form is well defined -- everywhere: labels do not depend on which of equal maxima argmax returns --, its
gt numbers wherever the anchor's maximum is reached by one gt only.  The device form is timed with device events around `--steps`
back-to-back calls, the torch form by the wall clock around synchronized calls (it reads on the host anyway); `--repeats` windows each,
the forms alternating, two warm-up calls first.

    python scripts/probe/anchors_ab.py [--frames 16] [--gt 64] [--steps 200] [--torch-steps 5] [--repeats 5] [--out profiles/anchors_ab.jsonl]
"""
import argparse
import json
import random
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

RANGE, GRID = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0), (176, 200)
SIZES, ROTATIONS, BOTTOMS = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73)), (0.0, np.pi / 2), (-1.78, -0.6, -0.6)
MATCHED, UNMATCHED = (0.6, 0.5, 0.5), (0.45, 0.35, 0.35)


def bev(torch, b):
    """x0, x1, y0, y1, area of the nearest axis-aligned BEV boxes, in b's dtype, in the definition's order."""
    h = b[:, 6]
    turn = (h - torch.floor(h / np.pi + 0.5) * np.pi).abs()
    keep = turn < np.pi / 4
    ex, ey = torch.where(keep, b[:, 3], b[:, 4]), torch.where(keep, b[:, 4], b[:, 3])
    x0, x1, y0, y1 = b[:, 0] - ex / 2, b[:, 0] + ex / 2, b[:, 1] - ey / 2, b[:, 1] + ey / 2
    return x0, x1, y0, y1, (x1 - x0) * (y1 - y0)


def torch_assign(torch, anchors_of, index_of, gt, A):
    """(label, gt_index) (F, A) as pcdet's assigner computes them: frame by frame, class by class."""
    F = gt.shape[0]
    label = torch.full((F, A), -1, dtype=torch.int32, device=gt.device)
    gt_index = torch.full((F, A), -1, dtype=torch.int32, device=gt.device)
    for f in range(F):
        for c, (an, at) in enumerate(zip(anchors_of, index_of)):
            own = (gt[f, :, 7] == c + 1).nonzero().view(-1)                 # the host reads its length
            lab = torch.zeros(an.shape[0], dtype=torch.int32, device=gt.device)
            idx = torch.full((an.shape[0],), -1, dtype=torch.int32, device=gt.device)
            if own.numel() > 0:
                g = gt[f, own]
                ax0, ax1, ay0, ay1, aa = (v[:, None] for v in bev(torch, an))
                gx0, gx1, gy0, gy1, ga = (v[None, :] for v in bev(torch, g))
                inter = (torch.minimum(ax1, gx1) - torch.maximum(ax0, gx0)).clamp(min=0) * (torch.minimum(ay1, gy1) - torch.maximum(ay0, gy0)).clamp(min=0)
                iou = inter / ((aa + ga) - inter).clamp(min=1e-6)
                best, arg = iou.max(dim=1)
                top = iou.max(dim=0).values
                top = torch.where(top > 0, top, torch.full_like(top, -1.0))
                forced = (iou == top[None, :]).nonzero()[:, 0]
                pos = (best >= MATCHED[c]).nonzero().view(-1)
                bg = (best < UNMATCHED[c]).nonzero().view(-1)
                lab.fill_(-1)
                lab[bg] = 0
                lab[forced] = c + 1
                lab[pos] = c + 1
                mine = own[arg].int()
                idx[forced] = mine[forced]
                idx[pos] = mine[pos]
                ties = (iou == best[:, None]).sum(dim=1) > 1
                idx = torch.where(ties & (idx >= 0), torch.full_like(idx, -2), idx)        # -2: argmax had a choice
            label[f, at] = lab
            gt_index[f, at] = idx
    return label, gt_index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--gt", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import AnchorTargetBatch, anchor_grid, assign_anchors
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F, B = args.frames, args.gt
    layers, azimuths, snowfall, velocity, rscale = bench.WORKLOADS["C2"]
    tables = bench.make_tables(layers, snowfall, velocity, distinct=min(layers, 64))
    frames, orders = [], []
    for f in range(F):
        frames.append(bench.make_frame(layers, azimuths, 1000 + f, rscale))
        random.seed(1000 + f)
        o = list(range(layers))
        random.shuffle(o)
        orders.append(o)
    n_per = frames[0].shape[0]
    n = F * n_per
    rows = torch.from_numpy(np.concatenate(frames)).to(dev)
    del frames
    off = torch.from_numpy(np.arange(F + 1, dtype=np.int64) * n_per).to(dev)
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    anchors, cls = anchor_grid(RANGE, GRID, SIZES, ROTATIONS, BOTTOMS, dtype=torch.float32, device=dev)
    A = anchors.shape[0]
    rng = np.random.default_rng(11)
    c = rng.integers(0, 3, (F, B))
    size = np.array(SIZES)[c] * rng.uniform(0.85, 1.15, (F, B, 3))
    gt = np.zeros((F, B, 8))
    gt[..., 0] = np.linspace(RANGE[0], RANGE[3], GRID[0])[rng.integers(0, GRID[0], (F, B))] + rng.uniform(-0.35, 0.35, (F, B)) * size[..., 0]
    gt[..., 1] = np.linspace(RANGE[1], RANGE[4], GRID[1])[rng.integers(0, GRID[1], (F, B))] + rng.uniform(-0.35, 0.35, (F, B)) * size[..., 1]
    gt[..., 2] = np.array(BOTTOMS)[c] + size[..., 2] / 2
    gt[..., 3:6], gt[..., 6], gt[..., 7] = size, rng.uniform(-np.pi, np.pi, (F, B)), c + 1
    gt = torch.from_numpy(gt.astype(np.float32)).to(dev)
    index_of = [(cls == k + 1).nonzero().view(-1) for k in range(3)]
    anchors_of = [anchors[at] for at in index_of]
    out_json = {"frames": F, "anchors": A, "gt": B, "steps": args.steps, "torch_steps": args.torch_steps, "device": torch.cuda.get_device_name(0), "dtype": "float32"}
    with torch.cuda.stream(s):
        bare = AnchorTargetBatch.empty(F, A, B, torch.float32, dev)
        full = AnchorTargetBatch.empty(F, A, B, torch.float32, dev, with_iou=True)
        forms = {"snowfall_aligned": snow,
                 "assign_anchors": lambda: assign_anchors(anchors, cls, gt, MATCHED, UNMATCHED, out=bare),
                 "assign_anchors_iou": lambda: assign_anchors(anchors, cls, gt, MATCHED, UNMATCHED, out=full, return_iou=True)}
        for form in forms.values():
            for _ in range(2):
                form()
        for _ in range(2):
            torch_assign(torch, anchors_of, index_of, gt, A)
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        count = full.count.cpu().numpy()
        out_json["count_mean"] = [round(float(v), 1) for v in count.mean(0)]
        # the torch form in float64 on the same values: equal labels everywhere, equal gts where argmax had no choice
        want_label, want_index = torch_assign(torch, [a.double() for a in anchors_of], index_of, gt.double(), A)
        s.synchronize()
        decided = want_index != -2
        out_json["labels_equal"] = bool(torch.equal(want_label, full.label))
        out_json["label_mismatches"] = int((want_label != full.label).sum())
        out_json["gt_index_equal_where_decided"] = bool(torch.equal(want_index[decided], full.gt_index[decided]))
        out_json["argmax_ties"] = int((~decided).sum())

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
            for _ in range(args.torch_steps):
                torch_assign(torch, anchors_of, index_of, gt, A)
            s.synchronize()
            return (time.perf_counter() - t0) * 1e3 / args.torch_steps

        runs = {k: [] for k in list(forms) + ["torch_assigner"]}
        for _ in range(args.repeats):
            for k, form in forms.items():
                runs[k].append(timed(form))
            runs["torch_assigner"].append(wall())
        out_json["ms_per_call"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        out_json["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    line = json.dumps(out_json)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fp:
            fp.write(line + "\n")
    assert out_json["labels_equal"] and out_json["gt_index_equal_where_decided"], "the torch formulation in float64 disagrees with the stage"


if __name__ == "__main__":
    main()
