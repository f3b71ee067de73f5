#!/usr/bin/env python3
"""What the centre heatmap targets (snowgpu_assign_centers_device) cost beside the write of their heatmap, beside the torch formulation they
replace, beside anchor target assignment and beside the aligned snowfall call, in one process.  Per configuration -- F frames of B
synthetic gts, float32, on KITTI CenterPoint's map (176 x 200, 3 classes, stride 8 of 0.05 m voxels) and on a 468 x 468 x 3 map (stride 4
of 0.08 m voxels over 150 m) --:

    assign_centers     the stage into out=, one head, max_objs 500
    zeros              torch.zeros of the heatmap's shape: the time to write it once
    pcdet_form         pcdet's assign_target_of_single_head as recalled, on the GPU: per frame and gt the radius in float32 tensors and its
                       .item(), the centre read on the host, the Gaussian built in NumPy and uploaded, torch.max(..., out=slice)
    assign_anchors     the anchor stage on SECOND's KITTI head (A = 211 200) against the same number of gts, for scale
    snowfall_aligned   the aligned snowfall call on 16 C2 sweeps (bench.py's synthetic 64 x 2048 sweeps), for scale; once, whatever F

The heatmap of pcdet_form is compared with the stage's: float32 arithmetic against float64, so the last bits differ and a radius may differ
by one at a truncation; the largest difference over the pixels of the gts whose radius agrees is reported.  The device forms are timed
with device events around `--steps` back-to-back calls, pcdet_form by the wall clock around synchronized calls (it reads on the host
anyway); `--repeats` windows each, the forms alternating, two warm-up calls first.

    python scripts/probe/centers_ab.py [--frames 16 256] [--gt 64] [--steps 100] [--repeats 5] [--out profiles/centers_ab.jsonl]
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

MAPS = {"kitti_176x200": dict(point_cloud_range=(0.0, -40.0, -3.0, 70.4, 40.0, 1.0), voxel_size=(0.05, 0.05, 0.1), stride=8, feature_map_size=(176, 200)),
        "468x468": dict(point_cloud_range=(-74.88, -74.88, -2.0, 74.88, 74.88, 4.0), voxel_size=(0.08, 0.08, 0.15), stride=4, feature_map_size=(468, 468))}
SIZES = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))
A_RANGE, A_GRID, A_ROT, A_BOTTOMS = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0), (176, 200), (0.0, np.pi / 2), (-1.78, -0.6, -0.6)
OVERLAP, MIN_RADIUS, MAX_OBJS = 0.1, 2, 500


def make_gts(rng, F, B, rng6):
    c = rng.integers(0, 3, (F, B))
    size = np.array(SIZES)[c] * rng.uniform(0.85, 1.15, (F, B, 3))
    gt = np.zeros((F, B, 8))
    gt[..., 0], gt[..., 1] = rng.uniform(rng6[0], rng6[3], (F, B)), rng.uniform(rng6[1], rng6[4], (F, B))
    gt[..., 2], gt[..., 3:6], gt[..., 6], gt[..., 7] = -1.0, size, rng.uniform(-np.pi, np.pi, (F, B)), c + 1
    return gt.astype(np.float32)


def gaussian2d(radius):
    d = 2 * radius + 1
    y, x = np.ogrid[-radius:radius + 1, -radius:radius + 1]
    h = np.exp(-(x * x + y * y) / (2 * (d / 6) ** 2))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    return h


def pcdet_form(torch, gt, cfg):
    """(heatmap (F, 3, H, W), radius (F, B)) the way pcdet's CenterHead makes them, as recalled: float32 tensors, host reads per gt."""
    W, H = cfg["feature_map_size"]
    F, B = gt.shape[:2]
    x0, y0 = cfg["point_cloud_range"][:2]
    vx, vy, stride = cfg["voxel_size"][0], cfg["voxel_size"][1], cfg["stride"]
    heat = gt.new_zeros((F, 3, H, W))
    radii = np.zeros((F, B), np.int32)
    for f in range(F):
        boxes = gt[f]
        coord_x, coord_y = (boxes[:, 0] - x0) / vx / stride, (boxes[:, 1] - y0) / vy / stride
        coord_x, coord_y = torch.clamp(coord_x, min=0, max=W - 0.5), torch.clamp(coord_y, min=0, max=H - 0.5)
        center_int = torch.stack((coord_x, coord_y), dim=-1).int()
        h, w = boxes[:, 3] / vx / stride, boxes[:, 4] / vy / stride
        b1, c1 = h + w, w * h * (1 - OVERLAP) / (1 + OVERLAP)
        r1 = (b1 + torch.sqrt(b1 ** 2 - 4 * c1)) / 2
        b2, c2 = 2 * (h + w), (1 - OVERLAP) * w * h
        r2 = (b2 + torch.sqrt(b2 ** 2 - 16 * c2)) / 2
        b3, c3 = -2 * OVERLAP * (h + w), (OVERLAP - 1) * w * h
        r3 = (b3 + torch.sqrt(b3 ** 2 - 16 * OVERLAP * c3)) / 2
        radius = torch.clamp_min(torch.min(torch.min(r1, r2), r3).int(), min=MIN_RADIUS)
        for k in range(B):
            if boxes[k, 3] <= 0 or boxes[k, 4] <= 0:                            # (a host read)
                continue
            r = int(radius[k].item())
            x, y = int(center_int[k, 0]), int(center_int[k, 1])
            radii[f, k] = r
            g = torch.from_numpy(gaussian2d(r)).to(gt.device).float()
            left, right, top, bottom = min(x, r), min(W - x, r + 1), min(y, r), min(H - y, r + 1)
            cls = int(boxes[k, 7].item()) - 1
            masked = heat[f, cls, y - top:y + bottom, x - left:x + right]
            torch.max(masked, g[r - top:r + bottom, r - left:r + right], out=masked)
    return heat, radii


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--gt", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import AnchorTargetBatch, CenterTargetBatch, anchor_grid, assign_anchors, assign_centers
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    B = args.gt
    s = torch.cuda.Stream()

    # the aligned snowfall call on 16 sweeps, as scripts/probe/anchors_ab.py sets it up
    SF = 16
    layers, azimuths, snowfall, velocity, rscale = bench.WORKLOADS["C2"]
    tables = bench.make_tables(layers, snowfall, velocity, distinct=min(layers, 64))
    frames, orders = [], []
    for f in range(SF):
        frames.append(bench.make_frame(layers, azimuths, 1000 + f, rscale))
        random.seed(1000 + f)
        o = list(range(layers))
        random.shuffle(o)
        orders.append(o)
    n_per = frames[0].shape[0]
    n = SF * n_per
    rows = torch.from_numpy(np.concatenate(frames)).to(dev)
    del frames
    off = torch.from_numpy(np.arange(SF + 1, dtype=np.int64) * n_per).to(dev)
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * SF, dtype=torch.float64, device=dev)
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(SF, dtype=torch.int64, device=dev), torch.zeros(SF, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def snow():
        eng.ctx.augment_batch_device_aligned(SF, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    anchors, acls = anchor_grid(A_RANGE, A_GRID, SIZES, A_ROT, A_BOTTOMS, dtype=torch.float32, device=dev)
    A = anchors.shape[0]

    def timed(form, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(steps):
            form()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b) / steps

    lines = []
    with torch.cuda.stream(s):
        for _ in range(2):
            snow()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        snow_ms = [timed(snow, args.steps) for _ in range(args.repeats)]
        for F in args.frames:
            steps = max(args.steps * 16 // F, 10)
            targets = AnchorTargetBatch.empty(F, A, B, torch.float32, dev)
            for name, cfg in MAPS.items():
                W, H = cfg["feature_map_size"]
                gt_np = make_gts(np.random.default_rng(11), F, B, cfg["point_cloud_range"])
                gt = torch.from_numpy(gt_np).to(dev)
                buf = CenterTargetBatch.empty(F, B, 3, 1, MAX_OBJS, (W, H), torch.float32, dev)
                forms = {"assign_centers": lambda: assign_centers(gt, **cfg, max_objs=MAX_OBJS, gaussian_overlap=OVERLAP, min_radius=MIN_RADIUS, out=buf),
                         "zeros": lambda: torch.zeros((F, 3, H, W), dtype=torch.float32, device=dev),
                         "assign_anchors": lambda: assign_anchors(anchors, acls, gt, out=targets)}
                for form in forms.values():
                    for _ in range(2):
                        form()
                for _ in range(2):
                    heat, radii = pcdet_form(torch, gt, cfg)
                s.synchronize()
                # pcdet's form in float32 against the stage: the radii, and the heat under the gts whose radius agrees
                mine = np.zeros((F, B), np.int32)
                gi, rad = buf.gt_index[:, 0].cpu().numpy(), buf.radius[:, 0].cpu().numpy()
                for f in range(F):
                    mine[f, gi[f][gi[f] >= 0]] = rad[f][gi[f] >= 0]
                agree = bool((mine == radii).all())
                diff = float((heat - buf.heatmap).abs().max()) if agree else None
                runs = {k: [] for k in list(forms) + ["pcdet_form"]}
                for _ in range(args.repeats):
                    for k, form in forms.items():
                        runs[k].append(timed(form, steps))
                    s.synchronize()
                    t0 = time.perf_counter()
                    pcdet_form(torch, gt, cfg)
                    s.synchronize()
                    runs["pcdet_form"].append((time.perf_counter() - t0) * 1e3)
                runs["snowfall_aligned_16"] = snow_ms
                line = {"map": name, "frames": F, "gt": B, "classes": 3, "heads": 1, "max_objs": MAX_OBJS, "dtype": "float32", "steps": steps, "anchors": A,
                        "device": torch.cuda.get_device_name(0), "heatmap_MB": round(F * 3 * H * W * 4 / 1e6, 1), "drawn": int(buf.mask.sum()),
                        "mean_radius": round(float(rad[gi >= 0].mean()), 2), "radii_differing_from_pcdet_form": int((mine != radii).sum()),
                        "heat_max_abs_diff_to_pcdet_form": diff, "ms_per_call": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                        "median_ms": {k: round(float(np.median(v)), 4) for k, v in runs.items()}}
                print(json.dumps(line), flush=True)
                lines.append(line)
                del buf, heat
            del targets
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fp:
            for line in lines:
                fp.write(json.dumps(line) + "\n")
    for line in lines:
        d = line["heat_max_abs_diff_to_pcdet_form"]
        assert d is None or d < 1e-5, "pcdet's formulation in float32 disagrees with the stage by more than float32 rounding"


if __name__ == "__main__":
    main()
