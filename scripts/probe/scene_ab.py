#!/usr/bin/env python3
"""What the scene transforms (snowgpu_transform_scene_device) cost beside the streaming copy their row pass should be, beside the aligned
snowfall call in front of them, beside points_in_boxes and beside the torch formulation they replace, in one process:

    world_only        transform_scene(..., local=None) on the ALIGNED RESULT of the snowfall call on F C2 sweeps (bench.py's synthetic
                      64 x 2048 sweeps), --gt synthetic gts a frame, float32, into out=
    local_box_of      the same with the local part at T = --tries and the caller's box_of (points_in_boxes, made once)
    local_internal    the same with box_of=None: the points_in_boxes kernels run inside the call
    world_in_place    world_only with in_place=True on a copy of the rows, without the scaling (repeated in place it would carry the rows
                      beyond 1e6, where they are copied, not transformed)
    clone_floor       rows.clone() and keep.clone() of the same batch: what a pass that reads and writes every row and its keep byte once
                      costs on this device, in this process
    snowfall_aligned  the aligned snowfall call on the same F sweeps, for scale
    points_in_boxes   the label stage on the same rows and boxes
    torch_scene       the torch formulation of rows and boxes in float64: a frame-wise draw (torch.rand), the world record gathered per
                      row, the local record gathered by box_of, elementwise arithmetic in the stage's order, a cast back.  It takes the
                      stage's own records for the arithmetic, so its rows can be held to the stage's: `torch_rows_equal` is the share of
                      present rows with equal bytes (it does not run the collision sweep: it takes `state` from the stage).

The 256-frame batch repeats the 16 distinct sweeps sixteen times (the draws differ by frame position).  Device events around `--steps`
back-to-back calls; `--repeats` windows each, the forms alternating, two warm-up calls first; medians.

    python scripts/probe/scene_ab.py [--frames 16,256] [--steps 50] [--repeats 5] [--out profiles/scene_ab.jsonl]
"""
import argparse
import json
import math
import random
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

SIZES = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))
LOCAL = dict(translation=(0.25, 0.25, 0.0), rotation=(-math.pi / 20, math.pi / 20), scaling=(1.0, 1.0))


def synthetic_gt(torch, dev, F, B, seed=6):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 3, (F, B))
    gt = np.zeros((F, B, 8))
    gt[..., 0:2], gt[..., 2] = rng.uniform(-60, 60, (F, B, 2)), rng.uniform(-1.5, -0.5, (F, B))
    gt[..., 3:6], gt[..., 6], gt[..., 7] = np.array(SIZES)[cls] * rng.uniform(0.85, 1.15, (F, B, 3)), rng.uniform(-np.pi, np.pi, (F, B)), cls + 1
    gt[rng.uniform(size=(F, B)) < 0.25] = 0
    return torch.from_numpy(gt.astype(np.float32)).to(dev)


def torch_scene(torch, rows, keep, frame_of, flat_box, gt, sb):
    """Rows and boxes the torch way, float64, with the stage's records: (rows, gt_boxes)."""
    F = gt.shape[0]
    torch.rand((F, 4), device=rows.device, dtype=torch.float64)                                # the frame-wise draw a torch route makes
    w = sb.world[frame_of]
    x, y, z = (rows[:, j].double() for j in range(3))
    usable = keep & (x.abs() <= 1e6) & (y.abs() <= 1e6) & (z.abs() <= 1e6)
    if flat_box is not None:
        at = flat_box.clamp(min=0)
        lc, c0 = sb.local.reshape(-1, 8)[at], gt.reshape(-1, gt.shape[2])[at, :3].double()
        m = (flat_box >= 0) & (sb.state.reshape(-1)[at] == 1)
        sx, sy, sz = x - c0[:, 0], y - c0[:, 1], z - c0[:, 2]
        rx, ry = sx * lc[:, 3] - sy * lc[:, 4], sx * lc[:, 4] + sy * lc[:, 3]
        x = torch.where(m, (rx * lc[:, 6] + c0[:, 0]) + lc[:, 0], x)
        y = torch.where(m, (ry * lc[:, 6] + c0[:, 1]) + lc[:, 1], y)
        z = torch.where(m, (sz * lc[:, 6] + c0[:, 2]) + lc[:, 2], z)
    y, x = torch.where(w[:, 0] != 0, -y, y), torch.where(w[:, 1] != 0, -x, x)
    nx, ny = x * w[:, 2] - y * w[:, 3], x * w[:, 3] + y * w[:, 2]
    out = rows.clone()
    new = torch.stack((nx * w[:, 5], ny * w[:, 5], z * w[:, 5]), dim=1).to(rows.dtype)
    out[:, :3] = torch.where(usable[:, None], new, rows[:, :3])
    return out, sb.apply_boxes(gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="16,256")
    ap.add_argument("--gt", type=int, default=32)
    ap.add_argument("--tries", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import DeviceBatch, SceneBatch, points_in_boxes, transform_scene
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    layers, azimuths, snowfall, velocity, rscale = bench.WORKLOADS["C2"]
    tables = bench.make_tables(layers, snowfall, velocity, distinct=min(layers, 64))
    distinct, orders16 = [], []
    for f in range(16):
        distinct.append(bench.make_frame(layers, azimuths, 1000 + f, rscale).astype(np.float32))
        random.seed(1000 + f)
        o = list(range(layers))
        random.shuffle(o)
        orders16.append(o)
    n_per = distinct[0].shape[0]
    local = dict(LOCAL, tries=args.tries)
    out_json = {"rows_per_frame": n_per, "gt": args.gt, "tries": args.tries, "steps": args.steps, "device": torch.cuda.get_device_name(0), "dtype": "float32",
                "date": time.strftime("%Y-%m-%d"), "batches": {}}
    s = torch.cuda.Stream()
    for F in [int(v) for v in args.frames.split(",")]:
        plain = torch.from_numpy(np.concatenate([distinct[f % 16] for f in range(F)])).to(dev)
        n = F * n_per
        offsets = np.arange(F + 1, dtype=np.int64) * n_per
        gt = synthetic_gt(torch, dev, F, args.gt)
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        off = torch.from_numpy(offsets).to(dev)
        tids = torch.tensor([eng.table_ids_from_arrays(tables, orders16[f % 16]) for f in range(F)], dtype=torch.int32, device=dev)
        plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
        rows, keep = torch.empty_like(plain), torch.empty(n, dtype=torch.bool, device=dev)
        cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

        def snow():
            eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), plain.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                                 rows.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

        with torch.cuda.stream(s):
            snow()                                                        # rows, keep: the aligned result the stage takes
            s.synchronize()
            assert int(status[0]) == 0, status.tolist()
            batch = DeviceBatch(rows, offsets)
            labels = points_in_boxes(batch, gt, keep=keep)
            frame_of = torch.repeat_interleave(torch.arange(F, device=dev), n_per)
            flat_box = labels.flat_index()
            w_out, l_out, i_out = (SceneBatch.empty(offsets, args.gt, 8, t, torch.float32, dev) for t in (0, args.tries, args.tries))
            spare = rows.clone()
            p_out = SceneBatch.empty(offsets, args.gt, 8, 0, torch.float32, dev)
            p_out.rows = spare
            common = dict(step=step, seed=3, keep=keep)
            forms = {"world_only": lambda: transform_scene(batch, gt, out=w_out, **common),
                     "local_box_of": lambda: transform_scene(batch, gt, local=local, box_of=labels.box_of, out=l_out, **common),
                     "local_internal": lambda: transform_scene(batch, gt, local=local, out=i_out, **common),
                     "world_in_place": lambda: transform_scene(DeviceBatch(spare, offsets), gt, scaling=None, in_place=True, out=p_out, **common),
                     "clone_floor": lambda: (rows.clone(), keep.clone()),
                     "snowfall_aligned": snow,
                     "points_in_boxes": lambda: points_in_boxes(batch, gt, keep=keep, out=labels),
                     "torch_world": lambda: torch_scene(torch, rows, keep, frame_of, None, gt, w_out),
                     "torch_local": lambda: torch_scene(torch, rows, keep, frame_of, flat_box, gt, l_out)}
            for form in forms.values():
                for _ in range(2):
                    form()
            s.synchronize()
            for f in ("rows", "gt_boxes", "state", "local"):
                assert torch.equal(getattr(l_out, f).view(torch.uint8), getattr(i_out, f).view(torch.uint8)), f
            states = np.bincount(l_out.state.cpu().numpy().ravel(), minlength=3).tolist()
            rec = {"frames": F, "rows": n, "kept": int(keep.sum()), "rows_in_boxes": int((labels.box_of >= 0).sum()), "states": states}
            for name, sb, fb in (("torch_world_rows_equal", w_out, None), ("torch_local_rows_equal", l_out, flat_box)):
                mine = torch_scene(torch, rows, keep, frame_of, fb, gt, sb)[0]
                rec[name] = round(float((mine.view(torch.int32) == sb.rows.view(torch.int32)).all(dim=1)[keep].double().mean()), 6)

            def timed(form, steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(steps):
                    form()
                b.record(s)
                b.synchronize()
                return a.elapsed_time(b) / steps

            runs = {k: [] for k in forms}
            for _ in range(args.repeats):
                for k, form in forms.items():
                    runs[k].append(timed(form, max(args.steps // 10, 3) if k.startswith("torch") else args.steps))
            rec["ms_per_call"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
            med = rec["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
            rec["world_over_clone_floor"] = round(med["world_only"] / med["clone_floor"], 3)
            rec["clone_floor_gb_s"] = round(n * 42 / med["clone_floor"] / 1e6, 1)                        # 20 + 1 bytes read and written per row
        out_json["batches"][str(F)] = rec
        del plain, rows, keep, spare, w_out, l_out, i_out, p_out, batch, labels, frame_of, flat_box
        torch.cuda.empty_cache()
    line = json.dumps(out_json)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
