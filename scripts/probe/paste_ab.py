#!/usr/bin/env python3
"""What the object paste (snowgpu_paste_objects_device) costs beside the streaming copy its row pass should be, beside the aligned snowfall
call and beside the torch formulation it replaces, in one process:

    paste_objects     the stage on F C2 sweeps (bench.py's synthetic 64 x 2048 sweeps) padded with --pad absent rows each to a common
                      Nmax, a synthetic bank of --objects objects and SAMPLE_GROUPS (15, 10, 10), float32, into out=
    paste_no_source   the same without the `source` output
    clone_floor       rows.clone() and keep.clone() of the same batch: what a pass that reads and writes every row and its keep byte once
                      costs on this device, in this process
    snowfall_aligned  the aligned snowfall call on the same F sweeps (without the padding), for scale
    torch_paste       (16 frames only) the dynamic-shape formulation frame by frame: the library's boxes_iou for candidates x gts and
                      candidates x candidates, the matrices read on the host, a greedy host sweep, the rows inside the chosen boxes by torch
                      arithmetic and boolean indexing, torch.cat of the rows left and the objects' points

The 256-frame batch repeats the 16 distinct sweeps sixteen times (the draws differ by frame position).  The device forms are timed with
device events around `--steps` back-to-back calls, the torch form by the wall clock around synchronized calls (it reads on the host
anyway); `--repeats` windows each, the forms alternating, two warm-up calls first.

    python scripts/probe/paste_ab.py [--frames 16,256] [--steps 50] [--repeats 5] [--out profiles/paste_ab.jsonl]
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

GROUPS = (15, 10, 10)
SIZES = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))


def synthetic_bank(torch, dev, n_objects, seed=5):
    """n_objects boxes of the three classes within +-60 m, 30 .. 400 points inside each, sorted by class."""
    from lidar_snow_sim_amd.tensors import ObjectBank
    rng = np.random.default_rng(seed)
    cls = np.sort(rng.integers(0, 3, n_objects))
    size = np.array(SIZES)[cls] * rng.uniform(0.85, 1.15, (n_objects, 3))
    boxes = np.column_stack((rng.uniform(-60, 60, (n_objects, 2)), rng.uniform(-1.5, -0.5, n_objects), size, rng.uniform(-np.pi, np.pi, n_objects), cls + 1))
    counts = rng.integers(30, 401, n_objects)
    pts = []
    for b, n in zip(boxes, counts):
        loc = rng.uniform(-0.45, 0.45, (n, 3)) * b[3:6]
        c, s = np.cos(b[6]), np.sin(b[6])
        pts.append(np.column_stack((b[0] + loc[:, 0] * c - loc[:, 1] * s, b[1] + loc[:, 0] * s + loc[:, 1] * c, b[2] + loc[:, 2], rng.integers(1, 255, n),
                                    rng.integers(0, 64, n))))
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    return ObjectBank(torch.from_numpy(np.concatenate(pts).astype(np.float32)).to(dev), offsets, torch.from_numpy(boxes.astype(np.float32)).to(dev)), offsets


def synthetic_gt(torch, dev, F, B, seed=6):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 3, (F, B))
    gt = np.zeros((F, B, 8))
    gt[..., 0:2], gt[..., 2] = rng.uniform(-60, 60, (F, B, 2)), rng.uniform(-1.5, -0.5, (F, B))
    gt[..., 3:6], gt[..., 6], gt[..., 7] = np.array(SIZES)[cls] * rng.uniform(0.85, 1.15, (F, B, 3)), rng.uniform(-np.pi, np.pi, (F, B)), cls + 1
    gt[rng.uniform(size=(F, B)) < 0.25] = 0
    return torch.from_numpy(gt.astype(np.float32)).to(dev)


def torch_paste(torch, boxes_iou, frame, gt, bank, offsets, objects):
    """One frame the dynamic way: (rows, gt boxes) of new lengths.  objects: the candidates' bank numbers (drawn on the host)."""
    cand = bank.boxes[objects]
    hit_gt = (boxes_iou(cand[None, :, :7].contiguous(), gt[None, :, :7].contiguous(), mode="bev").iou[0] > 0).any(1).cpu().numpy()       # read on the host
    hit = (boxes_iou(cand[None, :, :7].contiguous(), cand[None, :, :7].contiguous(), mode="bev").iou[0] > 0).cpu().numpy()
    chosen = []
    for q in range(len(objects)):
        if not hit_gt[q] and not any(hit[q, p] for p in chosen):
            chosen.append(q)
    if not chosen:
        return frame, gt
    b = cand[chosen].double()
    xyz = frame[:, :3].double()
    sx, sy, sz = xyz[:, None, 0] - b[None, :, 0], xyz[:, None, 1] - b[None, :, 1], xyz[:, None, 2] - b[None, :, 2]
    c, s = torch.cos(b[:, 6])[None], torch.sin(b[:, 6])[None]
    inside = ((sz.abs() <= b[None, :, 5] / 2) & ((sx * c + sy * s).abs() < b[None, :, 3] / 2 + 1e-5) & ((sy * c - sx * s).abs() < b[None, :, 4] / 2 + 1e-5)).any(1)
    pts = [bank.points[int(offsets[objects[q]]):int(offsets[objects[q] + 1])] for q in chosen]
    return torch.cat([frame[~inside]] + pts), torch.cat((gt, cand[chosen]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="16,256")
    ap.add_argument("--pad", type=int, default=8192)
    ap.add_argument("--objects", type=int, default=120)
    ap.add_argument("--gt", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--torch-steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import DeviceBatch, PasteBatch, boxes_iou, paste_objects
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
    n_per, pad = distinct[0].shape[0], args.pad
    n_max = n_per + pad
    bank, bank_offsets = synthetic_bank(torch, dev, args.objects)
    out_json = {"pad": pad, "rows_per_frame": n_max, "bank_objects": args.objects, "bank_points": int(bank_offsets[-1]), "gt": args.gt, "groups": list(GROUPS),
                "steps": args.steps, "device": torch.cuda.get_device_name(0), "dtype": "float32", "date": time.strftime("%Y-%m-%d"), "batches": {}}
    s = torch.cuda.Stream()
    for F in [int(v) for v in args.frames.split(",")]:
        plain = torch.from_numpy(np.concatenate([distinct[f % 16] for f in range(F)])).to(dev)
        rows = torch.full((F, n_max, 5), float("nan"), dtype=torch.float32, device=dev)
        rows[:, :n_per] = plain.view(F, n_per, 5)
        rows = rows.view(F * n_max, 5)
        keep = torch.zeros((F, n_max), dtype=torch.bool, device=dev)
        keep[:, :n_per] = True
        keep = keep.view(-1)
        offsets = np.arange(F + 1, dtype=np.int64) * n_max
        batch = DeviceBatch(rows, offsets)
        gt = synthetic_gt(torch, dev, F, args.gt)
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        n = F * n_per
        off = torch.from_numpy(np.arange(F + 1, dtype=np.int64) * n_per).to(dev)
        tids = torch.tensor([eng.table_ids_from_arrays(tables, orders16[f % 16]) for f in range(F)], dtype=torch.int32, device=dev)
        plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
        out, okeep = torch.empty_like(plain), torch.empty(n, dtype=torch.bool, device=dev)
        cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

        def snow():
            eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), plain.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                                 out.data_ptr(), okeep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

        with torch.cuda.stream(s):
            full = PasteBatch.empty(offsets, args.gt, sum(GROUPS), 8, torch.float32, dev)
            bare = PasteBatch.empty(offsets, args.gt, sum(GROUPS), 8, torch.float32, dev, with_source=False)
            forms = {"paste_objects": lambda: paste_objects(batch, gt, bank, GROUPS, step=step, seed=3, keep=keep, remove_extra_width=(0.2, 0.2, 0.2), out=full),
                     "paste_no_source": lambda: paste_objects(batch, gt, bank, GROUPS, step=step, seed=3, keep=keep, remove_extra_width=(0.2, 0.2, 0.2), out=bare,
                                                              return_source=False),
                     "clone_floor": lambda: (rows.clone(), keep.clone()),
                     "snowfall_aligned": snow}
            for form in forms.values():
                for _ in range(2):
                    form()
            s.synchronize()
            assert int(status[0]) == 0, status.tolist()
            count = full.count.cpu().numpy()
            states = np.bincount(full.state.cpu().numpy().ravel(), minlength=6).tolist()
            rec = {"frames": F, "rows": F * n_max, "count_mean": [round(float(v), 1) for v in count.mean(0)], "states": states}
            assert count[:, 0].min() >= 1 and count[:, 1].sum() == int((full.source >= 0).sum())

            def timed(form, steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(steps):
                    form()
                b.record(s)
                b.synchronize()
                return a.elapsed_time(b) / steps

            objects = [np.random.default_rng(100 + f).integers(0, args.objects, sum(GROUPS)).tolist() for f in range(F)]
            frames16 = [plain[f * n_per:(f + 1) * n_per] for f in range(min(F, 16))]

            def wall():
                s.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.torch_steps):
                    for f, fr in enumerate(frames16):
                        torch_paste(torch, boxes_iou, fr, gt[f], bank, bank_offsets, objects[f])
                s.synchronize()
                return (time.perf_counter() - t0) * 1e3 / args.torch_steps

            names = list(forms) + (["torch_paste"] if F == 16 else [])
            if F == 16:
                wall()
            runs = {k: [] for k in names}
            for _ in range(args.repeats):
                for k, form in forms.items():
                    runs[k].append(timed(form, args.steps))
                if F == 16:
                    runs["torch_paste"].append(wall())
            rec["ms_per_call"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
            med = rec["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
            rec["paste_over_clone_floor"] = round(med["paste_objects"] / med["clone_floor"], 3)
            rec["clone_floor_gb_s"] = round(F * n_max * 42 / med["clone_floor"] / 1e6, 1)                 # 20 + 1 bytes read and written per row
        out_json["batches"][str(F)] = rec
        del plain, rows, keep, out, okeep, full, bare, batch
        torch.cuda.empty_cache()
    line = json.dumps(out_json)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
