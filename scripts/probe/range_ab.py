#!/usr/bin/env python3
"""What the range image (snowgpu_range_image_device) costs behind the stage it follows: resident float32 C2 sweeps (bench.py's synthetic
64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process, on that call's rows and keep mask -- the projection to
64 x 2048 with num_features = 4,

    elevation   image rows from the pitch between fov_down = -25 and fov_up = 3 degrees
    ring        image rows from the input's column 4 (int32, one per row)

each without and with the per-pixel count.  Beside them
  * a torch route to the same image and index, FED OUR pixel_of: the range in float64, packed int64 keys bits(r) << 32 | row,
    scatter_reduce(amin), a decode and gathers -- held to the same bytes before either is timed;
  * torch's own float64 trigonometry to pixel_of (atan2, sqrt, floor, clamp), timed, with the number of rows whose pixel differs from ours.
Every form warmed up twice, device events around `--steps` back-to-back calls, `--repeats` times, medians reported.

    python scripts/probe/range_ab.py [--frames 256] [--steps 3] [--repeats 3] [--only range|snow|torch]

--only names the forms to run (under rocprofv3 --kernel-trace --stats: per-kernel times of those forms alone).
"""
import argparse
import json
import math
import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

H, W, C = 64, 2048, 4
FOV = (3.0, -25.0)
BIG = (1 << 63) - 1


def torch_image(torch, rows, pixel_of, F):
    """(image F x (1 + C) x H x W, index F x H x W) from the rows and OUR pixel_of, in torch ops."""
    n = rows.shape[0]
    x, y, z = rows[:, 0].double(), rows[:, 1].double(), rows[:, 2].double()
    r = ((x * x + y * y) + z * z).sqrt().float()
    key = (r.view(torch.int32).long() << 32) | torch.arange(n, dtype=torch.int64, device=rows.device)
    key = torch.where(pixel_of >= 0, key, BIG)
    best = torch.full((F * H * W,), BIG, dtype=torch.int64, device=rows.device).scatter_reduce(0, pixel_of.clamp(min=0).long(), key, "amin")
    empty = best == BIG
    index = torch.where(empty, -1, best & 0xffffffff).int()
    rr = torch.where(empty, -1.0, (best >> 32).int().view(torch.float32))
    cols = torch.where(empty[:, None], -1.0, rows[index.clamp(min=0).long(), :C])
    image = torch.cat((rr.view(F, 1, H * W), cols.view(F, H * W, C).permute(0, 2, 1)), dim=1).reshape(F, 1 + C, H, W).contiguous()
    return image, index.view(F, H, W)


def torch_pixels(torch, rows, keep, n_per, ring=None):
    """pixel_of from torch's own float64 trigonometry (image rows by elevation, or the ring's)."""
    n = rows.shape[0]
    x, y, z = rows[:, 0].double(), rows[:, 1].double(), rows[:, 2].double()
    r = ((x * x + y * y) + z * z).sqrt().float()
    ok = keep & (x.abs() <= 1e6) & (y.abs() <= 1e6) & (z.abs() <= 1e6) & (r > 0)
    yaw = -torch.atan2(y, x)
    col = ((0.5 * (yaw / math.pi + 1.0)) * W).floor().clamp(0, W - 1).long()
    if ring is None:
        fu, fd = (float(v) for v in np.radians(np.array(FOV)))
        pitch = torch.atan2(z, (x * x + y * y).sqrt())
        row = ((1.0 - (pitch - fd) / (fu - fd)) * H).floor().clamp(0, H - 1).long()
    else:
        row = ring.long()
        ok &= (row >= 0) & (row < H)
    f = torch.arange(n, dtype=torch.int64, device=rows.device) // n_per
    return torch.where(ok, f * (H * W) + row * W + col, -1).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F = args.frames
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
    ring = rows[:, 4].int().contiguous()                            # the input's channel: a scattered row keeps it
    off = torch.arange(0, F + 1, dtype=torch.int64, device=dev) * n_per
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    image = torch.empty((F, 1 + C, H, W), dtype=torch.float32, device=dev)
    index, count = torch.empty((F, H, W), dtype=torch.int32, device=dev), torch.empty((F, H, W), dtype=torch.int32, device=dev)
    pixel_of = torch.empty(n, dtype=torch.int32, device=dev)
    fov = np.radians(np.array(FOV, np.float64))

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    def project(by_ring, with_count):
        return lambda: eng.ctx.range_image_device(F, n, n_per, off.data_ptr(), out.data_ptr(), 0, H, W, None if by_ring else fov, ring.data_ptr() if by_ring else 0,
                                                  None, C, keep.data_ptr(), image.data_ptr(), index.data_ptr(), pixel_of.data_ptr(),
                                                  count.data_ptr() if with_count else 0, s.cuda_stream)

    modes = {"elevation": False, "ring": True}
    forms = {"snowfall_aligned": snow}
    forms.update({f"range_{m}{'_count' if c else ''}": project(b, c) for m, b in modes.items() for c in (False, True)})
    ours = {}
    forms.update({f"torch_image_from_our_pixel_of_{m}": (lambda m=m: torch_image(torch, out, ours[m], F)) for m in modes})
    forms.update({f"torch_pixels_float64_trig_{m}": (lambda b=b: torch_pixels(torch, out, keep, n_per, ring if b else None)) for m, b in modes.items()})
    if args.only:
        forms = {k: v for k, v in forms.items() if k.startswith(args.only)}

    def timed(step):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(args.steps):
            step()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    res = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0), "height": H, "width": W, "fov_deg": FOV,
           "num_features": C, "scratch_bytes": 8 * F * H * W}
    with torch.cuda.stream(s):
        snow()                                                    # the rows and the mask the projection reads
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        res["kept_share"] = round(float(keep.float().mean()), 4)
        for m, b in modes.items():
            project(b, True)()
            ours[m] = pixel_of.clone()
            s.synchronize()
            res[f"filled_pixels_{m}"] = round(float((index >= 0).float().mean()), 4)
            res[f"rows_per_filled_pixel_{m}"] = round(float(count.sum()) / max(1, int((index >= 0).sum())), 3)
            res[f"pixels_with_several_rows_{m}"] = int((count > 1).sum())
            if not args.only or args.only.startswith("torch"):
                t_image, t_index = torch_image(torch, out, ours[m], F)
                res[f"torch_image_equal_{m}"] = bool(torch.equal(t_image.view(torch.int32), image.view(torch.int32)) and torch.equal(t_index, index))
                del t_image, t_index
                theirs = torch_pixels(torch, out, keep, n_per, ring if b else None)
                res[f"torch_trig_rows_with_another_pixel_{m}"] = int((theirs != ours[m]).sum())
                del theirs
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        res["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        res["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
