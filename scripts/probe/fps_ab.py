#!/usr/bin/env python3
"""What farthest point sampling (snowgpu_fps_device) costs behind the stage it follows: resident float32 C2 sweeps (bench.py's synthetic
64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process, on that call's rows and keep mask -- the keypoint stage
under SECOND's range [0, -40, -3, 70.4, 40, 1] with K = 2048 and K = 4096 samples per frame,

    all     the keep mask of the snowfall call alone
    fov     that mask ANDed with a camera-view mask (snowgpu_fov_mask_device) in front: some three quarters of the rows absent
    fov4    every fourth row of `fov`: frames small enough for the register tiers (csrc/sg_fps.h)

for the whole batch and for ONE frame alone (a lone frame runs on one compute unit), and beside the K = 2048 forms a restatement of the
same walk in torch ops on the padded F x M tensor (subtract, multiply, add, minimum, argmax, gather per round: 10 000s of launches) that
is held to the same index and dist before either is timed.  Every device form warmed up twice, device events around `--steps`
back-to-back calls, `--repeats` times; the torch form is timed by the wall clock around `--torch-steps` synchronized calls.

    python scripts/probe/fps_ab.py [--frames 256] [--steps 3] [--repeats 3] [--torch-steps 1] [--only fps|snow]

--only names the one form to run (under rocprofv3 --kernel-trace --stats: per-kernel times of that form alone); it skips the torch form.
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

RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
C = 4


def torch_fps(torch, rows, keep, F, M, K, rng):
    """The walk of include/snowgpu.h in torch ops on the F x M tensor: (index F x K into the batch, dist F x K, usable F)."""
    dev = rows.device
    p = rows.view(F, M, 5)
    x, y, z = p[:, :, 0].contiguous(), p[:, :, 1].contiguous(), p[:, :, 2].contiguous()
    ok = keep.view(F, M).clone()
    for j, c in enumerate((x, y, z)):
        d = c.double()
        ok &= (d.abs() <= 1e6) & (d >= rng[j]) & (d < rng[3 + j])
    m = ok.sum(1).int()
    some = m > 0
    t = torch.where(ok, torch.full_like(x, float("inf")), torch.full_like(x, -1.0))
    index = torch.empty((F, K), dtype=torch.int64, device=dev)
    dist = torch.empty((F, K), dtype=rows.dtype, device=dev)
    s = torch.argmax(ok.to(torch.uint8), 1, keepdim=True)                # the first usable row
    index[:, 0:1] = s
    dist[:, 0] = float("inf")
    for j in range(1, K):
        dx, dy, dz = x - torch.gather(x, 1, s), y - torch.gather(y, 1, s), z - torch.gather(z, 1, s)
        t = torch.where(ok, torch.minimum(t, ((dx * dx) + (dy * dy)) + (dz * dz)), t)
        s = torch.argmax(t, 1, keepdim=True)
        index[:, j:j + 1] = s
        dist[:, j:j + 1] = torch.gather(t, 1, s)
    index += torch.arange(F, device=dev)[:, None] * M
    index[~some] = -1
    dist[~some] = -1.0
    return index.int(), dist, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=1)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.calibration import Calibration
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F = args.frames
    layers, azimuths, snowfall, velocity, rscale = bench.WORKLOADS["C2"]
    tables = bench.make_tables(layers, snowfall, velocity, distinct=min(layers, 64))
    cal = Calibration(P2=np.array([[700.0, 0, 960, 0], [0, 700.0, 512, 0], [0, 0, 1, 0]]), R0=np.eye(3),
                      V2C=np.array([[0, -1.0, 0, 0], [0, 0, -1.0, 0], [1.0, 0, 0, 0]]))
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
    off = torch.arange(0, F + 1, dtype=torch.int64, device=dev) * n_per
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    keep_fov = torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    keep_fov4 = torch.empty(n, dtype=torch.bool, device=dev)
    masks = {"all": keep, "fov": keep_fov, "fov4": keep_fov4}
    shapes = [(F, 2048), (F, 4096), (1, 2048)]
    bufs = {(nf, K): (torch.empty((nf, K), dtype=torch.int32, device=dev), torch.empty((nf, K, C), dtype=torch.float32, device=dev),
                      torch.empty((nf, K), dtype=torch.float32, device=dev), torch.empty(nf, dtype=torch.int32, device=dev)) for nf, K in shapes}

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    def fps(nf, K, mask):
        b = bufs[(nf, K)]
        return lambda: eng.ctx.fps_device(nf, nf * n_per, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, C, masks[mask].data_ptr(), b[0].data_ptr(),
                                          b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), s.cuda_stream)

    forms = {"snowfall_aligned": snow}
    forms.update({f"fps_{mask}_{'batch' if nf == F else 'one_frame'}_k{K}": fps(nf, K, mask) for mask in masks for nf, K in shapes})
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

    res = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0), "range": RANGE}
    with torch.cuda.stream(s):
        snow()                                                    # the rows and the mask the keypoint stage reads
        eng.ctx.fov_mask_device(n, out.data_ptr(), 0, cal, (1024, 1920), keep.data_ptr(), keep_fov.data_ptr(), s.cuda_stream)
        keep_fov4.copy_(keep_fov & (torch.arange(n, device=dev) % 4 == 0))
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        res["kept_share"] = {k: round(float(v.float().mean()), 4) for k, v in masks.items()}
        if not args.only:
            # the torch restatement: equal outputs first, then its time
            for mask in masks:
                if mask == "fov4":                                # (timed, and counted below; not walked once more in torch ops)
                    fps(F, 2048, mask)()
                    s.synchronize()
                    b = bufs[(F, 2048)]
                    res["usable_per_frame_" + mask] = {"min": int(b[3].min()), "median": int(b[3].median()), "max": int(b[3].max())}
                    continue
                step = fps(F, 2048, mask)
                step()
                s.synchronize()
                b = bufs[(F, 2048)]
                res["usable_per_frame_" + mask] = {"min": int(b[3].min()), "median": int(b[3].median()), "max": int(b[3].max())}
                want = torch_fps(torch, out, masks[mask], F, n_per, 2048, RANGE)
                res["torch_ops_equal_" + mask] = bool(torch.equal(b[0], want[0]) and torch.equal(b[2], want[1]) and torch.equal(b[3], want[2])
                                                      and torch.equal(b[1], out[b[0].long().clamp(min=0)][:, :, :C] * (b[0] >= 0)[:, :, None]))
                del want
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.torch_steps):
                    w = torch_fps(torch, out, masks[mask], F, n_per, 2048, RANGE)
                    torch.cuda.synchronize()
                    del w
                res["torch_ops_ms_k2048_" + mask] = round((time.perf_counter() - t0) * 1e3 / args.torch_steps, 1)
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        res["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        res["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
        res["us_per_round"] = {k: round(float(np.median(v)) * 1e3 / int(k.rsplit("_k", 1)[1]), 3) for k, v in runs.items() if k.startswith("fps_")}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
