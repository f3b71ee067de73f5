#!/usr/bin/env python3
"""What point-to-voxel grouping (snowgpu_voxelize_device) costs behind the stage it follows: resident float32 C2 sweeps (bench.py's
synthetic 64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process, on that call's rows and keep mask -- the voxel
stage under the two settings of the reference's detectors on DENSE,

    second    SECOND / PV-RCNN: range [0, -40, -3, 70.4, 40, 1], voxels (0.05, 0.05, 0.1), T = 5, V = 40 000
    pillars   PointPillars:     range [0, -39.68, -3, 69.12, 39.68, 1], voxels (0.16, 0.16, 4), T = 32, V = 16 000

and beside each a restatement in torch ops (floor-divide, torch.unique, scatter-min, sort: data-dependent shapes, host reads) that is
held to the same outputs.  Every device form warmed up three times, device events around `--steps` back-to-back calls, `--repeats`
times; the torch form is timed by the wall clock around `--torch-steps` synchronized calls.

    python scripts/probe/voxelize_ab.py [--frames 256] [--steps 20] [--repeats 3] [--torch-steps 3] [--only voxelize|snow]

--only names the one form to run (under rocprofv3 --kernel-trace --stats: per-kernel times of that form alone).
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

SETTINGS = {"second": ((0.0, -40.0, -3.0, 70.4, 40.0, 1.0), (0.05, 0.05, 0.1), 5, 40000),
            "pillars": ((0.0, -39.68, -3.0, 69.12, 39.68, 1.0), (0.16, 0.16, 4.0), 32, 16000)}
C = 4


def torch_voxelize(torch, rows, keep, n_per, F, rng, size, T, V):
    """The definition of include/snowgpu.h in torch ops: (voxels, coords, num_points, voxel_offsets)."""
    dev = rows.device
    r = torch.tensor(rng, dtype=torch.float64, device=dev)
    sz = torch.tensor(size, dtype=torch.float64, device=dev)
    n = torch.floor((r[3:] - r[:3]) / sz + 0.5)
    p = rows[:, :3].double()
    c = torch.floor((p - r[:3]) / sz)
    ok = keep & torch.isfinite(p).all(1) & ((c >= 0) & (c < n)).all(1)
    idx = ok.nonzero().squeeze(1)
    ci = c[idx].long()
    nx, ny, nz = (int(v) for v in n.tolist())
    f = idx // n_per
    key = ((f * nz + ci[:, 2]) * ny + ci[:, 1]) * nx + ci[:, 0]
    uniq, inv = torch.unique(key, return_inverse=True)
    first = torch.full((uniq.shape[0],), rows.shape[0], dtype=torch.int64, device=dev).scatter_reduce_(0, inv, idx, "amin")
    order = torch.argsort(first)                                  # cells by their first row: frame after frame
    place = torch.empty_like(order)
    place[order] = torch.arange(order.shape[0], device=dev)
    fu = first[order] // n_per
    per_frame = torch.bincount(fu, minlength=F)
    vnum = torch.arange(order.shape[0], device=dev) - (torch.cumsum(per_frame, 0) - per_frame)[fu]
    m = per_frame.clamp(max=V)
    voff = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    voff[1:] = torch.cumsum(m, 0)
    packed = torch.where(vnum < V, voff[:-1][fu] + vnum, torch.full_like(vnum, -1))
    pv = packed[place][inv]                                       # the packed voxel of every usable row
    sel = pv >= 0
    pvs, ridx = pv[sel], idx[sel]
    spv, perm = torch.sort(pvs, stable=True)
    total = int(voff[-1])
    counts = torch.bincount(pvs, minlength=total)
    pos = torch.arange(spv.shape[0], device=dev) - (torch.cumsum(counts, 0) - counts)[spv]
    st = pos < T
    voxels = torch.zeros((F * V, T, C), dtype=rows.dtype, device=dev)
    voxels[spv[st], pos[st]] = rows[ridx[perm][st], :C]
    num = torch.zeros(F * V, dtype=torch.int32, device=dev)
    num[:total] = counts.clamp(max=T).int()
    coords = torch.full((F * V, 4), -1, dtype=torch.int32, device=dev)
    live = packed >= 0
    cell = uniq[order][live]
    coords[packed[live]] = torch.stack((cell // (nx * ny * nz), cell // (nx * ny) % nz, cell // nx % ny, cell % nx), 1).int()
    return voxels, coords, num, voff.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=3)
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
    off = torch.arange(0, F + 1, dtype=torch.int64, device=dev) * n_per
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    bufs = {k: (torch.empty((F * V, T, C), dtype=torch.float32, device=dev), torch.empty((F * V, 4), **i32), torch.empty(F * V, **i32),
                torch.empty(F + 1, **i32)) for k, (_, _, T, V) in SETTINGS.items()}

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    def voxelize(name):
        rng, size, T, V = SETTINGS[name]
        b = bufs[name]
        return lambda: eng.ctx.voxelize_device(F, n, n_per, off.data_ptr(), out.data_ptr(), 0, rng, size, T, V, C, keep.data_ptr(), b[0].data_ptr(),
                                               b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), 0, s.cuda_stream)

    forms = {"snowfall_aligned": snow}
    forms.update({"voxelize_" + k: voxelize(k) for k in SETTINGS})
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

    res = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    with torch.cuda.stream(s):
        snow()                                                    # the rows and the mask the voxel stage reads
        for step in forms.values():
            for _ in range(3):
                step()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        res["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        res["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
        res["kept_share"] = round(float(keep.float().mean()), 4)
        for k, (rng, size, T, V) in SETTINGS.items():
            if "voxelize_" + k not in forms:
                continue
            b = bufs[k]
            res["voxels_" + k] = int(b[3][-1])
            res["frames_at_max_voxels_" + k] = int((b[3][1:] - b[3][:-1] == V).sum())
            res["stored_points_" + k] = int(b[2].sum())
            if args.only:
                continue
            want = torch_voxelize(torch, out, keep, n_per, F, rng, size, T, V)      # warm-up, and the comparison
            res["torch_ops_equal_" + k] = bool(all(torch.equal(g, w) for g, w in zip(b, want)))
            del want
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.torch_steps):
                w = torch_voxelize(torch, out, keep, n_per, F, rng, size, T, V)
                torch.cuda.synchronize()
                del w
            res["torch_ops_ms_" + k] = round((time.perf_counter() - t0) * 1e3 / args.torch_steps, 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
