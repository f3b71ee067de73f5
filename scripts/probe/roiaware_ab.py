#!/usr/bin/env python3
"""What RoI-aware voxel pooling (snowgpu_roi_voxel_pool_device) costs behind the stages it follows: resident float32 C2 sweeps (bench.py's
synthetic 64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process, on the M = 128 boxes BEV NMS kept from
clustered synthetic proposals as scripts/probe/roipool_ab.py makes them, out_size 12, T = 127, no extra width --

    roiaware_C{4,128}          the stage with max + avg (no index)
    roiaware_index             the stage with index alone (no features)
    roipool_M128_S512          roi_point_pool on the same rois: points and local
    snowfall_aligned

Beside them the same outputs from torch ops for --torch-frames frames -- the (M, N) float64 membership tensor of the definition, the
voxel of every pair, a stable sort per roi by voxel, the offsets, and the pooling slot after slot -- held to equal bytes first, then timed
by the wall clock around synchronized calls.  Every device form warmed up twice, device events around `--steps` back-to-back calls,
`--repeats` times, the forms alternating.

    python scripts/probe/roiaware_ab.py [--frames 16] [--steps 10] [--repeats 5] [--torch-frames 2] [--only roiaware|roipool|snow]
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

M, GRID, T, P, CHANNELS, S = 128, 12, 127, 8192, (4, 128), 512
IOU_THRESH = 0.7


def torch_voxels(torch, rows, keep, rois, pose, grid, max_points, cap, first):
    """(roi_count, count, index) of ONE frame in torch ops: include/snowgpu.h, step by step.  first: the frame's first global row."""
    n, dev = rows.shape[0], rows.device
    G = grid ** 3
    xyz = rows[:, :3].double()
    b = rois[:, :7].double()
    d = b[:, 3:6]
    c, s = pose[:, 0], pose[:, 1]
    ok = (b[:, :3].abs() <= 1e6).all(-1) & ((d > 0) & (d <= 1e6)).all(-1) & (b[:, 6].abs() <= 1e6) & (((c * c + s * s) - 1.0).abs() <= 1e-6)
    usable = keep & (xyz.abs() <= 1e6).all(-1)
    sx, sy, sz = (xyz[None, :, k] - b[:, None, k] for k in range(3))
    lx = sx * c[:, None] + sy * s[:, None]
    ly = sy * c[:, None] - sx * s[:, None]
    hx, hy, hz = d[:, 0] * 0.5 + 1e-5, d[:, 1] * 0.5 + 1e-5, d[:, 2] * 0.5
    inside = (sz.abs() <= hz[:, None]) & (lx.abs() < hx[:, None]) & (ly.abs() < hy[:, None]) & ok[:, None] & usable[None]
    roi_count = inside.sum(1)
    listed = inside & (inside.cumsum(1) <= cap)

    def axis(l, size):
        u = torch.floor((l + (size * 0.5)[:, None]) / (size / grid)[:, None])
        return torch.where(u >= 0, torch.where(u >= grid, grid - 1.0, u), 0.0).long()        # (NaN: 0)

    vox = (axis(lx, d[:, 0]) * grid + axis(ly, d[:, 1])) * grid + axis(sz, d[:, 2])
    key = torch.where(listed, vox, G)
    order = torch.argsort(key, dim=1, stable=True)                                           # row order within a voxel
    count = torch.zeros((rois.shape[0], G + 1), dtype=torch.int64, device=dev).scatter_add_(1, key, torch.ones_like(key))[:, :G]
    start = count.cumsum(1) - count
    slot = torch.arange(max_points, device=dev)
    at = torch.gather(order, 1, (start[:, :, None] + slot).clamp(max=n - 1).view(rois.shape[0], -1)).view(rois.shape[0], G, max_points)
    index = torch.where(slot < count[:, :, None], at + first, -1)
    return roi_count.int(), count.int(), index.int()


def torch_pool(torch, index, feats):
    """(max, argmax, avg) (..., Cf) from index (..., T) in torch ops, slot after slot: pcdet's loop and the float32 sum in row order."""
    shape = index.shape[:-1] + (feats.shape[1],)
    best, total = torch.zeros(shape, device=feats.device), torch.zeros(shape, device=feats.device)
    arg = torch.full(shape, -1, dtype=torch.int32, device=feats.device)
    for t in range(index.shape[-1]):
        at = index[..., t].long()
        has = (at >= 0)[..., None]
        x = feats[at.clamp(min=0)]
        wins = has & (((arg < 0) & ~torch.isnan(x)) | (x > best))
        best, arg = torch.where(wins, x, best), torch.where(wins, index[..., t, None].expand(shape), arg)
        total = total + torch.where(has, x, 0.0)
    n = (index >= 0).sum(-1)
    return torch.where(arg >= 0, best, 0.0), arg, torch.where(n[..., None] > 0, total / n.clamp(min=1)[..., None].float(), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import DeviceBatch, NmsBatch, RoiPointBatch, RoiVoxelBatch, nms, roi_point_pool, roi_voxel_pool
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F, TF = args.frames, min(args.torch_frames, args.frames)
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
    offsets = np.arange(F + 1, dtype=np.int64) * n_per
    off = torch.from_numpy(offsets).to(dev)
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    out_json = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0), "n_rois": M, "out_size": GRID,
                "max_points": T, "roi_capacity": P, "torch_frames": TF}
    with torch.cuda.stream(s):
        snow()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        B = 4096                                                          # clustered proposals about kept rows of their frame (roipool_ab.py)
        Cn = B // 16
        at = torch.multinomial(keep.view(F, n_per).float(), Cn, replacement=False, generator=g) + (torch.arange(F, device=dev) * n_per)[:, None]
        u = torch.rand((F, Cn, 4), device=dev, generator=g)
        cen = torch.zeros((F, Cn, 7), device=dev)
        cen[:, :, :3] = out[at.reshape(-1), :3].view(F, Cn, 3)
        cen[:, :, 3], cen[:, :, 4], cen[:, :, 5] = 3.5 + 1.5 * u[:, :, 0], 1.6 + 0.5 * u[:, :, 1], 1.4 + 0.6 * u[:, :, 2]
        cen[:, :, 6] = (2 * u[:, :, 3] - 1) * np.pi
        of = torch.randint(0, Cn, (F, B), device=dev, generator=g)
        props = torch.gather(cen, 1, of[:, :, None].expand(F, B, 7)).clone()
        props[:, :, :2] += 0.4 * torch.randn((F, B, 2), device=dev, generator=g)
        props[:, :, 3:6] *= 0.92 + 0.16 * torch.rand((F, B, 3), device=dev, generator=g)
        props[:, :, 6] += 0.1 * torch.randn((F, B), device=dev, generator=g)
        props, scores = props.contiguous(), torch.rand((F, B), device=dev, generator=g)
        rois = nms(props, scores, IOU_THRESH, post_max=M, out=NmsBatch.empty(F, B, M, 7, torch.float32, dev))
        batch = DeviceBatch(out, offsets)
        feats = {Cf: torch.randn((n, Cf), device=dev, generator=g) for Cf in CHANNELS}
        pooled = {Cf: RoiVoxelBatch.empty(F, M, GRID, T, Cf, dev) for Cf in CHANNELS}
        listed = RoiVoxelBatch.empty(F, M, GRID, T, None, dev, with_index=True)
        points = RoiPointBatch.empty(F, M, S, 4, torch.float32, dev, with_local=True)

        forms = {"snowfall_aligned": snow}
        for Cf in CHANNELS:
            forms[f"roiaware_C{Cf}"] = (lambda Cf=Cf: roi_voxel_pool(batch, rois, GRID, T, feats[Cf], roi_capacity=P, keep=keep, out=pooled[Cf]))
        forms["roiaware_index"] = lambda: roi_voxel_pool(batch, rois, GRID, T, roi_capacity=P, keep=keep, return_index=True, out=listed)
        forms[f"roipool_M{M}_S{S}"] = lambda: roi_point_pool(batch, rois, S, keep=keep, num_features=4, out=points, return_local=True)
        if args.only:
            forms = {k: v for k, v in forms.items() if k.startswith(args.only)}
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()

        def timed(step):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(args.steps):
                step()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b) / args.steps

        if not args.only:                                                 # what the rois are like, then the torch restatement: equal bytes first
            r = rois.boxes
            pose = torch.stack((torch.cos(r[..., 6].double()), torch.sin(r[..., 6].double())), -1).contiguous()
            Cf = CHANNELS[0]
            got = roi_voxel_pool(batch, r, GRID, T, feats[Cf], roi_capacity=P, pose=pose, keep=keep, return_index=True)
            s.synchronize()
            count, vox = got.roi_count.float(), got.count
            out_json["kept"] = round(float(rois.count.float().mean()), 1)
            out_json["members"] = {"mean": round(float(count.mean()), 1), "max": int(count.max()), "empty_share": round(float((count == 0).float().mean()), 4),
                                   "above_capacity_share": round(float((count > P).float().mean()), 4)}
            out_json["voxels"] = {"nonempty_share": round(float((vox > 0).float().mean()), 4), "max": int(vox.max()),
                                  "above_T_share": round(float((vox > T).float().mean()), 6)}

            def restated(nf):
                parts = [torch_voxels(torch, out[f * n_per:(f + 1) * n_per], keep[f * n_per:(f + 1) * n_per], r[f], pose[f], GRID, T, P, f * n_per) for f in range(nf)]
                roi_count, count, index = (torch.stack(x) for x in zip(*parts))
                return (roi_count, count, index) + torch_pool(torch, index, feats[Cf])

            want = restated(TF)
            s.synchronize()
            names = ("roi_count", "count", "index", "max", "argmax", "avg")
            same = {k: bool(torch.equal(getattr(got, k)[:TF].contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))) for k, y in zip(names, want)}
            assert all(same.values()), same
            out_json["torch_equal"] = same
            del want
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                restated(TF)
                torch.cuda.synchronize()
            out_json[f"torch_ms_C{Cf}_first_frames"] = round((time.perf_counter() - t0) * 1e3 / 2, 1)
            del got
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        out_json["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        out_json["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(out_json), flush=True)


if __name__ == "__main__":
    main()
