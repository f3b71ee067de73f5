#!/usr/bin/env python3
"""What RoI point pooling (snowgpu_roi_point_pool_device) costs behind the stages it follows: resident float32 C2 sweeps (bench.py's
synthetic 64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process --

    roipool_M{128,512}_S512[_index]    the stage on the boxes NMS kept (post_max 128 / 512) from clustered synthetic proposals as
                                       scripts/probe/iou_ab.py makes them, extra width 0.2 m, C = 4, points and local (_index: index and
                                       count alone)
    pib_B128                           points_in_boxes on the 128 kept boxes
    snowfall_aligned

Beside them the same outputs from torch ops for --torch-frames frames -- the (M, N) float64 membership tensor of the definition, a sort
per roi, the modulo fill and the gathers -- held to equal bytes first, then timed by the wall clock around synchronized calls.  Every
device form warmed up twice, device events around `--steps` back-to-back calls, `--repeats` times, the forms alternating.

    python scripts/probe/roipool_ab.py [--frames 16] [--steps 20] [--repeats 5] [--torch-frames 2] [--only roipool|pib|snow]
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

SIZES, S, C, EW = (128, 512), 512, 4, 0.2
IOU_THRESH = 0.7


def torch_pool(torch, rows, keep, rois, pose, ew, n_samples, n_features, first):
    """(index, count, points, local) of ONE frame in torch ops: include/snowgpu.h, step by step.  first: the frame's first global row."""
    n, M, dev = rows.shape[0], rois.shape[0], rows.device
    xyz = rows[:, :3].double()
    b = rois[:, :7].double()
    d = b[:, 3:6] + ew
    c, s = pose[:, 0], pose[:, 1]
    ok = ((b[:, :3].abs() <= 1e6).all(-1) & ((d > 0) & (d <= 1e6)).all(-1) & (b[:, 6].abs() <= 1e6) & (((c * c + s * s) - 1.0).abs() <= 1e-6) &
          (b[:, 3:6] > 0).all(-1))
    usable = keep & (xyz.abs() <= 1e6).all(-1)
    sx, sy, sz = (xyz[None, :, k] - b[:, None, k] for k in range(3))
    lx = sx * c[:, None] + sy * s[:, None]
    ly = sy * c[:, None] - sx * s[:, None]
    hx, hy, hz = d[:, 0] * 0.5 + 1e-5, d[:, 1] * 0.5 + 1e-5, d[:, 2] * 0.5
    inside = (sz.abs() <= hz[:, None]) & (lx.abs() < hx[:, None]) & (ly.abs() < hy[:, None]) & ok[:, None] & usable[None]
    cnt = inside.sum(1)
    ar = torch.arange(n, device=dev)
    order = torch.where(inside, ar[None], n).sort(1).values[:, :n_samples]
    if order.shape[1] < n_samples:
        order = torch.nn.functional.pad(order, (0, n_samples - order.shape[1]), value=n)
    j = torch.arange(n_samples, device=dev)[None] % cnt.clamp(min=1)[:, None]
    at = torch.gather(order, 1, j)
    has = (cnt > 0)[:, None].expand(M, n_samples)
    safe = torch.where(has, at, 0)
    m = torch.arange(M, device=dev)[:, None].expand(M, n_samples)
    points = torch.where(has[..., None], rows[safe][..., :n_features], 0.0)
    local = torch.where(has[..., None], torch.stack((lx[m, safe], ly[m, safe], sz[m, safe]), -1).to(rows.dtype), 0.0)
    return torch.where(has, at + first, -1).int(), cnt.int(), points, local


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import BoxLabelBatch, DeviceBatch, NmsBatch, RoiPointBatch, nms, points_in_boxes, roi_point_pool
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

    out_json = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0), "n_samples": S, "num_features": C,
                "extra_width": EW, "torch_frames": TF}
    with torch.cuda.stream(s):
        snow()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        B = 4096                                                          # clustered proposals about kept rows of their frame (iou_ab.py)
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
        rois = {M: nms(props, scores, IOU_THRESH, post_max=M, out=NmsBatch.empty(F, B, M, 7, torch.float32, dev)) for M in SIZES}
        batch = DeviceBatch(out, offsets)
        full = {M: RoiPointBatch.empty(F, M, S, C, torch.float32, dev, with_local=True) for M in SIZES}
        bare = {M: RoiPointBatch.empty(F, M, S, C, torch.float32, dev, with_points=False) for M in SIZES}
        lb_out = BoxLabelBatch.empty(offsets, SIZES[0], torch.float32)

        forms = {"snowfall_aligned": snow}
        for M in SIZES:
            forms[f"roipool_M{M}_S{S}"] = (lambda M=M: roi_point_pool(batch, rois[M], S, extra_width=EW, keep=keep, num_features=C, out=full[M], return_local=True))
            forms[f"roipool_M{M}_S{S}_index"] = (lambda M=M: roi_point_pool(batch, rois[M], S, extra_width=EW, keep=keep, out=bare[M], return_points=False))
        forms[f"pib_B{SIZES[0]}"] = lambda: points_in_boxes(batch, rois[SIZES[0]].boxes, keep=keep, out=lb_out)
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

        if not args.only:
            for M in SIZES:                                               # what the rois are like, then the torch restatement: equal bytes first
                r = rois[M].boxes
                pose = torch.stack((torch.cos(r[..., 6].double()), torch.sin(r[..., 6].double())), -1).contiguous()
                got = roi_point_pool(batch, r, S, extra_width=EW, pose=pose, keep=keep, num_features=C, return_local=True)
                s.synchronize()
                count = got.count.float()
                out_json[f"kept_M{M}"] = round(float(rois[M].count.float().mean()), 1)
                out_json[f"members_M{M}"] = {"mean": round(float(count.mean()), 1), "max": int(count.max()), "empty_share": round(float((count == 0).float().mean()), 4),
                                            "above_S_share": round(float((count > S).float().mean()), 4)}

                def restated(nf):
                    return [torch.stack(x) for x in zip(*(torch_pool(torch, out[f * n_per:(f + 1) * n_per], keep[f * n_per:(f + 1) * n_per], r[f], pose[f], EW, S, C,
                                                                      f * n_per) for f in range(nf)))]

                want = restated(TF)
                s.synchronize()
                same = {k: bool(torch.equal(x[:TF].contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)))
                        for k, x, y in zip(("index", "count", "points", "local"), (got.index, got.count, got.points, got.local), want)}
                assert all(same.values()), (M, same)
                out_json[f"torch_equal_M{M}"] = same
                del want
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2):
                    restated(TF)
                    torch.cuda.synchronize()
                out_json[f"torch_ms_M{M}_first_frames"] = round((time.perf_counter() - t0) * 1e3 / 2, 1)
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        out_json["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        out_json["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(out_json), flush=True)


if __name__ == "__main__":
    main()
