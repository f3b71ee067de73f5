#!/usr/bin/env python3
"""What the nearest-centres stage (snowgpu_nearest_centres_device) costs behind the stages it follows: resident float32 C2 sweeps
(bench.py's synthetic 64 x 2048 sweeps) through the aligned snowfall call and the keypoint stage (K = 2048 under SECOND's range
[0, -40, -3, 70.4, 40, 1]), then -- in the same process, on that call's rows, keep mask and keypoints -- the k = 3 and k = 1 nearest
keypoints of every row with weights,

    all     keypoints sampled from, and propagated to, the rows the snowfall call kept
    fov     keypoints sampled from, and propagated to, those rows behind a camera-view mask
    far     keypoints sampled behind the camera-view mask, propagated to ALL kept rows: most rows are far from every centre

for the whole batch and (k = 3) for the first --torch-frames frames alone.  Beside the latter a restatement in torch ops (per frame and
chunk of rows: broadcast differences, products and sums in the definition's order, a stable sort by distance -- centres ascending, so
the order is that of (distance, centre) -- and the float64 weight chain) that is held to the same index, dist2 and weight before either
is timed.  The ball query ((0.4, 16), (0.8, 16)) runs beside them.  Every device form warmed up twice, device events around `--steps`
back-to-back calls, `--repeats` times; the torch form is timed by the wall clock around `--torch-steps` synchronized calls.

    python scripts/probe/nn_ab.py [--frames 256] [--steps 3] [--repeats 3] [--torch-frames 16] [--torch-steps 1] [--only nn|ball|fps|snow]

--only names the forms to run (under rocprofv3 --kernel-trace --stats: per-kernel times of those forms alone); it skips the torch form.
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
C, K = 4, 2048
SETTINGS = {"all": ("all", "all"), "fov": ("fov", "fov"), "far": ("fov", "all")}          # (the keypoints' mask, the rows' mask)


def torch_nn(torch, rows, keep, centres, nf, M, k, rng, chunk=8192):
    """The definition of include/snowgpu.h in torch ops for the first nf frames of M rows: (index, dist2, weight), each nf M x k."""
    dev = rows.device
    p = rows[:nf * M].view(nf, M, 5)
    index = torch.empty((nf * M, k), dtype=torch.int32, device=dev)
    dist2 = torch.empty((nf * M, k), dtype=rows.dtype, device=dev)
    for f in range(nf):
        x, y, z = p[f, :, 0], p[f, :, 1], p[f, :, 2]
        ok = keep[f * M:(f + 1) * M].clone()
        for j, c in enumerate((x, y, z)):
            d = c.double()
            ok &= (d.abs() <= 1e6) & (d >= rng[j]) & (d < rng[3 + j])
        c = centres[f]
        cok = (c[:, :3].double().abs() <= 1e6).all(1)
        for r0 in range(0, M, chunk):
            sl = slice(r0, r0 + chunk)
            dx, dy, dz = x[sl, None] - c[None, :, 0], y[sl, None] - c[None, :, 1], z[sl, None] - c[None, :, 2]
            d = ((dx * dx) + (dy * dy)) + (dz * dz)
            d = torch.where(cok[None], d, torch.full_like(d, float("inf")))
            best, at = torch.sort(d, dim=1, stable=True)
            best, at = best[:, :k], at[:, :k].int()
            none = ~ok[sl, None] | torch.isinf(best)
            index[f * M + r0:f * M + r0 + chunk] = torch.where(none, -1, at)
            dist2[f * M + r0:f * M + r0 + chunk] = torch.where(none, float("inf"), best)
    u = torch.where(index >= 0, 1.0 / (dist2.double().sqrt() + 1e-8), 0.0)
    total = u[:, 0].clone()
    for j in range(1, k):
        total = total + u[:, j]
    weight = torch.where(index >= 0, u / total[:, None], 0.0).to(rows.dtype)
    return index, dist2, weight


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch-frames", type=int, default=16)
    ap.add_argument("--torch-steps", type=int, default=1)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.calibration import Calibration
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F, TF = args.frames, min(args.torch_frames, args.frames)
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
    masks = {"all": keep, "fov": keep_fov}
    kp = {m: (torch.empty((F, K), dtype=torch.int32, device=dev), torch.empty((F, K, C), dtype=torch.float32, device=dev),
              torch.empty(F, dtype=torch.int32, device=dev)) for m in masks}
    nn = {k: (torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev),
              torch.empty((n, k), dtype=torch.float32, device=dev)) for k in (1, 3)}
    nb = (torch.empty((F, K, 32), dtype=torch.int32, device=dev), torch.empty((F, K, 2), dtype=torch.int32, device=dev),
          torch.empty((F, K, 32, C), dtype=torch.float32, device=dev))

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    def fps(mask):
        b = kp[mask]
        return lambda: eng.ctx.fps_device(F, n, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, C, masks[mask].data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
                                          0, b[2].data_ptr(), s.cuda_stream)

    def ball():
        eng.ctx.ball_query_device(F, n, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, kp["all"][1].data_ptr(), C, (0.4, 0.8), (16, 16), C,
                                  keep.data_ptr(), nb[0].data_ptr(), nb[1].data_ptr(), nb[2].data_ptr(), s.cuda_stream)

    def nearest(k, setting, nf):
        centres, mask = SETTINGS[setting]
        b = nn[k]
        return lambda: eng.ctx.nearest_centres_device(nf, nf * n_per, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, kp[centres][1].data_ptr(), C, k,
                                                      masks[mask].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), s.cuda_stream)

    forms = {"snowfall_aligned": snow, "ball_two_all_batch": ball}
    forms.update({f"fps_{mask}_k{K}": fps(mask) for mask in masks})
    forms.update({f"nn_k{k}_{setting}_batch": nearest(k, setting, F) for k in (3, 1) for setting in SETTINGS})
    if TF != F:
        forms.update({f"nn_k3_{setting}_first_frames": nearest(3, setting, TF) for setting in SETTINGS})
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

    res = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0), "range": RANGE, "centres_per_frame": K,
           "torch_frames": TF}
    with torch.cuda.stream(s):
        snow()                                                    # the rows and the mask the later stages read
        eng.ctx.fov_mask_device(n, out.data_ptr(), 0, cal, (1024, 1920), keep.data_ptr(), keep_fov.data_ptr(), s.cuda_stream)
        for mask in masks:
            fps(mask)()                                           # the keypoints the rows look for
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        res["kept_share"] = {k: round(float(v.float().mean()), 4) for k, v in masks.items()}
        if not args.only:
            m = TF * n_per
            for setting, (centres, mask) in SETTINGS.items():
                nearest(3, setting, TF)()
                s.synchronize()
                got = tuple(t[:m].clone() for t in nn[3])
                found = got[0][:, 0] >= 0
                res[f"rows_with_a_neighbour_{setting}"] = round(float(found.float().mean()), 4)
                res[f"median_dist_m_{setting}"] = [round(float(v), 3) for v in got[1][found].sqrt().median(0).values]
                want = torch_nn(torch, out, masks[mask], kp[centres][1], TF, n_per, 3, RANGE)
                res[f"torch_ops_equal_{setting}"] = {name: bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                                                     for name, a, b in zip(("index", "dist2", "weight"), got, want)}
                del want, got
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.torch_steps):
                    w = torch_nn(torch, out, masks[mask], kp[centres][1], TF, n_per, 3, RANGE)
                    torch.cuda.synchronize()
                    del w
                res[f"torch_ops_ms_first_frames_k3_{setting}"] = round((time.perf_counter() - t0) * 1e3 / args.torch_steps, 1)
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        res["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        res["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
