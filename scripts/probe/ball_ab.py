#!/usr/bin/env python3
"""What the ball query (snowgpu_ball_query_device) costs behind the stages it follows: resident float32 C2 sweeps (bench.py's synthetic
64 x 2048 sweeps) through the aligned snowfall call and the keypoint stage (K = 2048 under SECOND's range [0, -40, -3, 70.4, 40, 1]),
then -- in the same process, on that call's rows, keep mask and keypoints -- the ball query with num_features = 4,

    two     the pairs ((0.4, 16), (0.8, 16))
    wide    the one pair (4.8, 32)

under the keep mask of the snowfall call alone (`all`) and under that mask ANDed with a camera-view mask (`fov`; its own keypoints), for
the whole batch and for the first --torch-frames frames alone.  Beside the latter a restatement in torch ops (per frame and chunk of
centres: broadcast differences, products, sums, a compare, a sum and a topk of masked row numbers) that is held to the same index, count
and points before either is timed.  Every device form warmed up twice, device events around `--steps` back-to-back calls, `--repeats`
times; the torch form is timed by the wall clock around `--torch-steps` synchronized calls.

    python scripts/probe/ball_ab.py [--frames 256] [--steps 3] [--repeats 3] [--torch-frames 16] [--torch-steps 1] [--only ball|fps|snow]

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
PAIRS = {"two": ((0.4, 0.8), (16, 16)), "wide": ((4.8,), (32,))}


def torch_ball(torch, rows, keep, centres, nf, M, radii, samples, rng, chunk=128):
    """The definition of include/snowgpu.h in torch ops for the first nf frames of M rows: (index nf x K x S, count nf x K x R)."""
    dev = rows.device
    p = rows.view(-1, M, 5)
    big = torch.iinfo(torch.int32).max
    number = torch.arange(M, dtype=torch.int32, device=dev)
    index = torch.empty((nf, K, sum(samples)), dtype=torch.int32, device=dev)
    count = torch.empty((nf, K, len(radii)), dtype=torch.int32, device=dev)
    for f in range(nf):
        x, y, z = p[f, :, 0], p[f, :, 1], p[f, :, 2]
        ok = keep.view(-1, M)[f].clone()
        for j, c in enumerate((x, y, z)):
            d = c.double()
            ok &= (d.abs() <= 1e6) & (d >= rng[j]) & (d < rng[3 + j])
        for k0 in range(0, K, chunk):
            c = centres[f, k0:k0 + chunk]
            dx, dy, dz = x[None] - c[:, 0:1], y[None] - c[:, 1:2], z[None] - c[:, 2:3]
            d = ((dx * dx) + (dy * dy)) + (dz * dz)
            s0 = 0
            for i, (r, S) in enumerate(zip(radii, samples)):
                r2 = torch.tensor(r, dtype=rows.dtype, device=dev)
                inside = (d < r2 * r2) & ok[None]
                n = inside.sum(1).int()
                first = torch.where(inside, number[None], big).topk(S, dim=1, largest=False, sorted=True).values
                first = torch.where(first == big, first[:, 0:1], first)
                first = torch.where(n[:, None] > 0, first + f * M, -1)
                index[f, k0:k0 + chunk, s0:s0 + S] = first
                count[f, k0:k0 + chunk, i] = n
                s0 += S
    return index, count


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
    nb = {(p, nf): (torch.empty((nf, K, sum(S)), dtype=torch.int32, device=dev), torch.empty((nf, K, len(S)), dtype=torch.int32, device=dev),
                    torch.empty((nf, K, sum(S), C), dtype=torch.float32, device=dev)) for p, (_, S) in PAIRS.items() for nf in {F, TF}}

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    def fps(mask):
        b = kp[mask]
        return lambda: eng.ctx.fps_device(F, n, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, C, masks[mask].data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
                                          0, b[2].data_ptr(), s.cuda_stream)

    def ball(pairs, mask, nf):
        b, (radii, samples) = nb[(pairs, nf)], PAIRS[pairs]
        return lambda: eng.ctx.ball_query_device(nf, nf * n_per, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, kp[mask][1].data_ptr(), C, radii, samples, C,
                                                 masks[mask].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), s.cuda_stream)

    forms = {"snowfall_aligned": snow}
    forms.update({f"fps_{mask}_k{K}": fps(mask) for mask in masks})
    forms.update({f"ball_{p}_{mask}_{'batch' if nf == F else 'first_frames'}": ball(p, mask, nf) for p in PAIRS for mask in masks for nf in sorted({F, TF}, reverse=True)})
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
           "pairs": {k: list(map(list, v)) for k, v in PAIRS.items()}, "torch_frames": TF}
    with torch.cuda.stream(s):
        snow()                                                    # the rows and the mask the later stages read
        eng.ctx.fov_mask_device(n, out.data_ptr(), 0, cal, (1024, 1920), keep.data_ptr(), keep_fov.data_ptr(), s.cuda_stream)
        for mask in masks:
            fps(mask)()                                           # the keypoints the ball query is centred on
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        res["kept_share"] = {k: round(float(v.float().mean()), 4) for k, v in masks.items()}
        if not args.only:
            for p, (radii, samples) in PAIRS.items():
                for mask in masks:
                    ball(p, mask, TF)()
                    s.synchronize()
                    b = nb[(p, TF)]
                    res[f"rows_per_ball_{p}_{mask}"] = {"median": [int(v) for v in b[1].view(-1, len(radii)).median(0).values],
                                                        "max": [int(v) for v in b[1].view(-1, len(radii)).max(0).values]}
                    want = torch_ball(torch, out, masks[mask], kp[mask][1], TF, n_per, radii, samples, RANGE)
                    res[f"torch_ops_equal_{p}_{mask}"] = bool(torch.equal(b[0], want[0]) and torch.equal(b[1], want[1]) and
                                                              torch.equal(b[2], out[b[0].long().clamp(min=0)][..., :C] * (b[0] >= 0)[..., None]))
                    del want
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.torch_steps):
                        w = torch_ball(torch, out, masks[mask], kp[mask][1], TF, n_per, radii, samples, RANGE)
                        torch.cuda.synchronize()
                        del w
                    res[f"torch_ops_ms_first_frames_{p}_{mask}"] = round((time.perf_counter() - t0) * 1e3 / args.torch_steps, 1)
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        res["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        res["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
