#!/usr/bin/env python3
"""What sectorized, proposal-centric sampling (snowgpu_fps_sectors_device) costs beside the plain walk (snowgpu_fps_device, unchanged):
resident float32 C2 sweeps (bench.py's synthetic 64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process, on that
call's rows and keep mask, under SECOND's range [0, -40, -3, 70.4, 40, 1], K = 2048 and K = 4096 --

    fps_*        the plain walk, as scripts/probe/fps_ab.py times it: the A side
    sec_*        S = 6 sectors, no rois
    roi_*        S = 6 sectors behind `--rois` synthetic car-sized rois per frame (3.9 x 1.6 x 1.56 m, centred on kept rows of the
                 frame, drawn once), margin 1.6

each on `all` (the keep mask of the snowfall call alone) and on `fov` (that mask ANDed with a camera-view mask: some three quarters of
the rows absent), for the whole batch and for ONE frame alone.  Every form warmed up twice, device events around `--steps` back-to-back
calls, `--repeats` windows, the median reported; every comparison within this one process.

    python scripts/probe/fps_sectors_ab.py [--frames 256] [--steps 3] [--repeats 5] [--rois 32] [--sectors 6] [--only sec|roi|fps|snow]

--only names the one family to run (under rocprofv3 --kernel-trace --stats: per-kernel times of that family alone).
"""
import argparse
import json
import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
C = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rois", type=int, default=32)
    ap.add_argument("--sectors", type=int, default=6)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.calibration import Calibration
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F, S, B = args.frames, args.sectors, args.rois
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
    shapes = [(F, 2048), (F, 4096), (1, 2048)]
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    bufs = {(nf, K): (i32(nf, K), torch.empty((nf, K, C), dtype=torch.float32, device=dev), torch.empty((nf, K), dtype=torch.float32, device=dev), i32(nf),
                      i32(nf, S + 1), i32(nf, S)) for nf, K in shapes}
    rois = torch.zeros((F, B, 7), dtype=torch.float32, device=dev)

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    def fps(nf, K, mask):
        b = bufs[(nf, K)]
        return lambda: eng.ctx.fps_device(nf, nf * n_per, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, C, masks[mask].data_ptr(), b[0].data_ptr(),
                                          b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), s.cuda_stream)

    def sec(nf, K, mask, with_rois):
        b = bufs[(nf, K)]
        return lambda: eng.ctx.fps_sectors_device(nf, nf * n_per, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, C, masks[mask].data_ptr(), S,
                                                  rois.data_ptr() if with_rois else 0, B, 7, 1.6, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(),
                                                  b[4].data_ptr(), b[5].data_ptr(), 0, 0, s.cuda_stream)

    def name(nf, K):
        return f"{'batch' if nf == F else 'one_frame'}_k{K}"

    forms = {"snowfall_aligned": snow}
    for mask in masks:
        for nf, K in shapes:
            forms[f"fps_{mask}_{name(nf, K)}"] = fps(nf, K, mask)
            forms[f"sec_{mask}_{name(nf, K)}"] = sec(nf, K, mask, False)
            forms[f"roi_{mask}_{name(nf, K)}"] = sec(nf, K, mask, True)
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

    res = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "repeats": args.repeats, "sectors": S, "rois_per_frame": B, "roi_margin": 1.6,
           "device": torch.cuda.get_device_name(0), "range": RANGE}
    with torch.cuda.stream(s):
        snow()                                                    # the rows and the mask the keypoint stage reads
        eng.ctx.fov_mask_device(n, out.data_ptr(), 0, cal, (1024, 1920), keep.data_ptr(), keep_fov.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        # the rois: car-sized boxes centred on kept rows of the frame inside the range (drawn once, on the host)
        g = torch.Generator().manual_seed(5)
        p = out.view(F, n_per, 5)
        inside = keep_fov.view(F, n_per) & (p[:, :, 0] >= RANGE[0]) & (p[:, :, 0] < RANGE[3]) & (p[:, :, 1] >= RANGE[1]) & (p[:, :, 1] < RANGE[4]) & \
            (p[:, :, 2] >= RANGE[2]) & (p[:, :, 2] < RANGE[5])
        pick = torch.multinomial(inside.float().cpu() + 1e-12, B, replacement=False, generator=g).to(dev)
        rois[:, :, :3] = torch.gather(p[:, :, :3], 1, pick[:, :, None].expand(F, B, 3))
        rois[:, :, 3:6] = torch.tensor([3.9, 1.6, 1.56], device=dev)
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()
        res["kept_share"] = {k: round(float(v.float().mean()), 4) for k, v in masks.items()}
        for fam in ("fps", "sec", "roi"):
            for mask in masks:
                k = f"{fam}_{mask}_{name(F, 2048)}"
                if k in forms:
                    forms[k]()
                    s.synchronize()
                    b = bufs[(F, 2048)]
                    res[f"usable_per_frame_{fam}_{mask}"] = {"min": int(b[3].min()), "median": int(b[3].median()), "max": int(b[3].max())}
                    if fam != "fps":
                        res[f"rows_per_sector_{fam}_{mask}"] = {"median": b[5].float().median(0).values.int().tolist(), "max": int(b[5].max())}
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        res["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        res["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
