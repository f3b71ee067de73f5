#!/usr/bin/env python3
"""What dynamic radius outlier removal (snowgpu_dror_mask_device) costs beside the stage it stands in front of: resident float32 C2 sweeps
(bench.py's synthetic 64 x 2048 sweeps), the filter under the default setting (0.45, 3, 3, 0.04) and under (0.16, 3, 3, 0.04), and -- in the
same process, on the same batch -- the aligned C2 snowfall call.  Every form warmed up three times, device events around `--steps`
back-to-back calls, `--repeats` times.  One CPU figure for context: SciPy's cKDTree on ONE sweep (the per-point radius query a CPU
implementation makes).

    python scripts/probe/dror_ab.py [--frames 256] [--steps 20] [--repeats 3] [--only dror|snow]

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

SETTINGS = {"default": (0.45, 3.0, 3, 0.04), "alpha016": (0.16, 3.0, 3, 0.04)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
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
    first = frames[0]
    n_per = first.shape[0]
    n = F * n_per
    rows = torch.from_numpy(np.concatenate(frames)).to(dev)
    del frames
    off = torch.arange(0, F + 1, dtype=torch.int64, device=dev) * n_per
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    mask = {k: torch.empty(n, dtype=torch.bool, device=dev) for k in SETTINGS}
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def dror(name):
        a, b, k, sr = SETTINGS[name]
        return lambda: eng.ctx.dror_mask_device(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, a, b, sr, k, 0, mask[name].data_ptr(), 0, s.cuda_stream)

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    forms = {"dror_" + k: dror(k) for k in SETTINGS}
    forms["snowfall_aligned"] = snow
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

    with torch.cuda.stream(s):
        for step in forms.values():
            for _ in range(3):
                step()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "ms_per_step": {k: [round(x, 4) for x in v] for k, v in runs.items()},
           "median_ms": {k: round(v, 4) for k, v in med.items()}}
    for k in SETTINGS:
        if "dror_" + k in med:
            res["kept_share_" + k] = round(float(mask[k].float().mean()), 4)
            if "snowfall_aligned" in med:
                res[f"dror_{k}_over_snowfall"] = round(med["dror_" + k] / med["snowfall_aligned"], 3)
    if not args.only:
        from scipy.spatial import cKDTree
        xyz = np.asarray(first[:, :3], np.float64)
        c = 3.0 * (0.45 * (np.pi / 180.0))
        t0 = time.perf_counter()
        tree = cKDTree(xyz)
        k_cpu = tree.query_ball_point(xyz, np.maximum(0.04, c * np.hypot(xyz[:, 0], xyz[:, 1])), return_length=True) - 1 >= 3
        res["cpu_ckdtree_one_sweep_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["cpu_mask_equals_device_first_sweep"] = bool(np.array_equal(k_cpu, mask["default"][:n_per].cpu().numpy()))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
