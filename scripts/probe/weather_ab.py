#!/usr/bin/env python3
"""A/B of the per-frame weather entry (snowgpu_augment_weather_batch_device_aligned) on resident float32 C2 sweeps:

  (a) all_on     every gate on, no mask: the new entry against snowgpu_augment_wet_batch_device_aligned on the same batch.  The gates are
                 device data, so the new entry pays the masked front end (one more copy of the rows, three small kernels) and the masked
                 finish that the existing one does not: (a) is the price of not knowing on the host that every frame is on.
  (b) mixed      the four gate pairs in equal shares, against today's route: index_select the frames of each pair into a sub-batch, one
                 existing call per pair that does anything -- (1, 1) the fused aligned chain, (1, 0) the aligned snowfall entry, (0, 1)
                 the aligned wet entry --, and the scatter back (index_copy_ of rows and keep bytes into the batch's result).

One process, the variants alternating, every shape warmed up, device events around `--steps` back-to-back steps, `--repeats` times.
Nothing is asserted about the times.  The results of the two sides of (a) are compared byte for byte; of (b) per frame.

    python scripts/probe/weather_ab.py [--frames 64] [--steps 20] [--repeats 3]
"""
import argparse
import json
import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

WET = (0.0008, 0.001, 0.7, 15.0, 0.5)          # water height, pavement depth, noise floor, power factor, delta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
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
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()

    class Buffers:
        """Offsets, planes and result tensors of a batch of k frames."""

        def __init__(self, k):
            self.k, self.n = k, k * n_per
            self.off = torch.arange(0, k + 1, dtype=torch.int64, device=dev) * n_per
            self.plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * k, dtype=torch.float64, device=dev)
            self.out, self.keep = torch.empty((self.n, 5), dtype=torch.float32, device=dev), torch.empty(self.n, dtype=torch.bool, device=dev)
            self.cnt, self.st = torch.zeros(k, dtype=torch.int64, device=dev), torch.zeros(k, 3, dtype=torch.int64, device=dev)
            self.flags, self.status = torch.zeros(k, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def snow_args(b, r, t):
        return (b.k, b.n, n_per, b.off.data_ptr(), r.data_ptr(), 0, t.data_ptr(), bench.BEAM_DIV, 0, b.plane.data_ptr(), 0.7, 0)

    def outs(b):
        return (b.out.data_ptr(), b.keep.data_ptr(), b.cnt.data_ptr(), b.st.data_ptr(), 0, b.status.data_ptr(), s.cuda_stream)

    def timed(step):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(args.steps):
            step()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    def records(gates):
        rec = torch.zeros(F, 8, dtype=torch.float64)
        rec[:, 0], rec[:, 1] = torch.tensor([g[0] for g in gates]), torch.tensor([g[1] for g in gates])
        rec[:, 2:7] = torch.tensor(WET, dtype=torch.float64)
        return rec.to(dev)

    with torch.cuda.stream(s):
        new, old = Buffers(F), Buffers(F)

        def weather(rec):
            eng.ctx.augment_weather_batch_device_aligned(*snow_args(new, rows, tids), 0, *outs(new), new.plane.data_ptr(), rec.data_ptr(), False, False,
                                                         new.flags.data_ptr())

        # ---- (a) every gate on ----------------------------------------------------------------------------------------------------------
        rec_on = records([(1, 1)] * F)

        def fused():
            eng.ctx.augment_wet_batch_device_aligned(*snow_args(old, rows, tids), *outs(old), old.plane.data_ptr(), *WET[:4], False, WET[4], False,
                                                     old.flags.data_ptr())

        for _ in range(3):
            weather(rec_on)
            fused()
        s.synchronize()
        assert int(new.status[0]) == 0 and int(old.status[0]) == 0
        same_a = bool(torch.equal(new.out.view(torch.int32), old.out.view(torch.int32)) and torch.equal(new.keep, old.keep) and
                      torch.equal(new.cnt, old.cnt) and torch.equal(new.st, old.st) and torch.equal(new.flags, old.flags))
        runs = {"weather_all_on": [], "fused_aligned": []}
        for _ in range(args.repeats):
            runs["weather_all_on"].append(timed(lambda: weather(rec_on)))
            runs["fused_aligned"].append(timed(fused))
        med = {k: float(np.median(v)) for k, v in runs.items()}
        print(json.dumps({"probe": "weather_ab", "part": "a_all_on", "workload": "C2", "frames": F, "rows": n, "steps": args.steps,
                          "ms_per_step": {k: [round(x, 4) for x in v] for k, v in runs.items()}, "median_ms": {k: round(v, 4) for k, v in med.items()},
                          "weather_minus_fused_ms": round(med["weather_all_on"] - med["fused_aligned"], 4),
                          "weather_over_fused": round(med["weather_all_on"] / med["fused_aligned"], 4), "same_bytes": same_a}), flush=True)

        # ---- (b) the four gate pairs in equal shares ------------------------------------------------------------------------------------
        pairs = ((1, 1), (1, 0), (0, 1), (0, 0))
        gates = [pairs[f % 4] for f in range(F)]
        rec_mix = records(gates)
        idx = {p: torch.tensor([f for f in range(F) if gates[f] == p], dtype=torch.int64, device=dev) for p in pairs}
        sub = {p: Buffers(len(idx[p])) for p in pairs[:3]}
        rows3 = rows.view(F, n_per, 5)
        res_rows, res_keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)

        def route():
            res_rows.copy_(rows)                                                  # (0, 0) frames: as they came
            res_keep.fill_(True)
            for p in pairs[:3]:
                b, ix = sub[p], idx[p]
                r = rows3.index_select(0, ix).view(-1, 5)
                t = tids.index_select(0, ix)
                if p == (1, 1):
                    eng.ctx.augment_wet_batch_device_aligned(*snow_args(b, r, t), *outs(b), b.plane.data_ptr(), *WET[:4], False, WET[4], False,
                                                             b.flags.data_ptr())
                elif p == (1, 0):
                    eng.ctx.augment_batch_device_aligned(*snow_args(b, r, t), *outs(b))
                else:
                    eng.ctx.wet_ground_batch_device_aligned(b.k, b.n, n_per, b.off.data_ptr(), r.data_ptr(), 0, 0, b.plane.data_ptr(), *WET[:4], False,
                                                            WET[4], False, b.out.data_ptr(), b.keep.data_ptr(), b.cnt.data_ptr(), b.flags.data_ptr(),
                                                            b.status.data_ptr(), s.cuda_stream)
                res_rows.view(F, n_per, 5).index_copy_(0, ix, b.out.view(b.k, n_per, 5))
                res_keep.view(F, n_per).index_copy_(0, ix, b.keep.view(b.k, n_per))

        for _ in range(3):
            weather(rec_mix)
            route()
        s.synchronize()
        assert int(new.status[0]) == 0
        same_b = bool(torch.equal(new.out.view(torch.int32), res_rows.view(torch.int32)) and torch.equal(new.keep, res_keep))
        runs = {"weather_mixed": [], "four_calls_and_scatter": []}
        for _ in range(args.repeats):
            runs["weather_mixed"].append(timed(lambda: weather(rec_mix)))
            runs["four_calls_and_scatter"].append(timed(route))
        med = {k: float(np.median(v)) for k, v in runs.items()}
        print(json.dumps({"probe": "weather_ab", "part": "b_mixed", "workload": "C2", "frames": F, "rows": n, "steps": args.steps,
                          "ms_per_step": {k: [round(x, 4) for x in v] for k, v in runs.items()}, "median_ms": {k: round(v, 4) for k, v in med.items()},
                          "weather_over_route": round(med["weather_mixed"] / med["four_calls_and_scatter"], 4), "same_bytes": same_b,
                          "flags": sorted(set(new.flags.tolist()))}), flush=True)


if __name__ == "__main__":
    main()
