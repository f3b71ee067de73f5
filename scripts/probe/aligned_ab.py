#!/usr/bin/env python3
"""A/B of the result layouts of the device entry: compact (snowgpu_augment_batch_device: count, scan, scatter), aligned
(snowgpu_augment_batch_device_aligned: one finishing kernel, rows at the input's index + keep flags) and aligned IN PLACE, on resident
float32 sweeps, channel-sorted (C2) and in firing order (C2fire).  One process, the variants alternating, every shape warmed up, device
events around `--steps` back-to-back steps, `--repeats` times; the in-place variant restores its input before every step inside the timed
region and the same number of restoring copies alone is timed and subtracted.  Asserts that rows[keep] re-ordered by src are the compact rows.

    python scripts/probe/aligned_ab.py [--frames 256] [--steps 20] [--repeats 3] [--workloads C2,C2fire]
"""
import argparse
import json
import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="C2,C2fire")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F = args.frames
    for wl in args.workloads.split(","):
        layers, azimuths, snowfall, velocity, rscale = bench.WORKLOADS[wl]
        tables = bench.make_tables(layers, snowfall, velocity, distinct=min(layers, 64))
        frames, orders = [], []
        for f in range(F):
            frames.append(bench.make_frame(layers, azimuths, 1000 + f, rscale, firing=wl in bench.FIRING_ORDER))
            random.seed(1000 + f)
            o = list(range(layers))
            random.shuffle(o)
            orders.append(o)
        n_per = frames[0].shape[0]
        n = F * n_per
        rows = torch.from_numpy(np.concatenate(frames)).to(dev)
        del frames
        rows_ip = rows.clone()                                                   # the in-place variant's input / output
        off = torch.arange(0, F + 1, dtype=torch.int64, device=dev) * n_per
        tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
        plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
        c_rows, a_rows = torch.empty_like(rows), torch.empty_like(rows)
        c_src = torch.empty(n, dtype=torch.int32, device=dev)
        keep, keep_ip = torch.empty(n, dtype=torch.bool, device=dev), torch.empty(n, dtype=torch.bool, device=dev)
        cnt = [torch.zeros(F, dtype=torch.int64, device=dev) for _ in range(3)]
        st = [torch.zeros(F, 3, dtype=torch.int64, device=dev) for _ in range(3)]
        status = [torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(3)]
        s = torch.cuda.Stream()
        common = lambda r: (F, n, n_per, off.data_ptr(), r.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0)   # noqa: E731

        def compact():
            eng.ctx.augment_batch_device(*common(rows), c_rows.data_ptr(), c_src.data_ptr(), cnt[0].data_ptr(), st[0].data_ptr(), 0, status[0].data_ptr(), s.cuda_stream)

        def aligned():
            eng.ctx.augment_batch_device_aligned(*common(rows), a_rows.data_ptr(), keep.data_ptr(), cnt[1].data_ptr(), st[1].data_ptr(), 0, status[1].data_ptr(), s.cuda_stream)

        def restore():
            rows_ip.copy_(rows)

        def in_place():
            restore()
            eng.ctx.augment_batch_device_aligned(*common(rows_ip), rows_ip.data_ptr(), keep_ip.data_ptr(), cnt[2].data_ptr(), st[2].data_ptr(), 0, status[2].data_ptr(), s.cuda_stream)

        def timed(step):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(args.steps):
                step()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b) / args.steps

        with torch.cuda.stream(s):
            for step in (compact, aligned, in_place):                            # warm-up: every variant, this shape
                for _ in range(3):
                    step()
            s.synchronize()
            assert all(int(x[0]) == 0 for x in status), [x.tolist() for x in status]
            # same result: rows[keep] re-ordered by src are the compact rows; in place = out of place
            valid = torch.arange(n_per, device=dev)[None, :] < cnt[0][:, None]
            gsrc = (c_src.view(F, n_per).long() + off[:F, None])[valid]
            assert torch.equal(a_rows[gsrc], c_rows.view(F, n_per, 5)[valid]) and bool(keep[gsrc].all())
            assert torch.equal(keep.view(F, n_per).sum(1), cnt[0]) and torch.equal(cnt[0], cnt[1]) and torch.equal(st[0], st[1])
            assert torch.equal(rows_ip, a_rows) and torch.equal(keep_ip, keep) and torch.equal(cnt[2], cnt[1]) and torch.equal(st[2], st[1])
            del valid, gsrc
            runs = {"compact": [], "aligned": [], "aligned_in_place": [], "restore_copy": []}
            for _ in range(args.repeats):
                runs["compact"].append(timed(compact))
                runs["aligned"].append(timed(aligned))
                both = timed(in_place)
                runs["restore_copy"].append(timed(restore))
                runs["aligned_in_place"].append(both - runs["restore_copy"][-1])
        med = {k: float(np.median(v)) for k, v in runs.items()}
        print(json.dumps({"workload": wl, "frames": F, "rows": n, "steps": args.steps, "ms_per_step": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                          "median_ms": {k: round(v, 4) for k, v in med.items()},
                          "aligned_over_compact": round(med["aligned"] / med["compact"], 4),
                          "in_place_over_compact": round(med["aligned_in_place"] / med["compact"], 4),
                          "kept_rows": int(cnt[0].sum())}), flush=True)
        if wl == "C2":
            assert med["aligned"] <= med["compact"] * 1.03, "C2 gate: aligned must be at most compact x 1.03"
        del rows, rows_ip, c_rows, a_rows, c_src, keep, keep_ip
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
