#!/usr/bin/env python3
"""A/B of the INPUT keep mask of the aligned snowfall entry on resident float32 C2 sweeps, under the camera-crop mask (k_fov_mask, a 108-degree
camera) and under a Bernoulli(0.7) mask:

  (a) masked     snowgpu_augment_batch_device_aligned_masked on the input as it lies: front end (count, two scans, scatter into context
                 scratch), the unmasked launch sequence on the scratch, the masked finish.  No host read.
  (b) torch      what a caller has to do without the entry: rows[mask] by torch (a boolean index: nonzero, a host read of its size, a
                 gather), the per-frame counts to the host, new offsets up, then snowgpu_augment_batch_device_aligned on the compacted rows.
                 Its result lies at the COMPACTED indices: the scatter back to the input's indices, which (a) includes, is not even in it.
  (c) floor      snowgpu_augment_batch_device_aligned on the ALREADY compacted input, offsets resident: what the per-beam work itself
                 costs.  (a) - (c) is the price of the front end and the masked finish; it is the comparison the overhead is read against.

One process, the three forms alternating, every shape warmed up, device events around `--steps` back-to-back steps, `--repeats` times.
Asserts that (a)'s present rows, keep bytes, counts and statistics equal (c)'s byte for byte.  Also times the mask producer alone.

    python scripts/probe/aligned_mask_ab.py [--frames 32] [--steps 20] [--repeats 3] [--masks fov,bernoulli]
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--masks", default="fov,bernoulli")
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

    def timed(step):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        for _ in range(args.steps):
            step()
        b.record(s)
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    for name in args.masks.split(","):
        mask = torch.empty(n, dtype=torch.bool, device=dev)

        def producer():
            eng.ctx.fov_mask_device(n, rows.data_ptr(), 0, cal, (1024, 1920), 0, mask.data_ptr(), s.cuda_stream)

        with torch.cuda.stream(s):
            if name == "fov":
                producer()
            else:
                mask.copy_(torch.from_numpy(np.random.default_rng(7).random(n) < 0.7).to(dev))
            s.synchronize()
            counts = mask.view(F, n_per).sum(1)
            sub = rows[mask].contiguous()                                        # (c)'s input: compacted once, outside every timed region
            sub_off = torch.zeros(F + 1, dtype=torch.int64, device=dev)
            sub_off[1:] = torch.cumsum(counts, 0)
            m = int(sub.shape[0])
            max_sub = int(counts.max())
            out_a, keep_a = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
            out_c, keep_c = torch.empty_like(sub), torch.empty(m, dtype=torch.bool, device=dev)
            cnt = [torch.zeros(F, dtype=torch.int64, device=dev) for _ in range(3)]
            st = [torch.zeros(F, 3, dtype=torch.int64, device=dev) for _ in range(3)]
            status = [torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(3)]

            def masked():
                eng.ctx.augment_batch_device_aligned_masked(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0,
                                                            plane.data_ptr(), 0.7, 0, mask.data_ptr(), out_a.data_ptr(), keep_a.data_ptr(),
                                                            cnt[0].data_ptr(), st[0].data_ptr(), 0, status[0].data_ptr(), s.cuda_stream)

            def by_torch():
                sel = rows[mask]                                                 # boolean index: a host read of the row count inside
                c = mask.view(F, n_per).sum(1).cpu().numpy()                     # counts to the host
                o = np.zeros(F + 1, np.int64)
                o[1:] = np.cumsum(c)
                d_o = torch.from_numpy(o).to(dev, non_blocking=True)
                r, k = torch.empty_like(sel), torch.empty(sel.shape[0], dtype=torch.bool, device=dev)
                eng.ctx.augment_batch_device_aligned(F, int(o[-1]), int(c.max()), d_o.data_ptr(), sel.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0,
                                                     plane.data_ptr(), 0.7, 0, r.data_ptr(), k.data_ptr(), cnt[1].data_ptr(), st[1].data_ptr(), 0,
                                                     status[1].data_ptr(), s.cuda_stream)
                return r, k

            def floor():
                eng.ctx.augment_batch_device_aligned(F, m, max_sub, sub_off.data_ptr(), sub.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0,
                                                     plane.data_ptr(), 0.7, 0, out_c.data_ptr(), keep_c.data_ptr(), cnt[2].data_ptr(), st[2].data_ptr(), 0,
                                                     status[2].data_ptr(), s.cuda_stream)

            for step in (masked, by_torch, floor):                               # warm-up: every form, this shape
                for _ in range(3):
                    step()
            s.synchronize()
            assert all(int(x[0]) == 0 for x in status), [x.tolist() for x in status]
            # same result: (a) at the present rows' own indices = (c) = (b), byte for byte
            assert torch.equal(out_a[mask].view(torch.int32), out_c.view(torch.int32)) and torch.equal(keep_a[mask], keep_c)
            assert not bool(keep_a[~mask].any()) and torch.equal(out_a[~mask].view(torch.int32), rows[~mask].view(torch.int32))
            assert torch.equal(cnt[0], cnt[2]) and torch.equal(st[0], st[2]) and torch.equal(cnt[1], cnt[2]) and torch.equal(st[1], st[2])
            r_b, k_b = by_torch()
            s.synchronize()
            assert torch.equal(r_b.view(torch.int32), out_c.view(torch.int32)) and torch.equal(k_b, keep_c)
            del r_b, k_b
            runs = {"masked": [], "torch_index_then_aligned": [], "floor_compacted_input": [], "fov_mask_producer": []}
            for _ in range(args.repeats):
                runs["masked"].append(timed(masked))
                runs["torch_index_then_aligned"].append(timed(by_torch))
                runs["floor_compacted_input"].append(timed(floor))
                runs["fov_mask_producer"].append(timed(producer) if name == "fov" else 0.0)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        print(json.dumps({"workload": "C2", "mask": name, "frames": F, "rows": n, "present_rows": m, "steps": args.steps,
                          "ms_per_step": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                          "median_ms": {k: round(v, 4) for k, v in med.items()},
                          "masked_over_torch": round(med["masked"] / med["torch_index_then_aligned"], 4),
                          "masked_minus_floor_ms": round(med["masked"] - med["floor_compacted_input"], 4),
                          "kept_rows": int(cnt[0].sum())}), flush=True)
        del sub, out_a, out_c, keep_a, keep_c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
