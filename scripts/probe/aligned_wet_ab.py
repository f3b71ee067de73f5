#!/usr/bin/env python3
"""A/B of the fused snowfall + wet-ground chain's result layouts on resident float32 sweeps with C3's settings: compact
(snowgpu_augment_wet_batch_device: five compaction passes, float64 rows out), aligned (snowgpu_augment_wet_batch_device_aligned: the aligned
finish, then the wet stage in place on its output; rows in the input's order and dtype + keep bytes) and aligned IN PLACE (the result written
over the input: the wet stage's stores are then the same, the snowfall finish writes where it read), on channel-sorted rows (C3) and on the
same sweeps in firing order (C2fire's order: the snowfall finish then stores through the sort's permutation).  One process, the three forms
alternating, every shape warmed up, device events around `--steps` back-to-back steps, `--repeats` times; the in-place form restores its
input before every step inside the timed region and the same number of restoring copies alone is timed and subtracted.  Asserts that
the aligned chain keeps exactly the rows the compact chain returns and that in place equals out of place byte for byte.

    python scripts/probe/aligned_wet_ab.py [--frames 256] [--steps 20] [--repeats 3] [--orders sorted,firing]
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
    ap.add_argument("--orders", default="sorted,firing")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F = args.frames
    layers, azimuths, snowfall, velocity, rscale = bench.WORKLOADS["C3"]
    tables = bench.make_tables(layers, snowfall, velocity, distinct=min(layers, 64))
    wet = bench.WET
    for order in args.orders.split(","):
        frames, orders = [], []
        for f in range(F):
            frames.append(bench.make_frame(layers, azimuths, 1000 + f, rscale, firing=order == "firing"))
            random.seed(1000 + f)
            o = list(range(layers))
            random.shuffle(o)
            orders.append(o)
        n_per = frames[0].shape[0]
        n = F * n_per
        rows = torch.from_numpy(np.concatenate(frames)).to(dev)
        del frames
        rows_ip = rows.clone()                                                   # the in-place form's input / output
        off = torch.arange(0, F + 1, dtype=torch.int64, device=dev) * n_per
        tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
        plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
        c_rows = torch.empty((n, 5), dtype=torch.float64, device=dev)
        c_src = torch.empty(n, dtype=torch.int32, device=dev)
        a_rows = torch.empty_like(rows)
        keep, keep_ip = torch.empty(n, dtype=torch.bool, device=dev), torch.empty(n, dtype=torch.bool, device=dev)
        cnt = [torch.zeros(F, dtype=torch.int64, device=dev) for _ in range(3)]
        st = [torch.zeros(F, 3, dtype=torch.int64, device=dev) for _ in range(3)]
        flags = [torch.zeros(F, dtype=torch.int32, device=dev) for _ in range(3)]
        status = [torch.zeros(8, dtype=torch.int32, device=dev) for _ in range(3)]
        s = torch.cuda.Stream()
        common = lambda r: (F, n, n_per, off.data_ptr(), r.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0)   # noqa: E731
        wet_args = (plane.data_ptr(), wet["water_height"], wet["pavement_depth"], wet["noise_floor"], wet["power_factor"], wet["flat_earth"],
                    wet["delta"], wet["replace"])

        def compact():
            eng.ctx.augment_wet_batch_device(*common(rows), *wet_args, c_rows.data_ptr(), c_src.data_ptr(), cnt[0].data_ptr(), st[0].data_ptr(),
                                             flags[0].data_ptr(), status[0].data_ptr(), s.cuda_stream)

        def aligned():
            eng.ctx.augment_wet_batch_device_aligned(*common(rows), a_rows.data_ptr(), keep.data_ptr(), cnt[1].data_ptr(), st[1].data_ptr(), 0,
                                                     status[1].data_ptr(), s.cuda_stream, *wet_args, flags[1].data_ptr())

        def restore():
            rows_ip.copy_(rows)

        def in_place():
            restore()
            eng.ctx.augment_wet_batch_device_aligned(*common(rows_ip), rows_ip.data_ptr(), keep_ip.data_ptr(), cnt[2].data_ptr(), st[2].data_ptr(), 0,
                                                     status[2].data_ptr(), s.cuda_stream, *wet_args, flags[2].data_ptr())

        def timed(step):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(args.steps):
                step()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b) / args.steps

        with torch.cuda.stream(s):
            for step in (compact, aligned, in_place):                            # warm-up: every form, this shape
                for _ in range(3):
                    step()
            s.synchronize()
            assert all(int(x[0]) == 0 for x in status), [x.tolist() for x in status]
            # same result: the aligned chain keeps exactly the rows the compact chain returns (the two fit over other tiles: the values
            # agree to rounding, the decisions do); in place = out of place, byte for byte
            valid = torch.arange(n_per, device=dev)[None, :] < cnt[0][:, None]
            gsrc = (c_src.view(F, n_per).long() + off[:F, None])[valid]
            want_keep = torch.zeros(n, dtype=torch.bool, device=dev)
            want_keep[gsrc] = True
            differ = int((want_keep != keep).sum())
            assert differ <= n // 1000000, f"{differ} keep flags differ from the compact chain's rows"
            assert torch.equal(flags[0], flags[1]) and torch.equal(st[0], st[1]) and int((cnt[0] - cnt[1]).abs().sum()) <= differ
            both = want_keep & keep
            sel = both.nonzero().flatten()
            back = torch.empty(n, dtype=torch.int64, device=dev)
            back[gsrc] = torch.arange(gsrc.shape[0], device=dev)
            c_sel = c_rows.view(F, n_per, 5)[valid][back[sel]]
            assert torch.equal(a_rows[sel][:, [0, 1, 2, 4]].double(), c_sel[:, [0, 1, 2, 4]])
            assert torch.allclose(a_rows[sel][:, 3].double(), c_sel[:, 3], rtol=1e-6, atol=0)
            assert torch.equal(rows_ip, a_rows) and torch.equal(keep_ip, keep) and torch.equal(cnt[2], cnt[1]) and torch.equal(st[2], st[1])
            del valid, gsrc, want_keep, both, sel, back, c_sel
            runs = {"compact": [], "aligned": [], "aligned_in_place": [], "restore_copy": []}
            for _ in range(args.repeats):
                runs["compact"].append(timed(compact))
                runs["aligned"].append(timed(aligned))
                both_ms = timed(in_place)
                runs["restore_copy"].append(timed(restore))
                runs["aligned_in_place"].append(both_ms - runs["restore_copy"][-1])
        med = {k: float(np.median(v)) for k, v in runs.items()}
        print(json.dumps({"workload": "C3", "row_order": order, "frames": F, "rows": n, "steps": args.steps,
                          "ms_per_step": {k: [round(x, 4) for x in v] for k, v in runs.items()},
                          "median_ms": {k: round(v, 4) for k, v in med.items()},
                          "aligned_over_compact": round(med["aligned"] / med["compact"], 4),
                          "in_place_over_compact": round(med["aligned_in_place"] / med["compact"], 4),
                          "kept_rows": int(cnt[1].sum()), "keep_flags_differing": differ, "frames_returned_as_they_came": int(flags[1].sum())}), flush=True)
        del rows, rows_ip, c_rows, a_rows, c_src, keep, keep_ip
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
