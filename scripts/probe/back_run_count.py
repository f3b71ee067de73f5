"""How many beams and work items the BACK runs of the dict queue hold on a bench workload (no GPU: the oracle counts).

The pass over all rows queues a beam that met 1 .. front_max flakes at the front of its region's slice -- a region is a (frame, channel)
segment -- and one that met front_max + 1 .. 4 at the back; k_power_plan cuts the back run into items of 64 slots for k_power_few<T, 4>.
The plan's counters stay on the device, so this counts the same thing from the input: the oracle's get_occlusions (sim:298-424) gives the
number of flakes every beam meets for the first sweeps of a bench batch (its 256 sweeps are draws of the same scene), and the
items follow as ceil(back run / 64) per channel.

usage: python scripts/probe/back_run_count.py [--workload C2] [--seeds 2] [--front-max 2]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from oracle import snow_oracle as so  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--seeds", type=int, default=2, help="sweeps to count (each stands for DEFAULT_FRAMES / seeds sweeps of the batch)")
    ap.add_argument("--front-max", type=int, default=2)
    args = ap.parse_args()
    so.build()
    layers, azimuths, snowfall, velocity, scale = bench.WORKLOADS[args.workload]
    tables = bench.make_tables(layers, snowfall, velocity, distinct=min(layers, 64))
    half = np.radians(bench.BEAM_DIV / 2)
    two_pi = 2 * np.pi
    hist = np.zeros(6, np.int64)                                     # beams that met 0, 1, 2, 3, 4, more flakes
    back = items = regions = 0
    for seed in range(args.seeds):
        pc = bench.make_frame(layers, azimuths, 1000 + seed, scale)          # the first sweeps of rank 0's batch
        d = np.linalg.norm(pc[:, :3], axis=1).astype(np.float64)
        th = np.arctan2(pc[:, 1], pc[:, 0])
        th = np.where(th < 0, th + pc.dtype.type(two_pi), th).astype(np.float64)
        ang = np.column_stack((th - half, th + half))
        ang = np.where(ang < 0, ang + two_pi, ang)
        ang = np.where(ang > two_pi, ang - two_pi, ang)
        for ch in range(layers):
            idx = np.flatnonzero(pc[:, 4] == ch)
            if idx.size == 0:
                continue
            n_hit = so.get_occlusions(ang[idx], d[idx], tables[ch], bench.BEAM_DIV)[4]
            hist += np.bincount(np.minimum(n_hit, 5), minlength=6)
            nb = int(((n_hit > args.front_max) & (n_hit <= 4)).sum())
            back += nb
            items += (nb + 63) // 64
            regions += 1
    k = bench.DEFAULT_FRAMES / args.seeds
    print(f"{args.workload}: {args.seeds} sweeps of {layers} x {azimuths} beams, front_max {args.front_max}")
    print(f"  beams by flakes met (0, 1, 2, 3, 4, more), per sweep: {(hist / args.seeds).round(1).tolist()}")
    print(f"  back runs per sweep: {back / args.seeds:.1f} beams in {items / args.seeds:.1f} items of up to 64 slots over {regions / args.seeds:.0f} regions "
          f"({back / max(items, 1):.1f} beams per item)")
    print(f"  per batch of {bench.DEFAULT_FRAMES} sweeps: {back * k:.0f} beams, {items * k:.0f} items; of them three-flake {hist[3] * k:.0f}, four-flake {hist[4] * k:.0f}")


if __name__ == "__main__":
    main()
