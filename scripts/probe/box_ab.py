#!/usr/bin/env python3
"""What the points-in-boxes stage (snowgpu_points_in_boxes_device) costs behind the stages it follows, and the A/B that decided its design:
resident float32 C2 sweeps (bench.py's synthetic 64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process, on that
call's rows and keep mask -- the box of every row, the count of every box and the local coordinates for B = 32 and B = 128 boxes per
frame, centred on kept rows, car-sized (3.5 .. 5 x 1.6 .. 2.1 x 1.4 .. 2 m), random headings, every fourth slot absent (zeros), the pose
computed on the device,

    all     on the rows the snowfall call kept
    fov     on those rows behind a camera-view mask

with the grid (the library) and, when scripts/build_variant.sh has built it

    SG_VARIANT_UNITS=snowgpu_box.hip scripts/build_variant.sh boxbrute -DSG_BOX_BRUTE=1

with the brute-force kernel of that variant, loaded beside the library: every row against every present box of its frame.  The two are
held to equal bytes before either is timed.  Beside them the same outputs from torch ops on the first --torch-frames frames (per frame
an N x B broadcast in float64 under the pose the device returned, held to equal box_of, count and local first), the nearest-keypoints
stage (K = 2048, k = 3) and the aligned snowfall call.  Every device form warmed up twice, device events around `--steps` back-to-back
calls, `--repeats` times, the forms alternating; the torch form is timed by the wall clock around synchronized calls.  The streaming
floor is 21 B read + 4 B written per row at the 6.29 TB/s of a device copy.

    python scripts/probe/box_ab.py [--frames 256] [--steps 20] [--repeats 5] [--torch-frames 16] [--only box|nn|snow]

--only names the forms to run (under rocprofv3 --kernel-trace --stats: per-kernel times of those forms alone); it skips the torch form.
"""
import argparse
import ctypes
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
SIZES = (32, 128)
VARIANT = ROOT / "lidar_snow_sim_amd" / "_variants" / "libsnowgpu_boxbrute.so"
COPY_RATE = 6.29e12


def torch_boxes(torch, rows, keep, boxes, pose, nf, M):
    """The definition of include/snowgpu.h in torch ops for the first nf frames of M rows under `pose`: box_of, count, local."""
    dev = rows.device
    B = boxes.shape[1]
    box_of = torch.empty(nf * M, dtype=torch.int32, device=dev)
    local = torch.empty((nf * M, 3), dtype=rows.dtype, device=dev)
    count = torch.empty((nf, B), dtype=torch.int32, device=dev)
    for f in range(nf):
        p = rows[f * M:(f + 1) * M, :3].double()
        ok = keep[f * M:(f + 1) * M] & (p.abs() <= 1e6).all(1)
        b = boxes[f, :, :7].double()
        c, s = pose[f, :, 0], pose[f, :, 1]
        present = ((b[:, :3].abs() <= 1e6).all(1) & ((b[:, 3:6] > 0) & (b[:, 3:6] <= 1e6)).all(1) & (b[:, 6].abs() <= 1e6) &
                   (((c * c + s * s) - 1.0).abs() <= 1e-6))
        sx, sy, sz = p[:, None, 0] - b[None, :, 0], p[:, None, 1] - b[None, :, 1], p[:, None, 2] - b[None, :, 2]
        lx, ly = sx * c + sy * s, sy * c - sx * s
        inside = ((sz.abs() <= b[None, :, 5] * 0.5) & (lx.abs() < b[None, :, 3] * 0.5 + 1e-5) & (ly.abs() < b[None, :, 4] * 0.5 + 1e-5) &
                  present[None] & ok[:, None])
        count[f] = inside.sum(0).int()
        hit = inside.any(1)
        first = inside.int().argmax(1)
        box_of[f * M:(f + 1) * M] = torch.where(hit, first.int(), -1)
        at = first[:, None]
        loc = torch.cat((lx.gather(1, at), ly.gather(1, at), sz.gather(1, at)), 1)
        local[f * M:(f + 1) * M] = torch.where(hit[:, None], loc, 0.0).to(rows.dtype)
    return box_of, count, local


class Variant:
    """The box entry of a second build of the library, loaded beside the first, with a context of its own."""

    def __init__(self, path):
        vp, i64 = ctypes.c_void_p, ctypes.c_int64
        self.L = ctypes.CDLL(str(path))
        self.L.snowgpu_create.restype = ctypes.c_int
        self.L.snowgpu_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        self.L.snowgpu_points_in_boxes_device.restype = ctypes.c_int
        self.L.snowgpu_points_in_boxes_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]
        self.h = vp()
        assert self.L.snowgpu_create(0, ctypes.byref(self.h)) == 0

    def points_in_boxes_device(self, nf, n, m, off, rows, dtype, B, boxes, cb, pose_in, keep, box_of, count, local, pose, stream):
        vp = ctypes.c_void_p
        rc = self.L.snowgpu_points_in_boxes_device(self.h, nf, n, m, vp(off), vp(rows), dtype, B, vp(boxes), cb, vp(pose_in or None), vp(keep or None), vp(box_of),
                                                   vp(count or None), vp(local or None), vp(pose or None), vp(stream))
        assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=16)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.calibration import Calibration
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    brute = Variant(VARIANT) if VARIANT.exists() else None
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
    kp = (torch.empty((F, K), dtype=torch.int32, device=dev), torch.empty((F, K, C), dtype=torch.float32, device=dev), torch.empty(F, dtype=torch.int32, device=dev))
    nn = (torch.empty((n, 3), dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev))
    boxes = {B: torch.zeros((F, B, 8), dtype=torch.float32, device=dev) for B in SIZES}
    res = {(B, who): (torch.empty(n, dtype=torch.int32, device=dev), torch.empty((F, B), dtype=torch.int32, device=dev),
                      torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((F, B, 2), dtype=torch.float64, device=dev))
           for B in SIZES for who in ("grid", "brute")}

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    def fps():
        eng.ctx.fps_device(F, n, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, C, keep.data_ptr(), kp[0].data_ptr(), kp[1].data_ptr(), 0, kp[2].data_ptr(), s.cuda_stream)

    def nearest():
        eng.ctx.nearest_centres_device(F, n, n_per, off.data_ptr(), out.data_ptr(), 0, RANGE, K, kp[1].data_ptr(), C, 3, keep.data_ptr(), nn[0].data_ptr(),
                                       nn[1].data_ptr(), nn[2].data_ptr(), s.cuda_stream)

    def box(B, who, mask, nf):
        ctx, r = (eng.ctx if who == "grid" else brute), res[(B, who)]
        return lambda: ctx.points_in_boxes_device(nf, nf * n_per, n_per, off.data_ptr(), out.data_ptr(), 0, B, boxes[B].data_ptr(), 8, 0, masks[mask].data_ptr(),
                                                  r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), r[3].data_ptr(), s.cuda_stream)

    builds = ("grid", "brute") if brute else ("grid",)
    forms = {"snowfall_aligned": snow, "nn_k3_all_batch": nearest}
    forms.update({f"box_{who}_B{B}_{mask}_batch": box(B, who, mask, F) for B in SIZES for mask in masks for who in builds})
    if TF != F:
        forms.update({f"box_grid_B{B}_all_first_frames": box(B, "grid", "all", TF) for B in SIZES})
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

    floor_ms = n * 25 / COPY_RATE * 1e3
    out_json = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0), "boxes_per_frame": list(SIZES),
                "torch_frames": TF, "brute_variant": bool(brute), "streaming_floor_ms": round(floor_ms, 4)}
    with torch.cuda.stream(s):
        snow()                                                    # the rows and the mask the later stages read
        eng.ctx.fov_mask_device(n, out.data_ptr(), 0, cal, (1024, 1920), keep.data_ptr(), keep_fov.data_ptr(), s.cuda_stream)
        fps()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        for B in SIZES:                                           # boxes centred on kept rows of their frame
            w = keep.view(F, n_per).float()
            at = torch.multinomial(w, B, replacement=False, generator=g) + (torch.arange(F, device=dev) * n_per)[:, None]
            u = torch.rand((F, B, 4), device=dev, generator=g)
            b = boxes[B]
            b[:, :, :3] = out[at.reshape(-1), :3].view(F, B, 3)
            b[:, :, 3] = 3.5 + 1.5 * u[:, :, 0]
            b[:, :, 4] = 1.6 + 0.5 * u[:, :, 1]
            b[:, :, 5] = 1.4 + 0.6 * u[:, :, 2]
            b[:, :, 6] = (2 * u[:, :, 3] - 1) * np.pi
            b[:, :, 7] = 1.0
            b[:, 1::4] = 0.0                                      # a quarter of the slots absent
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()
        out_json["kept_share"] = {k: round(float(v.float().mean()), 4) for k, v in masks.items()}
        if not args.only:
            m = TF * n_per
            for B in SIZES:
                for mask in masks:
                    box(B, "grid", mask, F)()
                    s.synchronize()
                    got = res[(B, "grid")]
                    if mask == "all":
                        out_json[f"rows_in_a_box_B{B}"] = round(float((got[0] >= 0).float().mean()), 5)
                        out_json[f"rows_per_present_box_B{B}"] = round(float(got[1][got[1] > 0].float().mean()), 1)
                    if brute:
                        box(B, "brute", mask, F)()
                        s.synchronize()
                        same = {name: bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for name, a, b in zip(("box_of", "count", "local", "pose"), got, res[(B, "brute")])}
                        assert all(same.values()), (B, mask, same)
                        out_json[f"grid_equals_brute_B{B}_{mask}"] = same
                box(B, "grid", "all", TF)()
                s.synchronize()
                got = tuple(t[:m].clone() if t.shape[0] == n else t[:TF].clone() for t in res[(B, "grid")][:3])
                want = torch_boxes(torch, out, keep, boxes[B], res[(B, "grid")][3], TF, n_per)
                same = {name: bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8))) for name, a, b in zip(("box_of", "count", "local"), got, want)}
                assert all(same.values()), (B, same)
                out_json[f"torch_ops_equal_B{B}"] = same
                del want, got
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.torch_steps):
                    w = torch_boxes(torch, out, keep, boxes[B], res[(B, "grid")][3], TF, n_per)
                    torch.cuda.synchronize()
                    del w
                out_json[f"torch_ops_ms_first_frames_B{B}"] = round((time.perf_counter() - t0) * 1e3 / args.torch_steps, 1)
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        out_json["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        out_json["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
        out_json["ratio_to_streaming_floor"] = {k: round(float(np.median(v)) / floor_ms, 2) for k, v in runs.items() if k.startswith("box_") and k.endswith("_batch")}
    print(json.dumps(out_json), flush=True)


if __name__ == "__main__":
    main()
