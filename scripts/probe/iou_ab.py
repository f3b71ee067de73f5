#!/usr/bin/env python3
"""What rotated NMS and the box IoU (snowgpu_nms_device, snowgpu_boxes_iou_device) cost behind the stages they sit between: resident float32
C2 sweeps (bench.py's synthetic 64 x 2048 sweeps) through the aligned snowfall call, then -- in the same process --

    nms_B{1024,4096,9000}_P{100,512}   BEV NMS, iou_thresh 0.7 (pcdet's proposal layer), on clustered synthetic proposals
    iou_{128x64,512x128}_{matrix,best,both}   the 3D IoU of rois against gt boxes, with and without materialising the matrix
    pib_B100, fps_rois_B100            points_in_boxes and sample_keypoints(rois=) (K = 2048, 6 sectors) on the boxes NMS kept (post_max 100)
    snowfall_aligned

The proposals: per frame B / 16 cluster centres on rows the snowfall call kept, car-sized (3.5 .. 5 x 1.6 .. 2.1 x 1.4 .. 2 m), random
headings; every proposal a member of a random cluster, its centre jittered by N(0, 0.4 m) in x and y, its heading by N(0, 0.1), its
extents by +-8 %; scores uniform in (0, 1).  The gt boxes are the centres of the first clusters, the rois of the IoU the first proposals.
The share an unlimited NMS suppresses is reported (post_max = B), and the kept count under each post_max.

Beside them the same outputs from a vectorised torch restatement of the definition (the clip as padded (P, 20) tensors, the definition's
order), held to equal bytes first: the IoU matrix and best for --torch-frames frames; NMS at B = 1024 for ONE frame the way pcdet runs
it -- the full suppression matrix on the device, the sequential sweep on the host.  Every device form warmed up twice, device events
around `--steps` back-to-back calls, `--repeats` times, the forms alternating; the torch forms are timed by the wall clock around
synchronized calls.

    python scripts/probe/iou_ab.py [--frames 16] [--steps 20] [--repeats 5] [--torch-frames 4] [--only nms|iou|pib|fps|snow]
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

NMS_SIZES, POST = (1024, 4096, 9000), (100, 512)
IOU_SIZES = ((128, 64), (512, 128))
CAP, K, S = 20, 2048, 6
IOU_THRESH = 0.7


def torch_area(torch, a, pa, b, pb):
    """area(a, b) of P present pairs (P, 7 float64; poses (P, 2)) in torch ops: include/snowgpu.h, step by step."""
    P, dev = a.shape[0], a.device
    ar = torch.arange(P, device=dev)
    hxa, hya, hxb, hyb = a[:, 3] * 0.5, a[:, 4] * 0.5, b[:, 3] * 0.5, b[:, 4] * 0.5
    pu, pv = torch.zeros((P, CAP), dtype=torch.float64, device=dev), torch.zeros((P, CAP), dtype=torch.float64, device=dev)
    for k in range(4):
        lx, ly = (hxa if k in (0, 3) else -hxa), (hya if k < 2 else -hya)
        x, y = a[:, 0] + (lx * pa[:, 0] - ly * pa[:, 1]), a[:, 1] + (lx * pa[:, 1] + ly * pa[:, 0])
        sx, sy = x - b[:, 0], y - b[:, 1]
        pu[:, k], pv[:, k] = sx * pb[:, 0] + sy * pb[:, 1], sy * pb[:, 0] - sx * pb[:, 1]
    n, top = torch.full((P,), 4, device=dev), 4
    for pas in range(4):
        on_v, neg = pas >= 2, bool(pas & 1)
        h = hyb if on_v else hxb
        qu, qv, m = torch.zeros_like(pu), torch.zeros_like(pv), torch.zeros_like(n)
        for i in range(top):
            act = i < n
            j = torch.where(i + 1 >= n, 0, i + 1)
            iu, iv, ju, jv = pu[:, i], pv[:, i], pu[ar, j], pv[ar, j]
            p_c, p_o, q_c, q_o = (iv, iu, jv, ju) if on_v else (iu, iv, ju, jv)
            dp, dq = (-p_c, -q_c) if neg else (p_c, q_c)
            in_p, in_q = dp <= h, dq <= h
            e1 = act & in_p & (m < CAP)
            at = m.clamp(max=CAP - 1)
            qu[ar, at], qv[ar, at] = torch.where(e1, iu, qu[ar, at]), torch.where(e1, iv, qv[ar, at])
            m = m + e1
            t = (h - dp) / (dq - dp)
            o, e = p_o + t * (q_o - p_o), (-h if neg else h)
            e2 = act & (in_p != in_q) & (m < CAP)
            at = m.clamp(max=CAP - 1)
            nu, nv = (o, e) if on_v else (e, o)
            qu[ar, at], qv[ar, at] = torch.where(e2, nu, qu[ar, at]), torch.where(e2, nv, qv[ar, at])
            m = m + e2
        pu, pv, n = qu, qv, m
        top = min(CAP, top + top // 2)                                    # (what a pass can emit: no host read)
    s = torch.zeros(P, dtype=torch.float64, device=dev)
    for i in range(top):
        j = torch.where(i + 1 >= n, 0, i + 1)
        s = torch.where(i < n, s + (pu[:, i] * pv[ar, j] - pu[ar, j] * pv[:, i]), s)
    return 0.5 * s.abs()


def torch_present(b, p):
    return ((b[..., :3].abs() <= 1e6).all(-1) & ((b[..., 3:6] > 0) & (b[..., 3:6] <= 1e6)).all(-1) & (b[..., 6].abs() <= 1e6) &
            (((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) - 1.0).abs() <= 1e-6))


def torch_iou(torch, a, pa, b, pb, mode):
    """(M, B) float64 IoU of one frame's boxes a (M, 7+) with b (B, 7+) under the poses, absent boxes 0."""
    M, B = a.shape[0], b.shape[0]
    a, b = a[:, :7].double(), b[:, :7].double()
    ok = (torch_present(a, pa)[:, None] & torch_present(b, pb)[None]).reshape(-1)
    A, PA = a[:, None].expand(M, B, 7).reshape(-1, 7), pa[:, None].expand(M, B, 2).reshape(-1, 2)
    Bb, PB = b[None].expand(M, B, 7).reshape(-1, 7), pb[None].expand(M, B, 2).reshape(-1, 2)
    inter = torch_area(torch, A, PA, Bb, PB)
    Aa, Ab = A[:, 3] * A[:, 4], Bb[:, 3] * Bb[:, 4]
    if mode == "bev":
        u = Aa + Ab - inter
        v = inter / torch.where(u > 1e-8, u, 1e-8)
    else:
        hza, hzb = A[:, 5] * 0.5, Bb[:, 5] * 0.5
        d = torch.minimum(A[:, 2] + hza, Bb[:, 2] + hzb) - torch.maximum(A[:, 2] - hza, Bb[:, 2] - hzb)
        i3 = inter * torch.where(d > 0, d, 0.0)
        u = Aa * A[:, 5] + Ab * Bb[:, 5] - i3
        v = i3 / torch.where(u > 1e-6, u, 1e-6)
    return torch.where(ok, v, 0.0).reshape(M, B)


def torch_nms_one(torch, boxes, scores, pose, post_max):
    """One frame the way pcdet runs nms_gpu: rank, the full matrix of iou(j, i) on the device, the sweep on the host.  Kept box numbers."""
    order = torch.sort(-scores.double(), stable=True).indices
    b, p = boxes[order], pose[order]
    over = (torch_iou(torch, b, p, b, p, "bev") > IOU_THRESH).cpu().numpy()          # [j, i]: area(j, i)
    kept = []
    for j in range(len(order)):
        if not over[j, kept].any():
            kept.append(j)
            if len(kept) == post_max:
                break
    return order[torch.tensor(kept, device=order.device)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=4)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    import bench
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import (BoxLabelBatch, DeviceBatch, IouBatch, KeypointBatch, NmsBatch, boxes_iou, nms, points_in_boxes,
                                            sample_keypoints)
    dev = torch.device("cuda:0")
    eng = engine.get_engine(0)
    F, TF = args.frames, min(args.torch_frames, args.frames)
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
    offsets = np.arange(F + 1, dtype=np.int64) * n_per
    off = torch.from_numpy(offsets).to(dev)
    tids = torch.tensor([eng.table_ids_from_arrays(tables, o) for o in orders], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    out, keep = torch.empty_like(rows), torch.empty(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)

    def snow():
        eng.ctx.augment_batch_device_aligned(F, n, n_per, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), bench.BEAM_DIV, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

    out_json = {"workload": "C2", "frames": F, "rows": n, "steps": args.steps, "device": torch.cuda.get_device_name(0), "iou_thresh": IOU_THRESH, "torch_frames": TF}
    with torch.cuda.stream(s):
        snow()
        s.synchronize()
        assert int(status[0]) == 0, status.tolist()
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        props, scores, centres = {}, {}, {}
        for B in NMS_SIZES:                                               # clustered proposals about kept rows of their frame
            Cn = B // 16
            at = torch.multinomial(keep.view(F, n_per).float(), Cn, replacement=False, generator=g) + (torch.arange(F, device=dev) * n_per)[:, None]
            u = torch.rand((F, Cn, 4), device=dev, generator=g)
            cen = torch.zeros((F, Cn, 7), device=dev)
            cen[:, :, :3] = out[at.reshape(-1), :3].view(F, Cn, 3)
            cen[:, :, 3], cen[:, :, 4], cen[:, :, 5] = 3.5 + 1.5 * u[:, :, 0], 1.6 + 0.5 * u[:, :, 1], 1.4 + 0.6 * u[:, :, 2]
            cen[:, :, 6] = (2 * u[:, :, 3] - 1) * np.pi
            of = torch.randint(0, Cn, (F, B), device=dev, generator=g)
            b = torch.gather(cen, 1, of[:, :, None].expand(F, B, 7)).clone()
            b[:, :, :2] += 0.4 * torch.randn((F, B, 2), device=dev, generator=g)
            b[:, :, 3:6] *= 0.92 + 0.16 * torch.rand((F, B, 3), device=dev, generator=g)
            b[:, :, 6] += 0.1 * torch.randn((F, B), device=dev, generator=g)
            props[B], scores[B], centres[B] = b.contiguous(), torch.rand((F, B), device=dev, generator=g), cen
        nms_out = {(B, P): NmsBatch.empty(F, B, P, 7, torch.float32, dev) for B in NMS_SIZES for P in POST}
        iou_in = {(M, G): (props[4096][:, :M].contiguous(), centres[4096][:, :G].contiguous()) for M, G in IOU_SIZES}
        iou_out = {(M, G): IouBatch.empty(F, M, G, torch.float32, dev, with_best=True) for M, G in IOU_SIZES}
        batch = DeviceBatch(out, offsets)
        kp_out = KeypointBatch.empty(F, K, 4, torch.float32, sectors=S)
        lb_out = BoxLabelBatch.empty(offsets, 100, torch.float32)
        rois = nms_out[(4096, 100)].boxes

        forms = {"snowfall_aligned": snow}
        for (B, P), o in nms_out.items():
            forms[f"nms_B{B}_P{P}"] = (lambda B=B, P=P, o=o: nms(props[B], scores[B], IOU_THRESH, post_max=P, out=o))
        for (M, G), o in iou_out.items():
            a, b = iou_in[(M, G)]
            forms[f"iou_{M}x{G}_matrix"] = (lambda a=a, b=b, o=o: boxes_iou(a, b, out=o))
            forms[f"iou_{M}x{G}_best"] = (lambda a=a, b=b, o=o: boxes_iou(a, b, out=o, return_iou=False, return_best=True))
            forms[f"iou_{M}x{G}_both"] = (lambda a=a, b=b, o=o: boxes_iou(a, b, out=o, return_best=True))
        forms["pib_B100"] = lambda: points_in_boxes(batch, rois, keep=keep, out=lb_out)
        forms["fps_rois_B100"] = lambda: sample_keypoints(batch, K, keep=keep, sectors=S, rois=rois, out=kp_out)
        if args.only:
            forms = {k: v for k, v in forms.items() if k.startswith(args.only)}
        for step in forms.values():
            for _ in range(2):
                step()
        s.synchronize()

        def timed(step):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(args.steps):
                step()
            b.record(s)
            b.synchronize()
            return a.elapsed_time(b) / args.steps

        if not args.only:
            for B in NMS_SIZES:                                           # what the proposals are like
                free = nms(props[B], scores[B], IOU_THRESH, post_max=B, return_boxes=False)
                s.synchronize()
                out_json[f"suppressed_share_B{B}"] = round(1.0 - float(free.count.float().mean()) / B, 4)
                for P in POST:
                    out_json[f"kept_B{B}_P{P}"] = round(float(nms_out[(B, P)].count.float().mean()), 1)
            for (M, G), o in iou_out.items():                             # the torch restatement: equal bytes first, then the clock
                a, b = iou_in[(M, G)]
                pa, pb = (torch.stack((torch.cos(x[..., 6].double()), torch.sin(x[..., 6].double())), -1).contiguous() for x in (a, b))
                got = boxes_iou(a, b, pose_a=pa, pose_b=pb, return_best=True)

                def restated(nf):
                    v = torch.stack([torch_iou(torch, a[f], pa[f], b[f], pb[f], "3d") for f in range(nf)])
                    top = v.max(-1)
                    return v.float(), torch.where(top.values > 0, top.indices.int(), -1), torch.where(top.values > 0, top.values, 0.0).float()

                want = restated(TF)
                s.synchronize()
                same = {k: bool(torch.equal(x[:TF].view(torch.uint8), y.view(torch.uint8))) for k, x, y in zip(("iou", "best", "best_iou"), (got.iou, got.best, got.best_iou), want)}
                assert all(same.values()), (M, G, same)
                out_json[f"torch_equal_iou_{M}x{G}"] = same
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2):
                    restated(TF)
                    torch.cuda.synchronize()
                out_json[f"torch_ms_iou_{M}x{G}_first_frames"] = round((time.perf_counter() - t0) * 1e3 / 2, 1)
            B = 1024
            pose = torch.stack((torch.cos(props[B][..., 6].double()), torch.sin(props[B][..., 6].double())), -1).contiguous()
            got = nms(props[B][:1].contiguous(), scores[B][:1].contiguous(), IOU_THRESH, post_max=100, pose=pose[:1].contiguous(), return_boxes=False)
            want = torch_nms_one(torch, props[B][0], scores[B][0], pose[0], 100)
            s.synchronize()
            k = int(got.count[0])
            assert k == len(want) and torch.equal(got.index[0, :k].long(), want), (k, len(want))
            out_json["torch_equal_nms_B1024_P100_one_frame"] = True
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                torch_nms_one(torch, props[B][0], scores[B][0], pose[0], 100)
                torch.cuda.synchronize()
            out_json["torch_ms_nms_B1024_P100_one_frame"] = round((time.perf_counter() - t0) * 1e3 / 2, 1)
            one = lambda: nms(props[B][:1], scores[B][:1], IOU_THRESH, post_max=100, return_boxes=False)
            one()
            out_json["ms_nms_B1024_P100_one_frame"] = round(timed(one), 4)
        runs = {k: [] for k in forms}
        for _ in range(args.repeats):
            for k, step in forms.items():
                runs[k].append(timed(step))
        out_json["ms_per_step"] = {k: [round(x, 4) for x in v] for k, v in runs.items()}
        out_json["median_ms"] = {k: round(float(np.median(v)), 4) for k, v in runs.items()}
    print(json.dumps(out_json), flush=True)


if __name__ == "__main__":
    main()
