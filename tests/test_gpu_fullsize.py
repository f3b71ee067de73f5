"""-m gpu: FULL-SIZE frames of every BASELINE.json config through the HIP path against the threaded C oracle,
with mismatch COUNTS (kept rows, labels, intensities) asserted to be zero and printed.

  C2     64 x 2048 sweeps, 2.5 mm/h @ 1.6 m/s (18 k flakes per line)            -- the headline workload
  C2fire the C2 sweeps with their rows in firing order (azimuth-major, channels interleaved: the row order of an STF .bin) -- the
         channel sort is a real permutation and the per-beam kernels read the sort's sorted copy
  C2far  the same sweeps with every range stretched x1.8 (long scatterer lists: capacity tiers 8 / 16 / 63 busy)
  C1     64 x 2048 sweeps, 0.5 mm/h @ 2.0 m/s (40 k flakes per line: the first tier is 8)
  C4     128 x 4096 sweeps, 10 mm/h @ 1.6 m/s, 128-entry laser table (the 64-entry one tiled)
  C3     snowfall + wet ground fused (pointcloud_viewer.py:2807-2821) on C2 sweeps

Both sides run end to end from the same frames, tables, channel permutations and ground plane: the HIP path with
its device prepass, the oracle with its NumPy/SciPy prepass (simulation.py:449-467).  Frames and tables are the ones
bench.py uses (SURVEY 8 d generator).  The counts also go to gpurun_out/fullsize_parity.jsonl.
"""
import json
import os
import random
import time
from pathlib import Path

import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded (one HIP runtime per process)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BD = float(np.degrees(3e-3))
PLANE = ([0.0, 0.0, -1.0], -1.7)
N_FRAMES = int(os.environ.get("SNOWGPU_FULLSIZE_FRAMES", "8"))
_TABLE_CACHE = {}


def _tables(workload):
    """bench.py's tables for the workload (dart_throwing(..., default_rng(42 + line)), R0 = 80 m); C1's 40 k-flake
    tables take 0.4 s each on the host, so 16 distinct ones are tiled over the 64 lines."""
    import bench
    layers, _, snowfall, velocity, _ = bench.WORKLOADS[workload]
    key = (snowfall, velocity, layers)
    if key not in _TABLE_CACHE:
        distinct = 16 if workload == "C1" else min(layers, 64)
        _TABLE_CACHE[key] = bench.make_tables(layers, snowfall, velocity, distinct=distinct)
    return _TABLE_CACHE[key]


def _frames(workload, dtype, n):
    import bench
    layers, azimuths, _, _, scale = bench.WORKLOADS[workload]
    out, orders = [], []
    for f in range(n):
        seed = 1000 + f
        pc = bench.make_frame(layers, azimuths, seed, scale, workload in bench.FIRING_ORDER)
        random.seed(seed)                                   # SURVEY 8 d: random.seed(f); random.shuffle(order)
        order = list(range(layers))
        random.shuffle(order)
        out.append(pc.astype(dtype))
        orders.append(order)
    return out, orders


def _report(capsys, rec):
    line = json.dumps(rec)
    with capsys.disabled():
        print("\n[fullsize-parity] " + line, flush=True)
    try:
        d = ROOT / "gpurun_out"
        d.mkdir(exist_ok=True)
        with open(d / "fullsize_parity.jsonl", "a") as fh:
            fh.write(line + "\n")
    except OSError:
        pass


def _count_mismatches(got_rows, got_src, ref_rows, ref_src, rtol):
    """Mismatch counts between two augment() results of one frame (rows in channel-sorted, stable order)."""
    rec = {"rows_gpu": int(got_rows.shape[0]), "rows_ref": int(ref_rows.shape[0])}
    rec["mismatched_src"] = int(np.setxor1d(got_src, ref_src).size)
    rec["same_order"] = bool(np.array_equal(got_src, ref_src))
    common, ig, ir = np.intersect1d(got_src, ref_src, return_indices=True)
    g, r = got_rows[ig], ref_rows[ir]
    rec["mismatched_labels"] = int((g[:, 4] != r[:, 4]).sum())
    rec["mismatched_intensity"] = int((g[:, 3] != r[:, 3]).sum())
    den = np.maximum(np.abs(r[:, :3].astype(np.float64)), 1e-30)
    rel = np.abs(g[:, :3].astype(np.float64) - r[:, :3].astype(np.float64)) / den
    rec["xyz_max_rel"] = float(rel.max()) if rel.size else 0.0
    rec["xyz_over_tol"] = int((rel > rtol).any(axis=1).sum()) if rel.size else 0
    return rec


def _sum_counts(recs):
    keys = ("mismatched_src", "mismatched_labels", "mismatched_intensity", "xyz_over_tol")
    tot = {k: int(sum(r[k] for r in recs)) for k in keys}
    tot["same_order"] = bool(all(r["same_order"] for r in recs))
    tot["xyz_max_rel"] = float(max(r["xyz_max_rel"] for r in recs))
    tot["rows_gpu"] = int(sum(r["rows_gpu"] for r in recs))
    tot["rows_ref"] = int(sum(r["rows_ref"] for r in recs))
    return tot


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("workload", ["C2", "C2fire", "C2far", "C1", "C4"])
def test_fullsize_parity(workload, dtype, capsys):
    """Every row of N_FRAMES full-size frames: kept-row indices, labels and intensities bit-exact, xyz within 1e-6
    (float32 rows) / 1e-12 (float64 rows) relative, statistics equal."""
    import bench
    from lidar_snow_sim_amd import engine
    from oracle import snow_oracle as so
    layers = bench.WORKLOADS[workload][0]
    n_frames = N_FRAMES if layers == 64 else max(2, N_FRAMES // 2)      # C4 frames hold 4 x the points
    tables = _tables(workload)
    frames, orders = _frames(workload, dtype, n_frames)
    lasers = engine.load_lasers() * (layers // 64)
    rtol = 1e-6 if dtype == np.float32 else 1e-12
    eng = engine.Engine(0, lasers=lasers)          # own context: the largest table drives the capacity-tier choice
    try:
        tids = [eng.table_ids_from_arrays(tables, o) for o in orders]
        rows = np.concatenate(frames)
        off = np.concatenate(([0], np.cumsum([f.shape[0] for f in frames]))).astype(np.int64)
        t0 = time.perf_counter()
        out, src, counts, stats, thr = eng.ctx.augment_batch(rows, off, tids, BD, plane=[[*PLANE[0], PLANE[1]]] * n_frames,
                                                             want_thr=True)
        t_gpu = time.perf_counter() - t0
    finally:
        eng.ctx.close()
    las_o = so.load_lasers() * (layers // 64)
    threads = max(1, min(os.cpu_count() or 1, layers))
    recs, stat_bad, t_cpu, thr_dev = [], 0, 0.0, 0.0
    for f in range(n_frames):
        t0 = time.perf_counter()
        s0, a0, src0, extra = so.augment(frames[f], tables, BD, orders[f], plane=PLANE, lasers=las_o, threads=threads,
                                         return_full=True)
        t_cpu += time.perf_counter() - t0
        n = int(counts[f])
        a = int(off[f])
        recs.append(_count_mismatches(out[a:a + n], src[a:a + n], a0, src0, rtol))
        stat_bad += tuple(int(v) for v in stats[f]) != tuple(int(v) for v in s0)
        dist = np.linspace(3.0, 119.0, 59)
        thr_dev = max(thr_dev, float(np.abs(np.polyval(thr[f], dist) - np.polyval(extra["thr_poly"], dist)).max()))
    tot = _sum_counts(recs)
    tot.update(workload=workload, dtype=np.dtype(dtype).name, frames=n_frames, points=int(off[-1]), mismatched_stats=int(stat_bad),
               max_threshold_deviation=thr_dev, gpu_call_s=round(t_gpu, 3), oracle_s=round(t_cpu, 2), oracle_threads=threads)
    _report(capsys, tot)
    assert tot["mismatched_src"] == 0 and tot["same_order"]
    assert tot["mismatched_labels"] == 0 and tot["mismatched_intensity"] == 0
    assert tot["xyz_over_tol"] == 0
    assert stat_bad == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_fullsize_parity_C3_snow_and_wet_fused(dtype, capsys):
    """C3: full-size C2 sweeps through the fused snowfall + wet-ground entry (snow rows never leave the device) against
    oracle augment() followed by oracle ground_water_augmentation() with the kwargs of pointcloud_viewer.py:2814-2821."""
    from lidar_snow_sim_amd import engine
    from oracle import snow_oracle as so
    tables = _tables("C2")
    frames, orders = _frames("C2", dtype, N_FRAMES)
    n_frames = len(frames)
    wet = dict(water_height=0.0008, pavement_depth=0.001, power_factor=15, flat_earth=False, delta=0.5, replace=False)
    eng = engine.Engine(0)
    try:
        tids = [eng.table_ids_from_arrays(tables, o) for o in orders]
        rows = np.concatenate(frames)
        off = np.concatenate(([0], np.cumsum([f.shape[0] for f in frames]))).astype(np.int64)
        pl = [[*PLANE[0], PLANE[1]]] * n_frames
        out, src, counts, stats, flags = eng.ctx.augment_wet_batch(rows, off, tids, BD, wet_plane=pl, plane=pl, wet_noise_floor=0.7, **wet)
    finally:
        eng.ctx.close()
    threads = max(1, min(os.cpu_count() or 1, 64))
    recs, stat_bad, int_bad, int_max = [], 0, 0, 0.0
    for f in range(n_frames):
        s0, a0, src0 = so.augment(frames[f], tables, BD, orders[f], plane=PLANE, threads=threads)
        o0, wsrc0 = so.ground_water_augmentation(a0, noise_floor=0.7, plane=PLANE, return_src=True, **wet)
        n, a = int(counts[f]), int(off[f])
        got, gsrc, rsrc = out[a:a + n], src[a:a + n], src0[wsrc0]
        rec = _count_mismatches(got, gsrc, o0, rsrc, 1e-6 if dtype == np.float32 else 1e-12)
        # wet-ground intensities are float64 values of a float chain, not integers: relative tolerance
        # (1e-7 on float32 frames, where the laser-power line amplifies float32 rounding; 1e-9 on float64 frames)
        common, ig, ir = np.intersect1d(gsrc, rsrc, return_indices=True)
        tol = 1e-6 if dtype == np.float32 else 1e-9
        rel = np.abs(got[ig, 3] - o0[ir, 3]) / np.maximum(np.abs(o0[ir, 3]), 1e-30)
        int_bad += int((rel > tol).sum())
        int_max = max(int_max, float(rel.max()) if rel.size else 0.0)
        rec["mismatched_intensity"] = int((rel > tol).sum())
        recs.append(rec)
        stat_bad += tuple(int(v) for v in stats[f]) != tuple(int(v) for v in s0)
        assert int(flags[f]) == 0
    tot = _sum_counts(recs)
    tot.update(workload="C3 (snow + wet fused)", dtype=np.dtype(dtype).name, frames=n_frames, points=int(off[-1]),
               mismatched_stats=int(stat_bad), wet_intensity_max_rel=int_max)
    _report(capsys, tot)
    assert tot["mismatched_src"] == 0 and tot["same_order"] and tot["mismatched_labels"] == 0
    assert tot["mismatched_intensity"] == 0 and tot["xyz_over_tol"] == 0 and stat_bad == 0


N_BATCH = int(os.environ.get("SNOWGPU_FULLSIZE_BATCH", "32"))


@pytest.mark.parametrize("workload", ["C2", "C2fire", "C3", "C2f64"])
def test_fullsize_parity_one_device_batch_of_32(workload, capsys):
    """The batch shape of the headline number: N_BATCH (32) full-size float32 sweeps as ONE device-resident batch through the torch-tensor
    boundary (augment_batch on CUDA tensors -> snowgpu_augment_batch_device / snowgpu_augment_wet_batch_device on torch's stream) --
    above the 16-frame switch of the prepass (k_pre_rowmin + k_lean_lines_solve instead of the fused finish), above the four-sweep
    schedule of the received-power phase (k_power_few first, long-tail order, separate compaction scan), none of which a host-entry
    batch reaches (the host pipeline cuts it into chunks of a dozen sweeps).  Every kept row, label and intensity against the threaded
    oracle; C3 = snowfall + wet ground fused (pointcloud_viewer.py:2807-2821)."""
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    from oracle import snow_oracle as so
    fused = workload == "C3"
    dtype = np.float64 if workload == "C2f64" else np.float32          # (C2f64: the same batch as float64 rows)
    wl = "C2" if workload in ("C3", "C2f64") else workload
    tables = _tables(wl)
    frames, orders = _frames(wl, dtype, N_BATCH)
    wet = dict(water_height=0.0008, pavement_depth=0.001, power_factor=15, flat_earth=False, delta=0.5, replace=False)
    dev = torch.device("cuda:0")
    t_frames = [torch.from_numpy(f).to(dev) for f in frames]
    assert sum(f.shape[0] for f in frames) > 16 * 131072
    kw = dict(wet=dict(wet, noise_floor=0.7, plane=PLANE)) if fused else {}
    t0 = time.perf_counter()
    res = augment_batch(t_frames, "unused", BD, planes=[PLANE] * N_BATCH, orders=orders, particles=tables, return_src=True, **kw)
    t_gpu = time.perf_counter() - t0
    assert all(r[1].is_cuda and r[2].is_cuda for r in res)
    threads = max(1, min(os.cpu_count() or 1, 64))
    recs, stat_bad, int_max = [], 0, 0.0
    for f in range(N_BATCH):
        s0, a0, src0 = so.augment(frames[f], tables, BD, orders[f], plane=PLANE, threads=threads)
        st, aug, src = res[f]
        got, gsrc = aug.cpu().numpy(), src.cpu().numpy()
        if fused:
            a0, wsrc0 = so.ground_water_augmentation(a0, noise_floor=0.7, plane=PLANE, return_src=True, **wet)
            src0 = src0[wsrc0]
        rec = _count_mismatches(got, gsrc, a0, src0, 1e-6 if dtype == np.float32 else 1e-12)
        if fused:                                   # wet-ground intensities are float64 values of a float chain: 1e-6 relative on float32 rows
            _, ig, ir = np.intersect1d(gsrc, src0, return_indices=True)
            rel = np.abs(got[ig, 3] - a0[ir, 3]) / np.maximum(np.abs(a0[ir, 3]), 1e-30)
            rec["mismatched_intensity"] = int((rel > 1e-6).sum())
            int_max = max(int_max, float(rel.max()) if rel.size else 0.0)
        recs.append(rec)
        stat_bad += tuple(int(v) for v in st) != tuple(int(v) for v in s0)
    tot = _sum_counts(recs)
    tot.update(workload=f"{workload} (one device batch, tensor boundary)", dtype=np.dtype(dtype).name, frames=N_BATCH, points=int(sum(f.shape[0] for f in frames)),
               mismatched_stats=int(stat_bad), gpu_call_s=round(t_gpu, 3), **({"wet_intensity_max_rel": int_max} if fused else {}))
    _report(capsys, tot)
    assert tot["mismatched_src"] == 0 and tot["same_order"] and tot["mismatched_labels"] == 0
    assert tot["mismatched_intensity"] == 0 and tot["xyz_over_tol"] == 0 and stat_bad == 0


@pytest.mark.parametrize("workload,dtype", [("C2", np.float32), ("C2far", np.float32), ("C2", np.float64)], ids=["C2-float32", "C2far-float32", "C2-float64"])
def test_cpu_twin_and_hip_path_give_the_same_bytes_at_full_size(workload, dtype, capsys):
    """libsnowcpu.so (include/snowgpu_cpu.h) is the kernels' per-beam device code compiled for the host; libsnowgpu.so runs it as a launch
    sequence of wave-level kernels (flattened scan, hand-over queues, capacity tiers, few-flake registers, compaction).  Same source, two
    builds: four full-size sweeps, threshold polynomials from the device prepass -- identical output rows, source indices and statistics."""
    import bench
    from lidar_snow_sim_amd import _cpu_twin, engine
    tables = _tables(workload)
    frames, orders = _frames(workload, dtype, 4)
    eng = engine.Engine(0)
    try:
        tids = [eng.table_ids_from_arrays(tables, o) for o in orders]
        rows = np.concatenate(frames)
        off = np.concatenate(([0], np.cumsum([f.shape[0] for f in frames]))).astype(np.int64)
        out, src, counts, stats, thr = eng.ctx.augment_batch(rows, off, tids, BD, plane=[[*PLANE[0], PLANE[1]]] * 4, want_thr=True)
    finally:
        eng.ctx.close()
    t0 = time.perf_counter()
    res = _cpu_twin.augment_batch(frames, tables, orders, BD, thr)
    t_cpu = time.perf_counter() - t0
    bad = 0
    for f, (st, aug, sidx) in enumerate(res):
        a, n = int(off[f]), int(counts[f])
        same = n == aug.shape[0] and np.array_equal(src[a:a + n], sidx) and out[a:a + n].tobytes() == aug.tobytes() \
            and tuple(int(v) for v in stats[f]) == tuple(int(v) for v in st)
        bad += not same
    _report(capsys, {"test": "cpu twin vs hip path", "workload": workload, "dtype": np.dtype(dtype).name, "frames": 4, "frames_differ": int(bad),
                     "rows_kept": int(counts.sum()), "cpu_twin_s": round(t_cpu, 3), "cpu_twin_points_per_s": round(float(off[-1]) / t_cpu)})
    assert bad == 0


def test_L5_counts_against_the_native_numpy_flavour(golden, tables, capsys):
    """The reference's own numbers depend on NumPy's SIMD dispatch: the product pins the portable
    flavour by default.  This test REPORTS how far the HIP path is from the AVX-512 flavour of the same reference on the L5
    fixtures -- the distance between the reference and itself on another CPU -- and checks the switch that follows the local
    NumPy instead: with q8='numpy' the threshold fit (wet_ground/augmentation.py:236, quirk Q8) is made by this host's
    np.argpartition, and on a host whose NumPy dispatches like the one the native fixtures were made on, what remains is the
    share of SVML's arctan2 / arccos (a last-bit difference in a beam azimuth or an incident angle)."""
    from conftest import numpy_is_portable
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment
    dn = golden("L5_augment", "native")
    dp = golden("L5_augment", "portable")
    tl = [tables["t"][i % 4] for i in range(64)]
    total_default = total_q8 = 0
    for case in range(8):
        pc = dp[f"c{case}_pc"]
        plane = (dp[f"c{case}_plane_w"], float(dp[f"c{case}_plane_h"]))
        stats, aug, src = augment(pc, "unused", float(dp["bd"]), only_camera_fov=False, plane=plane,
                                  order=list(dp[f"c{case}_order"]), particles=tl, return_src=True)
        rec = {"fixture": f"L5 case {case}", "dtype": pc.dtype.name}
        for name, d in (("vs_portable", dp), ("vs_native", dn)):
            o = np.argsort(d[f"c{case}_src"], kind="stable")
            g = np.argsort(src, kind="stable")
            c = _count_mismatches(aug[g], src[g], d[f"c{case}_aug"][o], d[f"c{case}_src"][o], 1e-6)
            rec[name] = {k: c[k] for k in ("mismatched_src", "mismatched_labels", "mismatched_intensity")}
            rec[name]["stats_equal"] = tuple(int(v) for v in stats) == tuple(int(v) for v in d[f"c{case}_stats"])
        s2, a2, src2 = augment(pc, "unused", float(dp["bd"]), only_camera_fov=False, plane=plane,
                               order=list(dp[f"c{case}_order"]), particles=tl, return_src=True, q8="numpy")
        o = np.argsort(dn[f"c{case}_src"], kind="stable")
        g = np.argsort(src2, kind="stable")
        c = _count_mismatches(a2[g], src2[g], dn[f"c{case}_aug"][o], dn[f"c{case}_src"][o], 1e-6)
        rec["q8_numpy_vs_native"] = {k: c[k] for k in ("mismatched_src", "mismatched_labels", "mismatched_intensity")}
        rec["q8_numpy_vs_native"]["stats_equal"] = tuple(int(v) for v in s2) == tuple(int(v) for v in dn[f"c{case}_stats"])
        rec["numpy_dispatch"] = "portable" if numpy_is_portable() else "simd"
        _report(capsys, rec)
        assert rec["vs_portable"]["mismatched_src"] == 0 and rec["vs_portable"]["stats_equal"]
        total_default += rec["vs_native"]["mismatched_src"]
        total_q8 += rec["q8_numpy_vs_native"]["mismatched_src"]
    from conftest import numpy_matches_native_fixtures
    if numpy_matches_native_fixtures():
        # on a NumPy that dispatches like the fixtures' host the switch must bring the product to the local reference: at most a handful of rows left
        assert total_q8 * 20 <= total_default, (total_q8, total_default)


def test_L6_wet_ground_follows_the_local_numpy_with_q8_numpy(golden, capsys):
    """The wet-ground model has the same machine dependence as the snowfall threshold (quirk Q8): the native-flavour L6 fixtures
    keep 572 .. 2515 rows where the portable ones keep 2278 .. 2664.  ground_water_augmentation(..., q8='numpy') fits the two
    lines on the host with this process' NumPy and hands them to the device: on a host whose NumPy dispatches like the one the
    native fixtures were made on, the result is the native fixture's (rows and labels exactly, intensities to 1e-7 / 1e-9)."""
    from conftest import numpy_is_portable
    from lidar_snow_sim_amd.tools.wet_ground.augmentation import ground_water_augmentation
    dn, dp = golden("L6_wet_ground", "native"), golden("L6_wet_ground", "portable")
    plane = (np.array([0.0, 0.0, -1.0]), -1.7)
    kw = dict(water_height=0.0008, pavement_depth=0.001, noise_floor=0.7, power_factor=15, estimation_method="linear", debug=False, delta=0.5)
    bad_default = bad_q8 = 0
    for case in range(int(dn["n_cases"])):
        pc = dn[f"c{case}_pc"]
        args = dict(kw, flat_earth=bool(dn[f"c{case}_flat"]), replace=bool(dn[f"c{case}_replace"]), plane=plane)
        out_first = ground_water_augmentation(pc, **args)
        out_numpy = ground_water_augmentation(pc, q8="numpy", **args)
        ref_n, ref_p = dn[f"c{case}_out"], dp[f"c{case}_out"]
        assert out_first.shape == ref_p.shape and np.array_equal(out_first[:, [0, 1, 2, 4]], ref_p[:, [0, 1, 2, 4]])   # the default: portable
        same_rows = out_numpy.shape == ref_n.shape and np.array_equal(out_numpy[:, [0, 1, 2, 4]], ref_n[:, [0, 1, 2, 4]])
        rel = float(np.max(np.abs(out_numpy[:, 3] - ref_n[:, 3]) / np.maximum(np.abs(ref_n[:, 3]), 1e-300))) if same_rows and len(ref_n) else None
        _report(capsys, {"fixture": f"L6 case {case}", "dtype": pc.dtype.name, "rows_portable": int(ref_p.shape[0]), "rows_native": int(ref_n.shape[0]),
                         "rows_default": int(out_first.shape[0]), "rows_q8_numpy": int(out_numpy.shape[0]), "q8_numpy_rows_equal_native": bool(same_rows),
                         "q8_numpy_intensity_max_rel": rel, "numpy_dispatch": "portable" if numpy_is_portable() else "simd"})
        bad_default += out_first.shape != ref_n.shape
        bad_q8 += not same_rows or (rel is not None and rel > (1e-7 if pc.dtype == np.float32 else 1e-9))
    from conftest import numpy_matches_native_fixtures
    if numpy_matches_native_fixtures():
        assert bad_default > 0 and bad_q8 == 0, (bad_default, bad_q8)


def test_L8_viewer_chain_follows_the_local_numpy_with_q8_numpy(golden, tables, capsys, tmp_path):
    """The viewer chain (pointcloud_viewer.py:2807-2821) with q8='numpy' in both stages against the NATIVE-flavour L8 fixture:
    what the reference prints on a SIMD-dispatching NumPy.  Rows by source index, labels and snowfall intensities exactly."""
    import random
    from conftest import canonical, numpy_is_portable
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment
    from lidar_snow_sim_amd.tools.wet_ground.augmentation import ground_water_augmentation
    from test_oracle_golden import match_rows_by_xyz
    d = golden("L8_viewer_chain", "native")
    tl = [tables["t"][i % 4] for i in range(64)]
    plane = (np.array([0.0, 0.0, -1.0]), -1.7)
    bad = 0
    for case in range(int(d["n_cases"])):
        pc = d[f"c{case}_pc"]
        pc6 = np.column_stack((pc, np.arange(len(pc)))).astype(pc.dtype)
        kw = dict(plane=plane) if bool(d[f"c{case}_inject"]) else {}
        random.seed(int(d[f"c{case}_seed"]))
        stats, snow = augment(pc=pc6, only_camera_fov=False, particle_file_prefix="unused", noise_floor=0.7, particles=tl,
                              beam_divergence=float(np.degrees(3e-3)), shuffle=True, show_progressbar=True, q8="numpy", **kw)
        a1, s1 = canonical(snow[:, :5], snow[:, 5].astype(np.int64))
        a2, s2 = canonical(d[f"c{case}_snow"], d[f"c{case}_snow_src"])
        snow_ok = tuple(int(v) for v in stats) == tuple(int(v) for v in d[f"c{case}_stats"]) and np.array_equal(s1, s2) \
            and np.array_equal(a1[:, 3:], a2[:, 3:])
        out = ground_water_augmentation(snow[:, :5], water_height=0.0008, pavement_depth=0.001, noise_floor=0.7, power_factor=15,
                                        flat_earth=False, estimation_method="linear", debug=False, delta=0.5, replace=False, q8="numpy", **kw)
        ref = d[f"c{case}_out"]
        wet_ok = False
        if snow_ok and out.shape == ref.shape:
            ids = match_rows_by_xyz(out, snow[:, :5], snow[:, 5].astype(np.int64))
            ref_ids = match_rows_by_xyz(ref, d[f"c{case}_snow"], d[f"c{case}_snow_src"])
            o1, o2 = out[np.argsort(ids, kind="stable")], ref[np.argsort(ref_ids, kind="stable")]
            wet_ok = bool(np.array_equal(np.sort(ids), np.sort(ref_ids)) and np.array_equal(o1[:, 4], o2[:, 4])
                          and np.allclose(o1[:, 3], o2[:, 3], rtol=1e-7 if pc.dtype == np.float32 else 1e-9, atol=0))
        _report(capsys, {"fixture": f"L8 native case {case}", "dtype": pc.dtype.name, "snow_equal": bool(snow_ok), "wet_equal": wet_ok,
                         "numpy_dispatch": "portable" if numpy_is_portable() else "simd"})
        bad += not (snow_ok and wet_ok)
    from conftest import numpy_matches_native_fixtures
    if numpy_matches_native_fixtures():
        assert bad == 0


def test_q8_numpy_device_half_keeps_the_rows_of_the_host_fit_at_full_size(capsys):
    """q8='numpy' has two routes to the threshold polynomial: the whole estimate on the host (device_prepass=False:
    noise_threshold_poly, the reference's own NumPy / SciPy calls) and the device half (default: histogram and sums from
    snowgpu_prepass_stats, row minima and the two fits in noise_polys_from_device_stats).  Both must keep the same rows of full
    C2 sweeps -- float32 and float64, channel-major and firing order: the polynomials agree to the rounding of the fit (the
    noise line is fitted with linregress's own expressions on the same compressed arrays; the quadratic from float64 normal
    equations against np.polyfit's SVD), and a row can only flip if its intensity sits within that distance of the threshold."""
    import bench
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    tables = _tables("C2")
    n = max(2, N_FRAMES // 2)
    total = {"frames": 0, "rows_kept": 0, "rows_differ": 0, "max_threshold_deviation": 0.0}
    for workload, dtype in (("C2", np.float32), ("C2fire", np.float32), ("C2", np.float64)):
        frames, orders = _frames(workload, dtype, n)
        planes = [PLANE] * n
        a = augment_batch(frames, "unused", BD, planes=planes, orders=orders, particles=tables, return_src=True, q8="numpy")
        b = augment_batch(frames, "unused", BD, planes=planes, orders=orders, particles=tables, return_src=True, q8="numpy", device_prepass=False)
        for (sa, ra, ia), (sb, rb, ib) in zip(a, b):
            total["frames"] += 1
            total["rows_kept"] += int(ia.shape[0])
            same = ia.shape == ib.shape and np.array_equal(ia, ib)
            total["rows_differ"] += 0 if same else int(np.setxor1d(ia, ib).size)
            if same:
                assert ra.tobytes() == rb.tobytes() and tuple(sa) == tuple(sb)
    _report(capsys, dict(total, test="q8_numpy device half vs host fit"))
    assert total["rows_differ"] == 0


def test_threshold_callback_inside_the_pipelined_call_equals_the_two_call_form(capsys):
    """snowgpu_set_threshold_callback (q8='numpy' since round 6): 40 full-size sweeps = four chunks of the pipelined host entry on two
    lanes; per chunk the library hands histograms and sums to the callback while the chunk's per-beam kernels run and finishes the chunk
    with the callback's polynomials.  Same rows, sources and statistics as the two-call form (snowgpu_prepass_stats, the same selection on
    the host, snowgpu_augment_batch with thr_poly) -- rows transfer and packed transfer, channel-major and firing-order sweeps; a callback
    that raises fails the call with its own exception and leaves the context usable."""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tools.wet_ground.augmentation import noise_polys_from_device_stats
    tables = _tables("C2")
    n = 40
    rec = {"test": "threshold callback vs two calls", "frames": 0, "frames_differ": 0, "callback_groups": 0}
    eng = engine.Engine(0)
    try:
        for workload in ("C2", "C2fire"):
            frames, orders = _frames(workload, np.float32, n)
            tids = [eng.table_ids_from_arrays(tables, o) for o in orders]
            rows = np.concatenate(frames)
            off = np.concatenate(([0], np.cumsum([f.shape[0] for f in frames]))).astype(np.int64)
            planes = [[*PLANE[0], PLANE[1]]] * n
            hist, stats_rec = eng.ctx.prepass_stats(rows, off, plane=planes)
            polys = noise_polys_from_device_stats(hist, stats_rec, 0.7)
            want = eng.ctx.augment_batch(rows, off, tids, BD, thr_poly=polys)
            groups = []

            def fit(first, h, r):
                groups.append((first, h.shape[0]))
                return noise_polys_from_device_stats(h, r, 0.7)

            for mode in ("rows", "packed"):
                eng.ctx.set_result_transfer(mode)
                eng.ctx.set_threshold_callback(fit)
                try:
                    got = eng.ctx.augment_batch(rows, off, tids, BD, plane=planes)
                finally:
                    eng.ctx.set_threshold_callback(None)
                    eng.ctx.set_result_transfer("rows")
                assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
                for f in range(n):
                    a, m = int(off[f]), int(want[2][f])
                    rec["frames"] += 1
                    rec["frames_differ"] += not (got[0][a:a + m].tobytes() == want[0][a:a + m].tobytes() and np.array_equal(got[1][a:a + m], want[1][a:a + m]))
            assert sorted(groups)[0][0] == 0 and sum(g[1] for g in groups) == 2 * n and len(groups) >= 2 * 2          # several groups per call
            rec["callback_groups"] += len(groups)

        def broken(first, h, r):
            raise KeyError("no fit today")

        eng.ctx.set_threshold_callback(broken)
        try:
            with pytest.raises(KeyError):
                eng.ctx.augment_batch(rows, off, tids, BD, plane=planes)
        finally:
            eng.ctx.set_threshold_callback(None)
        again = eng.ctx.augment_batch(rows, off, tids, BD, thr_poly=polys)                   # the context is still good
        assert np.array_equal(again[2], want[2]) and again[0][:int(want[2][0])].tobytes() == want[0][:int(want[2][0])].tobytes()
    finally:
        eng.ctx.close()
    _report(capsys, rec)
    assert rec["frames_differ"] == 0


def test_long_tail_order_of_the_received_power_phase_changes_no_byte(monkeypatch, capsys):
    """Large batches run k_power_few first; where k_power<4> goes after it depends on how many beams the 63-entry / global-list tiers held in
    the batches before (page-locked words the device leaves behind: snowgpu_batch.cpp, `heavy_tail`): behind k_power_few with those tiers
    behind it, or on the caller's stream ahead of the 8-entry tier with those tiers right behind k_power_few.  SNOWGPU_HEAVY_TAIL=0 / 1 forces
    either.  Six C1 sweeps (40 k flakes per line: thousands of beams in the 63-entry tier) in one device-entry batch: both orders, and the
    default called three times in a row (the third call sees the first calls' counts), give the same rows, sources, counts and statistics."""
    from lidar_snow_sim_amd import engine
    tl = _tables("C1")
    frames, orders = _frames("C1", np.float32, 6)
    off = np.concatenate(([0], np.cumsum([f.shape[0] for f in frames]))).astype(np.int64)
    rows = np.concatenate(frames)
    assert rows.shape[0] > (1 << 19)
    results = []
    for v in ("0", "1", None, "0+prepass", "1-prepass"):
        # ("0+prepass" / "1-prepass": the prepass beside k_power_few -- the long-tail order's companion -- forced on in the short-tail order and
        # off in the long-tail one: SNOWGPU_PREPASS_WITH_FEW)
        monkeypatch.delenv("SNOWGPU_PREPASS_WITH_FEW", raising=False)
        if v is None:
            monkeypatch.delenv("SNOWGPU_HEAVY_TAIL", raising=False)
        else:
            monkeypatch.setenv("SNOWGPU_HEAVY_TAIL", v[0])
            if len(v) > 1:
                monkeypatch.setenv("SNOWGPU_PREPASS_WITH_FEW", "1" if v[1] == "+" else "0")
        e = engine.Engine(0)
        try:
            tids = [e.table_ids_from_arrays(tl, o) for o in orders]
            planes = [[*PLANE[0], PLANE[1]]] * len(frames)
            for _ in range(3 if v is None else 1):
                res = e.ctx.augment_batch(rows, off, tids, BD, plane=planes)
                st = e.ctx.last_status()
            results.append((res, st))
        finally:
            e.ctx.close()
    (o0, s0, c0, t0, _), st0 = results[0]
    assert int(st0[4]) + int(st0[5]) > 500, st0                # beams in the 63-entry and the global-list tier
    n = int(c0.sum())
    same = True
    for (o1, s1, c1, t1, _), _ in results[1:]:
        same = same and np.array_equal(c0, c1) and np.array_equal(t0, t1) and np.array_equal(s0[:n], s1[:n]) and o0[:n].tobytes() == o1[:n].tobytes()
    _report(capsys, {"test": "long-tail order vs default order", "rows_kept": n, "tail_beams": int(st0[4]) + int(st0[5]), "same_bytes": bool(same)})
    assert same
