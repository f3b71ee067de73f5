#!/usr/bin/env python3
"""bench.py -- snowfall-augmentation throughput on MI355X, BASELINE.json's metric on its config C2.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--frames F] [--workload C2|C2far|C1|C4|C3|C5] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps (and with --dump-outputs writes what the last one computed) and prints the line.
The side measurements below -- value_pcie_inclusive, single_frame, batches in flight, the counter passes of roofline.traffic / valu,
cpu_baseline / cpu_twin -- take runs and processes of their own and are made with --full only.

`--gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset) re-executes itself under torch.distributed.run with
N ranks on 127.0.0.1, one rank per GPU; it fails loudly if the node has fewer devices.

A "step" is one pass of the hot path -- channel sort, noise-threshold prepass, per-beam occlusion /
received-power simulation, noise-floor filter, compaction, statistics (augment(), simulation.py:427-544,
only_camera_fov=False; workload C3 chains ground_water_augmentation() behind it, pointcloud_viewer.py:2807-2821) --
over one batch of F synthetic sweeps that already sit in HBM when the timed region starts.  Ranks own independent
batches (frames shard with no data-path collective): weak scaling, value = points of all ranks / max time.

Prints ONE JSON line on rank 0:
  value                  points/s with rows resident in HBM: augment_batch() on CUDA tensors (the Python boundary over the device entry of
                         the C ABI, lidar_snow_sim_amd/tensors.py), asynchronous on torch's stream
  value_pcie_inclusive   the same frames through the HOST entry: H2D of the rows and D2H of the results inside the clock
                         (page-locked buffers, ONE context and host thread: the library pipelines upload / kernels / download
                         in chunks), SURVEY 8(d)'s definition of the metric; never `value`
  single_frame           one sweep end to end (upload, all kernels, download, synchronise): through the C ABI with page-locked
                         buffers, and through the Python augment() with a pageable array, as the reference's callers have it
  roofline               per-beam region: achieved = algorithmic bytes / HIP-event time; `traffic` and `valu` from rocprofv3
                         --pmc passes of this same command, run as child processes (--full, N = 1 only; --no-pmc skips them;
                         otherwise `traffic` is the committed profiles/hbm_traffic.json figure where it matches the run)
  cpu_baseline           the CPU oracle on four frames of the same workload (all host cores, and one core)
"""
import argparse
import csv
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

# BASELINE.json's metric, and which of the line's figures `value` is (the round-4 review asked for the string to say so)
METRIC = ("augmented points/s/GPU (64x2048 sweep, 2.5 mm/h); HBM roofline % -- value: rows resident in HBM when the clock starts (device-resident API: "
          "augment_batch on CUDA tensors); "
          "with H2D of the rows and D2H of the results inside the clock: value_pcie_inclusive")
HBM_PEAK = 8.0e12          # B/s, MI355X_MICROARCH.md
PCIE_PEAK = 63.0e9         # B/s per direction, PCIe Gen5 x16 (same guide)
DEFAULT_FRAMES = 256       # sweeps per step and GPU (BASELINE.json's C3 streams 256-frame batches of the C2 sweep)
BEAM_DIV = float(np.degrees(3e-3))
SNOWFALL, VELOCITY = 2.5, 1.6
WET = dict(water_height=0.0008, pavement_depth=0.001, noise_floor=0.7, power_factor=15.0, flat_earth=False, delta=0.5, replace=False)


WORKLOADS = {   # name: (layers, azimuths, snowfall mm/h, terminal velocity m/s, range scale)  -- SURVEY 8 d
    "C2": (64, 2048, 2.5, 1.6, 1.0),       # BASELINE.json configs[1]: the headline workload
    "C2far": (64, 2048, 2.5, 1.6, 1.8),    # same sweep with every range stretched (clipped at 119 m): long scatterer lists
    "C1": (64, 2048, 0.5, 2.0, 1.0),       # configs[0]'s table density (40 k flakes per line)
    "C4": (128, 4096, 10.0, 1.6, 1.0),     # configs[3]: 128 x 4096 dense sweep, heavy snowfall, tiled laser table
    "C3": (64, 2048, 2.5, 1.6, 1.0),       # configs[2]: the C2 sweeps through snowfall + wet ground, fused on the device
    "C2fire": (64, 2048, 2.5, 1.6, 1.0),   # the C2 sweeps with their rows in FIRING order (azimuth-major, the 64 channels interleaved), as the
                                           # sensor writes an STF .bin (precompute.py:78): the channel sort is no longer the identity
}
FIRING_ORDER = {"C2fire"}
REGION_KERNELS = ("k_beams", "k_power", "k_tier")    # the per-beam region of roofline.avg_launch_ms
# rocprofv3's FETCH_SIZE x 1024 B is HALF the bytes a kernel reads on gfx950, for every access shape the engine uses (4- and
# 8-byte streams, 20-byte rows field by field, 64-byte records: ratio 0.5000 each), WRITE_SIZE x 1024 B is exact for streams:
# measured with kernels of known byte counts, scripts/probe/pmc_calib.hip -> profiles/r03_pmc_calibration.json.
FETCH_FACTOR, WRITE_FACTOR = 2.0, 1.0


def dart_line(occ, rate, line):
    from lidar_snow_sim_amd.tools.snowfall import sampling as smp
    return smp.dart_throwing(occ, rate, 80.0, np.random.default_rng(42 + line), "gunn")


def make_tables(n_lines=64, snowfall=SNOWFALL, velocity=VELOCITY, distinct=None, workers=1):
    """dart_throwing(occupancy, rain rate, 80 m, default_rng(42 + line), 'gunn') per line (SURVEY 8 d); cached on disk for
    the child processes of the counter passes (same seeds, same tables).  workers > 1 throws the lines in that many fresh
    (spawned) worker processes side by side -- each line has a generator of its own, so the tables do not depend on the split;
    one core takes ~0.2 s per C2 line.  Only main() asks for it: a spawned worker re-imports its parent's __main__ module,
    which for a script without an `if __name__ == "__main__"` guard would run that script (and open the GPU) again."""
    from lidar_snow_sim_amd.tools.snowfall import sampling as smp
    occ = smp.compute_occupancy(snowfall, velocity)
    rate = smp.snowfall_rate_to_rainfall_rate(snowfall, velocity)
    distinct = n_lines if distinct is None else distinct
    import hashlib
    import inspect
    key = hashlib.sha1(inspect.getsource(smp).encode()).hexdigest()[:12]      # a change of the sampler invalidates the cache
    uid = os.getuid() if hasattr(os, "getuid") else 0
    cache = Path(tempfile.gettempdir()) / f"snowgpu_bench_tables_u{uid}_{key}_{snowfall}_{velocity}_{distinct}.npz"
    tabs = None
    if cache.exists():
        try:
            z = np.load(cache)
            tabs = [z[f"t{i}"] for i in range(distinct)]
        except Exception:
            tabs = None
    if tabs is None:
        lines = list(range(1, distinct + 1))
        workers = min(workers, distinct)
        if workers > 1:
            import multiprocessing
            from concurrent.futures import ProcessPoolExecutor
            with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as ex:   # (spawn: no fork of a process that holds the GPU)
                tabs = list(ex.map(dart_line, [occ] * distinct, [rate] * distinct, lines))
        else:
            tabs = [dart_line(occ, rate, line) for line in lines]
        try:
            tmp = cache.with_suffix(f".{os.getpid()}.npz")
            np.savez(tmp, **{f"t{i}": t for i, t in enumerate(tabs)})
            os.replace(tmp, cache)
        except OSError:
            pass
    return [tabs[i % distinct] for i in range(n_lines)]


def make_frame(layers, azimuths, seed, scale, firing=False):
    from lidar_snow_sim_amd.synthetic import synthetic_sweep, firing_order
    pc = synthetic_sweep(layers, azimuths, seed=seed, intensity="lambert")
    if scale != 1.0:
        r = np.linalg.norm(pc[:, :3].astype(np.float64), axis=1)
        f = np.minimum(r * scale, 119.0) / r
        pc[:, :3] = (pc[:, :3] * f[:, None]).astype(np.float32)
    return firing_order(pc, layers, azimuths) if firing else pc


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cpus():
    """(threads worth starting, description): the logical CPUs this process may run on, capped by a cgroup CPU quota if one is set."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        txt = open("/sys/fs/cgroup/cpu.max").read().split()
        if txt and txt[0] != "max":
            quota = float(txt[0]) / float(txt[1])
    except (OSError, ValueError, IndexError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = q / per if q > 0 else None
        except (OSError, ValueError):
            quota = None
    use = n if quota is None else max(1, min(n, int(quota + 0.999)))
    return use, {"logical_cpus": os.cpu_count(), "affinity": n, "cgroup_cpu_quota": quota}


def short_kernel(name):
    return re.sub(r"\(.*", "", name).replace("void ", "")


def pmc_pass(counters, argv, steps_total):
    """One rocprofv3 --pmc pass of this script (child process, --inner).  Returns {kernel: {counter: mean per step}}."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not Path(exe).exists():
        return None
    out = tempfile.mkdtemp(prefix="snowgpu_pmc_")
    try:
        cmd = [exe, "--pmc", *counters, "--kernel-trace", "-d", out, "-o", "b", "--output-format", "csv", "--",
               sys.executable, str(ROOT / "bench.py"), "--inner", *argv]
        env = dict(os.environ, TMPDIR=tempfile.gettempdir())
        r = subprocess.run(cmd, cwd=tempfile.gettempdir(), env=env, capture_output=True, text=True, timeout=600)
        files = list(Path(out).rglob("*counter_collection.csv"))
        if r.returncode != 0 or not files:
            return None
        acc = {}
        with open(files[0], newline="") as fh:
            for row in csv.DictReader(fh):
                k = short_kernel(row["Kernel_Name"])
                acc.setdefault(k, {}).setdefault(row["Counter_Name"], 0.0)
                acc[k][row["Counter_Name"]] += float(row["Counter_Value"])
        return {k: {c: v / steps_total for c, v in d.items()} for k, d in acc.items()}
    except Exception:
        return None
    finally:
        shutil.rmtree(out, ignore_errors=True)


def spawn_ranks(n, dry):
    """Re-execute this command under torch.distributed.run with n ranks on this node (one per GPU)."""
    import socket
    if not dry:
        import torch
        have = torch.cuda.device_count()
        if have < n:
            raise SystemExit(f"bench.py --gpus {n}: this node exposes {have} GPU(s); refusing to report n_gpus={n}")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), *sys.argv[1:]]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


class DryBackend:
    """`--dry`: stands where libsnowgpu.so stands in lidar_snow_sim_amd.stream, so that the reader / sharding / writer machinery of a
    multi-rank C5 run can be exercised on a machine without a GPU.  It augments nothing: every frame comes back as it went in (and the
    line says "dry": true) -- a harness of this file, not a path of the product."""

    @staticmethod
    def alloc_rows(n_rows):
        return np.empty((n_rows, 5), np.float32)

    @staticmethod
    def augment_batch(frames, prefix, beam_divergence, **kw):
        return [((0, 0, 0), np.array(frames.frame(i), copy=True)) for i in range(len(frames))]


def c5_host_threads(world):
    """Reader / writer / GPU-worker threads of one rank of the C5 stream: the 6 + 8 + 2 a lone rank runs on the 16 CPUs a GPU box grants,
    scaled to this rank's share of the CPUs the process may use (a node's ranks share its cores and its page cache)."""
    usable, info = usable_cpus()
    share = max(1.0, usable / float(world))
    readers = int(os.environ.get("SNOWGPU_C5_READERS", max(1, min(6, round(share * 6 / 16)))))
    writers = int(os.environ.get("SNOWGPU_C5_WRITERS", max(1, min(8, round(share * 8 / 16)))))
    workers = 2 if share >= 4 else 1
    return readers, writers, workers, usable, info


def run_c5(args, rank, local_rank, world, dist, dev, ranks_seen):
    """BASELINE.json configs[4]: a stream of synthetic STF `.bin` frames sharded round-robin over the ranks, each rank through
    lidar_snow_sim_amd.stream (read .bin -> upload -> augment -> download -> write .bin; precompute.py:74-106).  The frame files of
    a rank are hard links to 64 distinct sweeps (bounded disk use; every frame is still read, processed and written); outputs
    are unlinked right after they have been written.  One "step" = the whole stream; value = points of all ranks / max time.
    The line carries every rank's stage times (read / gpu / write thread-seconds, wall) and the host-thread budget: the ranks of a node
    share its cores and its page cache, which is where the scaling curve is expected to bend."""
    import random
    import torch
    from lidar_snow_sim_amd import dist as sdist
    from lidar_snow_sim_amd import stream
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tools.snowfall import sampling as smp
    dry = args.dry
    n_all = args.frames or 10000
    ids = [f"2018-02-03_{i:05d}" for i in range(n_all)]
    mine = sdist.shard_indices(n_all, rank, world)
    shared = args.c5_dir is not None                       # one tree for all ranks (tests look at what every rank wrote); else one per rank
    base = Path(args.c5_dir) if shared else Path(tempfile.mkdtemp(prefix=f"snowgpu_c5_r{rank}_"))
    lidar = base / "lidar_hdl64_strongest"
    lidar.mkdir(parents=True, exist_ok=True)
    layers, azimuths = (64, 2048) if not dry else (64, 64)             # (dry: small sweeps -- the GPU work is what is skipped)
    try:
        n_dist = min(64, max(len(mine), 1))
        for i in range(n_dist):
            synthetic_sweep(layers, azimuths, seed=1000 + rank * 64 + i, intensity="lambert").tofile(lidar / f"src_r{rank}_{i:05d}.bin")
        for k, i in enumerate(mine):
            os.link(lidar / f"src_r{rank}_{k % n_dist:05d}.bin", lidar / f"{ids[i]}.bin")
        occ, rate = smp.compute_occupancy(SNOWFALL, VELOCITY), smp.snowfall_rate_to_rainfall_rate(SNOWFALL, VELOCITY)
        prefix = f"gunn_{rate}_{occ}"
        tables = None if dry else make_tables(64, SNOWFALL, VELOCITY)
        readers, writers, workers, usable, cpu_info = c5_host_threads(world)
        kw = dict(modes=("gunn",), combos=[(rate, occ)], batch=64 if not dry else 8, particles_by_prefix=None if dry else {prefix: tables},
                  planes=([0.0, 0.0, -1.0], -1.7), workers=workers, readers=readers, writers=writers, keep_outputs=args.c5_keep, device=local_rank,
                  backend=DryBackend() if dry else None)

        def sync():
            if not dry:
                torch.cuda.synchronize()
            if dist is not None:
                dist.barrier()

        sync()                                                                # every rank's input files exist before any rank plans
        if not dry:
            random.seed(0)                                                    # warm-up: table upload, allocations, page-locked pools
            stream.run(lidar, [ids[i] for i in mine[:128]], **kw)
            sync()
        rep = {}
        random.seed(1)
        t0 = time.perf_counter()
        n_files = stream.run(lidar, ids, rank=rank, world=world, report=rep, **kw)
        if not dry:
            torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        elapsed = sdist.max_over_ranks(wall, device=dev)
        tot = sdist.sum_over_ranks([n_files, rep["points_in"], rep["points_out"]], device=dev)
        # every rank's stage times, gathered by a sum of one-hot rows (no collective the barrier / max / sum above did not need already)
        mat = [0.0] * (4 * world)
        mat[4 * rank:4 * rank + 4] = [rep["read_s"], rep["gpu_s"], rep["write_s"], wall]
        mat = sdist.sum_over_ranks(mat, device=dev)
        per_rank = [{"rank": r, "read_s": mat[4 * r], "gpu_s": mat[4 * r + 1], "write_s": mat[4 * r + 2], "wall_s": mat[4 * r + 3]} for r in range(world)]
        seen = ranks_seen()
        if rank == 0:
            threads_all = world * (readers + writers + workers + 2)
            print(json.dumps({
                "metric": METRIC, "value": tot[1] / elapsed, "unit": "points/s",
                "n_gpus": world, "steps": 1, "warmup": 1, "ms_per_step": elapsed * 1e3, "higher_is_better": True, "scaling": "strong",
                "vs_baseline": None, "dtype": "f64", "data": "synthetic", **({"dry": True} if dry else {}),
                "config": {"workload": f"C5: {n_all}-frame synthetic STF stream ({layers} x {azimuths} float32 .bin files), 2.5 mm/h @ 1.6 m/s gunn tables, "
                                       "sharded round-robin over the ranks, file read + H2D + augment + D2H + file write inside the clock"
                                       + (" -- DRY: no GPU work, frames pass through unchanged" if dry else ""),
                           "frames": n_all, "files_written": int(tot[0]), "files_per_s": tot[0] / elapsed, "points_out": int(tot[2]),
                           "sharding": f"frame-parallel x{world}, no collective", "ranks_seen": seen, "batch": kw["batch"],
                           "stage_busy_s_per_rank": per_rank, "rank0_stage_busy_s": {k: rep[k] for k in ("read_s", "gpu_s", "write_s")},
                           "host": {"logical_cpus": os.cpu_count(), "cpus_usable": usable, "cpu_info": cpu_info,
                                    "threads_per_rank": {"readers": readers, "gpu_workers": workers, "writers": writers, "feeder_drainer": 2},
                                    "threads_all_ranks": threads_all, "threads_per_usable_cpu": threads_all / max(usable, 1),
                                    "note": "reader / writer threads per rank are capped to this rank's share of the usable CPUs (6 + 8 on the 16 of "
                                            "a one-GPU box); the ranks of a node share its page cache: wall_s of the slowest rank against its own "
                                            "read_s + write_s shows where the host, not the GPU, sets the pace"}},
                "per_gpu_value": tot[1] / elapsed / world}), flush=True)
    finally:
        if dist is not None:
            dist.barrier()
        if not shared:
            shutil.rmtree(base, ignore_errors=True)
    if dist is not None:
        dist.destroy_process_group()


def measure_host_entry(W):
    """value_pcie_inclusive and single_frame: the same frames through the HOST entry, in a child process without PyTorch and in process."""
    args, eng, torch, dist, dev, distributed, world, rank, local_rank = W.args, W.eng, W.torch, W.dist, W.dev, W.distributed, W.world, W.rank, W.local_rank
    F, n_per, n_total, host_rows, table_ids, planes, fused_wet, barrier = W.F, W.n_per, W.n_total, W.host_rows, W.table_ids, W.planes, W.fused_wet, W.barrier
    out_rows, out_counts, out_stats = W.out_rows, W.out_counts, W.out_stats
    # ---- the same frames through the HOST entry: H2D + D2H inside the clock (SURVEY 8 d; precompute.py:78 / :106 are the
    # reference's boundary).  ONE host thread, ONE context: snowgpu_augment_batch pipelines upload / kernels / download in
    # chunks of whole frames on its own streams.  Measured in a CHILD process that never loads PyTorch (scripts/pcie_bench.py):
    # the C ABI does not need it, and inside a process that has initialised PyTorch the HIP runtime moves device-to-host copies
    # with a full-grid blit kernel instead of the DMA engine (traced), which stalls every kernel beside it.  The in-process
    # figure is reported next to it.
    pcie, single = None, None
    if not args.no_pcie and not fused_wet and args.tables == "host":
        child = None
        try:
            env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
            barrier()
            r = subprocess.run([sys.executable, str(ROOT / "scripts" / "pcie_bench.py"), "--frames", str(F), "--reps", str(max(1, min(args.steps, 4))),
                                "--workload", args.workload, "--device", str(local_rank), "--seed-base", str(1000 + rank * F)],
                               capture_output=True, text=True, timeout=900, env=env)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            child = json.loads(lines[-1]) if r.returncode == 0 and lines else None
        except Exception:
            child = None
        # in-process (PyTorch initialised): same call, for comparison and as the fallback
        pin_in = eng.ctx.pinned_empty((n_total, 5), np.float32)
        pin_in[...] = host_rows
        pin_out = eng.ctx.pinned_empty((n_total, 5), np.float32)
        pin_src = eng.ctx.pinned_empty(n_total, np.int32)
        h_off = np.arange(F + 1, dtype=np.int64) * n_per
        h_ids = np.asarray(table_ids, np.int32)
        h_planes = np.asarray(planes, np.float64)

        def host_call(want_src=True):
            return eng.ctx.augment_batch(pin_in, h_off, h_ids, BEAM_DIV, plane=h_planes, out_rows=pin_out, out_src=pin_src, want_src=want_src)

        host_call(True)
        barrier()
        c0 = time.perf_counter()
        _, _, h_counts, h_stats, _ = host_call(True)
        inproc_s = time.perf_counter() - c0
        d_counts = out_counts.cpu().numpy()
        host_same = bool(np.array_equal(h_counts, d_counts) and np.array_equal(h_stats, out_stats.cpu().numpy())
                         and all(np.array_equal(pin_out[f * n_per:f * n_per + int(d_counts[f])],
                                                out_rows[f * n_per:f * n_per + int(d_counts[f])].cpu().numpy()) for f in (0, F // 2, F - 1)))
        digest = [int(h_counts.sum()), int(h_stats[:, 0].sum()), int(h_stats[:, 1].sum()), int(h_stats[:, 2].sum()),
                  float(pin_out[:int(h_counts[0]), 3].sum()), int(pin_src[:int(h_counts[0])].astype(np.int64).sum())]
        dp = (child or {}).get("default_plane") or {}
        mine = [child["points_per_s"], child["points_per_s_without_src"]] if child else [n_total / inproc_s, n_total / inproc_s]
        mine += [dp.get("c_abi_points_per_s_reference", 0.0), dp.get("c_abi_points_per_s_lsq", 0.0)]
        pk_all = (child or {}).get("packed") or {}
        pk_key = next(iter(pk_all), None)                   # first entry: the library's default thread count
        pk = pk_all.get(pk_key) if pk_key else None
        mine += [pk["points_per_s"] if pk else 0.0]
        if distributed:
            tt = torch.tensor(mine, dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.SUM)
            mine = [float(v) for v in tt.tolist()]
        pcie = {"value": mine[4] if pk else mine[0], "value_rows_transfer": mine[0], "value_rows_transfer_without_src": mine[1],
                "transfer": ("packed (snowgpu_set_result_transfer(ctx, 1, 0)): per kept row its source row | label and its intensity cross the link, "
                             "the moved coordinates of scattered rows apart; " + str(pk_key) + " host threads of the library assemble the caller's rows "
                             "from those and from its input rows -- same bytes in the caller's buffers as the rows transfer") if pk else "rows",
                "packed_by_host_threads": pk_all or None,
                "compact_input": (child or {}).get("compact_input"),
                "steps": max(1, min(args.steps, 4)),
                "process_affinity": (child or {}).get("process_affinity"),
                "frames_per_call": F, "contexts": 1, "host_threads": 1, "process": "child without PyTorch (scripts/pcie_bench.py)" if child else "in process",
                "bytes_per_point": {"h2d": 20, "h2d_compact_input": 17, "d2h_packed": 9.5, "d2h_rows": 24, "d2h_rows_without_src": 20},
                "link_bound_points_per_s": {"upload_20B": PCIE_PEAK / 20.0 * world, "download_rows_24B": PCIE_PEAK / 24.0 * world,
                                            "download_rows_without_src_20B": PCIE_PEAK / 20.0 * world},
                "frac_of_link_bound": {"packed_vs_upload_bound": (mine[4] / (PCIE_PEAK / 20.0 * world)) if pk else None,
                                       "rows_vs_download_bound": mine[0] / (PCIE_PEAK / 24.0 * world),
                                       "rows_without_src_vs_download_bound": mine[1] / (PCIE_PEAK / 20.0 * world)},
                "in_process_with_pytorch": n_total / inproc_s,
                "matches_device_entry": host_same and (child is None or child["digest"] == digest) and (pk is None or bool(pk.get("same_digest_as_rows_mode"))),
                "q8_numpy": (child or {}).get("q8_numpy"),
                "default_plane": dp or None, "default_plane_all_ranks": {"reference": mine[2], "lsq": mine[3]} if dp else None,
                "note": "snowgpu_augment_batch (host pointers) on frames held in page-locked memory, one call per step: the library streams "
                        "all uploads through one DMA queue, computes chunk after chunk and downloads chunk c while chunk c + 1 computes "
                        "(snowgpu_set_pipeline); ceilings at 63 GB/s per direction: 20 B per point up; 24 B per point down with the rows "
                        "transfer (20 with out_src = NULL), ~9.5 with the packed one, which the upload then bounds"}
        if child and rank == 0:
            single = {"c_abi_pinned": {"ms": child["single_frame_c_abi_ms"], "min_ms": child["single_frame_c_abi_min_ms"],
                                       "points_per_s": n_per / (child["single_frame_c_abi_ms"] * 1e-3)},
                      "python_augment_pageable": {"ms": child["single_frame_python_ms"], "min_ms": child["single_frame_python_min_ms"],
                                                  "points_per_s": n_per / (child["single_frame_python_ms"] * 1e-3)},
                      "python_augment_default": {"ms": child.get("single_frame_python_default_ms"), "min_ms": child.get("single_frame_python_default_min_ms"),
                                                 "note": "augment(pc, prefix, bd, only_camera_fov=False) with no plane and no order: calculate_plane on the "
                                                         "device by the default method (the plane the reference returns today), random.shuffle on the host"},
                      "python_augment_lsq_plane": {"ms": child.get("single_frame_python_lsq_ms"), "min_ms": child.get("single_frame_python_lsq_min_ms")},
                      "points": n_per,
                      "note": "median of 40 calls, one 64 x 2048 sweep per call, upload + all kernels + download + synchronise inside the clock "
                              "(child process without PyTorch)"}

    return pcie, single


def batches_in_flight(args, lanes, queues):
    """The same steps with `lanes` batches in flight (compute lanes of the tensor boundary: one engine context and ONE stream each), in a child
    process.  queues = None: the process as it is -- the HIP runtime serves its default of four hardware queues per stream priority, and the
    boundary puts its lanes on streams of different priorities so that they do not share one (snowgpu_lane_stream).  queues = 32:
    GPU_MAX_HW_QUEUES=32, every lane a queue of its own at ONE priority; with that many queues ONE batch on its four streams is slower, so it
    is a deployment of its own.  Both are measured apart from `value`, and BEFORE this process opens the device: two processes' queues on
    one GPU take turns."""
    try:
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        if queues:
            env["GPU_MAX_HW_QUEUES"] = str(queues)
        cmd = [sys.executable, str(ROOT / "bench.py"), "--lanes", str(lanes), "--steps", str(20 * lanes), "--warmup", str(4 * lanes),
               "--workload", args.workload, "--tables", args.tables, "--no-pmc", "--no-pcie", "--no-cpu-baseline"] + (["--frames", str(args.frames)] if args.frames else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        d = json.loads(lines[-1]) if r.returncode == 0 and lines else None
        if not d:
            return None
        return {"lanes": lanes, "value": d["value"], "ms_per_step": d["ms_per_step"], "steps": d["steps"],
                "hw_queues": queues or "runtime default (4 per stream priority)"}
    except Exception:
        return None


def counter_passes(W, alg_bytes):
    """roofline.traffic / traffic_detail / valu: rocprofv3 --pmc child passes of this command (FETCH_SIZE, WRITE_SIZE, SQ counters), or the committed figures."""
    args, F, world = W.args, W.F, W.world
    traffic, traffic_src, valu = None, None, None
    inner_argv = ["--steps", "2", "--warmup", "1", "--frames", str(F), "--workload", args.workload, "--tables", args.tables]
    if not args.no_pmc and world == 1:
        # (a child runs the first call of the size, one warm-up and two timed steps: four launch sequences per kernel)
        fetch = pmc_pass(["FETCH_SIZE"], inner_argv, 4)
        write = pmc_pass(["WRITE_SIZE"], inner_argv, 4) if fetch else None
        sq = pmc_pass(["SQ_ACTIVE_INST_VALU", "SQ_THREAD_CYCLES_VALU", "SQ_BUSY_CYCLES", "SQ_WAVES", "SQ_INSTS_VALU", "SQ_WAVE_CYCLES"],
                      inner_argv, 4) if write else None
        if fetch and write:
            in_region = lambda k: k.startswith(REGION_KERNELS)      # noqa: E731
            fb = sum(v.get("FETCH_SIZE", 0.0) for k, v in fetch.items() if in_region(k)) * 1024 * FETCH_FACTOR
            wb = sum(v.get("WRITE_SIZE", 0.0) for k, v in write.items() if in_region(k)) * 1024 * WRITE_FACTOR
            traffic = fb + wb
            whole = (sum(v.get("FETCH_SIZE", 0.0) for v in fetch.values()) * FETCH_FACTOR
                     + sum(v.get("WRITE_SIZE", 0.0) for v in write.values()) * WRITE_FACTOR) * 1024
            traffic_src = {"source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate child passes of this command (--steps 2 --warmup 1), "
                                     "kernels k_beams* / k_power* / k_tier*; counter x 1024 B x calibration factor (FETCH_SIZE x 2.0, "
                                     "WRITE_SIZE x 1.0: kernels of known byte counts, profiles/r03_pmc_calibration.json)",
                           "fetch_bytes": fb, "write_bytes": wb, "whole_step_bytes": whole,
                           "whole_step_over_algorithmic": whole / alg_bytes}
            dump = os.environ.get("SNOWGPU_BENCH_PMC_DUMP")
            if dump:                                    # per-kernel table for profiles/ (scripts/collect_profiles.sh)
                with open(dump, "w") as fh:
                    fh.write("kernel,FETCH_SIZE_KB_per_step_raw,WRITE_SIZE_KB_per_step_raw,read_bytes_per_step_calibrated,written_bytes_per_step\n")
                    for k in sorted(set(fetch) | set(write)):
                        f_kb, w_kb = fetch.get(k, {}).get("FETCH_SIZE", 0.0), write.get(k, {}).get("WRITE_SIZE", 0.0)
                        fh.write('"%s",%.1f,%.1f,%.0f,%.0f\n' % (k, f_kb, w_kb, f_kb * 1024 * FETCH_FACTOR, w_kb * 1024 * WRITE_FACTOR))
        if sq:
            dom = max((k for k in sq if k.startswith("k_beams")), key=lambda k: sq[k].get("SQ_INSTS_VALU", 0.0), default=None)
            if dom:
                d = sq[dom]
                valu = {"kernel": dom,
                        "lane_utilisation": d["SQ_THREAD_CYCLES_VALU"] / (64.0 * d["SQ_ACTIVE_INST_VALU"]) if d.get("SQ_ACTIVE_INST_VALU") else None,
                        "valu_instructions_per_wave": d["SQ_INSTS_VALU"] / d["SQ_WAVES"] if d.get("SQ_WAVES") else None,
                        "valu_issue_share_of_wave_cycles": d["SQ_ACTIVE_INST_VALU"] / d["SQ_WAVE_CYCLES"] if d.get("SQ_WAVE_CYCLES") else None,
                        "note": "SQ counters of the dominant kernel (rocprofv3 --pmc child pass): the path is bound by VALU issue and "
                                "latency, not by HBM -- these are the figures to read beside frac"}
    if traffic is None:
        pmc = ROOT / "profiles" / "hbm_traffic.json"
        if pmc.exists():
            try:
                rec = json.loads(pmc.read_text())
                if rec.get("frames") == F and rec.get("workload", "C2") == args.workload:
                    traffic = rec.get("bytes_per_launch")
                    traffic_src = {"source": "profiles/hbm_traffic.json (committed rocprofv3 passes of this command)"}
            except Exception:
                traffic = None
    return traffic, traffic_src, valu


def cpu_legs(W):
    """cpu_baseline (the oracle, kind "port") and cpu_twin (libsnowcpu.so) on a bounded sample of the batch, and the GPU's frames checked against both."""
    args, eng, torch = W.args, W.eng, W.torch
    F, n_per, layers, frames, orders, tables, plane, planes, table_ids, host_rows, fused_wet = W.F, W.n_per, W.layers, W.frames, W.orders, W.tables, W.plane, W.planes, W.table_ids, W.host_rows, W.fused_wet
    out_rows, out_src, out_counts, out_stats = W.out_rows, W.out_src, W.out_counts, W.out_stats
    out = {}
    from oracle import snow_oracle as so
    # (i) one host core on frame 0; (ii) ALL logical CPUs on frames 0..15 through the pthread driver of
    # oracle/snow_oracle.c (work item = 256 beams of one (frame, channel); SURVEY 8 d).  The prepass (NumPy, one core,
    # ~15 ms per frame) is inside both clocks, as it is inside the reference's augment().
    cores, cpu_info = usable_cpus()
    n_cpu = min(16, F)
    las = so.load_lasers() * (layers // 64)
    c0 = time.perf_counter()
    so.augment(frames[0], tables, BEAM_DIV, orders[0], plane=plane, lasers=las)
    one_s = time.perf_counter() - c0
    c0 = time.perf_counter()
    refs, used = so.augment_many(frames[:n_cpu], tables, BEAM_DIV, orders[:n_cpu], planes=[plane] * n_cpu, lasers=las, threads=cores)
    cpu_s = time.perf_counter() - c0
    same = True
    for fi in range(min(4, n_cpu)):
        s_ref, a_ref, src_ref = refs[fi]
        if fused_wet:
            a_ref, wsrc = so.ground_water_augmentation(a_ref, water_height=WET["water_height"], pavement_depth=WET["pavement_depth"],
                                                       noise_floor=WET["noise_floor"], power_factor=WET["power_factor"],
                                                       flat_earth=WET["flat_earth"], delta=WET["delta"], replace=WET["replace"],
                                                       plane=plane, return_src=True)
            src_ref = src_ref[wsrc]
        n0 = int(out_counts[fi].item())
        lo = fi * n_per
        got = out_rows[lo:lo + n0].cpu().numpy()
        got_src = out_src[lo:lo + n0].cpu().numpy()
        ok = n0 == a_ref.shape[0] and np.array_equal(got_src, src_ref) and np.array_equal(got[:, 4], a_ref[:, 4]) \
            and np.allclose(got[:, :3], a_ref[:, :3], rtol=1e-6, atol=0)
        ok = ok and (np.allclose(got[:, 3], a_ref[:, 3], rtol=1e-6, atol=0) if fused_wet else np.array_equal(got[:, 3], a_ref[:, 3]))
        if not fused_wet:
            ok = ok and tuple(int(v) for v in out_stats[fi].cpu().numpy()) == tuple(int(v) for v in s_ref)
        same = same and bool(ok)
    # (iii) the build's own CPU twin (libsnowcpu.so: the kernels' per-beam device code compiled for the host, binned tables and all;
    # include/snowgpu_cpu.h, SURVEY 8 b / 8 d) on the same frames, every usable CPU and one; the polynomials are the device prepass's
    twin = None
    if not fused_wet:
        try:
            from lidar_snow_sim_amd import _cpu_twin
            pin_rows = eng.ctx.pinned_empty((n_cpu * n_per, 5), np.float32)
            pin_rows[...] = host_rows[:n_cpu * n_per]
            _, _, _, _, thr_dev = eng.ctx.augment_batch(pin_rows, np.arange(n_cpu + 1, dtype=np.int64) * n_per, np.asarray(table_ids[:n_cpu], np.int32), BEAM_DIV,
                                                        plane=np.asarray(planes[:n_cpu], np.float64), want_thr=True, want_src=False)
            _cpu_twin.augment_batch(frames[:1], tables, orders[:1], BEAM_DIV, thr_dev[:1], lasers=las, threads=cores)      # (loads the library, files nothing twice)
            c0 = time.perf_counter()
            tw = _cpu_twin.augment_batch(frames[:n_cpu], tables, orders[:n_cpu], BEAM_DIV, thr_dev, lasers=las, threads=cores)
            tw_s = time.perf_counter() - c0
            c0 = time.perf_counter()
            _cpu_twin.augment_batch(frames[:1], tables, orders[:1], BEAM_DIV, thr_dev[:1], lasers=las, threads=1)
            tw1_s = time.perf_counter() - c0
            tw_same = True
            for fi in range(n_cpu):
                n0, lo = int(out_counts[fi].item()), fi * n_per
                tw_same = tw_same and n0 == tw[fi][1].shape[0] and out_rows[lo:lo + n0].cpu().numpy().tobytes() == tw[fi][1].tobytes() \
                    and np.array_equal(out_src[lo:lo + n0].cpu().numpy(), tw[fi][2])
            twin = {"value": n_cpu * n_per / tw_s, "unit": "points/s", "cores": cores, "single_core_value": n_per / tw1_s,
                    "kind": "the build's own restatement: libsnowcpu.so = the HIP kernels' per-beam device code (csrc/sg_beam.h, sg_table_host.h, sg_row.h) "
                            "compiled for the host, one beam at a time on host threads (include/snowgpu_cpu.h); table filing inside the clock, "
                            "threshold polynomials given (the device prepass's)",
                    "sample": f"frames 0..{n_cpu - 1} of the batch, {tw_s:.2f} s on {cores} threads; one thread on frame 0: {tw1_s:.2f} s",
                    "same_bytes_as_gpu": bool(tw_same)}
        except Exception as ex:      # the twin is a side measurement: the line does not depend on it
            twin = {"error": repr(ex)}
    if twin is not None:
        out["cpu_twin"] = twin
    out["cpu_baseline"] = {"value": n_cpu * n_per / cpu_s, "unit": "points/s", "cores": used, "kind": "port",
                              "cpu_model": cpu_model(), "host_logical_cpus": os.cpu_count(), "host_cpus_usable": cpu_info,
                              "sample": f"frames 0..{n_cpu - 1} of the batch ({n_cpu * n_per} points): oracle/snow_oracle.c (scalar C "
                                        f"restatement, per-beam scan of the whole table, float64) under its pthread driver -- work item = "
                                        f"256 beams of one (frame, channel), {used} threads = every CPU this process may use "
                                        f"(affinity / cgroup quota) -- plus the NumPy frame driver, {cpu_s:.1f} s wall; one core on frame 0: "
                                        f"{n_per / one_s:.0f} points/s ({one_s:.1f} s)",
                              "single_core_value": n_per / one_s,
                              "gpu_output_matches": bool(same),
                              # context only (SURVEY 8 d): the reference's own NumPy / Python path cannot run on the GPU box; BASELINE.md holds what it
                              # measured in the build container (8 vCPU, one 64 x 2048 sweep at 0.5 mm/h)
                              "reference_numpy_path_in_build_container": {"points_per_s_thread_pool_default": 229, "points_per_s_process_pool_8_vcpu": 5681,
                                                                           "points_per_s_single_thread_per_beam_loop": 400, "source": "BASELINE.md"}}
    return out


DUMP_BUDGET = 48 << 20      # bytes of sampled rows + source indices; counts, stats and flags of every frame come on top (a few KB)


def dump_outputs(r, F, n_per, out):
    """--dump-outputs: what the caller of augment_batch(..., sync=False) receives from the last timed step (a DeviceResult, the device
    synchronised): counts.npy and stats.npy of all F frames, flags.npy with the fused wet ground, and for a seeded sample of frames
    (frames.npy, ascending) their kept rows (rows.npy, the result's dtype) and the frame-local source row of each (src.npy)."""
    out.mkdir(parents=True, exist_ok=True)
    counts = r.counts.cpu().numpy()
    rows_bytes = n_per * (5 * r.rows.element_size() + 8)
    sel = np.sort(np.random.default_rng(0).choice(F, max(1, min(F, DUMP_BUDGET // rows_bytes)), replace=False))
    kept = [(int(r.offsets[f]), int(counts[f])) for f in sel]
    arrays = {"counts": counts.astype(np.float64), "stats": r.stats.cpu().numpy().astype(np.float64), "frames": sel.astype(np.float64),
              "rows": np.concatenate([r.rows[a:a + n].cpu().numpy() for a, n in kept]),
              "src": np.concatenate([r.src[a:a + n].cpu().numpy() for a, n in kept]).astype(np.float64)}
    if r.flags is not None:
        arrays["flags"] = r.flags.cpu().numpy().astype(np.float64)
    for name, a in arrays.items():
        np.save(out / f"{name}.npy", a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=None, help=f"frames per batch and GPU (default {DEFAULT_FRAMES}); C5: frames of the whole stream (default 10000)")
    ap.add_argument("--full", action="store_true",
                    help="also the side measurements: batches in flight and host entry (PCIe-inclusive) and single frame (both dropped by --no-pcie), "
                         "rocprofv3 counter passes (--no-pmc), CPU oracle and CPU twin (--no-cpu-baseline); without it a run times the steps and "
                         "prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float32 / float64, rank 0's batch): "
                         "counts and stats of every frame, the kept rows and source indices of a fixed, seeded sample of frames")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 counter passes (roofline.traffic / valu from profiles/)")
    ap.add_argument("--no-pcie", action="store_true", help="skip the host-entry (PCIe-inclusive) and single-frame measurements")
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)       # child of a counter pass: timed loop only
    ap.add_argument("--host-prepass", action="store_true", help="feed precomputed threshold polynomials (debug)")
    ap.add_argument("--workload", default="C2", choices=sorted(WORKLOADS) + ["C5"], help="C2 (default) is BASELINE.json's metric config")
    ap.add_argument("--dry", action="store_true", help="launch logic only: gloo on CPU, no GPU work (tests)")
    ap.add_argument("--c5-dir", default=None, help="C5: one input / output tree shared by all ranks (default: a temporary one per rank)")
    ap.add_argument("--c5-keep", action="store_true", help="C5: keep the written files (default: unlink each right after the write)")
    ap.add_argument("--lanes", type=int, default=1, help="batches in flight in the timed loop (compute lanes of the tensor boundary; 1: each step waits for the one before it)")
    ap.add_argument("--tables", default="host", choices=("host", "device"),
                    help="host: dart_throwing on the host (bit-exact mirror of sampling.py), uploaded once; device: sampled and filed on the GPU "
                         "(snowgpu_sample_table, seed = f(prefix, line)): no table ever crosses the link; reports sampler throughput")
    args = ap.parse_args()
    if args.inner or not args.full:
        args.no_cpu_baseline = args.no_pmc = args.no_pcie = True
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")
    if args.dump_outputs and (args.dry or args.workload == "C5"):
        raise SystemExit("--dump-outputs: a --dry run computes nothing, and C5 writes its outputs as .bin files (--c5-dir, --c5-keep)")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, args.dry))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} launched with WORLD_SIZE={world}: the two must agree")
    distributed = world > 1
    bif = bif_default = None
    if world == 1 and args.lanes == 1 and not (args.no_pcie or args.dry or args.workload == "C5" or args.host_prepass):
        bif = batches_in_flight(args, 3, 32)
        bif_default = batches_in_flight(args, 2, None)
    import torch
    dist = None
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dry:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    dev = torch.device("cpu") if args.dry else torch.device("cuda", local_rank)
    if not args.dry:
        torch.cuda.set_device(local_rank)

    def ranks_seen():
        """Every rank adds 1: the collective library's own count of the ranks behind the barrier."""
        if not distributed:
            return 1
        t = torch.ones(1, dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return int(t.item())

    if args.dry and args.workload == "C5":
        return run_c5(args, rank, local_rank, world, dist, dev, ranks_seen)
    if args.dry:
        # the launch / sharding / reduction logic of a multi-rank run without a GPU: seeds per rank, barrier, max over ranks
        from lidar_snow_sim_amd import dist as sdist
        F = args.frames or DEFAULT_FRAMES
        seeds = sdist.bench_frame_seeds(rank, F)
        if distributed:
            dist.barrier()
        t0 = time.perf_counter()
        time.sleep(0.01 * (rank + 1))
        elapsed = sdist.max_over_ranks(time.perf_counter() - t0)
        seen = ranks_seen()
        if rank == 0:
            print(json.dumps({"metric": METRIC, "value": 0.0, "unit": "points/s",
                              "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed * 1e3,
                              "higher_is_better": True, "scaling": "weak", "dry": True, "ranks_seen": seen, "backend": "gloo" if distributed else None,
                              "first_seed_of_rank0": seeds[0], "frames_per_step_per_gpu": F}), flush=True)
        if distributed:
            dist.barrier()
            dist.destroy_process_group()
        return
    if args.workload == "C5":
        return run_c5(args, rank, local_rank, world, dist, dev, ranks_seen)
    if args.frames is None:
        args.frames = DEFAULT_FRAMES

    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tools.wet_ground.augmentation import noise_threshold_poly

    layers, azimuths, snowfall, velocity, rscale = WORKLOADS[args.workload]
    fused_wet = args.workload == "C3"
    host_workers = max(1, min(16, usable_cpus()[0]) // world)       # set-up threads / processes: this rank's share of a 16-CPU grant
    eng = engine.get_engine(local_rank)
    if layers != 64:                                       # SURVEY 8 d: 128-entry laser table = the 64-entry one tiled
        eng.set_lasers(engine.load_lasers() * (layers // 64))
    sampler = None
    if args.tables == "device":
        from lidar_snow_sim_amd.tools.snowfall import sampling as smp
        occ, rate = smp.compute_occupancy(snowfall, velocity), smp.snowfall_rate_to_rainfall_rate(snowfall, velocity)
        prefix = f"gunn_{rate}_{occ}"
        eng.keep_sampled_rows = not args.no_cpu_baseline            # the CPU oracle needs the rows the device made
        torch.cuda.synchronize()
        c0 = time.perf_counter()
        dev_ids = [eng.sampled_table_id(prefix, line) for line in range(1, min(layers, 64) + 1)]
        torch.cuda.synchronize()
        samp_s = time.perf_counter() - c0
        flakes = [eng.sampled_flakes[(prefix, line)] for line in range(1, min(layers, 64) + 1)]
        tables = [eng.sampled_rows[(prefix, line)] for line in range(1, min(layers, 64) + 1)] if eng.keep_sampled_rows else None
        ktot = sum(flakes) * (layers // min(layers, 64))
        sampler = {"tables": len(dev_ids), "tables_per_s": len(dev_ids) / samp_s, "flakes": int(sum(flakes)), "flakes_per_s": sum(flakes) / samp_s,
                   "seconds": samp_s, "note": "snowgpu_sample_table: Philox dart throwing + filing (derive / bin / sort) on the device, "
                                              "one call per table, nothing downloaded" + (" except the rows the CPU oracle checks against" if eng.keep_sampled_rows else "")}
        if tables is not None:
            tables = [tables[i % len(tables)] for i in range(layers)]
    else:
        tables = make_tables(layers, snowfall, velocity, distinct=min(layers, 64), workers=host_workers)
        ktot = sum(t.shape[0] for t in tables)
    F = args.frames
    import random
    frames, orders, table_ids, planes, polys = [], [], [], [], []
    plane = ([0.0, 0.0, -1.0], -1.7)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(host_workers) as ex:                       # (the sweep generator is NumPy array work: it releases the GIL)
        made = list(ex.map(lambda f: make_frame(layers, azimuths, 1000 + rank * F + f, rscale, args.workload in FIRING_ORDER), range(F)))
    for f in range(F):
        seed = 1000 + rank * F + f
        pc = made[f]
        random.seed(seed)
        order = list(range(layers))
        random.shuffle(order)
        frames.append(pc)
        orders.append(order)
        table_ids.append([dev_ids[order[c] % len(dev_ids)] for c in range(layers)] if args.tables == "device"
                         else eng.table_ids_from_arrays(tables, order))
        planes.append([*plane[0], plane[1]])
        if args.host_prepass:
            polys.append(noise_threshold_poly(pc, plane[0], plane[1], 0.7))
    n_per = frames[0].shape[0]
    n_total = n_per * F
    host_rows = np.concatenate(frames)
    rows = torch.from_numpy(host_rows).to(dev)
    off = torch.arange(0, F + 1, dtype=torch.int64, device=dev) * n_per
    tids = torch.tensor(table_ids, dtype=torch.int32, device=dev)
    # The timed call goes through the PYTHON boundary a user has: augment_batch() on CUDA tensors (lidar_snow_sim_amd/tensors.py ->
    # snowgpu_augment_batch_device / snowgpu_augment_wet_batch_device on torch's current stream; rows read where they lie, results
    # left in device tensors, nothing waited for inside a step).  Channel permutations, planes and table lookup are the arguments of
    # every step, as in a training loop; their device copies (a few KB) are cached by value.
    from lidar_snow_sim_amd import tensors as snow_tensors
    batch = snow_tensors.DeviceBatch(rows, frame_rows=n_per)
    orders_np = np.asarray(orders, np.int64)
    if args.tables == "device":
        call_kw = dict(particles="device", orders=orders_np % len(dev_ids))          # (lines beyond the 64 sampled ones reuse them, as above)
        call_prefix = prefix
    else:
        call_kw = dict(particles=tables, orders=orders_np)
        call_prefix = "unused"
    if args.host_prepass:
        call_kw["thr_polys"] = np.asarray(polys, np.float64)
    else:
        call_kw["planes"] = np.asarray(planes, np.float64)
    if fused_wet:
        call_kw["wet"] = dict(WET, plane=plane)
    # --lanes L > 1: L batches in flight -- step k runs on compute lane k mod L (an engine context and stream of its own) and keeps its own
    # result tensors; nothing waits for a step but the next step on the same lane and the synchronise that ends the timed region.
    L = max(1, args.lanes)
    res = [None] * L
    side = torch.cuda.Stream(device=dev)       # (a stream of the caller's: on torch's legacy default stream the boundary forks to one of its own)
    step_no = [0]
    if L > 1 and layers != 64:
        for k in range(L):
            engine.get_engine(local_rank, snow_tensors.LANE_SLOT0 + k).set_lasers(engine.load_lasers() * (layers // 64))
    prof_ctx = engine.get_engine(local_rank, snow_tensors.LANE_SLOT0).ctx if L > 1 else eng.ctx       # (the per-beam region's events: lane 0's)

    def step():
        k = step_no[0] % L
        step_no[0] += 1
        with torch.cuda.stream(side):
            res[k] = snow_tensors.augment_batch(batch, call_prefix, BEAM_DIV, noise_floor=0.7, sync=False, out=res[k], lane=k if L > 1 else None, **call_kw)

    for _ in range(L - 1):
        step()

    step()                                                  # (first call of the size: result tensors, library scratch)
    torch.cuda.synchronize()
    out_rows, out_src, out_counts, out_stats, status = res[0].rows, res[0].src, res[0].counts, res[0].stats, res[0].status
    if L == 1:
        assert torch.equal(res[0]._keep[2].cpu(), tids.cpu()), "table ids of the tensor boundary differ from the direct lookup"

    def barrier():
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    st = status.cpu().numpy()
    if st[0] != 0:
        raise RuntimeError(f"device status {st} after warmup")
    prof_ctx.profile_begin(args.steps)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    beam_ms, n_launch = prof_ctx.profile_end()
    if distributed:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    st = status.cpu().numpy()
    if st[0] != 0:
        raise RuntimeError(f"device status {st} after the timed region")
    if args.dump_outputs and rank == 0:
        dump_outputs(res[(step_no[0] - 1) % L], F, n_per, Path(args.dump_outputs))
    if args.inner:
        return

    import types
    W = types.SimpleNamespace(args=args, eng=eng, torch=torch, dist=dist, dev=dev, distributed=distributed, world=world, rank=rank, local_rank=local_rank,
                              F=F, n_per=n_per, n_total=n_total, layers=layers, host_rows=host_rows, frames=frames, orders=orders, tables=tables,
                              table_ids=table_ids, plane=plane, planes=planes, fused_wet=fused_wet, barrier=barrier,
                              out_rows=out_rows, out_src=out_src, out_counts=out_counts, out_stats=out_stats)
    pcie, single = measure_host_entry(W)

    seen = ranks_seen()
    if rank == 0:
        pts_per_step = n_total * world
        value = pts_per_step * args.steps / elapsed
        # ALGORITHMIC bytes of one per-beam launch (SURVEY 8 d): 20 B read + 20 B written per point; the flake tables
        # (24 B per flake per channel per frame) stay in L2 / Infinity Cache across a batch (profiles/: the region fetches
        # far less than one pass over them per frame), so the table term is dropped -- the figure with it is given beside.
        alg_bytes = 40.0 * n_total
        alg_bytes_tables = alg_bytes + 24.0 * ktot * F
        avg_ms = beam_ms / max(n_launch, 1)
        achieved = alg_bytes / (avg_ms * 1e-3) if avg_ms > 0 else 0.0
        traffic, traffic_src, valu = counter_passes(W, alg_bytes)
        result = {
            "metric": METRIC,
            "value": value, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{args.workload}: synthetic {layers}-layer x {azimuths}-azimuth sweeps, snowfall_rate={snowfall} mm/h, "
                                   f"terminal_velocity={velocity} m/s, gunn tables R0=80 m ({ktot // layers} flakes/line), "
                                   f"beam_divergence=3 mrad, noise_floor=0.7, float32 rows resident in HBM"
                                   + ("" if rscale == 1.0 else f", ranges x{rscale} (clipped at 119 m)")
                                   + (", snowfall + wet ground fused (snowgpu_augment_wet_batch_device)" if fused_wet else ""),
                       "frames_per_step_per_gpu": F, "points_per_frame": n_per, "batches_in_flight": max(1, args.lanes),
                       "prepass": "host (outside the timed region)" if args.host_prepass else "device (timed)",
                       "sharding": f"frame-parallel x{world}, no collective", "ranks_seen": seen,
                       "backend": "nccl (RCCL)" if distributed else None,
                       "beams_per_capacity_tier": [int(n_total)] + [int(v) for v in st[2:6]]},
            "per_gpu_value": value / world,
            "value_note": "rows resident in HBM when the clock starts, through the Python boundary a user calls -- augment_batch() on torch CUDA "
                          "tensors (lidar_snow_sim_amd/tensors.py -> snowgpu_augment_batch_device on torch's stream) --, as the measurement contract of "
                          "this build prescribes; SURVEY 8(d)'s definition of the metric -- upload and download inside the clock -- is "
                          "value_pcie_inclusive",
            "roofline": {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK, "traffic": traffic, "traffic_detail": traffic_src,
                         "frac_tables_counted": alg_bytes_tables / (avg_ms * 1e-3) / HBM_PEAK if avg_ms > 0 else 0.0,
                         "valu": valu,
                         "kernel": "per-beam region of one step: k_beams<float,LMAX,BLOCK,LIST,DICT> (the pass over all rows and the later capacity "
                                   "tiers), k_power_plan + k_power (received power), k_tier_* (tier lists), k_beams_huge; one HIP event pair "
                                   "around the region on its launch stream",
                         "avg_launch_ms": avg_ms, "launches": n_launch,
                         "algorithmic_bytes_per_launch": alg_bytes,
                         "note": "40 B/point (20 read + 20 written); tables cache-resident across the batch, so SURVEY 8(d)'s table term "
                                 "(24 B per flake per channel per frame) is dropped -- frac_tables_counted keeps it (251.3 B/point on C2)"},
        }
        result["value_metric_definition"] = ("value: rows resident in HBM (device entry); SURVEY 8(d)'s metric with H2D + D2H inside the clock is "
                                             "value_pcie_inclusive (packed result transfer, plane injected) / value_pcie_inclusive_rows_transfer (whole rows + "
                                             "source indices down the link) / value_pcie_inclusive_default_plane (rows transfer, plane = NULL: estimated on the device)")
        if pcie is not None:
            result["value_pcie_inclusive"] = pcie["value"]
            result["value_pcie_inclusive_rows_transfer"] = pcie["value_rows_transfer"]
            if pcie.get("default_plane_all_ranks"):
                result["value_pcie_inclusive_default_plane"] = pcie["default_plane_all_ranks"]["reference"]
                result["value_pcie_inclusive_lsq_plane"] = pcie["default_plane_all_ranks"]["lsq"]
            ci = (pcie.get("compact_input") or {}).get("packed") or {}
            if ci.get("points_per_s") and world == 1:
                # (x, y, z, intensity) float32 + one channel byte per row up the link (snowgpu_augment_batch_compact), packed transfer down
                result["value_pcie_inclusive_compact_input"] = ci["points_per_s"]
            result["pcie_inclusive"] = pcie
        if single is not None:
            result["single_frame"] = single
        if bif:
            result["value_batches_in_flight"] = bif["value"]
            bif["note"] = ("step k runs on compute lane k mod lanes (augment_batch(..., sync=False, lane=k): an engine context of its own, every kernel of "
                           "the batch on ONE stream), nothing waits for a step but the next step on the same lane; the memory-bound sort and compaction of "
                           "one batch run beside the latency-bound per-beam kernels of the others.  Throughput of a pipelined consumer; a batch's own "
                           "latency is about lanes x ms_per_step.  Child processes of this command, run before it opened the device: three lanes with "
                           "GPU_MAX_HW_QUEUES=32 (`value_batches_in_flight`), two lanes in the unchanged environment (`default_environment`: the lanes' "
                           "streams differ in priority, include/snowgpu.h: snowgpu_lane_stream)")
            if bif_default:
                bif["default_environment"] = bif_default
            result["batches_in_flight"] = bif
        if sampler is not None:
            result["sampler"] = sampler
            result["config"]["tables"] = "sampled and filed on the device (snowgpu_sample_table, seed = f(prefix, line))"
        if not args.no_cpu_baseline and world == 1:      # rank 0, N = 1 only
            result.update(cpu_legs(W))
        print(json.dumps(result), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
