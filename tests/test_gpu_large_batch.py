"""-m gpu: device batches above the 16-frame switch of the prepass, at the shapes and settings the smaller tests do not reach.

  bench shape   256 C2 sweeps as ONE DeviceBatch through augment_batch(..., sync=False) on a side stream, called again with out= the
                first result (what every timed step of bench.py does): same tensors, same bytes; every frame against libsnowcpu.so,
                a spread of frames against the oracle
  C1 / C4       32-frame device batches (40 k flakes per line / 128 lasers): every frame against the CPU twin, a sample against the
                oracle; C1 twice on one context, so that the second call takes the long-tail order from the first call's tier counts
  plane=None    the device plane: 'reference' (flat earth, statistics inside the sort's first pass) and 'lsq' (statistics behind the
                plane estimate), at 32 frames and at 8
  stats early   SNOWGPU_STATS_EARLY = 0 / 1 / unset: the prepass statistics inside the sort or as a kernel of their own -- same bits
  degenerate    a ragged batch with the noise-line fallback, a firing-order sweep and a frame of a few hundred rows, at 24 frames
                (k_pre_rowmin + k_lean_lines_solve) and at 8 (k_lean_rowmin_solve); frames without ground rows raise as the reference
  error path    a frame without ground rows in a pipelined host call with the threshold callback and the packed result transfer
  callback      q8='numpy' with a calibration that set_fov rejects leaves no callback behind on the shared context

Every test prints one [fullsize-parity] line with its mismatch counts.
"""
import os
import random
import time

import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded (one HIP runtime per process)

from test_gpu_fullsize import BD, PLANE, _count_mismatches, _report, _sum_counts, _tables

pytestmark = pytest.mark.gpu

PLANE_ROW = [*PLANE[0], PLANE[1]]


def _threads():
    return max(1, min(os.cpu_count() or 1, 64))


def _frames_pool(workload, dtype, n):
    """_frames() of test_gpu_fullsize.py -- bench's sweeps (seed 1000 + f) and shuffled orders -- with the sweeps made on a thread pool,
    as bench.main does (the generator is NumPy array work: it releases the GIL)."""
    import bench
    from concurrent.futures import ThreadPoolExecutor
    layers, azimuths, _, _, scale = bench.WORKLOADS[workload]
    with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as ex:
        made = list(ex.map(lambda f: bench.make_frame(layers, azimuths, 1000 + f, scale, workload in bench.FIRING_ORDER), range(n)))
    orders = []
    for f in range(n):
        random.seed(1000 + f)                               # SURVEY 8 d: random.seed(f); random.shuffle(order)
        order = list(range(layers))
        random.shuffle(order)
        orders.append(order)
    return [pc.astype(dtype, copy=False) for pc in made], orders


def _offsets(frames):
    return np.concatenate(([0], np.cumsum([f.shape[0] for f in frames]))).astype(np.int64)


def _raw_device_call(eng, rows_t, off, tids, planes=None, thr_polys=None):
    """snowgpu_augment_batch_device on torch tensors, with the device's threshold polynomials (d_out_thr, which the tensor wrapper leaves
    at 0), on a stream of its own; waited for.  Returns host copies: rows, src, counts, stats, thr, status."""
    dev = rows_t.device
    nf, n = len(off) - 1, int(off[-1])
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    d_off, d_tids = up(off, np.int64), up(np.asarray(tids).reshape(nf, -1), np.int32)
    d_plane = None if planes is None else up(np.asarray(planes, np.float64).reshape(nf, 4), np.float64)
    d_poly = None if thr_polys is None else up(np.asarray(thr_polys, np.float64).reshape(nf, 3), np.float64)
    o_rows = torch.empty((n, 5), dtype=rows_t.dtype, device=dev)
    o_src = torch.empty(n, dtype=torch.int32, device=dev)
    o_cnt = torch.empty(nf, dtype=torch.int64, device=dev)
    o_st = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    o_thr = torch.zeros((nf, 3), dtype=torch.float64, device=dev)
    o_status = torch.empty(8, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
    with eng.batch_lock:
        eng.ctx.augment_batch_device(nf, n, int(np.diff(off).max()), d_off.data_ptr(), rows_t.data_ptr(), 0 if rows_t.dtype == torch.float32 else 1,
                                     d_tids.data_ptr(), BD, ptr(d_poly), ptr(d_plane), 0.7, 0, o_rows.data_ptr(), o_src.data_ptr(),
                                     o_cnt.data_ptr(), o_st.data_ptr(), o_thr.data_ptr(), o_status.data_ptr(), s.cuda_stream)
    s.synchronize()
    status = o_status.cpu().numpy()
    eng.ctx.check_status(status)
    return dict(rows=o_rows.cpu().numpy(), src=o_src.cpu().numpy(), counts=o_cnt.cpu().numpy(), stats=o_st.cpu().numpy(),
                thr=o_thr.cpu().numpy(), status=status)


def _frames_equal(a, b, off, f):
    """Frame f of two results (dicts of host arrays): same count, rows (bytes), sources and statistics."""
    n = int(a["counts"][f])
    s = int(off[f])
    return n == int(b["counts"][f]) and a["rows"][s:s + n].tobytes() == b["rows"][s:s + n].tobytes() \
        and np.array_equal(a["src"][s:s + n], b["src"][s:s + n]) and np.array_equal(a["stats"][f], b["stats"][f])


def _twin_mismatches(frames, tables, orders, res, off, lasers=None, group=32):
    """Frames whose rows, sources or statistics differ from libsnowcpu.so fed the same polynomials (groups of `group` frames)."""
    from lidar_snow_sim_amd import _cpu_twin
    bad = []
    for g0 in range(0, len(frames), group):
        g1 = min(len(frames), g0 + group)
        twin = _cpu_twin.augment_batch(frames[g0:g1], tables, orders[g0:g1], BD, res["thr"][g0:g1], lasers=lasers)
        for f, (st, aug, sidx) in zip(range(g0, g1), twin):
            a, n = int(off[f]), int(res["counts"][f])
            same = n == aug.shape[0] and np.array_equal(res["src"][a:a + n], sidx) and res["rows"][a:a + n].tobytes() == aug.tobytes() \
                and tuple(int(v) for v in res["stats"][f]) == tuple(int(v) for v in st)
            if not same:
                bad.append(f)
    return bad


def _oracle_recs(frames, tables, orders, res, off, sample, plane=PLANE, lasers=None, thr_from_res=False, cache=None):
    """Mismatch records of the sampled frames against the threaded oracle (and the number of frames whose statistics differ).
    thr_from_res: the oracle is given the device's polynomial (the prepass itself is compared elsewhere)."""
    from oracle import snow_oracle as so
    recs, stat_bad = [], 0
    for f in sample:
        key = (f, None if thr_from_res else repr(plane))
        ref = None if cache is None else cache.get(key)
        if ref is None:
            kw = dict(thr_poly=np.asarray(res["thr"][f], np.float64)) if thr_from_res else dict(plane=plane)
            ref = so.augment(frames[f], tables, BD, orders[f], lasers=lasers, threads=_threads(), **kw)
            if cache is not None:
                cache[key] = ref
        s0, a0, src0 = ref
        a, n = int(off[f]), int(res["counts"][f])
        rtol = 1e-6 if frames[f].dtype == np.float32 else 1e-12
        recs.append(_count_mismatches(res["rows"][a:a + n], res["src"][a:a + n], a0, src0, rtol))
        stat_bad += tuple(int(v) for v in res["stats"][f]) != tuple(int(v) for v in s0)
    return recs, stat_bad


def _assert_oracle(tot, stat_bad):
    assert tot["mismatched_src"] == 0 and tot["same_order"]
    assert tot["mismatched_labels"] == 0 and tot["mismatched_intensity"] == 0
    assert tot["xyz_over_tol"] == 0
    assert stat_bad == 0


def _host(t):
    return t.cpu().numpy()


# ---- 1. the shape bench.py times ------------------------------------------------------------------------------------------------------

def test_bench_shape_256_frames_with_reused_result_tensors(capsys):
    """bench.py's C2 step: 256 sweeps as ONE DeviceBatch(rows, frame_rows=n), augment_batch(..., sync=False) on a side stream with
    planes as an (F, 4) array, then the same call with out= the first result.  The second call writes the same tensors and the same bytes;
    every frame equals libsnowcpu.so fed the device's polynomials (from a raw call on the same batch, whose rows equal the wrapper's);
    16 frames spread over the batch -- 0, 15, 16 and 255 among them -- equal the oracle."""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd import tensors as snow_tensors
    F = 256
    tables = _tables("C2")
    frames, orders = _frames_pool("C2", np.float32, F)
    n = frames[0].shape[0]
    dev = torch.device("cuda:0")
    rows = torch.from_numpy(np.concatenate(frames)).to(dev)
    off = _offsets(frames)
    batch = snow_tensors.DeviceBatch(rows, frame_rows=n)
    assert np.array_equal(batch.offsets, off)
    orders_np = np.asarray(orders, np.int64)
    kw = dict(particles=tables, orders=orders_np, planes=np.asarray([PLANE_ROW] * F, np.float64))
    side = torch.cuda.Stream(device=dev)
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        r1 = snow_tensors.augment_batch(batch, "unused", BD, noise_floor=0.7, sync=False, **kw)
    r1.wait()
    t_gpu = time.perf_counter() - t0
    first = {k: getattr(r1, k).clone() for k in ("rows", "src", "counts", "stats")}
    ptrs = [t.data_ptr() for t in (r1.rows, r1.src, r1.counts, r1.stats, r1.status)]
    with torch.cuda.stream(side):
        r2 = snow_tensors.augment_batch(batch, "unused", BD, noise_floor=0.7, sync=False, out=r1, **kw)
    r2.wait()
    assert [t.data_ptr() for t in (r2.rows, r2.src, r2.counts, r2.stats, r2.status)] == ptrs
    wrap = {"rows": _host(r2.rows), "src": _host(r2.src), "counts": _host(r2.counts), "stats": _host(r2.stats)}
    before = {k: _host(v) for k, v in first.items()}
    del first
    assert np.array_equal(wrap["counts"], before["counts"]) and np.array_equal(wrap["stats"], before["stats"])
    reuse_differ = sum(not _frames_equal(wrap, before, off, f) for f in range(F))
    del before
    eng = engine.get_engine(0)
    tids = snow_tensors.table_ids_for(eng, F, "unused", None, tables, orders_np, True)
    raw = _raw_device_call(eng, rows, off, tids, planes=kw["planes"])
    raw_differ = sum(not _frames_equal(wrap, raw, off, f) for f in range(F))
    del rows, batch, r1, r2
    t0 = time.perf_counter()
    twin_bad = _twin_mismatches(frames, tables, orders, raw, off)
    t_twin = time.perf_counter() - t0
    sample = sorted({0, 15, 16, 255, *range(17, 255, 20)})
    assert len(sample) == 16
    t0 = time.perf_counter()
    recs, stat_bad = _oracle_recs(frames, tables, orders, raw, off, sample)
    t_cpu = time.perf_counter() - t0
    tot = _sum_counts(recs)
    tot.update(workload="C2 bench shape (256-frame DeviceBatch, sync=False, out= reused)", frames=F, points=int(off[-1]),
               reuse_frames_differ=int(reuse_differ), raw_vs_wrapper_frames_differ=int(raw_differ), twin_frames_differ=len(twin_bad),
               oracle_frames=sample, mismatched_stats=int(stat_bad), gpu_call_s=round(t_gpu, 3), twin_s=round(t_twin, 2), oracle_s=round(t_cpu, 2))
    _report(capsys, tot)
    assert reuse_differ == 0 and raw_differ == 0
    assert twin_bad == [], twin_bad[:8]
    _assert_oracle(tot, stat_bad)


# ---- 2. C1 and C4 as 32-frame device batches ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("workload", ["C1", "C4"])
def test_C1_and_C4_as_device_batches_of_32(workload, capsys):
    """C1 (40 k flakes per line: first tier 8, thousands of beams in the 63-entry and global-list tiers) and C4 (128 x 4096 sweeps, the
    128-entry laser table) as 32-frame device batches: every frame equals the CPU twin fed the device's polynomials, frames 0, 15, 16 and
    31 equal the oracle.  C1 runs twice on one context: the second call picks the long-tail order of the received-power phase from the
    first call's tier counts, and gives the same bytes."""
    import bench
    from lidar_snow_sim_amd import engine
    from oracle import snow_oracle as so
    F = 32
    layers = bench.WORKLOADS[workload][0]
    tables = _tables(workload)
    frames, orders = _frames_pool(workload, np.float32, F)
    lasers = engine.load_lasers() * (layers // 64)
    off = _offsets(frames)
    planes = [PLANE_ROW] * F
    dev = torch.device("cuda:0")
    eng = engine.Engine(0, lasers=lasers)                   # own context: tier counts of this workload only
    try:
        tids = [eng.table_ids_from_arrays(tables, o) for o in orders]
        rows = torch.from_numpy(np.concatenate(frames)).to(dev)
        t0 = time.perf_counter()
        res = [_raw_device_call(eng, rows, off, tids, planes=planes)]
        t_gpu = time.perf_counter() - t0
        if workload == "C1":
            res.append(_raw_device_call(eng, rows, off, tids, planes=planes))
        del rows
    finally:
        eng.ctx.close()
    r = res[0]
    st = r["status"]
    tail = int(st[4]) + int(st[5])                          # beams in the 63-entry and the global-list tier (status words 2 + tier)
    repeat_differ = 0
    if workload == "C1":
        r2 = res[1]
        repeat_differ = sum(not _frames_equal(r, r2, off, f) for f in range(F)) + int(not np.array_equal(r["thr"], r2["thr"]))
    t0 = time.perf_counter()
    twin_bad = _twin_mismatches(frames, tables, orders, r, off, lasers=lasers)
    t_twin = time.perf_counter() - t0
    sample = [0, 15, 16, 31]
    t0 = time.perf_counter()
    recs, stat_bad = _oracle_recs(frames, tables, orders, r, off, sample, lasers=so.load_lasers() * (layers // 64))
    t_cpu = time.perf_counter() - t0
    tot = _sum_counts(recs)
    tot.update(workload=f"{workload} (32-frame device batch)", frames=F, points=int(off[-1]), tier_beams=[int(v) for v in st[2:6]],
               repeat_frames_differ=int(repeat_differ), twin_frames_differ=len(twin_bad), oracle_frames=sample, mismatched_stats=int(stat_bad),
               gpu_call_s=round(t_gpu, 3), twin_s=round(t_twin, 2), oracle_s=round(t_cpu, 2))
    _report(capsys, tot)
    assert twin_bad == [], twin_bad[:8]
    _assert_oracle(tot, stat_bad)
    if workload == "C1":
        assert tail > 500, st
        # the second call's choice (snowgpu_batch.cpp, heavy_tail): tail >= 4096 and tail * 22 > beams of the 16-entry tier
        assert tail >= 4096 and tail * 22 > int(st[3]), st
        assert repeat_differ == 0


# ---- 3. the device plane at 32 frames (and 'lsq' at 8) --------------------------------------------------------------------------------

@pytest.mark.parametrize("method,F", [("reference", 32), ("lsq", 32), ("lsq", 8)], ids=["reference-32", "lsq-32", "lsq-8"])
def test_device_plane_in_large_device_batches(method, F, capsys):
    """plane=None: calculate_plane on the device.  'reference' is the flat-earth plane the reference returns today: the statistics then
    ride in the sort's first pass behind the device's plane, and the rows equal the oracle's with plane=None.  'lsq' keeps a statistics
    pass of its own behind the plane estimate: the planes equal NumPy's lstsq on the reference crop (test_gpu_plane.py's tolerance) and the
    rows equal the oracle's given those planes, every frame.  At 8 frames 'lsq' takes the other side of the 16-frame switch of the prepass."""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    from lidar_snow_sim_amd.tools.wet_ground.planes import ground_crop
    tables = _tables("C2")
    frames, orders = _frames_pool("C2", np.float32, F)
    off = _offsets(frames)
    dev = torch.device("cuda:0")
    t_frames = [torch.from_numpy(f).to(dev) for f in frames]
    t0 = time.perf_counter()
    got = augment_batch(t_frames, "unused", BD, planes=None, orders=orders, particles=tables, return_src=True, plane_method=method)
    t_gpu = time.perf_counter() - t0
    # the results back in frame slots (the wrapper returns views of the first counts[f] rows of every slot)
    res = {"rows": np.zeros((int(off[-1]), 5), np.float32), "src": np.zeros(int(off[-1]), np.int32),
           "counts": np.asarray([g[1].shape[0] for g in got], np.int64), "stats": np.asarray([[int(v) for v in g[0]] for g in got], np.int64)}
    for f, (_, aug, sidx) in enumerate(got):
        res["rows"][off[f]:off[f] + aug.shape[0]] = _host(aug)
        res["src"][off[f]:off[f] + aug.shape[0]] = _host(sidx)
    plane_dev = 0.0
    if method == "reference":
        plane_list = [None] * F
    else:
        eng = engine.get_engine(0)
        eng.ctx.set_plane_method("lsq", min_rows=5)
        try:
            pl, info = eng.ctx.estimate_planes(np.concatenate(frames), off)
        finally:
            eng.ctx.set_plane_method("reference")
        plane_list = []
        for f in range(F):
            sub = frames[f][ground_crop(frames[f])].astype(np.float64)
            A = np.column_stack((sub[:, 0], sub[:, 1], np.ones(len(sub))))
            c, *_ = np.linalg.lstsq(A, sub[:, 2], rcond=None)
            w0 = np.array([c[0], c[1], -1.0])
            w0 /= np.linalg.norm(w0)
            np.testing.assert_allclose(pl[f, :3], w0, rtol=0, atol=1e-12)
            np.testing.assert_allclose(pl[f, 3], c[2], rtol=1e-12, atol=1e-12)
            plane_dev = max(plane_dev, float(np.abs(pl[f, :3] - w0).max()), float(abs(pl[f, 3] - c[2])))
            plane_list.append((pl[f, :3].copy(), float(pl[f, 3])))
    from oracle import snow_oracle as so
    recs, stat_bad = [], 0
    t0 = time.perf_counter()
    for f in range(F):
        s0, a0, src0 = so.augment(frames[f], tables, BD, orders[f], plane=plane_list[f], threads=_threads())
        a, n = int(off[f]), int(res["counts"][f])
        recs.append(_count_mismatches(res["rows"][a:a + n], res["src"][a:a + n], a0, src0, 1e-6))
        stat_bad += tuple(int(v) for v in res["stats"][f]) != tuple(int(v) for v in s0)
    t_cpu = time.perf_counter() - t0
    tot = _sum_counts(recs)
    tot.update(workload=f"C2 plane=None plane_method={method} (device batch)", frames=F, points=int(off[-1]), mismatched_stats=int(stat_bad),
               plane_max_abs_dev=plane_dev, gpu_call_s=round(t_gpu, 3), oracle_s=round(t_cpu, 2))
    _report(capsys, tot)
    _assert_oracle(tot, stat_bad)


# ---- 4. where the statistics pass runs -------------------------------------------------------------------------------------------------

def test_stats_early_placements_give_the_same_bits(monkeypatch, capsys):
    """SNOWGPU_STATS_EARLY=0: the prepass statistics ride in the channel sort's first pass; =1: k_lean_stats runs on its own on the prepass
    stream; unset: the latter above 16 frames.  32 C2 sweeps with caller planes under each value (a fresh context each: the switch is read
    when a context is made) and =1 / unset at 8 frames: the device's polynomials and every row are byte-identical across the values, and
    every frame equals the oracle."""
    from lidar_snow_sim_amd import engine
    tables = _tables("C2")
    frames, orders = _frames_pool("C2", np.float32, 32)
    dev = torch.device("cuda:0")
    results = {}
    for F, values in ((32, ("0", "1", None)), (8, ("1", None))):
        fr, od = frames[:F], orders[:F]
        off = _offsets(fr)
        rows = torch.from_numpy(np.concatenate(fr)).to(dev)
        for v in values:
            if v is None:
                monkeypatch.delenv("SNOWGPU_STATS_EARLY", raising=False)
            else:
                monkeypatch.setenv("SNOWGPU_STATS_EARLY", v)
            eng = engine.Engine(0)
            try:
                tids = [eng.table_ids_from_arrays(tables, o) for o in od]
                results[(F, v)] = _raw_device_call(eng, rows, off, tids, planes=[PLANE_ROW] * F)
            finally:
                eng.ctx.close()
        monkeypatch.delenv("SNOWGPU_STATS_EARLY", raising=False)
        del rows
    rec = {"test": "SNOWGPU_STATS_EARLY placements", "frames": [32, 8]}
    differ = 0
    for (F, v), r in results.items():
        base = results[(F, None)]
        off = _offsets(frames[:F])
        d = int(r["thr"].tobytes() != base["thr"].tobytes()) + sum(not _frames_equal(r, base, off, f) for f in range(F))
        rec[f"{F}:{v or 'unset'}_differ_from_unset"] = d
        differ += d
    cache = {}
    recs, stat_bad = [], 0
    t0 = time.perf_counter()
    for (F, v), r in results.items():
        rr, sb = _oracle_recs(frames, tables, orders, r, _offsets(frames[:F]), range(F), cache=cache)
        recs += rr
        stat_bad += sb
    tot = _sum_counts(recs)
    tot.update(rec, mismatched_stats=int(stat_bad), oracle_s=round(time.perf_counter() - t0, 2))
    _report(capsys, tot)
    assert differ == 0
    _assert_oracle(tot, stat_bad)


# ---- 5. degenerate frames on both sides of the 16-frame switch ------------------------------------------------------------------------

def _degenerate_batch(F):
    """A ragged float32 batch: the noise-line fallback frame (every ground row nearer than 10 m, as
    test_noise_line_fallback_uses_numpy_float32_mean builds it), a firing-order sweep, a frame of a few hundred rows, full C2 sweeps."""
    import bench
    from lidar_snow_sim_amd.synthetic import firing_order
    full, orders = _frames_pool("C2", np.float32, F)
    rng = np.random.default_rng(9)
    m = 3000
    az = rng.uniform(-np.pi, np.pi, m)
    d = rng.uniform(3.0, 9.5, m)
    frames = list(full)
    frames[1] = np.column_stack((d * np.cos(az), d * np.sin(az), np.full(m, -1.7), rng.integers(5, 120, m),
                                 rng.integers(0, 64, m))).astype(np.float32)
    frames[2] = firing_order(full[2], 64, 2048)
    frames[F - 2] = np.ascontiguousarray(full[F - 2][::397])          # a few hundred rows
    assert 300 <= frames[F - 2].shape[0] <= 400 and bench.WORKLOADS["C2"][0] == 64
    return frames, orders


@pytest.mark.parametrize("F", [24, 8])
def test_degenerate_frames_in_a_ragged_device_batch(F, capsys):
    """A ragged list of CUDA tensors (uniform_rows = 0) holding the noise-line fallback frame, a firing-order sweep and a frame of a few
    hundred rows next to full C2 sweeps: the device polynomials equal noise_threshold_poly on the host (rtol 1e-5, atol 1e-4: float32
    rows) and every frame's rows equal the oracle's given the device's polynomial.  A frame without ground rows (z + 5 m), or an empty
    frame, makes the call raise the reference's TypeError; an empty frame with caller polynomials comes back empty and leaves the other
    frames' bytes alone; the next good call on the engine gives the first call's bytes.  24 frames: k_pre_rowmin + k_lean_lines_solve;
    8: k_lean_rowmin_solve."""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd import tensors as snow_tensors
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    from lidar_snow_sim_amd.tools.wet_ground.augmentation import noise_threshold_poly
    tables = _tables("C2")
    frames, orders = _degenerate_batch(F)
    off = _offsets(frames)
    dev = torch.device("cuda:0")
    t_frames = [torch.from_numpy(f).to(dev) for f in frames]
    planes = [PLANE] * F
    kw = dict(orders=orders, particles=tables, return_src=True)

    def wrapped(tf, **extra):
        out = augment_batch(tf, "unused", BD, **dict(dict(kw, planes=planes), **extra))
        return [(tuple(int(v) for v in s), _host(a), _host(i)) for s, a, i in out]

    first = wrapped(t_frames)
    eng = engine.get_engine(0)
    tids = snow_tensors.table_ids_for(eng, F, "unused", None, tables, np.asarray(orders, np.int64), True)
    raw = _raw_device_call(eng, torch.cat(t_frames).contiguous(), off, tids, planes=[PLANE_ROW] * F)
    raw_differ = 0
    for f, (st, aug, sidx) in enumerate(first):
        a, n = int(off[f]), int(raw["counts"][f])
        raw_differ += not (n == aug.shape[0] and raw["rows"][a:a + n].tobytes() == aug.tobytes() and np.array_equal(raw["src"][a:a + n], sidx)
                           and tuple(int(v) for v in raw["stats"][f]) == st)
    thr_dev = 0.0
    for f in range(F):
        srt = frames[f][np.argsort(frames[f][:, 4], kind="stable")]
        host = noise_threshold_poly(srt, PLANE[0], PLANE[1], 0.7)
        far = 10.0 if f == 1 else 80.0                      # (the fallback frame's ground ends at 9.5 m)
        dist = np.linspace(3.0, far, 50)
        np.testing.assert_allclose(np.polyval(raw["thr"][f], dist), np.polyval(host, dist), rtol=1e-5, atol=1e-4, err_msg=f"frame {f}")
        thr_dev = max(thr_dev, float(np.abs(np.polyval(raw["thr"][f], dist) - np.polyval(host, dist)).max()))
    recs, stat_bad = _oracle_recs(frames, tables, orders, raw, off, range(F), thr_from_res=True)
    # a frame without ground rows, then an empty frame: the reference's TypeError (simulation.py:462, quirk Q7)
    lifted = frames[5].copy()
    lifted[:, 2] += 5.0
    for bad in (lifted, np.zeros((0, 5), np.float32)):
        tf = list(t_frames)
        tf[5] = torch.from_numpy(bad).to(dev)
        with pytest.raises(TypeError, match="ground"):
            wrapped(tf)
    # an empty frame with caller polynomials: nothing to fit, nothing kept; the other frames as in the first call
    tf = list(t_frames)
    tf[5] = torch.empty((0, 5), dtype=torch.float32, device=dev)
    polys = raw["thr"].copy()
    polys[5] = [0.0, 0.0, 0.0]
    with_empty = wrapped(tf, thr_polys=polys, planes=None)
    empty_differ = int(with_empty[5][1].shape[0] != 0 or with_empty[5][0] != (0, 0, 0))
    for f in range(F):
        if f != 5:
            g, w = with_empty[f], first[f]
            empty_differ += not (g[0] == w[0] and g[1].tobytes() == w[1].tobytes() and np.array_equal(g[2], w[2]))
    again = wrapped(t_frames)
    again_differ = sum(not (g[0] == w[0] and g[1].tobytes() == w[1].tobytes() and np.array_equal(g[2], w[2])) for g, w in zip(again, first))
    tot = _sum_counts(recs)
    tot.update(workload=f"ragged degenerate batch of {F} (fallback, firing order, {frames[F - 2].shape[0]} rows)", frames=F, points=int(off[-1]),
               mismatched_stats=int(stat_bad), max_threshold_deviation=thr_dev, raw_vs_wrapper_frames_differ=int(raw_differ),
               empty_frame_call_frames_differ=int(empty_differ), after_error_frames_differ=int(again_differ))
    _report(capsys, tot)
    assert raw_differ == 0 and empty_differ == 0 and again_differ == 0
    _assert_oracle(tot, stat_bad)


# ---- 6. a status inside the pipelined host call -----------------------------------------------------------------------------------------

def test_ground_error_in_a_pipelined_chunk_leaves_the_callers_rows_alone(capsys):
    """The pipelined host entry with the threshold callback and the packed result transfer: a chunk whose device prepass reports a frame
    without ground rows stops before its compaction and downloads.  Its frames must not be assembled from staging words an earlier call
    left behind.  40 C2 sweeps, a good call first (it fills the staging counts), then frame 0 lifted off the ground with out_rows pre-filled
    with a NaN sentinel: E_GROUND, and every row of the failing chunk -- not the batch's last chunk -- is still the sentinel.  The same call
    with the rows transfer raises E_GROUND too, and a third good call gives the first call's bytes.  Then an error the caller causes: the
    callback raises on its second group.  The call re-raises it, and nothing of the call is in flight once it has returned -- out_rows
    overwritten with the sentinel right away is intact after a device synchronisation -- and a good call gives the first call's bytes."""
    from lidar_snow_sim_amd import _native, engine
    from lidar_snow_sim_amd.tools.wet_ground.augmentation import noise_polys_from_device_stats
    tables = _tables("C2")
    n = 40
    frames, orders = _frames_pool("C2", np.float32, n)
    off = _offsets(frames)
    planes = [PLANE_ROW] * n
    groups = []

    def fit(first, h, r):
        groups.append((first, h.shape[0]))
        return noise_polys_from_device_stats(h, r, 0.7)

    eng = engine.Engine(0)
    try:
        tids = [eng.table_ids_from_arrays(tables, o) for o in orders]
        rows = np.concatenate(frames)
        bad_rows = rows.copy()
        bad_rows[off[0]:off[1], 2] += 5.0
        eng.ctx.set_result_transfer("packed")
        eng.ctx.set_threshold_callback(fit)
        try:
            good = [np.copy(a) for a in eng.ctx.augment_batch(rows, off, tids, BD, plane=planes)[:4]]
            good_groups = sorted(groups)
            groups.clear()
            sentinel = np.full((int(off[-1]), 5), np.nan, np.float32)
            with pytest.raises(_native.SnowGPUError) as err:
                eng.ctx.augment_batch(bad_rows, off, tids, BD, plane=planes, out_rows=sentinel)
            assert err.value.code == _native.E_GROUND
            bad_groups = sorted(groups)
            eng.ctx.set_result_transfer("rows")
            with pytest.raises(_native.SnowGPUError) as err_rows:
                eng.ctx.augment_batch(bad_rows, off, tids, BD, plane=planes)
            assert err_rows.value.code == _native.E_GROUND
            eng.ctx.set_result_transfer("packed")
            third = eng.ctx.augment_batch(rows, off, tids, BD, plane=planes)
            seen = []

            def fit_raises(first, h, r):
                seen.append(first)
                if len(seen) == 2:
                    raise RuntimeError("the second group's fit failed")
                return noise_polys_from_device_stats(h, r, 0.7)

            eng.ctx.set_threshold_callback(fit_raises)
            overwritten = np.zeros((int(off[-1]), 5), np.float32)
            with pytest.raises(RuntimeError, match="second group"):
                eng.ctx.augment_batch(rows, off, tids, BD, plane=planes, out_rows=overwritten)
            overwritten[...] = np.nan                     # whatever the call left in flight would now land on top of this
            torch.cuda.synchronize()
            in_flight = int((~np.isnan(overwritten)).any(axis=1).sum())
            eng.ctx.set_threshold_callback(fit)
            fourth = eng.ctx.augment_batch(rows, off, tids, BD, plane=planes)
        finally:
            eng.ctx.set_threshold_callback(None)
            eng.ctx.set_result_transfer("rows")
    finally:
        eng.ctx.close()
    # chunk 0 (frame 0's group) reported the status, so the callback never saw it; the good call's groups give its extent
    assert good_groups[0][0] == 0 and sum(g[1] for g in good_groups) == n and len(good_groups) >= 2
    chunk0 = good_groups[0][1]
    assert chunk0 < n and all(g[0] != 0 for g in bad_groups)          # not the last chunk; its callback did not run
    untouched = int(np.isnan(sentinel[:off[chunk0]]).all(axis=1).sum())
    rows_chunk0 = int(off[chunk0])
    third_differ, fourth_differ = (int(not (np.array_equal(res[2], good[2]) and np.array_equal(res[3], good[3]))) for res in (third, fourth))
    for f in range(n):
        a, m = int(off[f]), int(good[2][f])
        third_differ += not (third[0][a:a + m].tobytes() == good[0][a:a + m].tobytes() and np.array_equal(third[1][a:a + m], good[1][a:a + m]))
        fourth_differ += not (fourth[0][a:a + m].tobytes() == good[0][a:a + m].tobytes() and np.array_equal(fourth[1][a:a + m], good[1][a:a + m]))
    _report(capsys, {"test": "E_GROUND in a pipelined chunk (callback, packed transfer)", "frames": n, "chunk0_frames": chunk0,
                     "groups_good_call": len(good_groups), "chunk0_rows": rows_chunk0, "chunk0_rows_untouched": untouched,
                     "third_call_frames_differ": third_differ, "groups_seen_by_the_raising_callback": len(seen),
                     "rows_written_after_the_raising_call_returned": in_flight, "call_after_the_raising_one_frames_differ": fourth_differ})
    assert untouched == rows_chunk0
    assert third_differ == 0
    assert len(seen) == 2 and in_flight == 0
    assert fourth_differ == 0


# ---- 7. a failed call takes its threshold callback off the shared context ----------------------------------------------------------

def test_failed_q8_numpy_call_leaves_no_threshold_callback(golden, tables, capsys):
    """augment_batch(..., q8='numpy') installs a threshold callback on the engine's shared context.  A calibration that set_fov rejects
    (a 2 x 2 V2C) fails the call; the callback must be gone afterwards, so that a later q8='first' call still makes the device fit:
    an L5 portable case then equals its fixture."""
    from conftest import canonical
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.calibration import Calibration
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment, augment_batch
    d = golden("L5_augment", "portable")
    tl = [tables["t"][i % 4] for i in range(64)]
    case = 0
    pc = d[f"c{case}_pc"]
    plane = (d[f"c{case}_plane_w"], float(d[f"c{case}_plane_h"]))
    order = list(d[f"c{case}_order"])
    calib = Calibration(V2C=np.eye(2), R0=np.eye(3), P2=np.zeros((3, 4)))
    eng = engine.get_engine(0)
    try:
        with pytest.raises(ValueError):
            augment_batch([pc], "unused", float(d["bd"]), planes=[plane], orders=[order], particles=tl, q8="numpy", calib=calib)
        leaked = eng.ctx.__dict__.get("_thr_cb") is not None
    finally:
        eng.ctx.set_threshold_callback(None)
        eng.ctx.set_fov(None)
    stats, aug, src = augment(pc, "unused", float(d["bd"]), only_camera_fov=False, plane=plane, order=order, particles=tl, return_src=True)
    a1, s1 = canonical(aug, src)
    a2, s2 = canonical(d[f"c{case}_aug"], d[f"c{case}_src"])
    same = tuple(int(s) for s in stats) == tuple(int(v) for v in d[f"c{case}_stats"]) and np.array_equal(s1, s2) and np.array_equal(a1[:, 3:], a2[:, 3:])
    _report(capsys, {"test": "q8='numpy' call failing in set_fov", "callback_left_behind": bool(leaked), "L5_case0_after_equal": bool(same)})
    assert not leaked
    assert same
