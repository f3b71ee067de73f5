"""-m gpu: batches past 256 frames, 64 tiles a frame and 1024 tiles a call -- the second trip, and the sums over earlier waves, of every
scan that carries a running total from trip to trip, which the other GPU tests never reach:

  kernel                                        trip / threshold                              crossed by
  k_mask_scan (csrc/snowgpu_mask.hip)           64 tiles of 1024 rows a trip, `run`           long(): frames of 131 073, 65 537 and 131 072 rows
  k_mask_offsets (snowgpu_mask.hip)             64 frames a wave (s_wave[]), 256 a trip       many(65 / 256 / 257 / 321)
  k_voxel_offsets (snowgpu_voxel.hip)           the same                                      many(65 / 256 / 257 / 321)
  k_voxel_tile_scan (snowgpu_voxel.hip)         64 tiles a wave (wave_sum[]), 1024 a trip     many(F): 80 and more tiles; voxel_batch(): 1025 tiles
  sg_find_frame / vox_firsts_before             frames that start inside a tile               many(F): hundreds of frames, empty ones in a row
  run bases of k_paste_frame (snowgpu_paste.hip) ceil(runs / 256) runs a thread               paste_long(): 257 runs, chunk = 2, the lo / hi clamps
  k_roi_count / k_roi_scan / k_roi_rank         a table row per 512-row run                   roi_long(): 257 runs, a frame of 129 beside it
  k_pre_means as the aligned wet entry runs it  64 tiles a trip                               long()

A wrong carry gives plausible, in-bounds output shifted by a few rows; every comparison here is with a reference that has no trips: the
CPU twin and the unmasked call on compacted frames (a), the sequential walk of tests/voxel_reference.py (b), the restatements of
tests/paste_reference.py and tests/roipool_reference.py (c, d), the oracle on the gathered rows (e).  Inputs: tests/batch_scale_inputs.py,
the smallest that cross each threshold (the largest is 21 MB of rows); tests/test_batch_scale_inputs.py shows on any machine that they
put present rows, opened cells and free rows on both sides of every border.  The comparators are those of the stages' own test files.
Every test prints one [batch-scale] line with the shape it ran: frames, rows, tiles, runs and the trips of each scan.

Not here: batches beyond 65 535 frames, which the y dimension of the frame-indexed grids bounds, not a scan; the device prepass
(planes=) of the masked snowfall call at these sizes -- the tiny frames of many(F) have too few ground rows for it, so the snowfall calls
take polynomials; the float64 rows of long() (the scans do not read the rows); a 256-sweep batch under a mask (nothing here needs one)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import batch_scale_inputs as bsi
import paste_reference as pr
import roipool_reference as rr
import test_gpu_aligned_mask as tgam
import test_gpu_paste as tgp
import test_gpu_roipool as tgr
import test_gpu_voxelize as tgv
import test_gpu_wet_aligned as tgw
import voxel_reference as vr

pytestmark = pytest.mark.gpu

BD, TILE, RUN = bsi.BD, bsi.TILE, bsi.RUN


@pytest.fixture(scope="module")
def eng():
    from lidar_snow_sim_amd import engine
    return engine.get_engine(0)


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    snow_oracle.build()
    return snow_oracle


@pytest.fixture(scope="module")
def tl(tables):
    return [tables["t"][i % 4] for i in range(64)]


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _trips(n, per):
    return -(-int(n) // per)


def _say(what, **shape):
    print(f"\n[batch-scale] {what}: " + ", ".join(f"{k} {v}" for k, v in shape.items()))


# ---- a. masked aligned snowfall ---------------------------------------------------------------------------------------------------------
def _masked_call(frames, masks, tl, orders):
    """augment_batch(..., layout='aligned', keep=, thr_polys=) -> (per frame (stats, rows, keep) as NumPy, counts)"""
    from lidar_snow_sim_amd.tensors import augment_batch
    nf = len(frames)
    res = augment_batch([_t(f) for f in frames], "unused", BD, particles=tl, orders=orders, thr_polys=[list(bsi.POLY)] * nf, layout="aligned",
                        keep=[_t(m) for m in masks], sync=False).wait()
    assert int(res.status[0]) == 0
    rows, keep, stats, off = res.rows.cpu().numpy(), res.keep.cpu().numpy(), res.stats.cpu().numpy(), res.offsets
    assert np.array_equal(off, bsi.offsets(frames))
    return [(tuple(int(v) for v in stats[f]), rows[off[f]:off[f + 1]], keep[off[f]:off[f + 1]]) for f in range(nf)], res.counts.cpu().numpy()


def _differs_from_the_twin(got, counts, frames, masks, tl, orders):
    """Frames whose present rows, keep bytes, counts or statistics differ from libsnowcpu.so's aligned entry on the compacted frames, or
    whose absent rows are not the input's bytes with keep 0 (as tests/test_gpu_large_batch.py compares a device batch with the twin)."""
    from lidar_snow_sim_amd import _cpu_twin
    sub = [np.ascontiguousarray(f[m]) for f, m in zip(frames, masks)]
    twin = _cpu_twin.augment_batch(sub, tl, orders, BD, [bsi.POLY] * len(frames), threads=16, layout="aligned")
    bad, changed = [], 0
    for f, ((st, rows, keep), (t_st, t_rows, t_keep)) in enumerate(zip(got, twin)):
        m = masks[f]
        same = st == tuple(int(v) for v in t_st) and rows[m].tobytes() == t_rows.tobytes() and np.array_equal(keep[m], t_keep) \
            and int(counts[f]) == int(t_keep.sum()) and not keep[~m].any() and rows[~m].tobytes() == frames[f][~m].tobytes()
        if not same:
            bad.append(f)
        changed += int((t_rows[:, 4] == 2).sum()) + int((~t_keep).sum())
    return bad, changed


def _snowfall(frames, masks, tl, what, **shape):
    orders = bsi.orders(len(frames))
    got, counts = _masked_call(frames, masks, tl, orders)
    bad, changed = _differs_from_the_twin(got, counts, frames, masks, tl, orders)
    ref = tgam._compacted_reference(frames, masks, tl, thr_polys=[list(bsi.POLY)] * len(frames), orders=orders)
    _say(what, frames=len(frames), rows=sum(len(f) for f in frames), present=sum(int(m.sum()) for m in masks), **shape,
         frames_that_differ_from_the_twin=len(bad), rows_the_twin_scatters_or_removes=changed)
    assert bad == [], bad[:8]
    scattered, removed = tgam._same_as_compacted(got, ref, frames, masks)
    assert changed > 0 and scattered + removed == changed
    return got, counts


@pytest.mark.parametrize("F, dtype", [(65, "float32"), (256, "float32"), (257, "float32"), (257, "float64"), (321, "float32")])
def test_masked_snowfall_past_a_wave_and_a_trip_of_frames(eng, tl, F, dtype):
    """k_mask_offsets walks the frames 256 a trip and sums the waves in front of a thread's own out of s_wave[]: 65 frames reach the
    second wave, 256 fill the trip, 257 and 321 reach the carry (with one frame, and with a wave and one frame, behind it).  A wrong
    offset moves every later frame's rows in the compacted batch: against the CPU twin and the call on compacted frames, frame by frame.
    Once, for 321 frames, through the C entry: status word 0 and the wrapper's bytes."""
    frames, masks = bsi.many(F, dtype)
    got, counts = _snowfall(frames, masks, tl, f"snowfall many({F}) {dtype}", tiles_a_frame=1, k_mask_scan_trips=1,
                            k_mask_offsets_waves=_trips(F, 64), k_mask_offsets_trips=_trips(F, 256))
    if F == 321:
        orders = bsi.orders(F)
        poly = torch.tensor([list(bsi.POLY)] * F, dtype=torch.float64, device="cuda:0")
        o, k, c, s, _, status = tgam._raw(eng, _t(np.concatenate(frames)), bsi.offsets(frames), tgam._tids(eng, tl, orders), keep=_t(np.concatenate(masks)), poly=poly)
        assert int(status[0]) == 0
        assert o.cpu().numpy().tobytes() == np.concatenate([g[1] for g in got]).tobytes() and np.array_equal(k.cpu().numpy(), np.concatenate([g[2] for g in got]))
        assert np.array_equal(c.cpu().numpy(), counts) and [tuple(r) for r in s.cpu().numpy().tolist()] == [g[0] for g in got]


def test_masked_snowfall_past_64_tiles_of_a_frame(tl):
    """k_mask_scan takes 64 tiles of a frame a trip and carries `run`: frames of 131 073 rows (three trips, the third for ONE present row),
    65 537 (two, the second for one present row), 65 536 (one trip, full), 131 072 in firing order (two), 700 and 0.  A wrong carry
    moves the present rows of tiles 64 and up inside the compacted frame."""
    frames, masks = bsi.long()
    tiles = [_trips(len(f), TILE) for f in frames]
    _snowfall(frames, masks, tl, "snowfall long()", tiles_a_frame=tiles, k_mask_scan_trips=[_trips(t, 64) for t in tiles], k_mask_offsets_trips=1)


# ---- b. voxelize --------------------------------------------------------------------------------------------------------------------------
def _voxel_case(rows, off, keep, V, what):
    from lidar_snow_sim_amd.tensors import DeviceBatch, voxelize
    rng, size, T = vr.STRADDLE[:3]
    want = vr.voxelize(rows, rng, size, T, V, 4, keep, off)
    got = voxelize(DeviceBatch(_t(rows), np.array(off)), rng, size, T, V, keep=None if keep is None else _t(keep), return_voxel_of=True)
    tgv._same(got, want, what)
    total = int(want["voxel_offsets"][-1])
    assert int(got.voxel_offsets[len(off) - 1]) == total == int((want["coords"][:, 0] >= 0).sum()) > 0
    return want


@pytest.mark.parametrize("F", bsi.SIZES)
def test_voxelize_past_a_wave_and_a_trip_of_frames(F):
    """k_voxel_offsets (64 frames a wave, 256 a trip, `carry`) under STRADDLE and with max_voxels = 40 -- frames above, below and at zero
    cells on both sides of frame 256 --, with and without the mask; k_voxel_tile_scan's sum over earlier waves (more than 64 tiles in the
    call); sg_find_frame and vox_firsts_before over hundreds of frames that start inside a tile, empty ones in a row.  All five
    outputs equal the sequential walk byte for byte; voxel_offsets[F] is the walk's total."""
    frames, masks = bsi.many(F)
    rows, keep, off = np.concatenate(frames), np.concatenate(masks), bsi.offsets(frames)
    totals = []
    for V in (vr.STRADDLE[3], 40):
        for kp in (None, keep):
            want = _voxel_case(rows, off, kp, V, (F, V, kp is not None))
            totals.append(int(want["voxel_offsets"][-1]))
    tiles = _trips(len(rows), TILE)
    _say(f"voxelize many({F})", frames=F, rows=len(rows), tiles=tiles, k_voxel_offsets_waves=_trips(F, 64), k_voxel_offsets_trips=_trips(F, 256),
         k_voxel_tile_scan_waves=_trips(tiles, 64), k_voxel_tile_scan_trips=_trips(tiles, 1024), voxels=totals)
    assert totals[0] > totals[1] > totals[3] and totals[0] > totals[2] > totals[3]


def test_voxelize_past_1024_tiles_of_a_call():
    """k_voxel_tile_scan takes 1024 tiles of the BATCH a trip: 1 049 278 rows are 1025 tiles, and the 700-row frame, which lies wholly in
    tile 1024 behind an empty frame, gets its voxel numbers from the carry.  Every full sweep opens more than 1024 voxels: k_voxel_span_scan
    makes a second trip too."""
    rows, off = bsi.voxel_batch()
    want = _voxel_case(rows, off, None, vr.STRADDLE[3], "voxel_batch")
    tiles, per_frame = _trips(len(rows), TILE), np.diff(want["voxel_offsets"])
    _say("voxelize voxel_batch()", frames=len(off) - 1, rows=len(rows), tiles=tiles, k_voxel_tile_scan_waves=_trips(tiles, 64),
         k_voxel_tile_scan_trips=_trips(tiles, 1024), voxels_a_frame=per_frame.tolist())
    assert tiles == 1025 and per_frame[-1] >= 10 and per_frame[-2] == 0 and per_frame[:9].min() > 1024


# ---- c. paste_objects ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _paste_expected(dtype):
    return pr.expected_of(bsi.paste_long(dtype))


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_paste_objects_with_two_runs_a_thread(dtype):
    """k_paste_frame gives each of its 256 threads ceil(runs / 256) runs: frames of 131 073 rows have 257 -- chunk = 2, thread 128 holds
    run 256 alone (`hi` clamped), threads 129 .. 255 hold none (`lo` clamped).  Objects run over the free rows of runs 127 / 128 (threads
    63 / 64, waves 0 / 1) and 255 / 256 through the frame's last row; rows, keep, gt boxes, object, state, source, the four counts and the
    pose equal the restatement byte for byte, and a second call gives the same bytes."""
    c, e = bsi.paste_long(dtype), _paste_expected(dtype)
    runs = _trips(max(bsi.PASTE_ROWS), RUN)
    got = tgp._run(c)
    tgp._same(got, e, ("paste_long", dtype))
    again = tgp._run(c)
    for f in tgp.FIELDS:
        assert torch.equal(getattr(got, f).view(torch.uint8), getattr(again, f).view(torch.uint8)), f
    _say(f"paste_objects paste_long({dtype})", frames=3, rows=len(c["rows"]), runs=runs, chunk=_trips(runs, 256), threads_with_runs=_trips(runs, _trips(runs, 256)),
         counts=e["count"].tolist())
    assert runs == 257 and _trips(runs, 256) == 2


# ---- d. roi_point_pool ----------------------------------------------------------------------------------------------------------------------
def test_roi_point_pool_over_a_table_of_257_runs():
    """k_roi_count files a table row per 512-row run, k_roi_scan turns the rows into prefixes, k_roi_rank starts every run from its
    prefix: the first two frames of long() under their masks -- 257 runs, and beside them a frame of 129 whose other runs lie beyond its
    length --, four rois of car size and one that holds the whole frame, S = 64.  Byte for byte against the restatement; the whole-frame
    roi counts the usable present rows and its 64 slots are the first 64 of them."""
    import box_reference as br
    c = bsi.roi_long()
    e = rr.pool_case(c)
    got = tgr._run(c)
    tgr._same(got, e, "roi_long")
    usable, off = br.usable_rows(c["rows"], c["keep"]), c["offsets"]
    count, index = got.count.cpu().numpy(), got.index.cpu().numpy()
    for f in range(2):
        a, b = int(off[f]), int(off[f + 1])
        assert count[f, 4] == usable[a:b].sum() and np.array_equal(index[f, 4], a + np.flatnonzero(usable[a:b])[:64])
    _say("roi_point_pool roi_long()", frames=2, rows=len(c["rows"]), runs=_trips(131073, RUN), runs_of_each_frame=[_trips(n, RUN) for n in np.diff(off)],
         counts=count.tolist())


# ---- e. wet_ground_batch_aligned -----------------------------------------------------------------------------------------------------------
def test_aligned_wet_ground_past_64_tiles_of_a_frame(so):
    """k_pre_means, as the aligned wet entry runs it, takes 64 tiles of a frame a trip: long() under its masks, with the expectation and
    the tolerances of tests/test_gpu_wet_aligned.py (the oracle on the gathered rows; intensities at rtol 1e-7 + 2^-23 on float32 rows).
    The 700-row frame and the empty one have fewer than 1000 ground rows: flag 1, rows as they came."""
    frames, masks = bsi.long()
    out, counts = tgw._run([np.array(f) for f in frames], list(masks), bsi.WET)          # (copies: the shared inputs are read-only)
    failures, worst = [], 0.0
    for f, (pc, m) in enumerate(zip(frames, masks)):
        rows, keep, flag = out[f]
        fl, rel = tgw._check(so, f"long[{f}]", pc, m, bsi.WET, rows, keep, counts[f], flag, "f32")
        failures += fl
        worst = max(worst, 0.0 if np.isnan(rel) else rel)
    tiles = [_trips(len(f), TILE) for f in frames]
    _say("wet_ground_batch_aligned long()", frames=len(frames), rows=sum(len(f) for f in frames), tiles_a_frame=tiles,
         k_pre_means_trips=[_trips(t, 64) for t in tiles], flags=[o[2] for o in out], largest_relative_intensity_error=f"{worst:.2e}")
    assert [o[2] for o in out] == [0, 0, 0, 0, 1, 1] and counts[5] == 0
    assert not failures, "\n".join(failures)
