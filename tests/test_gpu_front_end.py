"""-m gpu: the front end of every batch (csrc/snowgpu_sort.hip) at its structural edges, seen through what a call returns -- the stable
channel sort (k_sort_hist / k_sort_scan / k_sort_scatter), the per-frame verdict "channel-sorted as it stands: read in place"
(frame_unsorted) and the (table, frame, channel) segments (k_seg_small, or k_seg_count / k_seg_scan / k_seg_place) -- on the frames of
tests/front_end_inputs.py: one descent on and next to a round, wave or tile border, more than four ragged frames, more than 64 channel
values, and table arrays of 1501, 5001 and 70001 entries.  tests/test_front_end_inputs.py holds the CPU twin to the oracle on the same
frames and proves the conditions without which a frame wrongly read in place would go unnoticed here.

Column 4 of a result row is the reference's label (0, 1, 2) where the channel has a laser and the channel itself where it has none
(simulation.py:192), so "the output row's channel is that of frame[src]" is checked as: column 4 equals frame[src, 4] on the rows without
a laser, and x, y, z of every row that was not scattered are the bytes of frame[src]."""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded: PyTorch bundles its own HIP runtime, and the process must end up with one

import front_end_inputs as fei

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
BATCHES = ["thirteen", "levels", "ragged", "ranks"]


@pytest.fixture(scope="module")
def sets():
    return fei.table_sets()


@pytest.fixture(scope="module")
def frames_of():
    cache = {}

    def get(dtype):
        return cache.setdefault(np.dtype(dtype).name, fei.batches(dtype))
    return get


@pytest.fixture(scope="module")
def reference(sets, frames_of):
    """table set, dtype, batch -> the twin's [(stats, rows, src)], computed once"""
    from lidar_snow_sim_amd import build, _cpu_twin
    build.build_cpu_twin(verbose=False)
    cache = {}

    def get(name, dtype, batch):
        key = (name, np.dtype(dtype).name, batch)
        if key not in cache:
            fr = frames_of(dtype)[batch]
            cache[key] = _cpu_twin.augment_batch(fr, sets[name], fei.orders(len(fr)), fei.BD, [fei.POLY] * len(fr), threads=8)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def engine0():
    from lidar_snow_sim_amd import engine
    eng = engine.Engine(0)
    yield eng
    eng.ctx.close()


def _offsets(frames):
    return [0] + [int(v) for v in np.cumsum([f.shape[0] for f in frames])]


def _run(eng, frames, tids):
    """one compact call -> per frame (stats, rows, src), copies"""
    off = _offsets(frames)
    out, src, counts, stats, _ = eng.ctx.augment_batch(np.concatenate(frames), off, tids, fei.BD, thr_poly=[fei.POLY] * len(frames))
    res = []
    for f in range(len(frames)):
        a, m = off[f], int(counts[f])
        assert 0 <= m <= frames[f].shape[0], f
        res.append((tuple(int(v) for v in stats[f]), out[a:a + m].copy(), src[a:a + m].copy()))
    return res


@pytest.fixture(scope="module")
def compact(engine0, sets, frames_of):
    """table set, dtype, batch -> the library's per-frame (stats, rows, src) of the whole batch in one call, table ids 0 and 1; once"""
    cache = {}

    def get(name, dtype, batch):
        key = (name, np.dtype(dtype).name, batch)
        if key not in cache:
            fr = frames_of(dtype)[batch]
            tids = [engine0.table_ids_from_arrays(sets[name], o) for o in fei.orders(len(fr))]
            assert max(max(t) for t in tids) <= 2
            cache[key] = _run(engine0, fr, tids)
        return cache[key]
    return get


def _same_bytes(got, want):
    assert len(got) == len(want)
    for f, ((s1, r1, src1), (s0, r0, src0)) in enumerate(zip(got, want)):
        assert s1 == s0, (f, s1, s0)
        assert np.array_equal(src1, src0), f
        assert r1.dtype == r0.dtype and r1.tobytes() == r0.tobytes(), f


# ---- (a) the compact layout against the twin, and against the stable argsort itself -----------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("name", fei.SETS)
@pytest.mark.parametrize("batch", BATCHES)
def test_compact_results_match_the_twin_and_the_stable_sort(compact, reference, frames_of, batch, name, dtype):
    frames, got, want = frames_of(dtype)[batch], compact(name, dtype, batch), reference(name, dtype, batch)
    assert len(got) == len(want) == len(frames)
    changed = 0
    for f, (pc, (st, rows, src), (st0, aug, src0)) in enumerate(zip(frames, got, want)):
        assert st == tuple(int(v) for v in st0), (f, st, st0)
        assert np.array_equal(src, src0), f
        assert np.array_equal(rows[:, 3:], aug[:, 3:]), f
        np.testing.assert_allclose(rows[:, :3], aug[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
        # independent of the twin: src is a subsequence of the stable argsort by channel ...
        o = np.argsort(pc[:, 4], kind="stable")
        place = np.empty(o.shape[0], np.int64)
        place[o] = np.arange(o.shape[0])
        assert ((src >= 0) & (src < pc.shape[0])).all() and (np.diff(place[src]) > 0).all(), f
        # ... and every output row is the row of its source: the channel where column 4 still holds it, the coordinates where no flake moved them
        inp = pc[src]
        nolaser = inp[:, 4] >= fei.N_LASERS
        assert np.array_equal(rows[nolaser, 4], inp[nolaser, 4]) and np.isin(rows[~nolaser, 4], (0, 1, 2)).all(), f
        still = nolaser | (rows[:, 4] != 2)
        assert rows[still, :3].tobytes() == inp[still, :3].tobytes(), f
        changed += int(np.isin(rows[~nolaser, 4], (1, 2)).sum())
        if name == "empty":                                   # no flake anywhere: every row is its source row, the intensity rounded (simulation.py:516)
            assert rows[:, :3].tobytes() == inp[:, :3].tobytes() and np.array_equal(rows[:, 3], np.round(inp[:, 3])), f
            assert (rows[~nolaser, 4] == 0).all(), f
    assert changed == 0 if name == "empty" else changed > 20
    if batch == "ragged":
        assert got[6][1].shape[0] == 0 and got[6][0] == (0, 0, 0)          # the empty frame


# ---- (b) batching invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_a_frame_gives_the_same_bytes_alone_in_fours_and_in_the_batch_of_nine(engine0, compact, sets, frames_of, dtype):
    """Batches of up to four frames take k_seg_small on the caller's stream, the batch of nine the three-kernel builder beside the sort's
    second pass: the order inside a table differs (atomics), the bytes must not."""
    frames, nine = frames_of(dtype)["ragged"], compact("small", dtype, "ragged")
    orders = fei.orders(len(frames))
    tids = [engine0.table_ids_from_arrays(sets["small"], o) for o in orders]
    for f in range(len(frames)):
        _same_bytes(_run(engine0, frames[f:f + 1], tids[f:f + 1]), nine[f:f + 1])
    for pick in ([0, 1, 2, 3], [4, 5, 6, 7], [8, 6, 3, 7], [5, 2, 8, 0]):
        _same_bytes(_run(engine0, [frames[f] for f in pick], [tids[f] for f in pick]), [nine[f] for f in pick])


# ---- (c) the aligned layout -------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _aligned(frames, tl, keep=None):
    from lidar_snow_sim_amd.tensors import augment_batch
    res = augment_batch([_t(f) for f in frames], "unused", fei.BD, particles=tl, orders=fei.orders(len(frames)), thr_polys=[fei.POLY] * len(frames),
                        layout="aligned", keep=None if keep is None else [_t(k) for k in keep])
    return [(tuple(int(v) for v in s), r.cpu().numpy(), k.cpu().numpy()) for s, r, k in res]


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("batch", ["thirteen", "ragged"])
def test_aligned_rows_and_keep_mask_agree_with_the_compact_layout(compact, sets, frames_of, batch, dtype):
    """As tests/test_gpu_aligned.py compares the two layouts: rows[src] are the compact rows, keep is true exactly at src, statistics are
    equal.  (Thirteen equal-sized frames: the device entry takes the uniform_rows form of sg_frame_of.)"""
    frames, want = frames_of(dtype)[batch], compact("small", dtype, batch)
    got = _aligned(frames, sets["small"])
    assert len(got) == len(want)
    for f, (pc, (st, rows, keep), (st0, aug, src)) in enumerate(zip(frames, got, want)):
        assert rows.dtype == pc.dtype and rows.shape == pc.shape and keep.dtype == np.bool_ and keep.shape == (pc.shape[0],), f
        assert st == st0, (f, st, st0)
        assert rows[src].tobytes() == aug.tobytes(), f
        assert np.array_equal(np.flatnonzero(keep), np.sort(src)), f


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("batch", ["thirteen", "ragged"])
def test_a_keep_mask_that_removes_the_row_before_the_descent(sets, frames_of, batch, dtype):
    """An input keep mask without row p - 1 of every two_runs frame (the last row of the first run: the one lane 0 of a round would load as
    "the row before") gives what the unmasked call gives on the frames without that row; the absent row comes back as it came."""
    frames = frames_of(dtype)[batch]
    ps = fei.P_TWO_RUNS if batch == "thirteen" else [p for _, p in fei.RAGGED_TWO_RUNS]
    masks = [np.ones(f.shape[0], bool) for f in frames]
    for m, p in zip(masks, ps):
        m[p - 1] = False
    assert sum(int((~m).sum()) for m in masks) == len(ps)
    got = _aligned(frames, sets["small"], keep=masks)
    ref = _aligned([f[m] for f, m in zip(frames, masks)], sets["small"])
    for f, (pc, m, (s1, rows, keep), (s0, r0, k0)) in enumerate(zip(frames, masks, got, ref)):
        assert s1 == s0, (f, s1, s0)
        assert rows[m].tobytes() == r0.tobytes() and np.array_equal(keep[m], k0), f
        assert not keep[~m].any() and rows[~m].tobytes() == pc[~m].tobytes(), f
    assert sum(int(k.sum()) for _, _, k in ref) > 1000


# ---- (d) the size of the table array ----------------------------------------------------------------------------------------------------
# snowgpu_batch.cpp / snowgpu_sort.hip, with n_tables = the highest id ever uploaded + 1:
#   1500    n_tables + 1 > 1024: the scans of k_seg_small (four frames) and k_seg_scan (nine) own two tables per thread
#   5000    n_tables + 1 > SG_SEG_SMALL_TABLES (4096): four frames fall back to the three-kernel builder on the side stream; five per thread
#   70000   tables.size() > 65536: no segments -- k_resolve_tables, the linear order of k_beams and the q_chunk regions, with the device sort
HIGH = [1500, 5000, 70000]


def _high_ids(eng, sets, high, n_frames):
    """the two `small` tables at ids 0 and 1, copies of them at high - 1 and high; per frame a channel -> id list that mixes all four"""
    a, b = sets["small"][0], sets["small"][1]
    assert a is not b and all(t is (a, b)[c % 2] for c, t in enumerate(sets["small"]))
    for tid, t in ((0, a), (1, b), (high, a.copy()), (high - 1, b.copy())):
        eng.ctx.upload_table(tid, t)
    tids = []
    for f, o in enumerate(fei.orders(n_frames)):
        tids.append([(o[c] % 2) if (c // 2 + f) % 2 == 0 else high - (o[c] % 2) for c in range(fei.N_LASERS)])
    assert {v for t in tids for v in t} == {0, 1, high - 1, high}
    return tids


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("high", HIGH)
def test_table_array_sizes_change_no_byte(compact, sets, frames_of, high, dtype):
    from lidar_snow_sim_amd import engine
    frames, want = frames_of(dtype)["ragged"], compact("small", dtype, "ragged")
    eng = engine.Engine(0)
    try:
        tids = _high_ids(eng, sets, high, len(frames))
        _same_bytes(_run(eng, frames[:4], tids[:4]), want[:4])
        _same_bytes(_run(eng, frames, tids), want)
    finally:
        eng.ctx.close()


def test_an_id_inside_a_large_table_array_that_was_never_uploaded_fails_the_call(compact, sets, frames_of):
    """Table array of 1501 entries; channel 8 of frame 3 (2049 rows: the channel has some) names id 1400 -- inside the array, never uploaded:
    SNOWGPU_E_INVALID with the message of test_gpu_scan_segments.py::test_unknown_table_id_of_one_segment_fails_the_call, from the batch of
    four (k_seg_small) and of nine; the engine works afterwards."""
    from lidar_snow_sim_amd import engine, _native
    frames, want = frames_of(np.float32)["ragged"], compact("small", np.float32, "ragged")
    assert (frames[3][:, 4] == 8).sum() > 0
    eng = engine.Engine(0)
    try:
        tids = _high_ids(eng, sets, 1500, len(frames))
        good = tids[3][8]
        tids[3][8] = 1400
        for k in (4, 9):
            with pytest.raises(_native.SnowGPUError) as e:
                _run(eng, frames[:k], tids[:k])
            assert e.value.code == _native.E_INVALID
            assert "a table id in table_ids was never uploaded" in str(e.value)
        tids[3][8] = good
        _same_bytes(_run(eng, frames, tids), want)
    finally:
        eng.ctx.close()
