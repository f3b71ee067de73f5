"""CPU: the inputs of tests/test_gpu_batch_scale.py (tests/batch_scale_inputs.py) on any machine -- the conditions without which a GPU test
that crosses a scan's trip length would pass a wrong carry all the same: present rows, opened cells and free rows on BOTH sides of every
border (frames 64 and 256, tiles 63 / 64 and 1024, runs 127 / 128 and 255 / 256), so that a total dropped or doubled at the border moves
an output; and that the two references of the masked snowfall test, the CPU twin and the oracle, agree on these frames.  Every condition
is asserted on the references alone."""
from functools import lru_cache

import numpy as np
import pytest

import batch_scale_inputs as bsi
import paste_reference as pr
import voxel_reference as vr


@pytest.fixture(scope="module")
def twin():
    from lidar_snow_sim_amd import build, _cpu_twin
    build.build_cpu_twin(verbose=False)
    return _cpu_twin


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    snow_oracle.build()
    return snow_oracle


@pytest.fixture(scope="module")
def tl(tables):
    return [tables["t"][i % 4] for i in range(64)]


# ---- many(F) ------------------------------------------------------------------------------------------------------------------------------
def test_many_is_the_list_it_is_taken_for():
    frames, masks = bsi.many(321)
    n = np.array([len(f) for f in frames])
    assert len(frames) == 321 and n.max() == 512 and 80000 < n.sum() < 100000 and set(n // 64) == set(range(9)) and not (n % 64).any()
    assert sorted(np.flatnonzero(n == 0)) == sorted(bsi.EMPTY) and {10, 11, 258} <= set(bsi.EMPTY)
    for j, (f, m) in enumerate(zip(frames, masks)):
        assert f.dtype == np.float32 and f.shape == (n[j], 5) and m.dtype == np.bool_ and m.shape == (n[j],) and not f.flags.writeable and not m.flags.writeable
        descends = bool((np.diff(f[:, 4]) < 0).any())
        assert descends == (j % 7 == 0 and n[j] > 64), j                      # firing order: the channel sort permutes (one azimuth step is both orders)
        if j in bsi.ALL_ABSENT:
            assert n[j] and not m.any()
        elif j in bsi.ALL_PRESENT:
            assert n[j] and m.all()
    for j in bsi.MIXED:
        assert n[j] and masks[j].any() and not masks[j].all(), j
    for F in bsi.SIZES:
        fr, ms = bsi.many(F)
        assert len(fr) == len(ms) == F and F - 1 in bsi.MIXED and all(a is b for a, b in zip(fr, frames))
    assert bsi.many(257, "float64")[0][5].dtype == np.float64 and np.array_equal(bsi.many(257, "float64")[0][5], frames[5])


@pytest.mark.parametrize("F", bsi.SIZES)
def test_many_has_present_rows_on_both_sides_of_every_border(F):
    """k_mask_offsets / k_voxel_offsets: 64 frames a wave (s_wave[]), 256 a trip (carry)."""
    _, masks = bsi.many(F)
    present = np.array([int(m.sum()) for m in masks])
    cum = np.concatenate(([0], np.cumsum(present)))                           # cum[k]: the present rows in front of frame k
    spans = [(0, 64), (64, min(128, F))] + ([(192, 256)] if F >= 256 else []) + ([(256, F)] if F > 256 else [])
    for a, b in spans:
        assert present[a:b].sum() > 0, (a, b)
    assert (np.diff(cum[62:67]) > 0).all()
    if F > 256:
        assert (np.diff(cum[254:min(259, F + 1)]) > 0).all() and len(cum[254:min(259, F + 1)]) >= 4


def test_the_twin_changes_firing_order_rows_behind_frame_256(twin, tl):
    """A wrong offset behind the carry shows only in frames whose result differs from their input: behind frame 256 the CPU twin scatters
    or removes rows of frames in firing order (which the channel sort permutes as well), and in front of it rows of either kind."""
    frames, masks = bsi.many(321)
    sub = [np.ascontiguousarray(f[m]) for f, m in zip(frames, masks)]
    res = twin.augment_batch(sub, tl, bsi.orders(321), bsi.BD, [bsi.POLY] * 321, threads=4, layout="aligned")
    changed = 0
    for j in range(257, 321):
        if (np.diff(sub[j][:, 4]) < 0).any():
            _, rows, keep = res[j]
            changed += int((rows[:, 4] == 2).sum()) + int((~keep).sum())
    assert changed > 0
    assert sum(int((~k).sum()) for _, _, k in res[:256]) > 0 and sum(int((r[:, 4] == 2).sum()) for _, r, _ in res[:256]) > 0


# ---- long() -------------------------------------------------------------------------------------------------------------------------------
def test_long_has_present_and_absent_rows_on_both_sides_of_tile_64():
    """k_mask_scan, k_pre_means: 64 tiles of 1024 rows a trip."""
    frames, masks = bsi.long()
    assert tuple(len(f) for f in frames) == bsi.LONG_ROWS == (131073, 65537, 65536, 131072, 700, 0)
    for k, f in enumerate(frames):
        assert f.dtype == np.float32 and not f.flags.writeable and bool((np.diff(f[:, 4]) < 0).any()) == (k in bsi.LONG_FIRING)
    both = lambda m: m.any() and not m.all()          # noqa: E731
    for k in (0, 1, 3):
        m = masks[k]
        assert both(m[63 * bsi.TILE:64 * bsi.TILE]), k
        assert m[:64 * bsi.TILE].sum() != m[:63 * bsi.TILE].sum() and m[64 * bsi.TILE:].sum() > 0, k
    for k in (0, 3):
        assert both(masks[k][64 * bsi.TILE:65 * bsi.TILE]), k
    # tile 64 of frame 1 and tile 128 of frame 0 hold ONE row, which is present: the second (third) trip's only count
    assert len(masks[1]) - 64 * bsi.TILE == 1 and masks[1][-1] and len(masks[0]) - 128 * bsi.TILE == 1 and masks[0][-1]
    assert frames[0][-1, 4] == 63 and frames[1][-1, 4] == 63


def test_long_is_a_wet_setting_under_its_masks():
    """What tests/test_wet_aligned_reference.py asks of a masked wet frame, on the four long frames: at least 1000 present ground rows,
    more than 100 kept and more than 100 dropped, the float64 and the long-double chain agree on every row and every decision is clear by a
    relative 1e-7; the ground rows lie on both sides of tile 64.  The 700-row frame and the empty one stay below 1000: flag 1."""
    import prepass_reference as ppr
    frames, masks = bsi.long()
    for k, (f, m) in enumerate(zip(frames, masks)):
        r = ppr.wet_restated(np.ascontiguousarray(f[m]), **bsi.WET)
        if k >= 4:
            assert r.flag == 1
            continue
        assert r.flag == 0 and r.g.mask.sum() >= 1000
        kept, dropped = int(r.chain.keep.sum()), int((~r.chain.keep).sum())
        assert kept > 100 and dropped > 100 and np.array_equal(r.chain.keep, r.chain_ld.keep)
        assert float((np.abs(r.chain_ld.new_i - r.chain_ld.lim) / np.abs(r.chain_ld.lim)).min()) > 1e-7
        g = ppr.ground_rows(f, delta=bsi.WET["delta"]).mask & m
        assert g[:64 * bsi.TILE].sum() > 100 and (k in (1, 2) or g[64 * bsi.TILE:].sum() > 100), k


# ---- voxels -------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _firsts(which):
    """(first, offsets): first[i] = row i opens a cell of its frame under STRADDLE (no mask); from voxel_reference.cells alone."""
    rows, off = bsi.voxel_batch() if which == "voxel_batch" else (np.concatenate(bsi.many(321)[0]), bsi.offsets(bsi.many(321)[0]))
    rng, size = vr.STRADDLE[:2]
    ok, c = vr.cells(rows, rng, size)
    nx, ny, nz = vr.grid_dims(rng, size)
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    key = np.where(ok, ((frame * nz + c[:, 2]) * ny + c[:, 1]) * nx + c[:, 0], -1)
    u, at = np.unique(key, return_index=True)                                 # (the first occurrence of every key)
    first = np.zeros(len(rows), bool)
    first[at[u >= 0]] = True
    return first, off


def test_voxel_batch_opens_cells_in_tile_1024_and_in_most_tiles_before():
    """k_voxel_tile_scan: 64 tiles a wave (wave_sum[]), 1024 a trip over the batch (carry)."""
    rows, off = bsi.voxel_batch()
    assert tuple(np.diff(off)) == bsi.VOXEL_ROWS and len(rows) == 1049278 and -(-len(rows) // bsi.TILE) == 1025 and off[-2] >= 1024 * bsi.TILE
    first, _ = _firsts("voxel_batch")
    per_tile = np.add.reduceat(first, np.arange(0, len(rows), bsi.TILE))
    assert len(per_tile) == 1025 and int((per_tile > 0).sum()) >= 900
    assert per_tile[:64].sum() > 0 and per_tile[64:1024].sum() > 0 and int(first[off[-2]:].sum()) >= 10
    assert int(first[off[-2]:].sum()) == per_tile[1024] - int(first[1024 * bsi.TILE:off[-2]].sum())
    # the walk itself (the expectation of the GPU test) opens those voxels for the 700-row frame, behind 1024 tiles of others
    want = vr.voxelize(rows, *vr.STRADDLE, 4, None, off)
    vo = want["voxel_offsets"]
    assert vo[-1] - vo[-2] == int(first[off[-2]:].sum()) >= 10 and vo[-2] == vo[-3] and vo[-2] > 9 * 1000
    opened = np.flatnonzero(first[off[-2]:]) + off[-2]
    assert (opened >= 1024 * bsi.TILE).all() and np.array_equal(want["voxel_of"][opened], np.arange(vo[-2], vo[-1]))


def test_many_opens_more_and_fewer_than_40_cells_on_both_sides_of_frame_256():
    """k_voxel_offsets sums m_f = min(cells, V): with V = 40 frames above, below and at zero cells lie in front of and behind the carry."""
    first, off = _firsts("many")
    cells = np.array([int(first[a:b].sum()) for a, b in zip(off[:-1], off[1:])])
    for side in (cells[:256], cells[256:]):
        assert (side > 40).sum() >= 5 and ((side > 0) & (side < 40)).sum() >= 5 and (side == 0).sum() >= 1
    frames, masks = bsi.many(321)
    rows, keep = np.concatenate(frames), np.concatenate(masks)
    for kp in (None, keep):
        want = vr.voxelize(rows, *vr.STRADDLE[:3], 40, 4, kp, off)
        m = np.diff(want["voxel_offsets"])
        for side in (m[:256], m[256:]):
            assert (side == 40).sum() >= 5 and ((side > 0) & (side < 40)).sum() >= 5 and (side == 0).sum() >= 1
    assert (m[list(bsi.ALL_ABSENT)] == 0).all()


# ---- paste --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_paste_long_straddles_threads_63_and_64_and_ends_in_run_256(dtype):
    """k_paste_frame: 257 runs over 256 threads -- chunk = 2; thread 63 holds runs 126 and 127, thread 64 runs 128 and 129, thread 127
    runs 254 and 255, thread 128 run 256 alone (hi clamped to the runs), threads 129 .. 255 nothing (lo clamped)."""
    c = bsi.paste_long(dtype)
    e = pr.paste_objects(c["rows"], c["offsets"], c["keep"], c["gt_boxes"], c["pose"], c["bank"], c["groups"], c["seed"], c["step"], c["ew"])
    off, B = c["offsets"], c["gt_boxes"].shape[1]
    assert tuple(np.diff(off)) == bsi.PASTE_ROWS and -(-max(bsi.PASTE_ROWS) // bsi.RUN) == 257 and -(-257 // 256) == 2
    free0 = np.flatnonzero(~c["keep"][:off[1]])
    assert sorted(set(free0 // bsi.RUN)) == [0, 1, 127, 128, 129, 254, 255, 256] == [r for r, _, _ in bsi.PASTE_FREE]
    assert tuple(np.diff(c["bank"]["offsets"])) == bsi.PASTE_POINTS and e["state"].tolist() == [[1, 1, 1], [1, 1, 1], [1, 4, 4]]
    src0 = e["source"][:off[1]]
    runs_of = lambda q: sorted(set(np.flatnonzero(src0 == B + q) // bsi.RUN))          # noqa: E731
    assert runs_of(0) == [0, 1, 127] and runs_of(1) == [127, 128, 129] and runs_of(2) == [254, 255, 256]
    assert np.flatnonzero(src0 == B + 2)[-1] == bsi.PASTE_ROWS[0] - 1 == 131072       # ... through the frame's last row, the only row of run 256
    # Every free row of frame 0 is taken (an object that ends on the last row leaves none behind it); the remainder is frame 1's.
    assert e["count"][0].tolist()[:2] == [3, sum(bsi.PASTE_POINTS)] and e["count"][0, 3] == sum(bsi.PASTE_POINTS) == len(free0)
    assert e["count"][1, 3] == 120 == sum(bsi.PASTE_POINTS) + 35 and e["count"][1, 1] == sum(bsi.PASTE_POINTS)
    free1 = off[1] + np.flatnonzero(~c["keep"][off[1]:off[2]])
    assert sorted(set((free1 - off[1]) // bsi.RUN)) == [0, 255] and (e["source"][free1[:85]] >= B).all() and (e["source"][free1[85:]] == -1).all()
    assert e["count"][2].tolist() == [1, bsi.PASTE_POINTS[0], e["count"][2, 2], bsi.PASTE_FREE_2]
    # the removal clears scene rows behind run 128 (and in front of it)
    gone0 = np.flatnonzero(c["keep"][:off[1]] & ~e["keep"][:off[1]])
    assert len(gone0) == e["count"][0, 2] > 20 and (gone0 // bsi.RUN >= 128).sum() > 5 and (gone0 // bsi.RUN < 128).sum() > 5
    assert np.isnan(c["rows"][[58, 65536, 131072]]).all() and not np.isnan(e["rows"][[58, 65536, 131072]]).any()


# ---- roi pooling --------------------------------------------------------------------------------------------------------------------------
def test_roi_long_has_members_on_both_sides_of_run_128():
    """k_roi_count / k_roi_scan / k_roi_rank: a table row per 512-row run, 257 rows for both frames -- the short frame's runs 129 .. 256
    lie beyond its length."""
    import box_reference as br
    import roipool_reference as rr
    c = bsi.roi_long()
    e = rr.pool_case(c)
    off = c["offsets"]
    assert tuple(np.diff(off)) == bsi.LONG_ROWS[:2] and -(-131073 // bsi.RUN) == 257 and -(-65537 // bsi.RUN) == 129
    usable = br.usable_rows(c["rows"], c["keep"])
    for f in range(2):
        a, b = int(off[f]), int(off[f + 1])
        assert e["count"][f, 4] == usable[a:b].sum() > 40000 and np.array_equal(e["index"][f, 4], a + np.flatnonzero(usable[a:b])[:64])
        assert not usable[a:a + 64].all()                                       # (the first 64 members are not simply the first 64 rows)
        runs = set()
        for j in range(4):
            at = rr.members(c["rows"][a:b], c["rois"][f, j], c["pose"][f, j], c["ew"], c["keep"][a:b])[0]
            assert len(at) == e["count"][f, j] >= 3
            runs |= set(at // bsi.RUN)
        assert min(runs) < 64 and max(runs) >= (128 if f == 0 else 120) and len(runs) >= 6, sorted(runs)
    assert (e["count"][:, :4] < 64).any() or (e["count"][:, :4] > 64).any()


# ---- the two references of the masked snowfall test ------------------------------------------------------------------------------------------
def test_cpu_twin_equals_the_oracle_on_the_compacted_frames(twin, so, tl):
    """Every 20th frame of many(321) and the 65 537-row frame of long(), compacted by their masks: the aligned twin against the oracle as
    tests/test_front_end_inputs.py compares them -- statistics, the kept set, labels and intensities equal, coordinates at rtol 1e-6."""
    bd = bsi.BD
    frames, masks = bsi.many(321)
    picks = [(frames[j], masks[j], bsi.orders(321)[j]) for j in range(0, 321, 20)] + [(bsi.long()[0][1], bsi.long()[1][1], bsi.orders(6, 81)[1])]
    sub = [np.ascontiguousarray(f[m]) for f, m, _ in picks]
    res = twin.augment_batch(sub, tl, [o for _, _, o in picks], bd, [bsi.POLY] * len(sub), threads=4, layout="aligned")
    hit = removed = 0
    for pc, (_, _, order), (st, rows, keep) in zip(sub, picks, res):
        if len(pc) == 0:
            assert tuple(int(v) for v in st) == (0, 0, 0)
            continue
        s0, a0, src0 = so.augment(pc, tl, bd, order, thr_poly=np.array(bsi.POLY), threads=4)
        assert tuple(int(v) for v in st) == tuple(int(v) for v in s0)
        assert np.array_equal(np.flatnonzero(keep), np.sort(src0)) and np.array_equal(rows[src0][:, 3:], a0[:, 3:])
        np.testing.assert_allclose(rows[src0][:, :3], a0[:, :3], rtol=1e-6, atol=0)
        hit += int(np.isin(rows[keep, 4], (1, 2)).sum())
        removed += int((~keep).sum())
    assert hit > 20 and removed > 0
