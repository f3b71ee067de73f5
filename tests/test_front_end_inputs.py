"""The inputs of tests/test_gpu_front_end.py (tests/front_end_inputs.py): that the two references of that test -- the CPU twin and the
oracle -- agree on every frame, and the conditions without which the GPU test would pass a sort that reads an unsorted frame in place:
one descent exactly where it is claimed, rows that the stable sort moves, moved rows that survive into the result and that the
simulation changes.  No GPU."""
import numpy as np
import pytest

import front_end_inputs as fei


@pytest.fixture(scope="module")
def twin():
    from lidar_snow_sim_amd import build, _cpu_twin
    build.build_cpu_twin(verbose=False)
    return _cpu_twin


@pytest.fixture(scope="module")
def small(twin):
    """dtype -> batch name -> (frames, the twin's [(stats, rows, src)]) under the `small` tables, computed once"""
    cache = {}

    def get(dtype):
        key = np.dtype(dtype).name
        if key not in cache:
            tl = fei.table_sets()["small"]
            cache[key] = {name: (fr, twin.augment_batch(fr, tl, fei.orders(len(fr)), fei.BD, [fei.POLY] * len(fr), threads=4))
                          for name, fr in fei.batches(dtype).items()}
        return cache[key]
    return get


def test_shapes_and_orders():
    b = fei.batches()
    assert [len(b[k]) for k in ("thirteen", "levels", "ragged", "ranks")] == [13, 3, 9, 4]
    assert all(f.shape == (fei.N, 5) and f.dtype == np.float32 for k in ("thirteen", "levels", "ranks") for f in b[k])
    assert fei.N == 2500 and 2 * fei.TILE < fei.N < 3 * fei.TILE                     # three tiles, the last partial
    assert fei.P_TWO_RUNS == [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2499] and fei.P_LEVEL == [64, 256, 1024]
    assert [f.shape[0] for f in b["ragged"]] == [2, 65, 1025, 2049, 1023, 1024, 0, 1, 2049]
    assert fei.RAGGED_TWO_RUNS == [(2, 1), (65, 64), (1025, 1024), (2049, 1024)]
    o = fei.orders(13)
    assert all(sorted(v) == list(range(fei.N_LASERS)) for v in o) and o[0] != o[1] != o[2] != o[0] and o[3] == o[0]
    assert fei.batches(np.float64)["ragged"][3].dtype == np.float64
    for k, frames in b.items():                                                      # rows are re-ordered, nothing else
        for f in frames:
            ch = f[:, 4]
            assert ((ch == np.round(ch)) & (ch >= 0) & (ch < 256)).all(), k


def test_two_runs_have_one_descent_where_it_is_claimed():
    b = fei.batches()
    cases = list(zip(b["thirteen"], [(fei.N, p) for p in fei.P_TWO_RUNS])) + list(zip(b["ragged"][:4], fei.RAGGED_TWO_RUNS))
    assert len(cases) == 17
    for f, (n, p) in cases:
        assert f.shape[0] == n and fei.descents(f).tolist() == [p], (n, p)
        assert f[p, 4] < f[p - 1, 4]
        assert fei.moved(f).shape[0] >= (64 if 64 <= p <= 2048 else 1), (n, p, fei.moved(f).shape[0])
    # a descent seen by lane 0 of a round only: p on a round (64), wave (256) and tile (1024) border, in the first tile and in later ones
    assert {p % 64 for _, (_, p) in cases} >= {0, 1, 63} and {64, 256, 1024, 2048} <= {p for _, (_, p) in cases}


def test_level_and_sorted_frames_have_no_descent():
    b = fei.batches()
    for f, p in zip(b["levels"], fei.P_LEVEL):
        assert fei.descents(f).size == 0 and f[p, 4] == f[p - 1, 4] and fei.moved(f).size == 0
    for f, kind in zip(b["ragged"], fei.RAGGED_KIND):
        if kind in ("sorted", "one_row", "empty"):
            assert fei.descents(f).size == 0
    assert fei.RAGGED_KIND.count("sorted") == 2 and fei.descents(b["ragged"][8]).size >= 60      # descending: every change of channel
    assert (np.diff(b["ragged"][8][:, 4]) <= 0).all()


def test_rank_frames_are_what_they_are_taken_for():
    all256, one, alt, mixed = (f[:, 4] for f in fei.rank_frames())
    assert np.array_equal(all256, np.arange(fei.N) % 256) and np.unique(all256).size == 256
    assert (one == 5).all() and one.size > 2 * fei.TILE                              # one channel over three tiles
    assert np.array_equal(alt[:4], [63, 0, 63, 0]) and set(np.unique(alt)) == {0.0, 63.0}
    waves = [mixed[a:a + 64] for a in range(0, fei.N - 63, 64)]
    kinds = [np.unique(w).size for w in waves]
    assert set(kinds) == {1, 64} and all(a != b for a, b in zip(kinds, kinds[1:]))   # one channel, 64 channels, in turn
    assert len({w[0] for w, k in zip(waves, kinds) if k == 1}) > 10
    for f in fei.rank_frames()[2:]:
        assert fei.moved(f).size > 1000


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", fei.SETS)
def test_cpu_twin_equals_the_oracle_on_the_gpu_test_inputs(twin, name, dtype):
    """As tests/test_scan_segments.py: the oracle runs every frame without raising, and the twin gives its rows: rows kept, labels,
    intensities, statistics; moved coordinates to the parity tests' tolerance."""
    from oracle import snow_oracle
    snow_oracle.build()
    tl = fei.table_sets()[name]
    hit = through = 0
    for batch, frames in fei.batches(dtype).items():
        orders = fei.orders(len(frames))
        res = twin.augment_batch(frames, tl, orders, fei.BD, [fei.POLY] * len(frames), threads=4)
        for pc, order, (st, aug, src) in zip(frames, orders, res):
            if pc.shape[0] == 0:
                assert aug.shape[0] == 0 and tuple(int(v) for v in st) == (0, 0, 0)
                continue
            s0, a0, src0 = snow_oracle.augment(pc, tl, fei.BD, order, thr_poly=np.array(fei.POLY), threads=4)
            assert tuple(int(v) for v in st) == tuple(int(v) for v in s0), batch
            assert np.array_equal(src, src0) and np.array_equal(aug[:, 3:], a0[:, 3:]), batch
            np.testing.assert_allclose(aug[:, :3], a0[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
            hit += int((aug[:, 4] == 2).sum()) + int((aug[:, 4] == 1).sum())
            nolaser = pc[src][:, 4] >= fei.N_LASERS
            through += int(nolaser.sum())
            thru = pc[src][nolaser].copy()                                            # copied through (simulation.py:516 rounds every intensity)
            thru[:, 3] = np.round(thru[:, 3])
            assert np.array_equal(aug[nolaser], thru, equal_nan=True)
    assert hit == 0 if name == "empty" else hit > 20
    assert through > 100


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moved_rows_survive_and_are_changed_by_the_simulation(small, dtype):
    """Read in place, a two_runs frame would hand the rows that the sort moves to the wrong channel's segment.  That shows in the GPU test
    only if such rows are in the result (src) and carry something the simulation did to them."""
    got = small(dtype)
    cases = list(zip(*got["thirteen"])) + list(zip(*got["ragged"]))[:4]
    changed = 0
    for pc, (_, aug, src) in cases:
        mv = np.isin(src, fei.moved(pc))
        assert mv.any(), pc.shape
        changed += int(np.isin(aug[mv, 4], (1, 2)).sum())                             # attenuated or scattered (rows with a laser: a label)
    assert changed >= 100, changed
    for pc, (_, aug, src) in zip(*got["ranks"]):                                      # the rank frames, likewise
        assert pc[0, 4] == 5 or np.isin(src, fei.moved(pc)).any()
