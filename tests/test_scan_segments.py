"""The inputs of tests/test_gpu_scan_segments.py (tests/scan_segment_inputs.py): what they are taken for, and that the two references of that
test -- the CPU twin and the oracle -- agree on them.  No GPU."""
import numpy as np
import pytest

import scan_segment_inputs as ssi


def test_inputs_are_what_they_are_taken_for():
    fr = ssi.frames()
    assert [f.shape[0] > 0 for f in fr] == [True, True, False, True] and all(f.dtype == np.float32 and f.shape[1] == 5 for f in fr)
    assert all(2000 < f.shape[0] < 6000 for f in fr if f.shape[0])
    want = {c: n for c, n in ssi.counts().items() if n}
    for f in fr[:2]:
        ch, n = np.unique(f[:, 4], return_counts=True)
        assert dict(zip(ch.astype(int).tolist(), n.tolist())) == want
    rows = set(want.values()) | {0}
    assert {0, 1, 63, 64, 65, 255, 256, 257, 300} <= rows
    c = ssi.counts()
    assert c[0] == ssi.BLOCK and c[1] == 0 and c[2] > ssi.BLOCK                   # an empty channel between full ones
    assert any(k >= ssi.N_LASERS for k in want)                                   # channels without a laser
    assert (np.diff(fr[0][:, 4]) >= 0).all() and (np.diff(fr[3][:, 4]) >= 0).all()    # read in place ...
    assert (np.diff(fr[1][:, 4]) < 0).any()                                       # ... and through the sorted copy
    for f in fr:
        if not f.shape[0]:
            continue
        sim = f[f[:, 4] < ssi.N_LASERS].astype(np.float64)
        d = np.linalg.norm(sim[:, :3], axis=1)
        az = np.mod(np.arctan2(sim[:, 1], sim[:, 0]), 2 * np.pi)
        far = d >= 120.002                                                        # where the reference raises once a flake is met
        assert far.any() and ((az[far] > ssi.FREE[0] - 1e-6) & (az[far] < ssi.FREE[1] + 1e-6)).all()
        assert np.isnan(d).any()
        assert (az[~np.isnan(az)] < 0.011).any() and (az[~np.isnan(az)] > 2 * np.pi - 0.009).any()      # both sides of the seam
    a = fr[0]
    assert ((a[:, 3] != np.round(a[:, 3])) | (a[:, 3] > 255) | (a[:, 3] < 0)).sum() >= 3 * 50   # intensities that no record can carry
    # the wide-wedge case: the wedge +- margin spans three bins or more for every beam
    assert np.radians(ssi.BD * ssi.WIDE) > 2 * (2 * np.pi / 2048)
    assert sorted(ssi.table_sets()) == ["empty", "heavy", "small"]
    assert all(sorted(o) == list(range(ssi.N_LASERS)) for o in ssi.orders()) and len(ssi.orders()) == len(fr)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,wide", ssi.CASES)
def test_cpu_twin_equals_the_oracle_on_the_gpu_test_inputs(name, wide, dtype):
    """The oracle runs every case without raising, and the twin gives its rows: rows kept, labels, intensities, statistics; moved
    coordinates to the parity tests' tolerance."""
    from lidar_snow_sim_amd import build, _cpu_twin
    from oracle import snow_oracle
    snow_oracle.build()
    build.build_cpu_twin(verbose=False)
    tl = ssi.table_sets()[name]
    frames, orders = ssi.frames(dtype), ssi.orders()
    bd = ssi.BD * wide
    res = _cpu_twin.augment_batch(frames, tl, orders, bd, [ssi.POLY] * len(frames), threads=4)
    moved = 0
    for pc, order, (st, aug, src) in zip(frames, orders, res):
        if pc.shape[0] == 0:
            assert aug.shape[0] == 0 and tuple(int(v) for v in st) == (0, 0, 0)
            continue
        s0, a0, src0 = snow_oracle.augment(pc, tl, bd, order, thr_poly=np.array(ssi.POLY), threads=4)
        assert tuple(int(v) for v in st) == tuple(int(v) for v in s0)
        assert np.array_equal(src, src0) and np.array_equal(aug[:, 3:], a0[:, 3:])
        np.testing.assert_allclose(aug[:, :3], a0[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
        moved += int((aug[:, 4] == 2).sum()) + int((aug[:, 4] == 1).sum())
        nolaser = pc[src][:, 4] >= ssi.N_LASERS
        assert nolaser.any() or pc is frames[3]
        thru = pc[src][nolaser].copy()                                                # copied through (simulation.py:516 rounds every intensity)
        thru[:, 3] = np.round(thru[:, 3])
        assert np.array_equal(aug[nolaser], thru, equal_nan=True)
    assert moved == 0 if name == "empty" else moved > 20
