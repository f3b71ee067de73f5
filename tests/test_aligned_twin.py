"""The ALIGNED result layout without a GPU: snowgpu_cpu_augment_batch_aligned (include/snowgpu_cpu.h) -- every input row's output row at
the input's own index plus one keep flag per row -- against the twin's compacted entry and against the oracle, on the reference's L5
golden fixtures (float32 and float64 rows) and on the frame shapes the device kernel treats apart (firing order, a tile plus one row,
an empty frame).  This pins the bytes of REMOVED rows too: what aug_pc held just before simulation.py:523."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    snow_oracle.build()
    return snow_oracle


@pytest.fixture(scope="module")
def twin():
    from lidar_snow_sim_amd import build, _cpu_twin
    build.build_cpu_twin(verbose=False)
    assert hasattr(_cpu_twin.lib(), "snowgpu_cpu_augment_batch_aligned")
    return _cpu_twin


@pytest.fixture(scope="module")
def l5(twin, so, golden, tables):
    """Per L5 case: the input, its polynomial, the oracle's result, the twin's compacted and aligned results (computed once, read only)."""
    d = golden("L5_augment")
    tl = [tables["t"][i % 4] for i in range(64)]
    cases = []
    for case in range(8):
        pc, order = d[f"c{case}_pc"], list(d[f"c{case}_order"])
        plane = (d[f"c{case}_plane_w"], float(d[f"c{case}_plane_h"]))
        s0, a0, src0, extra = so.augment(pc, tl, float(d["bd"]), order, plane=plane, return_full=True)
        thr = np.asarray(extra["thr_poly"], np.float64)
        (st, aug, src), = twin.augment_batch([pc], tl, [order], float(d["bd"]), [thr], threads=2)
        (st_a, rows, keep), = twin.augment_batch([pc], tl, [order], float(d["bd"]), [thr], threads=2, layout="aligned")
        cases.append(dict(pc=pc, thr=thr, oracle=(s0, a0, src0), compact=(st, aug, src), aligned=(st_a, rows, keep)))
    return cases


def test_aligned_rows_and_flags_are_the_compacted_result_in_input_order(l5):
    """rows[keep] taken in src order equals the compacted rows byte for byte (the twin's and the oracle's), keep is true exactly at src,
    statistics (and so the counts) are equal; both row dtypes occur."""
    for c in l5:
        st, aug, src = c["compact"]
        s0, a0, src0 = c["oracle"]
        st_a, rows, keep = c["aligned"]
        assert rows.shape == c["pc"][:, :5].shape and rows.dtype == c["pc"].dtype and keep.dtype == np.bool_ and keep.shape == (len(rows),)
        assert rows[src].tobytes() == aug.tobytes() and rows[src0].tobytes() == a0.tobytes()
        assert np.array_equal(np.flatnonzero(keep), np.sort(src)) and np.array_equal(np.sort(src), np.sort(src0))
        assert int(keep.sum()) == len(aug)
        assert tuple(int(v) for v in st_a) == tuple(int(v) for v in st) == tuple(int(v) for v in s0)
    assert {c["pc"].dtype for c in l5} == {np.dtype(np.float32), np.dtype(np.float64)}


def test_removed_rows_hold_what_the_reference_held_before_it_dropped_them(l5):
    """A removed row: the input's coordinates (their bytes), a label other than 2 (scattered rows are always kept without the camera
    crop), np.round of the input's intensity where the label is 0, and an intensity at most the threshold polynomial at the ORIGINAL
    range (d and d^2 in the row dtype, simulation.py:465-469, :518-520) -- that is why it was removed."""
    n_removed = n_lab0 = n_lab1 = 0
    for c in l5:
        pc, (p0, p1, p2) = c["pc"][:, :5], c["thr"]
        _, rows, keep = c["aligned"]
        rem = ~keep
        n_removed += int(rem.sum())
        assert rows[rem, :3].tobytes() == pc[rem, :3].tobytes()
        lab = rows[rem, 4]
        assert not np.any(lab == 2)
        z = lab == 0
        n_lab0 += int(z.sum())
        n_lab1 += int((lab == 1).sum())
        assert np.array_equal(rows[rem, 3][z], np.round(pc[rem, 3][z]))
        x, y, zz = pc[rem, 0], pc[rem, 1], pc[rem, 2]
        d = np.sqrt((x * x + y * y) + zz * zz)                                   # (row dtype throughout)
        assert d.dtype == pc.dtype
        thr = (p0 * (d * d).astype(np.float64) + p1 * d.astype(np.float64)) + p2
        assert np.all(rows[rem, 3].astype(np.float64) <= thr)
        # ... and every kept row that is not scattered lies above it
        k = keep & (rows[:, 4] != 2)
        dk = np.sqrt((pc[k, 0] * pc[k, 0] + pc[k, 1] * pc[k, 1]) + pc[k, 2] * pc[k, 2])
        assert np.all(rows[k, 3].astype(np.float64) > (p0 * (dk * dk).astype(np.float64) + p1 * dk.astype(np.float64)) + p2)
    assert n_removed > 0 and n_lab0 + n_lab1 == n_removed, (n_removed, n_lab0, n_lab1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_firing_order_a_tile_plus_one_row_and_an_empty_frame_in_one_batch(twin, tables, dtype):
    """One frame in firing order (azimuth-major: the channel sort really permutes), one of 1025 rows, one empty frame: aligned against the
    compacted entry of the same batch."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    full = synthetic_sweep(64, 2048, seed=1400, intensity="lambert").reshape(64, 2048, 5)
    firing = np.ascontiguousarray(full[:, ::64].transpose(1, 0, 2).reshape(-1, 5)).astype(dtype)          # 32 azimuths x 64 channels
    assert np.any(np.diff(firing[:, 4]) < 0)
    frames = [firing, np.ascontiguousarray(full[:, 5::32].reshape(-1, 5)[:1025]).astype(dtype), np.zeros((0, 5), dtype)]
    tl = [tables["t"][i % 4] for i in range(64)]
    orders = [list(np.random.default_rng(21 + f).permutation(64)) for f in range(3)]
    polys = [[1e-3, 0.05, 12.0], [0.0, 0.2, 15.0], [0.0, 0.0, 0.0]]          # (input intensities: 8 .. 199, a quarter of them below 20)
    bd = float(np.degrees(3e-3))
    compact = twin.augment_batch(frames, tl, orders, bd, polys, threads=3)
    aligned = twin.augment_batch(frames, tl, orders, bd, polys, threads=3, layout="aligned")
    removed = 0
    for pc, (st, aug, src), (st_a, rows, keep) in zip(frames, compact, aligned):
        assert rows.shape == pc.shape and keep.shape == (len(pc),)
        assert tuple(int(v) for v in st_a) == tuple(int(v) for v in st)
        assert rows[src].tobytes() == aug.tobytes() and np.array_equal(np.flatnonzero(keep), np.sort(src))
        assert rows[~keep, :3].tobytes() == pc[~keep, :3].tobytes()
        removed += int((~keep).sum())
    assert removed > 0 and int(aligned[2][2].size) == 0
    assert np.any(np.diff(compact[0][2]) < 0)                 # (the compacted rows of the firing-order frame are NOT in input order)
