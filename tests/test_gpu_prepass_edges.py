"""-m gpu: the noise-threshold prepass (csrc/snowgpu_prepass.hip, sg_lean.h, sg_prepass_dev.h) against the restatement of
tests/prepass_reference.py, on the frames of its settings table: row counts around the 1024-row tile and the 64-tile trip, NumPy's
float32 mean by ground count, range rows on the histogram's edges, tied row minima, exactly three and four usable range rows, both
batch paths of sg_prepass_run, channel-major and shuffled frames.  tests/test_prepass_reference.py shows on any machine that each
setting decides what it is listed for, that every discrete decision is clear of rounding, and that NumPy's own float64 answers lie
inside the bounds used here.

Exact: the histogram (np.histogram2d with its empty bins set to the ground count, element for element), the ground count, the float32
mean of the float32 range column (bit for bit).  Inside the bounds derived in tests/prepass_reference.py (first order, from the
long-double restatement): the record's means, maximum, slope, intercept and 11 sums; the device's polynomial at the frame's ground
ranges.  The polynomial also lies within the 1e-4 intensity units of DESIGN.md section 9 of the oracle's own np.polyfit.

Observed on an MI355X, largest |device - long double| / bound per setting (every test prints its own with -s), beside NumPy / SciPy's
own float64 fraction from tests/test_prepass_reference.py:
  record of prepass_stats (worst field)      float32 rows            float64 rows
    setting                                  device     NumPy        device     NumPy
    tiles (1: 1023 .. 66 561 rows)           0.20       2.4e-3       0.22       2.5e-3
    mean  (2: 3 .. 4099 ground rows)         0.23       7.5e-2       0.30       1.1e-1
    edges (3, 4, 5, 7)                       0.20       6.8e-4       0.17       5.7e-4
  The device's worst field is always the maximum of I / cos (bound: e_row alone -- it takes c where the reference takes cos(arccos(c)));
  every sum, mean, slope and intercept stays below 0.11 of its bound (below 4.3e-3 on the frames of 341 and more ground rows).  The
  float32 mean was bit-equal to np.mean for all 23 float32 frames; histograms and counts were equal everywhere.
  polynomial at the ground ranges            float32 rows                       float64 rows
    setting                                  device     NumPy     vs oracle     device     NumPy     vs oracle
    tiles                                    1.5e-4     1.1e-5    7.5e-8        1.8e-4     1.7e-5    2.1e-13
    mean                                     7.9e-4     1.3e-4    9.3e-6        1.1e-3     1.3e-4    4.5e-13
    edges                                    1.8e-5     8.9e-6    3.4e-8        2.9e-5     4.5e-6    2.6e-13
    batch of 16 / of 17 (6)                  1.5e-4     8.9e-6    7.5e-8        1.2e-4     1.1e-5    2.6e-13
  ("vs oracle": intensity units from oracle.snow_oracle.noise_threshold_poly, whose np.polyfit builds a float32 Vandermonde matrix on
  float32 rows; DESIGN.md section 9 allows 1e-4.)  The two batch paths gave the same bits for every frame.

Which frames reach the float32 mean through augment_batch: only those whose noise line falls back to the regression line (three usable
range rows at most) -- mean3, m3, m3sorted and the group `fallback` (fb129, fb136, fb257, fb1000: shuffled rows, ground counts across
NumPy's 128-term leaf and its splits).  Their ground ranges are compacted by k_lean_gather in the reference's order, channel-sorted
(simulation.py:447; an unsorted frame from the sort's sorted copy), summed by k_pre_mean32, which then writes the deferred quadratic.
NumPy's float32 pairwise sum depends on the order: for every fb frame the mean of the sorted order differs from the mean of the arrival
order, which moves the polynomial by 170 .. 1800 times its bound (tests/test_prepass_reference.py asserts both).  Every other frame of
setting 2 has a fitted noise line; its float32 mean is held through prepass_stats alone, which takes the rows as they come.
NOT YET RUN on a device: the group `fallback`, the batches of setting 6 with fb136 and fb1000 in them (the figures above are of the
batches without the two), and three variants of k_lean_gather that these frames are there to catch -- gathering an unsorted frame
from the rows as they came, and the sorted-copy walk without its wave offset or without `run +=`.

That the tests bite (each one-line variant of the library built apart from the tree and run once on the same device; test names
shortened: stats = test_histogram_and_record_of_prepass_stats, poly = test_device_polynomial_of_augment_batch, paths =
test_both_batch_paths_give_the_same_polynomial_bits):
  - hist_bin without its settle loops: stats[edges-f64], poly[edges-f64], paths[f64];
  - last edge exclusive: stats[every group, both dtypes], poly[mean-*];
  - tie-break to the last minimum in k_pre_rowmin: paths[*] (and 16 tests of tests/test_gpu_wet_edges.py); in k_lean_rowmin_solve:
    poly[every group, both dtypes], paths[*];
  - sequential np_leaf_sum_f32: stats[tiles-f32, mean-f32, edges-f32]; split without `% 8`: the same three and paths[f32];
  - k_lean_gather without the wave offset: stats[tiles-f32, mean-f32, edges-f32], paths[f32];
  - k_lean_means without `run +=` on the second 64-tile trip: stats[tiles-*], poly[tiles-*];
  - `m >= 3` in lean_lines_wave: poly[mean-f64, edges-*], paths[*].
  lean_lines_frame's copy of the `m > 3` rule feeds nothing prepass_stats returns (the record carries the regression line only), and
  k_pre_gather with k_pre_means' prefix is never launched by sg_wet_run (exact_f32_mean = false): neither is reachable from outside.
"""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded (one HIP runtime per process)

import prepass_reference as pr

pytestmark = pytest.mark.gpu

TAGS = ("f32", "f64")
BD = float(np.degrees(3e-3))
STATS_GROUPS = {
    "tiles": tuple(f"tiles{n}" for n in pr.TILE_ROWS),
    "mean": tuple(f"mean{k}" for k in pr.MEAN32_COUNTS),
    "edges": ("edges", "ties", "m3", "m4", "sorted"),
    "fallback": pr.FALLBACK_FRAMES + ("m3sorted",),
}


@pytest.fixture(scope="module")
def eng():
    from lidar_snow_sim_amd import engine
    return engine.get_engine(0)


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    return snow_oracle


@pytest.fixture(scope="module")
def tids(eng, tables):
    return eng.table_ids_from_arrays([tables["t"][i % 4] for i in range(64)], list(range(64)))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("group", list(STATS_GROUPS))
def test_histogram_and_record_of_prepass_stats(eng, group, tag):
    """Context.prepass_stats on one ragged batch per group: histogram and count exact, NumPy's float32 mean bit for bit (float32
    rows: every count of setting 2, the tile settings with their second 64-tile trip, the edge frames), the other fields in bounds."""
    names = STATS_GROUPS[group]
    rows, off = pr.concat([pr.frame(n, tag) for n in names])
    hist, rec = eng.ctx.prepass_stats(rows, off, plane=[pr.PLANE4] * len(names))
    worst, failures = {}, []
    for f, name in enumerate(names):
        g, e, ld = pr.stats_frame(pr.frame(name, tag))
        want = e.hist.hist.astype(np.int32)
        bad = np.argwhere(hist[f] != want)
        if bad.size:
            failures.append(f"{name}: {len(bad)} histogram bins differ, first (range row, bin) {bad[0].tolist()}: device {hist[f][tuple(bad[0])]}, NumPy {want[tuple(bad[0])]}")
        if rec[f, 0] != len(g.dist):
            failures.append(f"{name}: ground count {rec[f, 0]}, NumPy {len(g.dist)}")
        if tag == "f32":
            m32 = np.mean(g.dist)
            assert m32.dtype == np.float32
            if np.float64(m32) != rec[f, 2]:
                failures.append(f"{name}: float32 mean of {len(g.dist)} ranges {rec[f, 2]!r}, np.mean {float(m32)!r}")
        frac = np.abs(rec[f].astype(pr.L) - ld.rec) / np.where(ld.b_rec > 0, ld.b_rec, 1)
        frac[2] = 0.0                                                    # (float32 rows: exact, above; float64 rows: not filled in)
        for k in np.nonzero(frac > 1)[0]:
            failures.append(f"{name}: record field {pr.REC_FIELDS[k]} = {rec[f, k]!r}, long double {ld.rec[k]!r}, error / bound {float(frac[k]):.3g}")
        for k, v in enumerate(frac):
            worst[pr.REC_FIELDS[k]] = max(worst.get(pr.REC_FIELDS[k], 0.0), float(v))
    print(f"\n[prepass-edges] stats {group} {tag}: largest error / bound per field " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items() if k not in ("n", "xmean32")))
    assert not failures, "\n".join(failures)


def _polys(eng, tids, names, tag):
    rows, off = pr.concat([pr.frame(n, tag) for n in names])
    thr = eng.ctx.augment_batch(rows, off, [tids] * len(names), BD, plane=[pr.PLANE4] * len(names), want_thr=True)[4]
    return thr


def _check_polys(so, thr, names, tag, label):
    worst_b, worst_o, failures = 0.0, 0.0, []
    for f, name in enumerate(names):
        pc = pr.frame(name, tag)
        g, e, ld = pr.snow_frame(pc)
        err = np.abs(pr.poly_at(thr[f], ld) - ld.poly_at)
        frac = float(np.max(err / ld.b_poly_at))
        host = so.noise_threshold_poly(pc[np.argsort(pc[:, 4], kind="stable")], pr.PLANE_W, pr.PLANE_H, 0.7)
        vs_oracle = float(np.max(np.abs(pr.poly_at(thr[f], ld) - pr.poly_at(host, ld))))
        worst_b, worst_o = max(worst_b, frac), max(worst_o, vs_oracle)
        if frac > 1:
            failures.append(f"{name} (frame {f}, {e.m} usable range rows): polynomial off by {float(err.max()):.3e} at its ground ranges, error / bound {frac:.3g}")
        if vs_oracle > 1e-4:
            failures.append(f"{name} (frame {f}): {vs_oracle:.3e} intensity units from the oracle's np.polyfit")
    print(f"\n[prepass-edges] polynomial {label} {tag}: largest error / bound {worst_b:.2e}; largest distance from the oracle's np.polyfit {worst_o:.2e}")
    return failures


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("group", list(STATS_GROUPS))
def test_device_polynomial_of_augment_batch(eng, so, tids, group, tag):
    """augment_batch(want_thr=True) on the same groups (each below the batch switch: k_lean_rowmin_solve).  The frames whose noise
    line falls back to the regression line -- mean3, m3, m3sorted and the group `fallback` (129, 136, 257 and 1000 ground rows) -- take
    its intercept from NumPy's float32 mean on float32 rows (k_lean_gather, k_pre_mean32, which then writes the deferred quadratic).
    The other frames of setting 2 have a fitted noise line: their float32 means are held through prepass_stats alone."""
    names = STATS_GROUPS[group]
    assert len(names) <= pr.small_batch_limit()
    failures = _check_polys(so, _polys(eng, tids, names, tag), names, tag, group)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tag", TAGS)
def test_both_batch_paths_give_the_same_polynomial_bits(eng, so, tids, tag):
    """Setting 6: the same ragged frames in a batch at the switch of sg_prepass_run (k_lean_rowmin_solve) and in one just above it
    (k_pre_rowmin + k_lean_lines_solve) -- fallback and fitted noise lines, channel-major and shuffled frames mixed.  Every frame
    inside its bound in both, and the same polynomial bits whichever batch it sits in (the two paths share every sum's order).
    An empty frame is left out here: without the caller's polynomials it raises the reference's TypeError
    (tests/test_gpu_large_batch.py); the wet batches of tests/test_gpu_wet_edges.py carry one."""
    lim = pr.small_batch_limit()
    small, large = pr.batch_names(lim), pr.batch_names(lim + 1)
    t_small, t_large = _polys(eng, tids, small, tag), _polys(eng, tids, large, tag)
    failures = _check_polys(so, t_small, small, tag, f"batch of {lim}") + _check_polys(so, t_large, large, tag, f"batch of {lim + 1}")
    by_name = {}
    for names, thr in ((small, t_small), (large, t_large)):
        for f, name in enumerate(names):
            by_name.setdefault(name, []).append(thr[f].tobytes())
    differ = [n for n, v in by_name.items() if len(set(v)) > 1]
    assert not failures, "\n".join(failures)
    assert not differ, f"polynomial bits depend on the batch for {differ}"
