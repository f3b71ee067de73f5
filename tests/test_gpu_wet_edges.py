"""-m gpu: the wet-ground model (csrc/snowgpu_wet.hip: the full estimator, k_wet_apply, k_wet_scan, k_wet_scatter) through
Context.wet_ground_batch against oracle.snow_oracle.ground_water_augmentation, on the wet settings of tests/prepass_reference.py:
water_height / pavement_depth in {0, 0.4, 0.8, 1, 2}, flat_earth and replace on and off, delta 0.2 and 0.5, a second noise_floor /
power_factor pair that puts ground rows above rho = 1, exactly three and four usable range rows, 65 tiles + 1, the 1000-row rule, an
empty frame in the middle of every batch -- and, with the caller's lines (lines=), one frame that reaches every branch of the per-row
chain, against the restatement with the same lines.  tests/test_prepass_reference.py shows on any machine that the restatement equals
the oracle bit for bit, that every setting reaches its branches and that every keep / drop decision is clear by a relative 1e-7.

Exact: the rows kept, the [non-ground ; kept ground] order, labels, source rows, counts and flags.  Intensities at rtol 1e-9 on float64
rows and 1e-7 on float32 rows (the tolerances of tests/test_gpu_parity.py::test_L6_wet_ground); with lines= 1e-9 for both, because the
fit no longer enters.  The two fitted lines (wet_last_fit) inside the bounds derived in tests/prepass_reference.py.

Observed on an MI355X (every test prints its own with -s), beside NumPy / SciPy's own float64 fraction of the lines' bounds:
  parameters (WET_PARAMS index)    largest relative intensity error     fitted lines: largest error / bound
                                   float32 rows    float64 rows         device f32 / f64       NumPy f32 / f64
    0  ratio 0                     3.7e-16         3.0e-16              8.9e-4 / 1.2e-3        7.0e-4 / 1.2e-3
    1  ratio 0.4, flat earth       6.2e-15         6.1e-15              6.1e-4 / 1.2e-3        6.1e-4 / 1.2e-3
    2  ratio 0.8, delta 0.2        3.3e-14         3.4e-14              1.6e-3 / 9.5e-4        3.5e-4 / 6.0e-4
    3  ratio 1, flat, delta 0.2    2.4e-14         2.5e-14              1.6e-3 / 9.5e-4        3.5e-4 / 6.0e-4
    4  ratio 2                     2.7e-14         2.5e-14              6.1e-4 / 1.2e-3        6.1e-4 / 1.2e-3
    5  ratio 0.8, rho above 1      4.7e-14         4.9e-14              6.1e-4 / 1.2e-3        6.1e-4 / 1.2e-3
    6  ratio 2, flat, rho above 1  8.8e-15         9.8e-15              6.1e-4 / 1.2e-3        6.1e-4 / 1.2e-3
    caller's lines                 2.7e-13         5.7e-14
  Rows kept, order, labels, sources, counts and flags were equal everywhere.

That the tests bite (each one-line variant of the library built apart from the tree and run once on the same device; settings =
test_wet_settings_against_the_oracle, rule = test_the_1000_row_rule_in_one_batch, lines = test_the_callers_lines_through_every_branch):
  - rho unclipped at 1: settings[5-*, 6-*], lines[*];          - fw unclipped: settings[4-*, 6-*];
  - min_ground 1001: rule[*];                                  - k_wet_scan without `+= na`: all 18 tests;
  - `m >= 3` in k_pre_lines: settings[0, 1, 4, 5, 6 -*] (delta 0.5: the m3 frame is fitted);
  - tie-break to the last minimum in k_pre_rowmin: settings[*], rule[*].
"""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded (one HIP runtime per process)

import prepass_reference as pr

pytestmark = pytest.mark.gpu

TAGS = ("f32", "f64")


@pytest.fixture(scope="module")
def eng():
    from lidar_snow_sim_amd import engine
    return engine.get_engine(0)


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    return snow_oracle


def _run(eng, names, tag, kw, lines=None):
    frames = [pr.frame(n, tag) for n in names]
    rows, off = pr.concat(frames)
    out, src, counts, flags = eng.ctx.wet_ground_batch(rows, off, [pr.PLANE4] * len(names), kw["water_height"], kw["pavement_depth"], kw["noise_floor"],
                                                      kw["power_factor"], kw["flat_earth"], kw["delta"], kw["replace"],
                                                      lines=None if lines is None else [list(lines)] * len(names))
    fits = eng.ctx.wet_last_fit(len(names))
    return frames, off, out, src, counts, flags, fits


def _compare(name, pc, ref, ref_src, ref_flag, out, src, count, flag, rtol):
    """-> (failures, largest relative intensity error)"""
    fails = []
    if int(flag) != ref_flag:
        fails.append(f"{name}: flag {int(flag)}, reference {ref_flag}")
    if int(count) != ref.shape[0]:
        return fails + [f"{name}: {int(count)} rows, reference {ref.shape[0]}"], np.nan
    if not np.array_equal(src, ref_src):
        i = int(np.nonzero(src != ref_src)[0][0])
        fails.append(f"{name}: output row {i} comes from input row {src[i]}, reference {ref_src[i]}")
    if not np.array_equal(out[:, [0, 1, 2, 4]], np.asarray(ref, np.float64)[:, [0, 1, 2, 4]]):
        fails.append(f"{name}: coordinates or labels differ")
    a, b = out[:, 3], np.asarray(ref, np.float64)[:, 3]
    if not np.array_equal(a == 0, b == 0):
        fails.append(f"{name}: {int(((a == 0) != (b == 0)).sum())} rows are zero on one side only")
    nz = (b != 0) & (a != 0)
    rel = float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0
    if rel > rtol:
        fails.append(f"{name}: intensities off by a relative {rel:.3e} (rtol {rtol:g})")
    return fails, rel


def _fit_fraction(fit, r, kw):
    ld = pr.estimate_ld(r.g, r.e64, kw["noise_floor"])
    want = (ld.p[0], ld.p[1], ld.pmin[0], ld.pmin[1])
    bound = (ld.b_p[0], ld.b_p[1], ld.b_pmin[0], ld.b_pmin[1])
    got = (fit[1], fit[2], fit[4], fit[5])
    assert fit[0] == 0 and fit[3] == 0 and fit[6] == len(r.g.dist)
    return max(float(abs(pr.L(g) - w) / b) for g, w, b in zip(got, want, bound))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("i", range(len(pr.WET_PARAMS)))
def test_wet_settings_against_the_oracle(eng, so, i, tag):
    """Setting 8 (and 1, 5 on the first parameter set): one ragged batch with an empty frame in the middle per parameter set."""
    kw = pr.WET_PARAMS[i]
    names = ("wet", "empty", "m3", "m4") + (("wet_tiles",) if i == 0 else ())
    frames, off, out, src, counts, flags, fits = _run(eng, names, tag, kw)
    failures, worst_i, worst_fit = [], 0.0, 0.0
    for f, (name, pc) in enumerate(zip(names, frames)):
        r = pr.wet_restated(pc, **kw)                                    # (equal to the oracle bit for bit: the CPU test; asked again here)
        ref, ref_src = so.ground_water_augmentation(pc, plane=(pr.PLANE_W, pr.PLANE_H), return_src=True, **kw)
        assert np.array_equal(np.asarray(ref, np.float64), r.out) and np.array_equal(ref_src, r.src)
        a, n = int(off[f]), int(counts[f])
        fl, rel = _compare(name, pc, ref, ref_src, r.flag, out[a:a + n], src[a:a + n], counts[f], flags[f], 1e-9 if tag == "f64" else 1e-7)
        failures += fl
        worst_i = max(worst_i, rel)
        if r.flag == 0:
            frac = _fit_fraction(fits[f], r, kw)
            worst_fit = max(worst_fit, frac)
            if frac > 1:
                failures.append(f"{name}: fitted lines {fits[f][[1, 2, 4, 5]].tolist()} are {frac:.3g} of their bound from the long-double ones")
    print(f"\n[wet-edges] parameters {i} {tag}: largest relative intensity error {worst_i:.2e}; fitted lines: largest error / bound {worst_fit:.2e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tag", TAGS)
def test_the_1000_row_rule_in_one_batch(eng, so, tag):
    """Setting 9: 999 ground rows come back unchanged with out_flags = 1, 1000 are processed; an empty frame between them."""
    kw = pr.WET_PARAMS[2] | dict(delta=0.5)
    names = ("g999", "empty", "g1000")
    frames, off, out, src, counts, flags, fits = _run(eng, names, tag, kw)
    assert flags.tolist() == [1, 1, 0] and counts[1] == 0
    failures = []
    for f, (name, pc) in enumerate(zip(names, frames)):
        r = pr.wet_restated(pc, **kw)
        a, n = int(off[f]), int(counts[f])
        failures += _compare(name, pc, r.out, r.src, r.flag, out[a:a + n], src[a:a + n], counts[f], flags[f], 1e-9 if tag == "f64" else 1e-7)[0]
    assert counts[0] == frames[0].shape[0] and np.array_equal(out[:int(counts[0])], frames[0].astype(np.float64))    # unchanged: labels too
    assert counts[2] < frames[2].shape[0] and fits[2][6] == 1000 and fits[0][6] == 999
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tag", TAGS)
def test_the_callers_lines_through_every_branch(eng, tag):
    """Setting 10 (lines=: k_wet_apply, k_wet_scan and k_wet_scatter without the fit): rho below 0.05, inside and above 1, rows clipped
    to 0 and to the input intensity, kept and dropped rows, negative thresholds (kept with intensity 0) in one frame; a second frame
    and an empty one beside it.  rtol 1e-9 for both dtypes."""
    names = ("lines", "empty", "wet")
    frames, off, out, src, counts, flags, fits = _run(eng, names, tag, pr.LINES_PARAMS, lines=pr.LINES)
    failures, worst = [], 0.0
    for f, (name, pc) in enumerate(zip(names, frames)):
        r = pr.wet_restated(pc, lines=pr.LINES, **pr.LINES_PARAMS)
        a, n = int(off[f]), int(counts[f])
        fl, rel = _compare(name, pc, r.out, r.src, r.flag, out[a:a + n], src[a:a + n], counts[f], flags[f], 1e-9)
        failures += fl
        worst = max(worst, rel)
        if r.flag == 0:
            assert fits[f][[1, 2, 4, 5]].tolist() == list(pr.LINES)
    print(f"\n[wet-edges] caller's lines {tag}: largest relative intensity error {worst:.2e}")
    assert not failures, "\n".join(failures)
