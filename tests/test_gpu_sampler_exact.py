"""-m gpu: the on-device snowflake sampler (csrc/snowgpu_sampler.hip) row for row against the same-draw restatement of
tests/seeded_reference.py -- a sequential NumPy program that replays the sampler's Philox draws and runs the reference's
dart-throwing process on them.  A wrong accept or reject, or a wrong cut, shifts every later row and fails.
tests/test_seeded_reference.py shows on any machine that each setting decides what it is listed for (overlap rejects, chain
accepts, full conflict lists, the doubling loop, ...), with every decision clear of rounding by a relative 1e-9.

Tolerances (derived, not measured).  The restatement follows k_samp_gen operation for operation (-ffp-contract=off) and
evaluates cos, sin and log1p in np.longdouble, rounded to float64; the device differs from it only through its math library's
cos, sin and log1p.  The ROCm installation carries no document with that library's ULP bounds, so B = 2 ULP each is ASSUMED.
With u = 2^-53:
  x, y   |delta| <= (B + 1) u length                 B ULP of a cosine in [-1, 1] (ULP <= u below 1), one product rounding
         This counts the device's side only.  The restatement's own cosine (long double, rounded to float64: 0.5 u) and its
         product rounding (u) are left out, so device minus restatement can strictly reach (B + 2.5) u length; the bound is
         kept at (B + 1) u length all the same -- the tighter of the two -- and a row beyond it would be a finding.
  r      |delta| <= r u (a + b / q),  a = 2 B + 8, b = 1,  q = 0.25 - (u_h - 0.5)^2
         r = d sqrt(q) with d = -scale log1p(-e) / 1000: the error of d passes to r unamplified -- log1p B ULP <= 2 B u on the
         device and <= u in the reference, one product and one division rounding on either side (4 u): (2 B + 5) u.  Given d,
         A = (d/2)^2 carries one rounding and H = ((u_h - 0.5) d)^2 three (u_h - 0.5 is exact), so S = A - H = d^2 q is off by
         (A + 3 H) u <= d^2 u, relatively u / q; the subtraction and the square root add u and u / 2 + ... : r is off by
         (0.5 / q + 1.5) u per side, (1 / q + 3) u for both.  Together (1 / q + 2 B + 8) u.  q reaches 1e-5 in these tables:
         a flat rtol would be blind or flaky.

Observed on an MI355X (ROCm's OCML), largest |device - restatement| / bound per column (every comparison prints its own
with -s):
  setting    x      y      r      rows bit-equal        setting    x      y      r      rows bit-equal
  s4         0.641  0.615  0.317  0.933                 double     0.642  0.658  0.320  0.918
  s5         0.602  0.600  0.200  0.939                 gunn7      0.648  0.643  0.338  0.926
  d1         0.588  0.608  0.266  0.921                 gunn100    0.622  0.641  0.354  0.923
  d2         0.581  0.619  0.294  0.931                 sekhon7    0.648  0.643  0.314  0.925
  d3         0.610  0.644  0.255  0.924                 filed900   0.579  0.652  0.272  0.932
  d7         0.343  0.433  0.000  0.953                 inv41      0.524  0.502  0.185  0.924
  wide       0.576  0.597  0.270  0.936
Over all settings: x 0.648, y 0.658, r 0.354 of the bound; every row count equals the restatement's.  x and y reach two
thirds of (B + 1) u length, i.e. 2 u length: the device's cosine and sine are off by at most about 1 ULP here, inside the
assumed 2.  Filed table (rho, phi, right and left tangent angle): 0.222, 0.198, 0.198, 0.198 of the bound derived in
test_a_table_filed_in_place_is_the_restated_table.

That the tests bite (each variant of the library built apart from the tree and run once on the same device):
  - k_samp_resolve blocking on ANY earlier valid overlap: s4, d1, d2 and inv41 fail at the first chain accept (s4: row 2892
    is not candidate 2979), the settings without chain accepts pass;
  - sg_sample_table without the `cut >= first overflow` comparison: overflow_cut returns a table (DID NOT RAISE), all else passes;
  - the sampler as it was before the smallest-overflow index: d1, d2, d3, d7 and inv41 raise SNOWGPU_E_TABLE.
"""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded (one HIP runtime per process)

import seeded_reference as sr

pytestmark = pytest.mark.gpu

B_ULP = 2.0                     # assumed bound of the device's cos / sin / log1p in double (see the module docstring)
U = 2.0 ** -53
R_A, R_B = 2 * B_ULP + 8, 1.0


@pytest.fixture(scope="module")
def eng():
    from lidar_snow_sim_amd import engine
    return engine.get_engine(0)


def _restated(name):
    s = sr.sampler_settings()[name]
    return s, sr.dart_throw_restated(s["seed"], s["occupancy"], s["scale_mm"], s["R0"])


def _assert_rows_are_the_restated_darts(name, dev, r):
    """Row k of the device is candidate r.index[k]: equal row counts, every column within its derived bound."""
    n = min(len(dev), len(r.rows))
    bound = np.column_stack(((B_ULP + 1) * U * r.length, (B_ULP + 1) * U * r.length, r.rows[:, 2] * U * (R_A + R_B / r.q)))
    err = np.abs(dev[:n] - r.rows[:n]) / bound[:n]
    worst = err.max(axis=0)
    print(f"\n[sampler-exact] {name}: rows {len(dev)} (restated {len(r.rows)}), cut {r.cut}, rejects {r.rejects}, chain accepts "
          f"{r.chain_accepts}, redrew {r.redrew}; largest error / bound: x {worst[0]:.3f} y {worst[1]:.3f} r {worst[2]:.3f}; "
          f"rows bit-equal {np.mean((dev[:n] == r.rows[:n]).all(axis=1)):.4f}")
    bad = np.nonzero((err > 1.0).any(axis=1))[0]
    assert not bad.size, f"{name}: row {bad[0]} is not candidate {r.index[bad[0]]}: device {dev[bad[0]]}, restated {r.rows[bad[0]]}, error / bound {err[bad[0]]}"
    assert len(dev) == len(r.rows), f"{name}: {len(dev)} rows, the restatement cuts after {len(r.rows)}"


@pytest.mark.parametrize("name", ["s4", "s5", "d1", "d2", "d3", "d7", "inv41", "wide", "double"])
def test_small_dense_tables_equal_the_restatement(eng, name):
    """s4 / s5: overlap rejects, chain accepts (accepted although an earlier, REJECTED dart overlaps), conflict lists filled to
    SG_SAMP_MAXCONF, chains of depth 3.  d1, d2, d3, d7: the same, and a spare candidate far beyond the cut overlaps more than
    SG_SAMP_MAXCONF earlier ones -- by its code the sampler answered these with SNOWGPU_E_TABLE ("occupancy too high") although
    no dart it needed was undecidable (k_samp_overlap raised one flag for any overflowing candidate; observed on an MI355X with
    the earlier sampler: all four, and inv41, raised "a dart overlaps more than 4 earlier darts"); it now refuses only when the overflow lies at or before the cut.  inv41: as d1,
    with a dart over the origin BEFORE the cut -- the valid test (x*x + y*y > r*r) decides emitted rows.  wide: a scale at which the
    20 mm redraw runs.  double: the first n_cand = 1.3 * target / mean_area + 4096 candidates fall short (the mean area of the
    TRUNCATED exponential is a fifth of the untruncated one's), so the entry's doubling loop runs."""
    s, r = _restated(name)
    dev = eng.ctx.sample_table(-1, s["occupancy"], s["scale_mm"], s["R0"], s["seed"])
    _assert_rows_are_the_restated_darts(name, dev, r)


@pytest.mark.parametrize("name", ["gunn7", "gunn100", "sekhon7"])
def test_full_size_tables_equal_the_restatement(eng, name):
    """R0 = 80 m at 2.5 mm/h @ 1.6 m/s through dart_throwing_device: the statistical 3 % of test_gpu_sampler.py as an exact
    row count, for both scale laws."""
    from lidar_snow_sim_amd.tools.snowfall import sampling as smp
    s, r = _restated(name)
    dev = smp.dart_throwing_device(s["occupancy"], s["floors"]["rate"], s["R0"], seed=s["seed"], distribution=s["floors"]["distribution"])
    _assert_rows_are_the_restated_darts(name, dev, r)


def test_a_table_filed_in_place_is_the_restated_table(eng):
    """file_table=True: the sampler's output is derived, binned and sorted where it lies.  The per-flake quantities read back
    through the debug tap (rho, phi, the two tangent angles phi -+ alpha, alpha = asin(r / rho)) equal those of the same rows
    filed by the host (snowgpu_upload_table) within the tolerance of
    test_filed_per_flake_quantities_match_the_reference_geometry (1 ULP, and that in under 0.5 % of the values).  Against the
    host filing of the RESTATED rows the same holds wherever the device's row is the restated row bit for bit; on every other
    row the inputs differ by at most the bounds bx = by and br of the module docstring, which the geometry passes on as
      |d rho| <= sqrt(2) bx,  |d phi| <= sqrt(2) bx / rho,  |d alpha| <= (br + (r / rho) sqrt(2) bx) / sqrt(rho^2 - r^2)
    (first order; doubled below for the higher orders, which are ~1e-16 of it), plus 4 ULP of the value for the two filings' own
    arithmetic (the 1 ULP asserted above, on either side, twice for the sum phi -+ alpha)."""
    s, r = _restated("filed900")
    tid, t_dev_rows, t_restated = eng.user_table_id(), eng.user_table_id(), eng.user_table_id()
    rows = eng.ctx.sample_table(tid, s["occupancy"], s["scale_mm"], s["R0"], s["seed"])
    _assert_rows_are_the_restated_darts("filed900", rows, r)
    k = len(rows)
    eng.ctx.upload_table(t_dev_rows, rows)
    eng.ctx.upload_table(t_restated, r.rows)
    q, q_rows, q_rest = (eng.ctx.debug_table(t, k) for t in (tid, t_dev_rows, t_restated))
    np.testing.assert_allclose(q, q_rows, rtol=2.3e-16, atol=0)
    assert (q != q_rows).mean() < 0.005
    same = (rows == r.rows).all(axis=1)
    np.testing.assert_allclose(q[same], q_rest[same], rtol=2.3e-16, atol=0)
    assert (q[same] != q_rest[same]).mean() < 0.005
    bx = (B_ULP + 1) * U * r.length
    br = r.rows[:, 2] * U * (R_A + R_B / r.q)
    rho, rad = np.hypot(r.rows[:, 0], r.rows[:, 1]), r.rows[:, 2]
    d_phi = np.sqrt(2.0) * bx / rho
    d_alpha = (br + (rad / rho) * np.sqrt(2.0) * bx) / np.sqrt(rho * rho - rad * rad)
    first = np.column_stack((np.sqrt(2.0) * bx, d_phi, d_phi + d_alpha, d_phi + d_alpha))
    bound = 2.0 * first + 4.0 * np.spacing(np.abs(q_rest))
    err = np.abs(q - q_rest) / bound
    print(f"\n[sampler-exact] filed: {k} rows, {same.mean():.4f} bit-equal to the restatement; largest error / bound per quantity "
          f"{err.max(axis=0).round(3).tolist()}")
    assert (err <= 1.0).all(), (np.argwhere(err > 1.0)[:4].tolist(), float(err.max()))


@pytest.mark.parametrize("name", ["overflow", "overflow_cut"])
def test_an_overflow_the_process_needs_is_still_refused(eng, name):
    """A dart AT OR BEFORE the cut with more than SG_SAMP_MAXCONF earlier overlapping valid darts cannot be decided with the
    conflict lists the sampler keeps: the entry keeps returning SNOWGPU_E_TABLE ("occupancy too high") -- an error return.
    overflow: the entry's first n_cand candidates do not reach the target, so the host sees an overflow and no cut.
    overflow_cut: they do, and the cut the device finds lies beyond the first overflow -- a table it could emit, and must not."""
    from lidar_snow_sim_amd import _native
    s, r = _restated(name)
    assert r.max_conf > sr.SG_SAMP_MAXCONF and r.first_overflow <= r.cut
    assert (r.cut < r.n_cand_entry) == s["floors"]["cut_in_first_attempt"]
    with pytest.raises(_native.SnowGPUError) as e:
        eng.ctx.sample_table(-1, s["occupancy"], s["scale_mm"], s["R0"], s["seed"])
    assert e.value.code == _native.E_TABLE and "occupancy too high" in str(e.value)
    # the context is usable afterwards
    s5, r5 = _restated("s5")
    assert len(eng.ctx.sample_table(-1, s5["occupancy"], s5["scale_mm"], s5["R0"], s5["seed"])) == len(r5.rows)
