"""Inputs of tests/test_table_filing.py and tests/test_gpu_table_filing.py, made on any machine (NumPy only): named snowflake tables
(K x 3 float64: x, y, disk radius; fixed seeds) that lean on every branch of table filing, and the restatement of filing by its
definition (csrc/sg_table_host.h, csrc/snowgpu_tables.hip, csrc/sg_range_index.h):

  rho = sqrt(x^2 + y^2), phi = arctan2(y, x) folded to [0, 2 pi), alpha = arcsin(min(1, r / rho));
  the flake is filed under every azimuth bin of [phi - alpha - SG_BIN_MARGIN, phi + alpha + SG_BIN_MARGIN]: first and last bin are
  floor(fmod(theta, 2 pi) * 2048 / (2 pi)) after adding 2 pi to a negative remainder, clamped to [0, 2047]; the span is circular;
  every bin is ordered by (rho, table row); flags bit 0 marks the copy in the flake's first bin;
  bin_q[b][k] = records of bin b nearer than 8 k metres (16 steps); bin_qs[k][b] = that count for steps of 2 m (64 steps) in the low 16
  bits and the count of the next step -- for the last step the bin's length -- in the high 16 bits, a row being 2048 + 1 words of
  which the last repeats bin 0; no bin_qs when a bin holds more than 65 535 records.

Guard band.  lo and hi carry a few ulps of 2 pi, about 4e-15 rad, from phi -+ alpha -+ margin and the bin arithmetic; the two filings'
phi may differ by 1 ulp (glibc's atan2 against the device's correctly rounded one) and asin is OCML's on the device.  A flake whose lo
or hi lies within GUARD = 1e-12 rad of a bin edge is therefore undetermined.  That is a condition on the inputs, not a tolerance: no
table here holds such a flake (tests/test_table_filing.py asserts it on the restatement alone, and that the same decisions taken in
np.longdouble are the float64 ones), so every comparison of structure is exact."""
from functools import lru_cache

import numpy as np

NBINS = 2048
BIN_MARGIN = 1e-6
TWO_PI = 2 * 3.141592653589793            # SG_TWO_PI
BIN_W = TWO_PI / NBINS
QSTEPS, QSTEP_M = 16, 8.0                 # bin_q (SG_QSTEPS, SG_QSTEP_M)
QS_STEPS, QS_STEP_M = 64, 2.0             # bin_qs as the library files it (SG_QS_FILE_STEPS, SG_QS_FILE_STEP_M)
QS_MAX_BIN = 65535
GUARD = 1e-12                             # rad
EDGE_BINS = (0, 1, 512, 1024, 2047)
EDGE_DELTA = 1e-9                         # rad: far above the arithmetic noise (4e-15), far below the margin (1e-6)

ENTRY_DTYPE = np.dtype([("phi", "f8"), ("x", "f8"), ("y", "f8"), ("r", "f8"), ("t0", "f8"), ("t1", "f8"), ("rho", "f8"),
                        ("flags", "u4"), ("src", "u4")])           # SgEntry (csrc/sg_common.h), 64 bytes


def entry_limit(k):
    """records beyond which a table is refused: flakes so close to the sensor that they cover most azimuths"""
    return 64 * max(int(k), 1) + 4096


# ---- the restatement -----------------------------------------------------------------------------------------------
def _bin_of(theta, ft):
    two_pi, inv_w = ft(TWO_PI), ft(NBINS) / ft(TWO_PI)
    t = np.fmod(theta, two_pi)
    t = np.where(t < 0, t + two_pi, t)
    s = t * inv_w
    b = np.clip(np.floor(s), 0, NBINS - 1).astype(np.int64)
    dist = np.abs(s - np.rint(s)) / inv_w                # to the nearest bin edge (0 and 2 pi are edges too), rad
    return b, dist.astype(np.float64)


def interval_bins(xyr, ft=np.float64):
    """Per flake: rho, phi, first bin, last bin, span (circular, 1 .. 2048), and the distances of lo and hi to the nearest bin edge,
    all computed in the float type ft."""
    t = np.asarray(xyr, np.float64).reshape(-1, 3).astype(ft)
    x, y, r = t[:, 0], t[:, 1], t[:, 2]
    rho = np.sqrt(x * x + y * y)
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0, phi + ft(TWO_PI), phi)
    alpha = np.arcsin(np.minimum(ft(1.0), r / rho))
    lo, hi = phi - alpha - ft(BIN_MARGIN), phi + alpha + ft(BIN_MARGIN)
    # alpha <= pi / 2: the interval never reaches the whole circle less two bins, from where on the filings put a flake into every bin
    assert not (hi - lo >= ft(TWO_PI) - 2 * ft(BIN_W)).any()
    first, d_lo = _bin_of(lo, ft)
    last, d_hi = _bin_of(hi, ft)
    span = np.mod(last - first, NBINS) + 1
    return dict(rho=rho, phi=phi, first=first, last=last, span=span, d_lo=d_lo, d_hi=d_hi)


def valid_rows(xyr):
    """rows that are disks clear of the origin (finite, r > 0, rho > r)"""
    t = np.asarray(xyr, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        rho = np.sqrt(t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1])
        return np.isfinite(t).all(axis=1) & (t[:, 2] > 0) & (rho > t[:, 2])


def restate(xyr):
    """The filed table of K valid rows by its definition: dict of rho, phi, first, last, span, d_lo, d_hi (per flake), n_flakes,
    n_entries, bin_start (2049), bin (per record), src, flags (per record, bins concatenated, each ordered by (rho, src)), max_bin,
    bin_q (2048 x 16), bin_qs (64 x 2049, or None)."""
    t = np.asarray(xyr, np.float64).reshape(-1, 3)
    k = t.shape[0]
    f = interval_bins(t)
    src = np.repeat(np.arange(k, dtype=np.int64), f["span"])
    step = np.arange(src.size, dtype=np.int64) - np.repeat(np.cumsum(f["span"]) - f["span"], f["span"])      # 0 .. span - 1 per flake
    b = np.mod(f["first"][src] + step, NBINS)
    rho = f["rho"].astype(np.float64)[src]
    order = np.lexsort((src, rho, b))                    # by bin, then range, then table row
    b, src, step, rho = b[order], src[order], step[order], rho[order]
    count = np.bincount(b, minlength=NBINS)
    bin_start = np.concatenate(([0], np.cumsum(count))).astype(np.uint32)
    out = dict(f, n_flakes=k, n_entries=int(src.size), bin_start=bin_start, bin=b, src=src.astype(np.uint32),
               flags=(step == 0).astype(np.uint32), max_bin=int(count.max()))
    out["bin_q"] = np.stack([np.bincount(b[rho < QSTEP_M * s], minlength=NBINS) for s in range(QSTEPS)], axis=1).astype(np.uint32)
    if out["max_bin"] <= QS_MAX_BIN:
        below = [np.bincount(b[rho < QS_STEP_M * s], minlength=NBINS) for s in range(QS_STEPS)] + [count]      # the last upper count: the bin
        qs = np.zeros((QS_STEPS, NBINS + 1), np.uint32)
        for s in range(QS_STEPS):
            qs[s, :NBINS] = below[s].astype(np.uint32) | (below[s + 1].astype(np.uint32) << np.uint32(16))
            qs[s, NBINS] = qs[s, 0]                      # bin 0 again: the bin after the last needs no wrap-around test
        out["bin_qs"] = qs
    else:
        out["bin_qs"] = None
    return out


def assert_structure_is_the_restatement(got, want, what):
    """bin offsets, per-record src and flags, the longest bin and both indexes of a filed table (dict of arrays) against restate()"""
    assert got["n_entries"] == want["n_entries"] and got["max_bin"] == want["max_bin"], what
    assert np.array_equal(got["bin_start"], want["bin_start"]), what
    assert np.array_equal(got["src"], want["src"]), (what, "order inside the bins")
    assert np.array_equal(got["flags"], want["flags"]), (what, "first-bin flags")
    assert np.array_equal(np.asarray(got["bin_q"]).reshape(NBINS, QSTEPS), want["bin_q"]), (what, "bin_q")
    if want["bin_qs"] is None:
        assert got["bin_qs"] is None or np.asarray(got["bin_qs"]).size == 0, (what, "a bin_qs where none is filed")
    else:
        assert got["bin_qs"] is not None and np.array_equal(np.asarray(got["bin_qs"]).reshape(QS_STEPS, NBINS + 1), want["bin_qs"]), (what, "bin_qs")


def guard_rows(xyr):
    """rows whose lo or hi lies within GUARD of a bin edge: their first or last bin is undetermined"""
    f = interval_bins(xyr)
    return np.nonzero((f["d_lo"] <= GUARD) | (f["d_hi"] <= GUARD))[0]


# ---- the tables ----------------------------------------------------------------------------------------------------
def _polar(rho, phi, r):
    rho, phi, r = np.broadcast_arrays(np.asarray(rho, np.float64), np.asarray(phi, np.float64), np.asarray(r, np.float64))
    return np.ascontiguousarray(np.column_stack((rho * np.cos(phi), rho * np.sin(phi), r)))


@lru_cache(maxsize=None)
def _random6000():
    rng = np.random.default_rng(9101)
    return _polar(rng.uniform(0.5, 80.0, 6000), rng.uniform(0.0, TWO_PI, 6000), rng.uniform(0.5e-3, 5e-3, 6000))


def _seam():
    phi = np.linspace(-3 * BIN_W, 3 * BIN_W, 41)
    t = _polar(7.0, phi, 4e-3)
    extra = np.array([[7.0, 0.0, 4e-3], [7.0, -0.0, 4e-3], [7.0 * np.cos(1e-12), 7.0 * np.sin(1e-12), 4e-3],
                      [7.0 * np.cos(-1e-12), 7.0 * np.sin(-1e-12), 4e-3]])
    return np.ascontiguousarray(np.vstack((t, extra)))


def _edges():
    """lo (kind 0) or hi (kind 1) of a flake EDGE_DELTA below or above the bin edge j: filed one bin wider or not by the margin and the
    floor alone.  Rows in the order (j, kind, side)."""
    rho, r = 11.0, 3e-3
    alpha = np.arcsin(r / rho)
    phi = [j * BIN_W + side * EDGE_DELTA + (alpha + BIN_MARGIN if kind == 0 else -(alpha + BIN_MARGIN))
           for j in EDGE_BINS for kind in (0, 1) for side in (-1.0, 1.0)]
    return _polar(rho, np.mod(np.array(phi), TWO_PI), r)


def _wide():
    ratio = np.array([0.5, 0.9, 0.99, 0.999, 0.999999])
    rho = np.array([2.0, 0.5, 1.0, 0.25, 0.125])
    phi = np.array([0.1, 2.0, TWO_PI - 0.3, 4.0, 5.0002])           # the first, third and fifth straddle the seam
    return _polar(rho, phi, ratio * rho)


def _one_bin(n, seed, b=700):
    rng = np.random.default_rng(seed)
    return _polar(rng.uniform(1.0, 60.0, n), (b + 0.5) * BIN_W + rng.uniform(-1e-4, 1e-4, n), 1e-3)


def _long():
    t = _one_bin(1500, 9102)
    return np.ascontiguousarray(np.vstack((t, np.repeat(t[:1], 200, axis=0))))


def _ties():
    rng = np.random.default_rng(9103)
    rows = []
    for x, y, r in ((5.0, 1e-3, 0.02), (9.0, 2e-3, 0.03), (23.5, 1.5e-3, 0.05)):     # mirror pairs next to the seam: equal rho
        rows += [[x, y, r], [x, -y, r]]
    for x, y, r in ((3.0, 3.002, 0.01), (-6.0, -6.003, 0.02), (12.0, -12.004, 0.04)):  # swapped pairs: equal rho, shared bins
        rows += [[x, y, r], [y, x, r]]
    dup = _polar(rng.uniform(2.0, 30.0, 4), rng.uniform(0.0, TWO_PI, 4), 4e-3)
    rows += np.repeat(dup, 3, axis=0).tolist()                                         # exact duplicates
    rows += _polar(rng.uniform(2.0, 30.0, 12), rng.uniform(-0.004, 0.004, 12), 5e-3).tolist()   # company in the pairs' bins
    t = np.array(rows, np.float64)
    return np.ascontiguousarray(t[rng.permutation(len(t))])


def _tangent():
    r = 4e-3
    return np.array([[r, 10.0, r], [-r, -10.0, r], [r, -3.0, r]], np.float64)


@lru_cache(maxsize=None)
def tables():
    """name -> K x 3 float64, the cases both filings run (read-only arrays)"""
    rnd = _random6000()[:3001]
    t = {"random": rnd, "seam": _seam(), "edges": _edges(), "wide": _wide(), "long": _long(), "ties": _ties(), "tangent": _tangent()}
    for k in (0, 1, 255, 256, 257):
        t[f"sizes{k}"] = rnd[:k]
    for v in t.values():
        v.setflags(write=False)
    return t


DEVICE_CASES = ("random", "seam", "edges", "wide", "long", "ties", "tangent", "sizes0", "sizes1", "sizes255", "sizes256", "sizes257")


@lru_cache(maxsize=None)
def longbin_host():
    """66 000 flakes in one bin: filed by the host only (k_file_sort's rank sort is quadratic in a bin's length)"""
    t = _one_bin(66000, 9104, b=1300)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=None)
def too_close():
    """120 flakes with r / rho = 0.99: more than 900 bins each, far more than 64 K + 4096 records"""
    rng = np.random.default_rng(9105)
    rho = rng.uniform(0.05, 0.5, 120)
    return _polar(rho, rng.uniform(0.0, TWO_PI, 120), 0.99 * rho)


BAD_KINDS = ("nan_x", "nan_r", "inf_y", "inf_r", "r_zero", "r_negative", "rho_equals_r", "rho_below_r", "origin")
BAD_SINGLE_ROW = 1234
BAD_TOGETHER = (5000, 300, 700)          # rows of the 6000-row table: three different 256-thread blocks, the smallest is reported


def _bad_row(kind, row):
    x, y, r = row
    return {"nan_x": [np.nan, y, r], "nan_r": [x, y, np.nan], "inf_y": [x, np.inf, r], "inf_r": [x, y, np.inf], "r_zero": [x, y, 0.0],
            "r_negative": [x, y, -r], "rho_equals_r": [3.0, 4.0, 5.0], "rho_below_r": [3.0, 4.0, 5.5], "origin": [0.0, 0.0, 1e-3]}[kind]


@lru_cache(maxsize=None)
def bad_rows():
    """name -> (table, first bad row): `random` with one bad row of each kind, and the 6000-row table with three"""
    out = {}
    for kind in BAD_KINDS:
        t = _random6000()[:3001].copy()
        t[BAD_SINGLE_ROW] = _bad_row(kind, t[BAD_SINGLE_ROW])
        out[kind] = (t, BAD_SINGLE_ROW)
    t = _random6000().copy()
    for row, kind in zip(BAD_TOGETHER, ("nan_x", "r_zero", "rho_below_r")):
        t[row] = _bad_row(kind, t[row])
    out["together"] = (t, min(BAD_TOGETHER))
    return out
