"""Table filing without a GPU: the inputs of tests/test_gpu_table_filing.py are what they are taken for, and the product's HOST filing
(csrc/sg_table_host.h: sg_file_table_host, with the range index of csrc/sg_range_index.h as k_table_index files it), compiled into
tests/host_harness/table_filing.cpp, equals the NumPy restatement of tests/table_filing_inputs.py exactly: bin offsets, the (rho, row)
order and the first-bin flag of every record, the longest bin, both range indexes word for word, and rho bit for bit.

Why "exactly".  The only rounding that could move a flake into another bin is that of lo = phi - alpha - margin and hi = phi + alpha +
margin (a few ulps of 2 pi, about 4e-15 rad) and of the libraries' atan2 / asin (1 ulp).  The inputs hold no flake whose lo or hi lies
within the guard band of 1e-12 rad of a bin edge -- asserted below on the restatement alone, together with the agreement of float64 and
np.longdouble on every bin decision -- so no comparison here or in the GPU test carries a tolerance for the structure.  phi, t0 and t1
are held to the reference by the golden tests (tests/test_gpu_sampler.py, tests/test_kernel_math.py) and are not redone here."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import table_filing_inputs as tfi
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---- the inputs ----------------------------------------------------------------------------------------------------
def _all_valid_tables():
    return dict(tfi.tables(), longbin_host=tfi.longbin_host(), too_close=tfi.too_close())


def test_no_flake_lies_in_the_guard_band_and_longdouble_decides_the_same_bins():
    smallest = {}
    for name, t in _all_valid_tables().items():
        assert t.dtype == np.float64 and t.ndim == 2 and t.shape[1] == 3 and tfi.valid_rows(t).all(), name
        if not len(t):
            continue
        assert tfi.guard_rows(t).size == 0, (name, tfi.guard_rows(t)[:5])
        f64, fld = tfi.interval_bins(t), tfi.interval_bins(t, np.longdouble)
        for key in ("first", "last", "span"):
            assert np.array_equal(f64[key], fld[key]), (name, key)
        smallest[name] = float(min(f64["d_lo"].min(), f64["d_hi"].min()))
    print("\n[table-filing] smallest distance of lo / hi to a bin edge, rad:", {k: f"{v:.3g}" for k, v in smallest.items()})
    assert min(smallest.values()) > 100 * tfi.GUARD                   # nowhere near the band: 1 ulp of phi or OCML's asin cannot reach it
    assert abs(smallest["edges"] - tfi.EDGE_DELTA) < 1e-14            # the intended 1e-9, give or take the arithmetic's 4e-15


def test_inputs_are_what_they_are_taken_for():
    t = tfi.tables()
    assert tuple(t) == tfi.DEVICE_CASES
    assert len(t["random"]) == 3001 and 3001 % 256 != 0
    f = tfi.interval_bins(t["random"])
    assert f["span"].min() == 1 and f["span"].max() == 6 and (np.bincount(tfi.restate(t["random"])["bin"], minlength=2048) == 0).mean() > 0.1
    assert [len(t[f"sizes{k}"]) for k in (0, 1, 255, 256, 257)] == [0, 1, 255, 256, 257]
    assert all(np.array_equal(t[f"sizes{k}"], t["random"][:k]) for k in (0, 1, 255, 256, 257))

    # seam: lo < 0 and hi > 2 pi both occur; spans wrap from bin 2047 to bin 0 (first bin on the high side); y = +0.0 and -0.0
    f = tfi.interval_bins(t["seam"])
    wraps = f["last"] < f["first"]
    assert wraps.sum() >= 5 and ((f["first"][wraps] == 2047) & (f["last"][wraps] == 0)).all()
    assert ((f["phi"] < 1e-3) & wraps).any() and ((f["phi"] > 6.0) & wraps).any()      # lo < 0 of a flake beyond the seam, hi > 2 pi of one before it
    ys = t["seam"][:, 1]
    assert (ys == 0).sum() >= 2 and np.signbit(ys[ys == 0]).any() and not np.signbit(ys[ys == 0]).all()

    # edges: for every edge j both outcomes of lo (first bin j - 1 or j) and of hi (last bin j - 1 or j); some spans wrap
    f = tfi.interval_bins(t["edges"])
    first, last = f["first"].reshape(5, 2, 2), f["last"].reshape(5, 2, 2)              # (edge, lo / hi, below / above)
    for i, j in enumerate(tfi.EDGE_BINS):
        assert first[i, 0].tolist() == [(j - 1) % 2048, j] and last[i, 1].tolist() == [(j - 1) % 2048, j], j
    assert (f["last"] < f["first"]).any()

    r = tfi.restate(t["long"])
    assert r["max_bin"] == 1700 >= 1500 and (r["span"] == 1).all() and (np.diff(r["bin_start"]) > 0).sum() == 1
    assert (t["long"][1500:] == t["long"][0]).all()                                    # 200 equal rows: ordered by src alone, beyond one wave
    r = tfi.restate(t["wide"])
    assert r["span"].max() == 1024 and ((r["last"] < r["first"]).sum() >= 2) and 4000 < r["n_entries"] <= tfi.entry_limit(5)
    np.testing.assert_allclose(t["wide"][:, 2] / np.hypot(t["wide"][:, 0], t["wide"][:, 1]), [0.5, 0.9, 0.99, 0.999, 0.999999], rtol=1e-12)

    # ties: bit-equal rho of different rows that share a bin, so that the order inside the bin is the rows'
    r = tfi.restate(t["ties"])
    rho = r["rho"][r["src"]]
    tied = (r["bin"][1:] == r["bin"][:-1]) & (rho[1:] == rho[:-1])
    assert tied.sum() >= 12 and (r["src"][1:][tied] > r["src"][:-1][tied]).all()
    tt = t["ties"]
    assert any((tt[i, 0] == tt[j, 0]) and (tt[i, 1] == -tt[j, 1]) and tt[i, 1] != 0 for i in range(len(tt)) for j in range(i))
    assert any((tt[i, 0] == tt[j, 1]) and (tt[i, 1] == tt[j, 0]) and tt[i, 0] != tt[i, 1] for i in range(len(tt)) for j in range(i))

    tg = t["tangent"]
    assert (np.abs(tg[:, 0]) - tg[:, 2] == 0).all() and len(tg) == 3                   # the vertical-tangent branch of derive_flake

    r = tfi.restate(tfi.longbin_host())
    assert r["n_flakes"] == 66000 and r["max_bin"] == 66000 > tfi.QS_MAX_BIN and r["bin_qs"] is None


def test_refusal_inputs_exceed_what_they_are_meant_to():
    t = tfi.too_close()
    assert len(t) == 120 and int(tfi.interval_bins(t)["span"].sum()) > 5 * tfi.entry_limit(120)
    for name, t in _all_valid_tables().items():
        if name != "too_close":
            assert int(tfi.interval_bins(t)["span"].sum()) <= tfi.entry_limit(len(t)) if len(t) else True, name
    bad = tfi.bad_rows()
    assert tuple(bad) == tfi.BAD_KINDS + ("together",)
    for kind in tfi.BAD_KINDS:
        t, row = bad[kind]
        assert len(t) == 3001 and row == tfi.BAD_SINGLE_ROW and np.nonzero(~tfi.valid_rows(t))[0].tolist() == [row], kind
        keep = np.arange(3001) != row
        assert np.array_equal(t[keep], tfi.tables()["random"][keep])
    t, row = bad["together"]
    assert len(t) == 6000 and row == 300 and np.nonzero(~tfi.valid_rows(t))[0].tolist() == [300, 700, 5000]
    assert len({r // 256 for r in tfi.BAD_TOGETHER}) == 3 and tfi.BAD_TOGETHER[0] != min(tfi.BAD_TOGETHER)     # three blocks; not in row order


def test_restated_index_words_follow_the_documented_layout():
    """The restatement's bin_qs on a table small enough to count by hand."""
    t = np.array([[1.0, 0.0005, 1e-4], [3.0, 0.0015, 1e-4], [3.5, 0.001, 1e-4], [200.0, 0.5, 1e-4]])      # bin 0 at 1 m, 3 m, 3.5 m; bin 0 at 200 m
    r = tfi.restate(t)
    assert r["bin_start"][1] == 4 and r["src"].tolist() == [0, 1, 2, 3]
    assert r["bin_q"][0].tolist() == [0] + [3] * 15
    qs = r["bin_qs"]
    assert qs.shape == (64, 2049) and [int(qs[s, 0]) for s in (0, 1, 2, 63)] == [0 | 1 << 16, 1 | 3 << 16, 3 | 3 << 16, 3 | 4 << 16]
    assert np.array_equal(qs[:, 2048], qs[:, 0]) and not qs[:, 1:2048].any()


# ---- the host filing against the restatement -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("table_filing")
    exe = tmp / "table_filing"
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17", "-ffp-contract=off", "-w",
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"),
           str(ROOT / "tests" / "host_harness" / "table_filing.cpp"), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(name, table):
        fin, fout = tmp / f"{name}.in", tmp / f"{name}.out"
        t = np.ascontiguousarray(table, np.float64)
        with open(fin, "wb") as f:
            f.write(np.int64(t.shape[0]).tobytes())
            f.write(t.tobytes())
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        raw = fout.read_bytes()
        head = np.frombuffer(raw, np.dtype([("rc", "<i4"), ("bad", "<i8"), ("max_bin", "<u4"), ("n_entries", "<u4"), ("has_qs", "<i4")]), 1)[0]
        out = {k: int(head[k]) for k in head.dtype.names}
        pos = 24
        if out["rc"] == 0:
            n = out["n_entries"]
            for key, dt, count in (("bin_start", "<u4", tfi.NBINS + 1), ("src", "<u4", n), ("flags", "<u4", n), ("rho", "<f8", n),
                                   ("spare_zero", "<i4", 1), ("bin_q", "<u4", tfi.NBINS * tfi.QSTEPS),
                                   ("bin_qs", "<u4", tfi.QS_STEPS * (tfi.NBINS + 1) if out["has_qs"] else 0)):
                out[key] = np.frombuffer(raw, dt, count, pos)
                pos += count * np.dtype(dt).itemsize
        assert pos == len(raw)
        return out
    return run


@pytest.mark.parametrize("name", tfi.DEVICE_CASES + ("longbin_host",))
def test_host_filing_equals_the_restatement(harness, name):
    table = tfi.longbin_host() if name == "longbin_host" else tfi.tables()[name]
    got, want = harness(name, table), tfi.restate(table)
    assert got["rc"] == 0 and got["bad"] == -1 and got["spare_zero"] == 1
    assert got["has_qs"] == (want["bin_qs"] is not None) == (name != "longbin_host")
    tfi.assert_structure_is_the_restatement(got, want, name)
    assert got["rho"].tobytes() == want["rho"][want["src"]].astype(np.float64).tobytes()         # IEEE products, sum and square root


def test_host_filing_refuses_bad_rows_and_crowded_tables(harness):
    got = harness("too_close", tfi.too_close())
    assert (got["rc"], got["bad"]) == (2, -1)
    for name, (table, row) in tfi.bad_rows().items():
        got = harness(f"bad_{name}", table)
        assert (got["rc"], got["bad"]) == (1, row), name
