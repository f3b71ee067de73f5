"""-m gpu: the DEVICE filing of a snowflake table (csrc/snowgpu_tables.hip: k_file_derive, k_file_scan, k_file_scatter, k_file_sort,
k_table_index) against the host filing (csrc/sg_table_host.h) and the NumPy restatement of tests/table_filing_inputs.py, read back
whole through snowgpu_debug_table_bins: bin offsets, every copy of every flake in every bin, the order inside the bins, the first-bin
flag, the longest bin, the spare record, and both range indexes word for word.  tests/test_table_filing.py holds the host filing to
the same restatement on any machine and shows that the inputs reach the branches they are listed for.

Exact, and why.  Which bins a flake is filed under depends on lo = phi - alpha - margin and hi = phi + alpha + margin.  These carry a
few ulps of 2 pi (about 4e-15 rad) from the sums and the bin arithmetic; the two filings' phi may differ by 1 ulp (glibc's atan2
against the device's correctly rounded one, csrc/sg_atan_cr.h) and asin is OCML's on the device.  A flake whose lo or hi lies within
the GUARD BAND of 1e-12 rad of a bin edge is therefore undetermined -- and the named inputs hold no such flake (asserted without a GPU),
so the structure is compared exactly, with no tolerance.  x, y, r and rho are bit-equal between the filings (no fast-math; products,
sums and square roots are IEEE); phi, t0 and t1 are within 1 ulp, rtol = 2.3e-16: correctly rounded atan2 / atan on the device against
glibc's, which are off by up to 0.506 ulp -- the bound of test_filed_per_flake_quantities_match_the_reference_geometry
(tests/test_gpu_sampler.py), here without its 0.5 % share, which a 20-row case cannot express.

Only the rows of a SAMPLED table cannot be chosen away from the bin edges; test_a_sampled_table_filed_in_place counts those inside the
guard band and lets their first or last bin, and nothing else, differ by one."""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded (one HIP runtime per process)

import table_filing_inputs as tfi

pytestmark = pytest.mark.gpu

ULP_RTOL = 2.3e-16


@pytest.fixture(scope="module")
def eng():
    from lidar_snow_sim_amd import engine
    return engine.get_engine(0)


def _file_host(eng, tid, table):
    eng.ctx.upload_table(tid, table)


def _file_device(eng, tid, table):
    d = torch.from_numpy(np.ascontiguousarray(table, np.float64).copy()).to("cuda:0")
    eng.ctx.file_table_device(tid, d.data_ptr(), int(table.shape[0]))


FILINGS = {"host": _file_host, "device": _file_device}


def _tap(eng, tid):
    """the tap's dict with the records split: src, flags, bin of every record, and the spare record apart"""
    t = eng.ctx.debug_table_bins(tid)
    n = t["n_entries"]
    assert t["entries"].shape == (n + 1,) and t["entries"].dtype.itemsize == 64 and t["bin_start"].shape == (tfi.NBINS + 1,)
    assert t["bin_start"][0] == 0 and t["bin_start"][-1] == n and (np.diff(t["bin_start"].astype(np.int64)) >= 0).all()
    t["spare"], t["entries"] = t["entries"][n:], t["entries"][:n]
    t["src"], t["flags"] = t["entries"]["src"], t["entries"]["flags"]
    t["bin"] = np.repeat(np.arange(tfi.NBINS), np.diff(t["bin_start"].astype(np.int64)))
    return t


_filed = {}


def _both(eng, name):
    """the case `name` filed by the host and by the device on one engine, both read back through the tap (once per module)"""
    if name not in _filed:
        table = tfi.tables()[name]
        out = {}
        for how, file in FILINGS.items():
            tid = eng.user_table_id()
            try:
                file(eng, tid, table)
                out[how] = _tap(eng, tid)
            finally:
                eng.ctx.free_table(tid)
        _filed[name] = out
    return _filed[name]


def _assert_records(dev, host, rest, guard=()):
    """Items 2 and 3 of the module docstring: the device-filed table `dev` against the host-filed `host` of the same rows, `rest` their
    restatement.  Rows in `guard` (inside the guard band) may lie in a first or last bin that differs by one; everything else is exact."""
    guard = np.asarray(guard, np.int64)
    assert dev["n_flakes"] == host["n_flakes"] == rest["n_flakes"]
    assert dev["spare"].tobytes() == bytes(64) and host["spare"].tobytes() == bytes(64)       # the scan prefetches record e + 1
    if not guard.size:
        assert dev["n_entries"] == host["n_entries"] and dev["max_bin"] == host["max_bin"]
        assert np.array_equal(dev["bin_start"], host["bin_start"])
    kd, kh = ~np.isin(dev["src"], guard), ~np.isin(host["src"], guard)
    for key in ("bin", "src", "flags"):                                                     # the same records in the same order in every bin
        assert np.array_equal(dev[key][kd], host[key][kh]), key
    for g in guard:                                                                            # a guard row: first / last bin within one
        bd, bh = dev["bin"][dev["src"] == g], host["bin"][host["src"] == g]
        fd, fh = dev["bin"][(dev["src"] == g) & (dev["flags"] & 1 == 1)], host["bin"][(host["src"] == g) & (host["flags"] & 1 == 1)]
        assert fd.size == fh.size == 1 and abs(int(bd.size) - int(bh.size)) <= 2
        assert min((int(fd[0]) - int(fh[0])) % tfi.NBINS, (int(fh[0]) - int(fd[0])) % tfi.NBINS) <= 1
        assert len(set(bd.tolist()) ^ set(bh.tolist())) <= 2
    ed, eh = dev["entries"][kd], host["entries"][kh]
    for key in ("x", "y", "r", "rho"):
        assert ed[key].tobytes() == eh[key].tobytes(), key
    for key in ("phi", "t0", "t1"):
        np.testing.assert_allclose(ed[key], eh[key], rtol=ULP_RTOL, atol=0, err_msg=key)
    # every copy of a flake, across its bins, is the same record apart from flags; one copy carries bit 0, in the restated first bin
    for t in (dev, host):
        e = t["entries"].copy()
        e["flags"] = 0
        raw = np.ascontiguousarray(e).view(np.uint64).reshape(-1, 8)
        order = np.argsort(t["src"], kind="stable")
        s, raw_s = t["src"][order], raw[order]
        same_flake = s[1:] == s[:-1]
        assert np.array_equal(raw_s[1:][same_flake], raw_s[:-1][same_flake])
        assert (t["flags"] <= 1).all()
        flagged = t["flags"] == 1
        assert np.array_equal(np.sort(t["src"][flagged]), np.arange(t["n_flakes"], dtype=np.uint32))       # exactly one per flake
        fb = np.empty(t["n_flakes"], np.int64)
        fb[t["src"][flagged]] = t["bin"][flagged]
        exact = ~np.isin(np.arange(t["n_flakes"]), guard)
        assert np.array_equal(fb[exact], rest["first"][exact])
        copies = np.bincount(t["src"], minlength=t["n_flakes"])
        assert np.array_equal(copies[exact], rest["span"][exact])


# ---- 1 .. 4: every named case, both filings -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", tfi.DEVICE_CASES)
def test_host_filed_table_read_through_the_tap_is_the_restatement(eng, name):
    """Also the proof of the tap: what it returns for a host-filed table is what sg_file_table_host made, by its definition."""
    got, want = _both(eng, name)["host"], tfi.restate(tfi.tables()[name])
    assert got["n_flakes"] == want["n_flakes"] == len(tfi.tables()[name])
    tfi.assert_structure_is_the_restatement(got, want, name)
    assert got["entries"]["rho"].tobytes() == want["rho"][want["src"]].tobytes()
    assert got["entries"]["x"].tobytes() == tfi.tables()[name][want["src"], 0].tobytes()


@pytest.mark.parametrize("name", tfi.DEVICE_CASES)
def test_device_filed_table_is_the_host_filed_table(eng, name):
    """Structure exactly -- bin offsets, the src sequence and flags of every bin, longest bin, record count, an all-zero spare record --
    and the record fields: x, y, r, rho bit for bit, phi, t0, t1 within 1 ulp; every copy of a flake identical apart from flags."""
    both, want = _both(eng, name), tfi.restate(tfi.tables()[name])
    _assert_records(both["device"], both["host"], want)
    tfi.assert_structure_is_the_restatement(both["device"], want, name)


@pytest.mark.parametrize("name", tfi.DEVICE_CASES)
@pytest.mark.parametrize("how", ["host", "device"])
def test_range_indexes_of_both_filings_are_the_plain_counts(eng, name, how):
    """bin_q and bin_qs as k_table_index wrote them on the GPU, including the repeated bin-0 word of every row and the last step's upper
    count (the bin's length), and the shape the library files: 64 steps of 2 m."""
    got, want = _both(eng, name)[how], tfi.restate(tfi.tables()[name])
    assert np.array_equal(got["bin_q"], want["bin_q"])
    assert got["bin_qs"] is not None and got["bin_qs"].shape == (tfi.QS_STEPS, tfi.NBINS + 1)
    assert np.array_equal(got["bin_qs"], want["bin_qs"])
    assert np.array_equal(got["bin_qs"][:, tfi.NBINS], got["bin_qs"][:, 0])
    assert np.array_equal(got["bin_qs"][-1, :tfi.NBINS] >> 16, np.diff(got["bin_start"].astype(np.int64)))
    assert got["qs_steps"] == tfi.QS_STEPS == 64 and got["qs_per_m"] == 1.0 / tfi.QS_STEP_M == 0.5


def test_the_tap_refuses_unknown_ids_null_pointers_and_small_buffers(eng):
    import ctypes
    from lidar_snow_sim_amd import _native
    L, h, tid = eng.ctx._L, eng.ctx.handle, eng.user_table_id()
    with pytest.raises(_native.SnowGPUError) as e:
        eng.ctx.debug_table_bins(tid)                                      # never filed
    assert e.value.code == _native.E_INVALID and "unknown table id" in str(e.value)
    eng.ctx.upload_table(tid, tfi.tables()["edges"])
    try:
        want = tfi.restate(tfi.tables()["edges"])
        n = want["n_entries"]
        start, ent = np.zeros(tfi.NBINS + 1, np.uint32), np.full(n + 2, 0xff, np.uint8).repeat(64).view(tfi.ENTRY_DTYPE)
        q, qs = np.zeros(tfi.NBINS * tfi.QSTEPS, np.uint32), np.zeros(tfi.QS_STEPS * (tfi.NBINS + 1), np.uint32)
        info, per_m = np.zeros(5, np.int64), np.zeros(1, np.float64)
        bufs = [(start, start.size), (ent, n + 1), (q, q.size), (qs, qs.size)]

        def call(bufs, info=info, per_m=per_m, table=tid):
            args = [a for b, cap in bufs for a in (None if b is None else ctypes.c_void_p(b.ctypes.data), cap)]
            return L.snowgpu_debug_table_bins(h, table, *args, None if info is None else ctypes.c_void_p(info.ctypes.data),
                                              None if per_m is None else ctypes.c_void_p(per_m.ctypes.data))
        assert call(bufs) == _native.E_OK and info.tolist() == [20, n, want["max_bin"], 64, 1] and per_m[0] == 0.5
        assert ent[n].tobytes() == bytes(64) and ent[n + 1].tobytes() == b"\xff" * 64       # n + 1 records written, not one more
        for i in range(4):
            assert call([(None, c) if j == i else (b, c) for j, (b, c) in enumerate(bufs)]) == _native.E_INVALID
            assert call([(b, c - 1) if j == i else (b, c) for j, (b, c) in enumerate(bufs)]) == _native.E_INVALID
        assert call(bufs, info=None) == _native.E_INVALID and call(bufs, per_m=None) == _native.E_INVALID
        assert call(bufs, table=-1) == _native.E_INVALID and call(bufs, table=1 << 21) == _native.E_INVALID
    finally:
        eng.ctx.free_table(tid)
    with pytest.raises(_native.SnowGPUError) as e:
        eng.ctx.debug_table_bins(tid)                                      # freed
    assert e.value.code == _native.E_INVALID


# ---- 5: a bin beyond the 16-bit counts ------------------------------------------------------------------------------------
def test_a_table_with_a_bin_of_66000_records_has_no_step_major_index(eng):
    """Host filing only (k_file_sort's rank sort is quadratic in a bin's length); bin_q is filed by k_table_index on the GPU all the same."""
    table, tid = tfi.longbin_host(), eng.user_table_id()
    want = tfi.restate(table)
    try:
        eng.ctx.upload_table(tid, table)
        got = _tap(eng, tid)
    finally:
        eng.ctx.free_table(tid)
    assert got["max_bin"] == 66000 and got["bin_qs"] is None and got["qs_steps"] == 0
    tfi.assert_structure_is_the_restatement(got, want, "longbin_host")
    assert got["n_flakes"] == 66000 and got["spare"].tobytes() == bytes(64)


# ---- 6: filing over a table -------------------------------------------------------------------------------------------------
def test_refiling_an_id_on_the_device_leaves_nothing_of_the_old_table(eng):
    tid = eng.user_table_id()
    try:
        _file_device(eng, tid, tfi.tables()["long"])
        assert _tap(eng, tid)["max_bin"] == 1700
        _file_device(eng, tid, tfi.tables()["random"])
        got = _tap(eng, tid)
    finally:
        eng.ctx.free_table(tid)
    want = tfi.restate(tfi.tables()["random"])
    assert got["n_flakes"] == 3001
    tfi.assert_structure_is_the_restatement(got, want, "random over long")
    _assert_records(got, _both(eng, "random")["host"], want)


# ---- 7: a sampled table, filed where it was made ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["filed900", "s5"])
def test_a_sampled_table_filed_in_place(eng, name):
    """sample_table(tid, ...) files the sampler's output in place; the structure read through the tap equals the host filing of the rows
    it returned: same bins, same order, same flags, fields as above (1 ulp).  Rows inside the guard band (1e-12 rad from a bin edge) cannot
    be chosen away here: for them, and only them, the first or last bin may differ by one.  Their count is asserted below 1e-6 of the
    records and printed.  Measured without a GPU on the restated rows (tests/seeded_reference.py): filed900 -- 4220 rows, 4329 records, 0
    rows in the band, smallest distance to an edge 1.1e-7 rad; s5 -- 1235 rows, 4380 records, 0 rows in the band, smallest distance
    1.8e-6 rad.  The expected count is zero."""
    import seeded_reference as sr
    s = sr.sampler_settings()[name]
    tid, t_host = eng.user_table_id(), eng.user_table_id()
    try:
        rows = eng.ctx.sample_table(tid, s["occupancy"], s["scale_mm"], s["R0"], s["seed"])
        dev = _tap(eng, tid)
        eng.ctx.upload_table(t_host, rows)
        host = _tap(eng, t_host)
    finally:
        for t in (tid, t_host):
            try:
                eng.ctx.free_table(t)
            except Exception:
                pass
    want = tfi.restate(rows)
    guard = tfi.guard_rows(rows)
    print(f"\n[table-filing] {name}: {len(rows)} rows, {want['n_entries']} records, {guard.size} rows inside the guard band")
    assert guard.size < 1e-6 * want["n_entries"]
    tfi.assert_structure_is_the_restatement(host, want, name)
    _assert_records(dev, host, want, guard)
    for key in ("bin_q", "bin_qs"):                      # the device-filed table's indexes: the plain counts over ITS records
        assert np.array_equal(dev[key], host[key]) or guard.size


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------
def _assert_refused(eng, how, table, *words):
    from lidar_snow_sim_amd import _native
    tid = eng.user_table_id()
    with pytest.raises(_native.SnowGPUError) as e:
        FILINGS[how](eng, tid, table)
    assert e.value.code == _native.E_TABLE, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    with pytest.raises(_native.SnowGPUError) as e:        # no half-registered table under the refused id
        eng.ctx.debug_table_bins(tid)
    assert e.value.code == _native.E_INVALID
    return tid


def _assert_files_random(eng, how, tid):
    try:
        FILINGS[how](eng, tid, tfi.tables()["random"])
        got = _tap(eng, tid)
    finally:
        eng.ctx.free_table(tid)
    tfi.assert_structure_is_the_restatement(got, tfi.restate(tfi.tables()["random"]), f"random after a refusal ({how})")


@pytest.mark.parametrize("how", ["host", "device"])
def test_a_table_that_covers_most_azimuths_is_refused(eng, how):
    tid = _assert_refused(eng, how, tfi.too_close(), "cover most azimuths")
    _assert_files_random(eng, how, tid)


@pytest.mark.parametrize("how", ["host", "device"])
def test_a_bad_row_is_refused_by_its_number(eng, how):
    """NaN, inf, r = 0, r < 0, rho <= r, each alone at row 1234 of `random`; then rows 5000, 300 and 700 of a 6000-row table, which three
    different blocks of k_file_derive see: the smallest, row 300, is the one named (the device keeps it as the largest 0x7fffffff - row)."""
    for kind, (table, row) in tfi.bad_rows().items():
        tid = _assert_refused(eng, how, table, f"row {row} ", "is not a disk clear of the origin")
        if kind == "together":
            assert row == 300
            _assert_files_random(eng, how, tid)
