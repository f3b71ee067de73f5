"""Sectorized keypoint sampling without a GPU: the conditions under which the comparisons of tests/test_gpu_fps_sectors.py are not vacuous,
asserted on the shared inputs of tests/fps_sectors_reference.py; the reach, the near test, the sector, the quota and the ballot rank of
csrc/sg_fps_sectors.h compiled for the host (tests/host_harness/fps_sectors.cpp, once more under the address and undefined-behaviour
sanitizers as a stand-alone program) against the restatement and against libm; and what snowgpu_fps_sectors_device refuses, in which
words (tests/host_harness/fps_sectors_refusals.cpp)."""
import itertools
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import fps_reference as fr
import fps_sectors_reference as sr
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = sr.DTYPES


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
def test_every_sector_edge_has_rows_on_both_sides_one_step_apart():
    xy, pairs = sr.edge_points()
    assert sorted({(S, k) for S, k, _, _ in pairs}) == [(S, k) for S in sr.EDGE_SECTORS for k in range(1, S)]
    for S, k, i, j in pairs:
        (xa, ya), (xb, yb) = xy[i], xy[j]
        assert sr._sec1(xa, ya, S) == k - 1 and sr._sec1(xb, yb, S) == k, (S, k)
        moved = [(a, b) for a, b in ((xa, xb), (ya, yb)) if a != b]
        assert len(moved) == 1 and np.nextafter(moved[0][0], moved[0][1]) == moved[0][1], (S, k)      # ONE float32 step
    for dtype in DTYPES:
        rows, at = sr.edges_case(dtype)
        assert np.array_equal(rows[at, :2].astype(np.float32), xy) and (rows[at, 2] == 0.5).all()
        for S in sr.EDGE_SECTORS:
            e = sr.expected("edges", dtype, S)
            sec = e["sector_of"][at]
            assert (sec >= 0).all() and e["usable"][0] == len(rows) > 20 * 32
            for S2, k, i, j in pairs:
                if S2 == S:
                    assert (sec[i], sec[j]) == (k - 1, k), (dtype, S, k)


def test_origin_seam_and_axes():
    xy, pairs = sr.edge_points()
    tail = xy[2 * len(pairs):]
    assert len(tail) == 14
    seam, origin, axes = tail[:4], tail[4:8], tail[8:]
    assert (seam[:, 0] < 0).all() and not seam[:, 1].any() and np.signbit(seam[:, 1]).tolist() == [True, False, True, False]
    assert not origin.any() and len({(bool(np.signbit(a)), bool(np.signbit(b))) for a, b in origin}) == 4
    assert ((axes == 0).sum(axis=1) == 1).all()
    for S in sr.EDGE_SECTORS:
        s = sr.sector_of(seam[:, 0], seam[:, 1], S)
        assert s.tolist() == [0, S - 1, 0, S - 1]                              # y = -0 below the seam, y = +0 above it
        o = sr.sector_of(origin[:, 0], origin[:, 1], S)
        assert ((o >= 0) & (o < S)).all()
    # S = 1: everything is sector 0
    assert not sr.sector_of(xy[:, 0], xy[:, 1], 1).any()


def _quota_facts(n, K):
    q, m = sr.quota(n, K), sum(n)
    if m < K:
        assert q == list(n)
        return 0, ()
    floors, rem = [v * K // m for v in n], [v * K % m for v in n]
    L = K - sum(floors)
    assert sum(q) == K and all(a <= b for a, b in zip(q, n)) and 0 <= L < len(n)
    winners = [s for s in range(len(n)) if q[s] == floors[s] + 1]
    assert len(winners) == L and all(rem[s] > 0 for s in winners) and all(q[s] in (floors[s], floors[s] + 1) for s in range(len(n)))
    return L, rem


def test_quota_facts_on_an_exhaustive_sweep():
    for n in itertools.product(range(7), repeat=4):
        for K in range(1, 15):
            _quota_facts(n, K)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quota_frames_meet_the_conditions(dtype):
    rows, offsets, _, _, (_, K, _) = sr.case("quota", dtype)
    e = sr.expected("quota", dtype, 4)
    assert K == sr.QUOTA_K and e["sector_count"].tolist() == [list(c) for c in sr.QUOTA_COUNTS]
    assert (np.diff(offsets) == e["usable"] + 3).all()                          # three unusable rows per frame
    L0, rem0 = _quota_facts(sr.QUOTA_COUNTS[0], K)
    assert L0 > 0 and 0 in sr.QUOTA_COUNTS[0] and 1 in sr.QUOTA_COUNTS[0]          # one more for some, an empty sector, a sector of one row
    assert e["sector_offsets"][0].tolist() == [0, 5, 5, 6, 12]
    L1, rem1 = _quota_facts(sr.QUOTA_COUNTS[1], K)
    assert L1 == 2 and len(set(rem1)) == 1 and e["sector_offsets"][1].tolist() == [0, 4, 8, 10, 12]      # equal remainders: the smaller s first
    m = e["usable"].tolist()
    assert 0 < m[2] < K and m[3] == K and m[4] == 0
    assert e["sector_offsets"][2, -1] == m[2] and (e["index"][2, m[2]:] == e["index"][2, 0]).all() and not e["dist"][2, m[2]:].any()
    assert sorted(e["index"][3].tolist()) == sorted(np.flatnonzero(e["sector_of"][offsets[3]:offsets[4]] >= 0) + offsets[3])
    assert (e["index"][4] == -1).all() and (e["dist"][4] == -1).all() and not e["points"][4].any() and not e["sector_offsets"][4].any()
    for f in range(4):                                                          # the first sample of every sector has dist +inf
        o = e["sector_offsets"][f]
        starts = [o[s] for s in range(4) if o[s + 1] > o[s]]
        assert np.isinf(e["dist"][f, starts]).all() and np.isinf(e["dist"][f]).sum() == len(starts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_roi_frames_meet_the_conditions(dtype):
    rows, offsets, _, rois, (_, K, margin) = sr.case("roi", dtype)
    present, r2 = sr.reach2_of(rois, margin)
    assert present.tolist() == [[True, True, True, False, False, False], [False] * 6] and not rois[0, 3, :7].any()      # zero padding; a frame without a roi
    assert r2[0, 0] == sr.ROI_REACH2 and not r2[~present].any()
    p = rows[:3, :3].astype(np.float64)
    d = np.add(np.add(np.multiply(p[:, 0], p[:, 0]), np.multiply(p[:, 1], p[:, 1])), np.multiply(p[:, 2], p[:, 2]))
    assert d.tolist() == [64.0, np.nextafter(64.0, 65.0), np.nextafter(64.0, 0.0)]
    near0 = sr.near_any(rows[:3, :3], rois[0, :1], margin)
    assert near0.tolist() == [False, False, True]                                # the comparison is strict
    both = sr.near_any(rows[:1500, :3], rois[0, 1:2], margin) & sr.near_any(rows[:1500, :3], rois[0, 2:3], margin)
    assert both.sum() >= 10                                                      # overlapping rois
    for S in sr.SECTORS:
        e = sr.expected("roi", dtype, S)
        assert K < e["usable"][0] < 1500 and e["usable"][1] == 0 and (e["index"][1] == -1).all()
        assert (e["sector_of"][:3] >= 0).tolist() == [False, False, True] and (e["sector_of"][1500:] == -1).all()
        assert e["reach2"].tobytes() == r2.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_sector_without_rois_is_the_plain_walk(dtype):
    for name in ("batch", "constructed", "fewer37", "fewer0"):
        rows, offsets, keep, (rng, K) = fr.case(name, dtype)
        want, got = fr.expected(name, dtype), sr.fps_sectors(rows, K, 1, rng, 4, keep, offsets)
        for f in ("index", "points", "dist", "usable"):
            assert got[f].tobytes() == want[f].tobytes(), (name, f)


def test_tier_frames_straddle_the_capacities():
    from lidar_snow_sim_amd.fps import TIER_ROWS
    for dtype in DTYPES:
        _, _, sizes, e = sr.tier_case(dtype)
        t0, t1, t2 = TIER_ROWS[dtype]
        assert e["sector_count"].tolist() == [list(s) for s in sizes] == [[t1, t1 + 1], [t0 - 1, t0 + 1], [t2 - 1, t2 + 1]]
        assert (np.diff(e["sector_offsets"], axis=1) >= 11).all()               # every walk runs rounds


def test_coverage_radius_of_sectors_beside_one_walk():
    """Printed, not asserted: what a user trades.  One synthetic sweep under SECOND's range, K = 2048."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    rows = np.ascontiguousarray(synthetic_sweep(64, 512, seed=7))
    ok = fr.usable_rows(rows, fr.SECOND_RANGE)
    for K in (512, 2048):
        for S in (1, 6):
            e = sr.fps_sectors(rows, K, S, fr.SECOND_RANGE)
            print(f"coverage radius: usable rows {int(ok.sum())} K {K} S {S}: {sr.coverage_radius(rows[ok], np.searchsorted(np.flatnonzero(ok), e['index'][0])):.3f} m")


# ---- csrc/sg_fps_sectors.h on the host ----------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra,
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "fps_sectors.cpp"),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("fpss"), "fps_sectors")


@pytest.fixture(scope="module")
def harness_sanitized(tmp_path_factory):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    return _compile(tmp_path_factory.mktemp("fpss_san"), "fps_sectors_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _self(exe, points):
    r = subprocess.run([str(exe), "self", str(points)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert "ranks ok" in lines and "quota swept %d" % (7 ** 4 * 14) in lines
    mismatches = int(re.fullmatch(r"sector points (\d+) mismatches (\d+)", next(ln for ln in lines if ln.startswith("sector points"))).group(2))
    assert mismatches < 16 * points // 500                                      # (glibc's atan2 is not correctly rounded everywhere)
    settled = 0
    for ln in lines:
        if ln.startswith("q "):
            v = [int(t) for t in ln.split()[1:]]
            assert sr.quota(v[:4], v[4]) == v[5:], ln
        elif ln.startswith("M "):                                               # ours is the sector of the correctly rounded angle
            _, S, xs, ys, ours, _ = ln.split()
            a = np.add(_atan2_70_digits(float.fromhex(ys), float.fromhex(xs)), np.pi)
            assert min(int(np.floor(np.divide(a, np.divide(2 * np.pi, int(S))))), int(S) - 1) == int(ours), ln
            settled += 1
    assert settled == mismatches
    return lines


def _atan2_70_digits(y, x):
    """atan2 of two non-zero doubles in 70-digit arithmetic, rounded once to the nearest double."""
    from decimal import Decimal, getcontext
    sys.path.insert(0, str(ROOT / "scripts"))
    import gen_atan_table as gen
    getcontext().prec = 70
    ay, ax = abs(Decimal(y)), abs(Decimal(x))
    t = gen.atan_dec(min(ay, ax) / max(ay, ax))
    if ay > ax:
        t = gen.PI / 2 - t
    if x < 0:
        t = gen.PI - t
    return np.float64(float(-t if y < 0 else t))


def _rows(exe, tmp_path, rows, rois, margin, S, dtype):
    fi, fb, fo = tmp_path / "p.in", tmp_path / "b.in", tmp_path / "s.out"
    np.ascontiguousarray(np.asarray(rows)[:, :3], np.float64).tofile(fi)
    if rois is not None:
        np.ascontiguousarray(np.asarray(rois)[:, :6], np.float64).tofile(fb)
    r = subprocess.run([str(exe), "rows", str(DTYPES.index(dtype)), str(S), repr(float(margin)), str(fi), str(fb) if rois is not None else "-", str(fo)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = fo.read_bytes()
    return np.frombuffer(raw[:len(rows)], np.int8), np.frombuffer(raw[len(rows):], np.float64)


def _check_rows(exe, tmp_path, sectors=sr.SECTORS):
    for dtype in DTYPES:
        for S in sectors:
            rows = sr.case("edges", dtype)[0]
            sec, _ = _rows(exe, tmp_path, rows, None, 0.0, S, dtype)
            assert np.array_equal(sec, sr.expected("edges", dtype, S)["sector_of"]), (dtype, S)
            rows, offsets, _, rois, (_, _, margin) = sr.case("roi", dtype)
            e = sr.expected("roi", dtype, S)
            for f in range(2):
                a, b = offsets[f], offsets[f + 1]
                sec, r2 = _rows(exe, tmp_path, rows[a:b], rois[f], margin, S, dtype)
                assert np.array_equal(sec, e["sector_of"][a:b]) and r2.tobytes() == e["reach2"][f].tobytes(), (dtype, S, f)


def test_host_functions_equal_libm_and_the_quota_sweep(harness):
    _self(harness, 250000)                                                      # 16 x 250 000 = 4 000 000 points at the edges


def test_host_functions_equal_the_restatement(harness, tmp_path):
    _check_rows(harness, tmp_path)


def test_host_functions_under_sanitizers(harness_sanitized, tmp_path):
    _self(harness_sanitized, 20000)
    _check_rows(harness_sanitized, tmp_path, (6,))


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_fps_sectors_device"
APART = {"keep_in": " overlaps d_keep_in; the mask is read while the samples are written: pass a buffer apart from it",
         "rows": " overlaps d_rows; the rows are read while the samples are written: pass a buffer apart from them",
         "rois": " overlaps d_rois; the rois are read while the samples are written: pass a buffer apart from them"}
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "features": WHO + ": n_features must be 3, 4 or 5: the columns of a row that a keypoint carries",
    "least_1": WHO + ": n_samples must be at least 1",
    "slots": WHO + ": n_frames * n_samples exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "nan": WHO + ": a bound of the range is NaN; pass NULL for no range, or infinite bounds",
    "order": WHO + ": the range needs lo < hi on every axis",
    "sectors": WHO + ": n_sectors must lie in 1 .. 16",
    "n_rois": WHO + ": n_rois must lie in 1 .. 256",
    "roi_features": WHO + ": roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first",
    "margin": WHO + ": roi_margin must be finite and at least 0",
    "roi_slots": WHO + ": n_frames * n_rois exceeds 2^31 - 1; split the batch",
    "reach2": WHO + ": d_out_reach2 without d_rois; there is no reach to write",
    "tiles": WHO + ": n_frames * ceil(max_frame_rows / 1024) exceeds 2^27 - 1; split the batch",
    "index_keep": WHO + ": d_out_index" + APART["keep_in"],
    "sector_of_keep": WHO + ": d_out_sector_of" + APART["keep_in"],
    "points_rows": WHO + ": d_out_points" + APART["rows"],
    "count_rows": WHO + ": d_out_sector_count" + APART["rows"],
    "dist_rois": WHO + ": d_out_dist" + APART["rois"],
    "reach2_rois": WHO + ": d_out_reach2" + APART["rois"],
    "points_index": WHO + ": d_out_points overlaps d_out_index" + OWN,
    "usable_dist": WHO + ": d_out_usable overlaps d_out_dist" + OWN,
    "offsets_usable": WHO + ": d_out_sector_offsets overlaps d_out_usable" + OWN,
    "count_offsets": WHO + ": d_out_sector_count overlaps d_out_sector_offsets" + OWN,
    "sector_of_count": WHO + ": d_out_sector_of overlaps d_out_sector_count" + OWN,
    "reach2_sector_of": WHO + ": d_out_reach2 overlaps d_out_sector_of" + OWN,
}
ACCEPTED = ("clean", "null_out_points", "null_out_dist", "null_out_sector_of", "null_out_reach2", "null_keep_in", "null_range", "null_rois", "float64",
            "empty_null_rows", "samples_1", "range_infinite", "sectors_1", "sectors_16", "rois_1", "rois_256", "roi_features_10", "margin_0",
            "sector_of_behind_keep_in", "dist_behind_rois", "count_behind_offsets")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_out_index", "null_out_usable", "null_out_sector_offsets", "null_out_sector_count", "bad_dtype",
             "no_frames", "negative_rows", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_features_2"),
    "features": ("features_2", "features_6", "features_2_and_samples_0"),
    "least_1": ("samples_0",),
    "slots": ("frames_times_samples_2p31", "frames_times_samples_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_range_nan"),
    "nan": ("range_nan_lo", "range_nan_and_range_lo_is_hi"),
    "order": ("range_lo_is_hi", "range_lo_is_hi_and_sectors_0"),
    "sectors": ("sectors_0", "sectors_17", "sectors_0_and_rois_0"),
    "n_rois": ("rois_0", "rois_257", "rois_0_and_roi_features_6"),
    "roi_features": ("roi_features_6", "roi_features_11", "roi_features_6_and_margin_nan"),
    "margin": ("margin_negative", "margin_nan", "margin_inf", "margin_nan_and_frames_times_rois_2p31"),
    "roi_slots": ("frames_times_rois_2p31", "frames_times_rois_2p31_and_tiles_2p27"),
    "reach2": ("reach2_without_rois", "reach2_without_rois_and_tiles_2p27"),
    "tiles": ("tiles_2p27", "tiles_2p27_and_index_overlaps_rows"),
    "index_keep": ("index_is_keep_in",),
    "sector_of_keep": ("sector_of_overlaps_keep_in",),
    "points_rows": ("points_are_rows",),
    "count_rows": ("count_overlaps_rows",),
    "dist_rois": ("dist_overlaps_rois",),
    "reach2_rois": ("reach2_are_rois",),
    "points_index": ("points_overlap_index",),
    "usable_dist": ("usable_overlaps_dist",),
    "offsets_usable": ("offsets_are_usable",),
    "count_offsets": ("count_overlaps_offsets",),
    "sector_of_count": ("sector_of_overlaps_count",),
    "reach2_sector_of": ("reach2_overlaps_sector_of",),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "fps_sectors_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "fps_sectors_refusals.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split("|", 1) for ln in r.stdout.splitlines())
    want = {case: "0|OK" for case in ACCEPTED}
    for key, cases in REFUSED.items():
        want.update({case: "1|" + MESSAGES[key] for case in cases})
    assert got == want
    assert set(MESSAGES) == set(REFUSED)              # every message is reached


def test_the_entry_is_declared_and_bound():
    import inspect
    from lidar_snow_sim_amd import _native, fps, tensors
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_fps_sectors_device(" in header and "snowgpu_fps_sectors_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_fps_sectors_device") and hasattr(_native.Context, "fps_sectors_device")
    par = inspect.signature(tensors.sample_keypoints).parameters
    assert [par[k].default for k in ("sectors", "rois", "roi_margin", "return_sector_of")] == [None, None, 1.6, False]
    par = inspect.signature(tensors.KeypointBatch.empty).parameters
    assert "sectors" in par and "with_sector_of" in par
    assert list(inspect.signature(fps.sectorized_sample).parameters)[:5] == ["pc", "n_samples", "n_sectors", "rois", "roi_margin"]
    assert inspect.signature(fps.sectorized_sample).parameters["n_sectors"].default == 6
