"""Farthest point sampling without a GPU: the conditions under which the comparisons of tests/test_gpu_fps.py are not vacuous, asserted on
the shared inputs of tests/fps_reference.py; the usable test, the distance, the candidate key and its fold of csrc/sg_fps.h, compiled for
the host and walked over 1024 "lanes" in the kernel's assignment and in scrambled ones (tests/host_harness/fps_walk.cpp, once more under
the address and undefined-behaviour sanitizers as a stand-alone program), against the restatement; and what snowgpu_fps_device refuses,
in which words (tests/host_harness/fps_refusals.cpp)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fps_reference as fr
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = fr.DTYPES


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_is_decided_by_the_tie_rule(dtype):
    rows, _, _, (rng, K) = fr.case("lattice", dtype)
    e = fr.expected("lattice", dtype)
    assert rows.shape == (16 * 16 * 4 + 200, 5) and rng is None and K == 64
    assert len({tuple(r) for r in rows[:, :3].tolist()}) == 1024 and e["usable"][0] == len(rows)
    tied = int((e["ties"][0] >= 2).sum())
    print("rounds decided by the tie rule:", tied, "distinct samples:", len(set(e["index"][0].tolist())))
    assert tied >= 16
    assert len({tuple(r) for r in e["points"][0, :, :3].tolist()}) == 64          # coincident rows are never both chosen
    assert e["dist"][0, 0] == np.inf and (e["dist"][0, 1:] > 0).all() and (np.diff(e["dist"][0, 1:]) <= 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_frame_meets_the_conditions(dtype):
    rows, _, keep, (rng, K) = fr.case("constructed", dtype)
    _, _, kinds = fr.constructed_case(dtype)
    ok = fr.usable_rows(rows, rng, keep)
    assert rows.shape == (3000, 5)
    for kind in ("nan", "far", "below", "on_hi", "masked"):
        assert (kinds == kind).sum() >= 16 and not ok[kinds == kind].any(), kind
    assert (kinds == "on_lo").sum() >= 16 and ok[kinds == "on_lo"].all() and ok[kinds == "plain"].all()
    assert np.isnan(rows[kinds == "nan", :3]).any(axis=1).all() and (np.abs(rows[kinds == "far", :3]) > 1e6).any(axis=1).all()
    on_lo = rows[kinds == "on_lo", :3].astype(np.float64)
    assert (on_lo == np.array(rng[:3])).any(axis=1).all()
    e = fr.expected("constructed", dtype)
    assert e["usable"][0] == ok.sum() and ok[e["index"][0]].all() and len(set(e["index"][0].tolist())) == K


@pytest.mark.parametrize("dtype", DTYPES)
def test_frames_of_fewer_rows_than_samples(dtype):
    e = fr.expected("fewer37", dtype)
    rows, _, _, (rng, K) = fr.case("fewer37", dtype)
    u = np.flatnonzero(fr.usable_rows(rows, rng))
    assert len(u) == 37 and K == 64 and len({tuple(r) for r in rows[u, :3].tolist()}) == 37
    assert sorted(e["index"][0, :37].tolist()) == u.tolist() and (e["index"][0, 37:] == u[0]).all() and e["index"][0, 0] == u[0]
    assert (e["dist"][0, 1:37] > 0).all() and not e["dist"][0, 37:].any()
    e = fr.expected("fewer1", dtype)
    u = np.flatnonzero(fr.usable_rows(fr.case("fewer1", dtype)[0], rng))
    assert len(u) == 1 and u[0] > 0 and (e["index"][0] == u[0]).all() and e["dist"][0, 0] == np.inf and not e["dist"][0, 1:].any()
    e = fr.expected("fewer0", dtype)
    assert e["usable"][0] == 0 and (e["index"] == -1).all() and not e["points"].any() and (e["dist"] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_of_frames(dtype):
    rows, offsets, keep, (rng, K) = fr.case("batch", dtype)
    assert np.array_equal(np.diff(offsets), (6000, 0, 1500, 300)) and all(int(o) % 64 for o in offsets[1:])
    assert not keep[offsets[3]:].any() and 0.7 < keep[:offsets[3]].mean() < 0.9
    assert rows[2000:3500].tobytes() == rows[6000:7500].tobytes()      # the same coordinates in two frames
    e = fr.expected("batch", dtype)
    assert 4000 < e["usable"][0] < 6000 and e["usable"][1] == 0 and 1000 < e["usable"][2] < 1500 and e["usable"][3] == 0
    assert (e["index"][[1, 3]] == -1).all() and (e["dist"][[1, 3]] == -1).all() and not e["points"][[1, 3]].any()
    assert ((e["index"][0] >= 0) & (e["index"][0] < 6000)).all() and ((e["index"][2] >= 6000) & (e["index"][2] < 7500)).all()
    assert keep[e["index"][0]].all() and keep[e["index"][2]].all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_difference_of_coordinates_is_tiny(dtype):
    """No non-zero coordinate difference below 2^-20: no product of the distance is subnormal, so a device that flushed could not hide."""
    for name in fr.CASES:
        rows, _, keep, (rng, _) = fr.case(name, dtype)
        p = rows[fr.usable_rows(rows, rng, keep), :3].astype(np.float64)
        for j in range(3):
            d = np.diff(np.unique(p[:, j]))
            assert not len(d) or d.min() >= 2.0 ** -20, (name, j)


def test_tier_rows_are_whole_pieces():
    """The register tiers hold whole rows per lane, the LDS tier whole 16-byte pieces of four rows, 156 KiB of them."""
    from lidar_snow_sim_amd.fps import TIER_ROWS
    assert set(TIER_ROWS) == set(DTYPES)
    for dtype, tiers in TIER_ROWS.items():
        assert len(tiers) == 3 and list(tiers) == sorted(set(tiers))
        assert tiers[0] % 1024 == 0 and tiers[1] % 1024 == 0 and tiers[2] % 4 == 0 and tiers[2] * np.dtype(dtype).itemsize == 156 * 1024


# ---- csrc/sg_fps.h on the host ----------------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra,
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "fps_walk.cpp"),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("fps"), "fps_walk")


@pytest.fixture(scope="module")
def harness_sanitized(tmp_path_factory):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    return _compile(tmp_path_factory.mktemp("fps_san"), "fps_walk_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _run(exe, rows, keep, rng, K, dtype, tmp_path, tag, seed):
    fi, fk, fo = tmp_path / f"{tag}.in", tmp_path / f"{tag}.keep", tmp_path / f"{tag}.out"
    np.ascontiguousarray(np.asarray(rows)[:, :3], np.float64).tofile(fi)
    (np.ones(len(rows), np.uint8) if keep is None else np.asarray(keep).astype(np.uint8)).tofile(fk)
    bounds = (-np.inf,) * 3 + (np.inf,) * 3 if rng is None else rng
    cmd = [str(exe), str(DTYPES.index(dtype)), str(K), *(repr(float(v)) for v in bounds), str(fi), str(fk), str(fo), str(seed)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = fo.read_bytes()
    m = int(np.frombuffer(raw[:4], np.int32)[0])
    return m, np.frombuffer(raw[4:4 + 4 * K], np.int32), raw[4 + 4 * K:], r.stdout.split()


def _check_one(exe, tmp_path, rows, keep, rng, K, dtype, want, f, base, seeds, what):
    for seed in seeds:
        m, index, dist, words = _run(exe, rows, keep, rng, K, dtype, tmp_path, "w", seed)
        assert m == want["usable"][f], (what, seed)
        assert np.array_equal(np.where(index >= 0, index + base, -1), want["index"][f]), (what, seed)
        assert dist == want["dist"][f].tobytes(), (what, seed)
        from lidar_snow_sim_amd.fps import TIER_ROWS
        assert words == ["tiers", *map(str, TIER_ROWS["float32"] + TIER_ROWS["float64"])]


def _check_against_restatement(exe, tmp_path, names, seeds, dtypes=DTYPES):
    for dtype in dtypes:
        for name in names:
            rows, offsets, keep, (rng, K) = fr.case(name, dtype)
            want = fr.expected(name, dtype)
            for f, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
                _check_one(exe, tmp_path, rows[a:b], None if keep is None else keep[a:b], rng, K, dtype, want, f, int(a), seeds, (name, dtype, f))


def test_host_walk_equals_the_restatement(harness, tmp_path):
    _check_against_restatement(harness, tmp_path, fr.CASES, (0, 1, 2))


def test_host_walk_in_the_streamed_assignment(harness, tmp_path):
    """A frame beyond the register tiers: the kernel's other assignment of points to lanes (float64: 8193 usable rows)."""
    n, K = 8193, 24
    _check_one(harness, tmp_path, fr.cloud_case(n, "float64"), None, fr.RANGE, K, "float64", fr.cloud_expected(n, "float64", K), 0, 0, (0, 3), n)


def test_host_walk_under_sanitizers(harness_sanitized, tmp_path):
    _check_against_restatement(harness_sanitized, tmp_path, ("lattice", "constructed", "fewer37", "fewer0"), (0, 5))


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_fps_device"
APART = {"keep_in": " overlaps d_keep_in; the mask is read while the samples are written: pass a buffer apart from it",
         "rows": " overlaps d_rows; the rows are read while the samples are written: pass a buffer apart from them"}
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "features": WHO + ": n_features must be 3, 4 or 5: the columns of a row that a keypoint carries",
    "least_1": WHO + ": n_samples must be at least 1",
    "slots": WHO + ": n_frames * n_samples exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "nan": WHO + ": a bound of the range is NaN; pass NULL for no range, or infinite bounds",
    "order": WHO + ": the range needs lo < hi on every axis",
    "index_keep": WHO + ": d_out_index" + APART["keep_in"],
    "points_keep": WHO + ": d_out_points" + APART["keep_in"],
    "dist_keep": WHO + ": d_out_dist" + APART["keep_in"],
    "index_rows": WHO + ": d_out_index" + APART["rows"],
    "points_rows": WHO + ": d_out_points" + APART["rows"],
    "dist_rows": WHO + ": d_out_dist" + APART["rows"],
}
ACCEPTED = ("clean", "null_out_points", "null_out_dist", "null_keep_in", "null_range", "float64", "empty_null_rows", "features_3", "features_5",
            "samples_1", "frames_times_samples_2p31_minus_1", "frame_2p30_rows", "range_infinite", "keep_in_behind_index", "index_behind_keep_in",
            "index_behind_rows", "dist_is_points")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_out_index", "null_out_usable", "bad_dtype", "no_frames", "negative_rows", "empty_null_out_index", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_features_2"),
    "features": ("features_2", "features_6", "features_2_and_samples_0"),
    "least_1": ("samples_0", "samples_negative"),
    "slots": ("frames_times_samples_2p31", "frames_times_samples_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_range_nan"),
    "nan": ("range_nan_lo", "range_nan_hi", "range_nan_and_range_reversed"),
    "order": ("range_reversed", "range_lo_is_hi", "range_inf_lo_is_hi", "range_reversed_and_index_is_keep_in"),
    "index_keep": ("index_is_keep_in", "index_overlaps_keep_in"),
    "points_keep": ("points_overlap_keep_in",),
    "dist_keep": ("dist_overlaps_keep_in",),
    "index_rows": ("index_overlaps_rows",),
    "points_rows": ("points_are_rows",),
    "dist_rows": ("dist_overlaps_rows",),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "fps_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "fps_refusals.cpp"), "-o", str(exe)]
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
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_fps_device(" in header and "snowgpu_fps_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_fps_device") and hasattr(_native.Context, "fps_device")
    assert "snowgpu_fps.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import tensors
    assert callable(tensors.sample_keypoints) and callable(tensors.KeypointBatch.empty)
