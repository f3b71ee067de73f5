"""Ball query without a GPU: the conditions under which the comparisons of tests/test_gpu_ball_query.py are not vacuous, asserted on the
shared inputs of tests/ball_reference.py; the index and window functions of csrc/sg_ball.h compiled for the host -- every (centre, row)
pair inside a ball has the row's cell in the centre's window -- and whole frames walked through count / scan / scatter / query on the
host (tests/host_harness/ball_cells.cpp) against the restatement; the compare-exchange network and the merge over 64 host "lanes"
against a sort (tests/host_harness/ball_select.cpp, once more under the address and undefined-behaviour sanitizers as a stand-alone
program); and what snowgpu_ball_query_device refuses, in which words (tests/host_harness/ball_refusals.cpp)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ball_reference as br
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = br.DTYPES
ROLE = br.ROLE


def _ball(rows, centre, radius, rng=None, keep=None):
    """The usable rows strictly within `radius` of `centre`, ascending."""
    return np.flatnonzero(br.usable_rows(rows, rng, keep) & (_d(rows, centre) < br.squared_radius(radius, rows.dtype)))


def _d(rows, c):
    dx, dy, dz = (np.subtract(rows[:, j], c[j]) for j in range(3))
    return np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_frame_meets_the_conditions(dtype):
    rows, _, _, centres, (rng, (r,), (S,)) = br.case("constructed", dtype)
    e = br.expected("constructed", dtype)
    count, index = e["count"][0, :, 0], e["index"][0]
    assert 380 <= len(rows) <= 430 and centres.shape == (1, 24, 3) and S == 16 and r == 1.0
    # n = 0, S - 1, S, S + 1 and more than three batches of 64
    assert [int(count[ROLE[k]]) for k in ("n0", "n15", "n16", "n17")] == [0, 15, 16, 17] and count[ROLE["high_cells_first"]] > 64 * 3
    assert (index[ROLE["n0"]] == -1).all() and (index[ROLE["n15"], 15] == index[ROLE["n15"], 0]) and len(set(index[ROLE["n16"]].tolist())) == 16
    assert (np.diff(index[ROLE["n17"]]) > 0).all()
    # a row at exactly d == r2 is out, its neighbour one ulp inside is in
    c = centres[0, ROLE["on_the_sphere"]]
    d = _d(rows, c)
    r2 = br.squared_radius(r, dtype)
    on = np.flatnonzero(d == r2)
    assert len(on) >= 3 and count[ROLE["on_the_sphere"]] == 1
    inside = int(index[ROLE["on_the_sphere"], 0])
    assert rows[inside, 0] == np.nextafter(rows[on[0], 0], rows.dtype.type(0)) and inside == on[0] + 1 and d[inside] < r2
    # a centre whose membership differs between float32 and float64
    both = [int(br.expected("constructed", t)["count"][0, ROLE["dtype"], 0]) for t in DTYPES]
    assert both == [0, 1]
    # the grid is within its budget here; the 16 smallest indices of one ball lie in its highest-numbered cells, of another in its lowest
    g = br.grid(rng, (r,), len(rows))
    assert g["wanted"] == g["nx"] * g["ny"] == 33 * 33 <= g["budget"]
    for role, sign in (("high_cells_first", -1), ("low_cells_first", 1)):
        members = _ball(rows, centres[0, ROLE[role]], r, rng)
        cell = sign * br.cells(g, rows[members, :2])
        assert len(members) > 64 and len(set(cell.tolist())) >= 12
        assert cell[:16].max() <= cell[16:].min() and cell[:16].max() < cell[64:].min(), role      # (a walk the other way meets them last)
    # centres at the corners of the domain, on and off cell boundaries, and outside the range
    cen = centres[0].astype(np.float64)
    assert tuple(cen[ROLE["corner_lo"], :2]) == rng[:2] and tuple(cen[ROLE["corner_hi"], :2]) == rng[3:5] and cen[ROLE["outside_range"], 0] < rng[0]
    on_edge = ((cen[:, :2] - (g["x0"], g["y0"])) * g["inv"]) % 1.0 == 0
    assert on_edge[ROLE["n15"]].all() and not on_edge[ROLE["off_boundary"]].any()
    for role in ("corner_lo", "corner_hi", "off_boundary", "outside_range"):
        assert 0 < count[ROLE[role]] <= 12, role
    assert not br.usable_rows(rows, rng).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_and_centres_beyond_the_grid_and_a_budget_exceeded(dtype):
    rows, _, _, centres, (rng, (r,), (S,)) = br.case("outside", dtype)
    e = br.expected("outside", dtype)
    assert rng is None and len(rows) == 300
    g = br.grid(rng, (r,), len(rows))
    assert g["wanted"] > 1000 * g["budget"] and g["nx"] * g["ny"] <= g["budget"] == 1200 and 1.0 / g["inv"] > 10 * r      # the cells were widened
    far = np.abs(rows[:, :2].astype(np.float64)).max(axis=1) > br.SENSOR
    assert far.sum() > 150 and (~far).sum() >= 75 and (np.abs(rows[far, 0]) > 600).any()
    cen = centres[0].astype(np.float64)
    assert abs(cen[0, 0]) - br.SENSOR == 500 and (np.abs(cen[1, :2]) > br.SENSOR).all()
    count = e["count"][0, :, 0]
    assert (count[:6] > 0).all() and count[:4].max() > S and not count[6:].any() and (e["index"][0, 6:] == -1).all()
    assert not br.centre_usable(centres[0, 6:]).any() and br.centre_usable(centres[0, :6]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_and_degenerate_frames(dtype):
    rows, offsets, _, centres, (rng, radii, samples) = br.case("batch", dtype)
    e = br.expected("batch", dtype)
    assert np.diff(offsets).tolist() == [0, 1, 37, 300, 1500] and centres.shape == (5, 8, 4)
    assert not e["count"][0].any() and (e["index"][0] == -1).all() and e["count"][1].max() == 1 and e["count"][4].max() > 16
    for f in range(1, 5):
        got = e["index"][f][e["index"][f] >= 0]
        assert len(got) and got.min() >= offsets[f] and got.max() < offsets[f + 1]
    e = br.expected("unusable", dtype)
    assert not e["count"].any() and (e["index"] == -1).all() and not e["points"].any()
    rows, offsets, keep, centres, _ = br.case("absent", dtype)
    e = br.expected("absent", dtype)
    assert not keep[100:].any() and not e["count"][1].any() and (e["count"][0] > 0).sum() >= 6 and keep[e["index"][0][e["index"][0] >= 0]].all()
    e = br.expected("cluster", dtype)
    assert e["count"][0, :, 0].tolist() == [5000, 40, 0]
    g = br.grid(br.RANGE, (0.5,), 5040)
    rows, _, _, centres, _ = br.case("cluster", dtype)
    assert len(set(br.cells(g, rows[_d(rows, centres[0, 0]) < 0.01, :2]).tolist())) == 1          # 5000 rows in one cell


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_difference_of_coordinates_is_tiny(dtype):
    """Apart from the rows placed an ulp or 1e-9 beside the sphere, coordinates are multiples of 2^-10: no product of a distance is
    subnormal, so a device that flushed could not hide."""
    for name in br.CASES:
        rows, _, _, centres, _ = br.case(name, dtype)
        p = rows[np.isfinite(rows[:, :3]).all(axis=1), :3].astype(np.float64)
        assert (np.mod(p, br.STEP) == 0).mean() > 0.99, name


# ---- csrc/sg_ball.h on the host ---------------------------------------------------------------------------------------------------------------
def _compile(tmp, source, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra,
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / source),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def cells_harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("ball"), "ball_cells.cpp", "ball_cells")


def test_every_ball_lies_in_its_window(cells_harness):
    r = subprocess.run([str(cells_harness), "cover"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    word, settings, pairs = r.stdout.split()
    assert word == "cover" and int(settings) == 2 * 7 * 3 and int(pairs) > int(settings) * 1100000


def _walk(exe, tmp_path, rows, keep, centres, rng, radii, samples, dtype, max_frame, seed):
    fi, fk, fc, fo = (tmp_path / f"w.{s}" for s in ("in", "keep", "centres", "out"))
    np.ascontiguousarray(np.asarray(rows)[:, :3], np.float64).tofile(fi)
    (np.ones(len(rows), np.uint8) if keep is None else np.asarray(keep).astype(np.uint8)).tofile(fk)
    np.ascontiguousarray(np.asarray(centres)[:, :3], np.float64).tofile(fc)
    bounds = (0.0,) * 6 if rng is None else rng
    cmd = [str(exe), "walk", str(DTYPES.index(dtype)), str(int(rng is not None)), *(repr(float(v)) for v in bounds), str(max_frame), str(len(radii)),
           *(repr(float(v)) for v in radii), *(str(int(s)) for s in samples), str(fi), str(fk), str(fc), str(fo), str(seed)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    K, S, R = len(centres), sum(samples), len(radii)
    raw = np.fromfile(fo, np.int32)
    assert len(raw) == K * (S + R)
    return raw[:K * S].reshape(K, S), raw[K * S:].reshape(K, R), [int(w) for w in r.stdout.split()[1:]]


def _walk_case(exe, tmp_path, name, dtype, seeds, radii=None, samples=None):
    rows, offsets, keep, centres, (rng, r, s) = br.case(name, dtype)
    radii, samples = radii or r, samples or s
    want = br.expected(name, dtype, radii=radii, samples=samples)
    g = br.grid(rng, radii, int(np.diff(offsets).max()))
    for f, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        for seed in seeds:
            index, count, cells = _walk(exe, tmp_path, rows[a:b], None if keep is None else keep[a:b], centres[f], rng, radii, samples, dtype,
                                        int(np.diff(offsets).max()), seed)
            assert cells == [g["nx"], g["ny"]], (name, cells, g)                    # the Python restatement of the grid is the header's
            assert np.array_equal(np.where(index >= 0, index + a, -1), want["index"][f]), (name, dtype, f, seed)
            assert np.array_equal(count, want["count"][f]), (name, dtype, f, seed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_walk_equals_the_restatement(cells_harness, tmp_path, dtype):
    for name in br.CASES:
        _walk_case(cells_harness, tmp_path, name, dtype, (0, 1, 2))
    _walk_case(cells_harness, tmp_path, "constructed", dtype, (0, 3), radii=(0.5, 1.0, 2.5, 1000.0), samples=(1, 16, 64, 63))
    _walk_case(cells_harness, tmp_path, "cluster", dtype, (4,), radii=(0.01, 0.5), samples=(64, 1))


def test_selection_network_equals_a_sort(tmp_path):
    exe = _compile(tmp_path, "ball_select.cpp", "ball_select")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) == 5 * 12 * 3 * 2


def test_selection_network_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    exe = _compile(tmp_path, "ball_select.cpp", "ball_select_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok" and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-2000:]


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_ball_query_device"
APART = {"keep_in": " overlaps d_keep_in; the mask is read while the groups are written: pass a buffer apart from it",
         "rows": " overlaps d_rows; the rows are read while the groups are written: pass a buffer apart from them",
         "centres": " overlaps d_centres; the centres are read while the groups are written: pass a buffer apart from them"}
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "features": WHO + ": n_features must be 3, 4 or 5: the columns of a row that a neighbour carries",
    "centre_features": WHO + ": centre_features must be 3, 4 or 5: x, y, z first",
    "centres": WHO + ": n_centres must be at least 1",
    "n_radii": WHO + ": n_radii must lie in 1 .. 4",
    "radius": WHO + ": a radius must be finite, above 0 and at most 1e6",
    "samples": WHO + ": the samples of a radius must lie in 1 .. 64",
    "slots": WHO + ": n_frames * n_centres * samples exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "cells": WHO + ": too many frames for the cell lists; split the batch",
    "nan": WHO + ": a bound of the range is NaN; pass NULL for no range, or infinite bounds",
    "order": WHO + ": the range needs lo < hi on every axis",
    "index_keep": WHO + ": d_out_index" + APART["keep_in"],
    "count_keep": WHO + ": d_out_count" + APART["keep_in"],
    "points_keep": WHO + ": d_out_points" + APART["keep_in"],
    "index_rows": WHO + ": d_out_index" + APART["rows"],
    "count_rows": WHO + ": d_out_count" + APART["rows"],
    "points_rows": WHO + ": d_out_points" + APART["rows"],
    "index_centres": WHO + ": d_out_index" + APART["centres"],
    "count_centres": WHO + ": d_out_count" + APART["centres"],
    "points_centres": WHO + ": d_out_points" + APART["centres"],
}
ACCEPTED = ("clean", "null_out_points", "null_keep_in", "null_range", "float64", "empty_null_rows", "features_3", "features_5", "centre_features_5",
            "radii_1", "radii_4", "radius_1e6", "radius_tiny", "samples_1", "samples_64", "slots_2p31_minus_1", "frame_2p30_rows", "cell_lists_fit",
            "range_infinite", "keep_in_behind_index", "index_behind_rows", "index_behind_centres", "count_is_index")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_centres", "null_radii", "null_samples", "null_out_index", "null_out_count", "bad_dtype", "no_frames",
             "negative_rows", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_features_2"),
    "features": ("features_2", "features_6", "features_2_and_centre_features_2"),
    "centre_features": ("centre_features_2", "centre_features_6", "centre_features_2_and_centres_0"),
    "centres": ("centres_0", "centres_negative", "centres_0_and_radii_0"),
    "n_radii": ("radii_0", "radii_5", "radii_5_and_radius_0"),
    "radius": ("radius_0", "radius_negative", "radius_nan", "radius_inf", "radius_above_1e6", "radius_0_and_samples_0"),
    "samples": ("samples_0", "samples_65"),
    "slots": ("slots_2p31", "slots_overflowing", "slots_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_cell_lists_too_large"),
    "cells": ("cell_lists_too_large", "cell_lists_too_large_and_range_nan"),
    "nan": ("range_nan_lo", "range_nan_hi", "range_nan_and_range_reversed"),
    "order": ("range_reversed", "range_lo_is_hi", "range_reversed_and_index_is_keep_in"),
    "index_keep": ("index_is_keep_in", "index_overlaps_keep_in"),
    "count_keep": ("count_overlaps_keep_in",),
    "points_keep": ("points_overlap_keep_in",),
    "index_rows": ("index_overlaps_rows",),
    "count_rows": ("count_overlaps_rows",),
    "points_rows": ("points_are_rows",),
    "index_centres": ("index_overlaps_centres",),
    "count_centres": ("count_is_centres",),
    "points_centres": ("points_overlap_centres",),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "ball_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "ball_refusals.cpp"), "-o", str(exe)]
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
    assert "int snowgpu_ball_query_device(" in header and "snowgpu_ball_query_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_ball_query_device") and hasattr(_native.Context, "ball_query_device")
    assert "snowgpu_ball.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import ball, tensors
    assert callable(tensors.ball_query) and callable(tensors.NeighbourBatch.empty) and callable(ball.ball_query)
