"""Nearest centres without a GPU: the conditions under which the comparisons of tests/test_gpu_nearest.py are not vacuous, asserted on the
shared inputs of tests/nn_reference.py; csrc/sg_nn.h compiled for the host (tests/host_harness/nn_walk.cpp) -- whole frames through the
filing and the ring walk, with the order inside the cells scrambled, against the restatement; the stopping bound over millions of
(row, visited block, outside centre) triples; the k-best insertion against a sort -- once more under the address and
undefined-behaviour sanitizers as a stand-alone program; and what snowgpu_nearest_centres_device refuses, in which words
(tests/host_harness/nn_refusals.cpp)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import nn_reference as nr
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = nr.DTYPES
FRAME = nr.FRAME


def _d(row, centres):
    return nr.distances(np.ascontiguousarray(row[None, :3]), np.ascontiguousarray(centres[:, :3]))[0]


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_batch_meets_the_conditions(dtype):
    rows, offsets, keep, centres, rng = nr.case("constructed", dtype)
    sp = nr.special(dtype)
    e = nr.expected("constructed", dtype, 3)
    g = nr.grid(rng, centres.shape[1])
    assert centres.shape == (11, nr.CONSTRUCTED_K, 3) and (g["nx"], g["ny"], g["edge"]) == (4, 4, 4.0) and g["budget"] == 16
    with np.errstate(invalid="ignore"):
        cell = lambda p: tuple(int(v[0]) for v in nr.cells(g, np.asarray(p, np.float64)[None, :2]))
    # two centres at bitwise equal d: the larger number in the row's own cell, the smaller two rings out; the smaller comes first
    i, c = sp["tie"], centres[FRAME["tie"]]
    d = _d(rows[i], c)
    assert d[0].tobytes() == d[5].tobytes() and d[0] == 64 and cell(c[5]) == cell(rows[i]) and cell(c[0])[0] - cell(rows[i])[0] == 2
    assert e["index"][i].tolist() == [0, 5, 2] and np.nanmin(np.delete(d, [0, 5])) > 64
    # a row an ulp inside its cell's edge: the nearest centre across the edge, a farther decoy in the row's cell
    i, c = sp["edge"], centres[FRAME["edge"]]
    assert rows[i, 0] == np.nextafter(rows.dtype.type(8), rows.dtype.type(0)) and cell(rows[i]) == cell(c[1]) and cell(c[0])[0] == cell(rows[i])[0] + 1
    assert e["index"][i, :2].tolist() == [0, 1] and _d(rows[i], c)[1] > 8
    # centres exactly on cell boundaries and on the domain's corners
    c = centres[FRAME["boundaries"]].astype(np.float64)
    assert all(((c[j, :2] - (g["x0"], g["y0"])) * g["inv"] % 1.0 == 0).all() for j in range(8))
    assert {tuple(c[j, :2]) for j in range(4, 8)} == {(rng[0], rng[1]), (rng[3], rng[4]), (rng[0], rng[4]), (rng[3], rng[1])}
    # a row that coincides with a centre, and duplicate centres in centre order
    i = sp["duplicates"]
    assert e["index"][i].tolist() == [3, 7, 9] and not e["dist2"][i].any() and (e["weight"][i] == rows.dtype.type(1 / 3)).all()
    assert e["index"][i + 1, 0] == -1 and not keep[i + 1]                            # an absent row between them
    # frames with 0, 1, k - 1 and k usable centres, of 0 rows and of 1 row
    usable = nr.centre_usable(centres).sum(axis=1)
    assert [int(usable[FRAME[n]]) for n in ("no_centre", "one_centre", "two_centres", "three_centres")] == [0, 1, 2, 3]
    assert not np.isfinite(centres[FRAME["no_centre"], :5]).all(axis=1).all() and np.isinf(centres[FRAME["no_centre"]]).any()
    for name, m in (("no_centre", 0), ("one_centre", 1), ("two_centres", 2), ("three_centres", 3)):
        a, b = offsets[FRAME[name]], offsets[FRAME[name] + 1]
        assert b - a == 20 and ((e["index"][a:b] >= 0).sum(axis=1) == m).all() and (np.isinf(e["dist2"][a:b]).sum(axis=1) == 3 - m).all(), name
        assert (e["weight"][a:b][:, m:] == 0).all()
    assert np.diff(offsets)[FRAME["no_row"]] == 0 and np.diff(offsets)[FRAME["one_row"]] == 1
    # the order of a row's neighbours differs between float32 and float64
    both = [nr.expected("constructed", t, 3)["index"][nr.special(t)["dtype"], :2].tolist() for t in DTYPES]
    assert both == [[0, 1], [1, 0]]
    # non-finite and out-of-range rows, and absent rows
    i = sp["dtype"]
    assert np.isnan(rows[i + 1, 0]) and rows[i + 2, 2] > nr.BOUND and rows[i + 3, 1] == rng[4] and rows[i + 4, 0] < rng[0] and np.isinf(rows[i + 5, 2])
    assert (e["index"][i + 1:i + 6] == -1).all() and np.isinf(e["dist2"][i + 1:i + 6]).all() and not e["weight"][i + 1:i + 6].any()
    assert (~keep).sum() == 41 and (e["index"][~keep] == -1).all() and (e["index"][keep][:, 0] >= 0).sum() > 700


@pytest.mark.parametrize("dtype", DTYPES)
def test_far_rows_clusters_and_the_domain(dtype):
    # rows and centres beyond the domain: no range, 600 m out, and centres that are not usable
    rows, _, _, centres, rng = nr.case("beyond", dtype)
    e = nr.expected("beyond", dtype, 3)
    assert rng is None and len(rows) == 300 and centres.shape == (1, 24, 3)
    far = np.abs(rows[:, :2].astype(np.float64)).max(axis=1) > nr.SENSOR
    assert far.sum() >= 170 and (np.abs(rows[far, 0]) > 600).sum() > 50 and (np.abs(centres[0, :20, :2]).max(axis=1) > nr.SENSOR).sum() >= 12
    assert not nr.centre_usable(centres[0, 20:]).any() and (e["index"] < 20).all() and (e["index"] >= 0).all()
    assert len(set((e["index"][:, 0] // 4).tolist())) == 5                           # every cluster of rows finds its own centres
    # all centres in one corner cell, rows in the opposite corner
    rows, _, _, centres, rng = nr.case("corner", dtype)
    g = nr.grid(rng, centres.shape[1])
    cx, cy = nr.cells(g, centres[0, :, :2])
    rx, ry = nr.cells(g, rows[:500, :2])
    assert set(cx.tolist()) == {0} and set(cy.tolist()) == {0} and set(rx.tolist()) == {g["nx"] - 1} and set(ry.tolist()) == {g["ny"] - 1} and g["nx"] >= 4
    # 5000 centres in one cell of the largest grid
    rows, _, _, centres, rng = nr.case("cluster", dtype)
    g = nr.grid(rng, centres.shape[1])
    cx, cy = nr.cells(g, centres[0, :, :2])
    assert centres.shape[1] == 5000 and g["budget"] == nr.MAX_CELLS and 0.9 * nr.MAX_CELLS < g["nx"] * g["ny"] <= nr.MAX_CELLS
    assert len(set(cx.tolist())) == 1 and len(set(cy.tolist())) == 1
    assert nr.grid(nr.RANGE, 4096)["budget"] == nr.MAX_CELLS and nr.grid(nr.RANGE, 1)["budget"] == nr.MIN_CELLS
    # frames of the batch
    rows, offsets, _, centres, _ = nr.case("batch", dtype)
    e = nr.expected("batch", dtype, 3)
    assert np.diff(offsets).tolist() == [0, 1, 37, 300, 1500] and (e["index"] >= 0).all() and (e["dist2"][:, 0] == 0).sum() >= 6 * 3 + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_difference_of_coordinates_is_tiny(dtype):
    """Apart from the points placed an ulp or 1e-9 beside something, coordinates are multiples of 2^-11 (the cluster's rows sit half a
    step above its centres): no product of a distance is subnormal, so a device that flushed could not hide."""
    for name in nr.CASES:
        rows, _, _, centres, _ = nr.case(name, dtype)
        for a in (rows[:, :3], centres.reshape(-1, centres.shape[-1])[:, :3]):
            p = a[np.isfinite(a).all(axis=1)].astype(np.float64)
            assert (np.mod(p, nr.STEP / 2) == 0).mean() > 0.99, name


def test_weights_of_the_restatement():
    index = np.array([[4, 2, -1], [-1, -1, -1], [0, 1, 2]], np.int32)
    dist2 = np.array([[0.0, 4.0, np.inf], [np.inf] * 3, [1.0, 1.0, 4.0]], np.float32)
    w = nr.weights(index, dist2)
    u0, u1 = 1.0 / 1e-8, 1.0 / (2.0 + 1e-8)
    assert w.dtype == np.float32 and w[0].tolist() == [np.float32(u0 / (u0 + u1)), np.float32(u1 / (u0 + u1)), 0.0] and not w[1].any()
    assert abs(float(w[2].sum()) - 1) < 1e-6 and w[2, 0] == w[2, 1] > w[2, 2]


# ---- csrc/sg_nn.h on the host -----------------------------------------------------------------------------------------------------------------
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
def harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("nn"), "nn_walk.cpp", "nn_walk")


def _walk(exe, tmp_path, rows, keep, centres, rng, k, dtype, seed):
    fi, fk, fc, fo = (tmp_path / f"w.{s}" for s in ("in", "keep", "centres", "out"))
    np.ascontiguousarray(np.asarray(rows)[:, :3], np.float64).tofile(fi)
    (np.ones(len(rows), np.uint8) if keep is None else np.asarray(keep).astype(np.uint8)).tofile(fk)
    np.ascontiguousarray(np.asarray(centres)[:, :3], np.float64).tofile(fc)
    bounds = (0.0,) * 6 if rng is None else rng
    cmd = [str(exe), "walk", str(DTYPES.index(dtype)), str(int(rng is not None)), *(repr(float(v)) for v in bounds), str(len(centres)), str(k),
           str(fi), str(fk), str(fc), str(fo), str(seed)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    n, t = len(rows), np.dtype(dtype)
    raw = fo.read_bytes()
    assert len(raw) == n * k * (4 + 2 * t.itemsize)
    index = np.frombuffer(raw, np.int32, n * k).reshape(n, k)
    dist2 = np.frombuffer(raw, t, n * k, n * k * 4).reshape(n, k)
    weight = np.frombuffer(raw, t, n * k, n * k * (4 + t.itemsize)).reshape(n, k)
    return dict(index=index, dist2=dist2, weight=weight), [int(w) for w in r.stdout.split()[1:]]


def _walk_case(exe, tmp_path, name, dtype, ks, seeds):
    rows, offsets, keep, centres, rng = nr.case(name, dtype)
    g = nr.grid(rng, centres.shape[1])
    for k in ks:
        want = nr.expected(name, dtype, k)
        for f, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
            for seed in seeds:
                got, cells = _walk(exe, tmp_path, rows[a:b], None if keep is None else keep[a:b], centres[f], rng, k, dtype, seed)
                assert cells == [g["nx"], g["ny"]], (name, cells, g)                  # the Python restatement of the grid is the header's
                for field in ("index", "dist2", "weight"):
                    assert got[field].tobytes() == want[field][a:b].tobytes(), (name, dtype, k, f, seed, field)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_walk_equals_the_restatement(harness, tmp_path, dtype):
    _walk_case(harness, tmp_path, "constructed", dtype, (1, 2, 3, 8), (0, 1))
    _walk_case(harness, tmp_path, "batch", dtype, (1, 3, 5), (2,))
    for name in ("beyond", "corner", "cluster"):
        _walk_case(harness, tmp_path, name, dtype, (3,), (3,))
    _walk_case(harness, tmp_path, "sized4096", dtype, (3,), (4,))


def test_the_stopping_bound_holds(harness):
    r = subprocess.run([str(harness), "bound", "1", "3"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    word, triples = r.stdout.split()
    assert word == "bound" and int(triples) >= 6_000_000


def test_insertion_equals_a_sort(harness):
    r = subprocess.run([str(harness), "insert"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["insert", str(2 * 8 * 400)], r.stdout[-2000:] + r.stderr[-2000:]


def test_harness_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    exe = _compile(tmp_path, "nn_walk.cpp", "nn_walk_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for args in (("insert",), ("bound", "2", "0.3")):
        r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.split()[0] == args[0] and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-2000:]
    rows, offsets, keep, centres, rng = nr.case("constructed", "float32")
    for f in (FRAME["tie"], FRAME["boundaries"], FRAME["no_centre"], FRAME["no_row"]):
        a, b = offsets[f], offsets[f + 1]
        got, _ = _walk(exe, tmp_path, rows[a:b], keep[a:b], centres[f], rng, 3, "float32", 5)
        assert np.array_equal(got["index"], nr.expected("constructed", "float32", 3)["index"][a:b])
    rows, _, _, centres, rng = nr.case("beyond", "float64")
    got, _ = _walk(exe, tmp_path, rows, None, centres[0], rng, 8, "float64", 6)
    assert np.array_equal(got["index"], nr.expected("beyond", "float64", 8)["index"])


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_nearest_centres_device"
APART = {"keep_in": " overlaps d_keep_in; the mask is read while the neighbours are written: pass a buffer apart from it",
         "rows": " overlaps d_rows; the rows are read while the neighbours are written: pass a buffer apart from them",
         "centres": " overlaps d_centres; the centres are read while the neighbours are written: pass a buffer apart from them"}
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "centre_features": WHO + ": centre_features must be 3, 4 or 5: x, y, z first",
    "centres": WHO + ": n_centres must be at least 1",
    "k": WHO + ": k must lie in 1 .. 8",
    "slots": WHO + ": n_frames * n_centres exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "cells": WHO + ": too many frames for the cell lists; split the batch",
    "nan": WHO + ": a bound of the range is NaN; pass NULL for no range, or infinite bounds",
    "order": WHO + ": the range needs lo < hi on every axis",
    "index_keep": WHO + ": d_out_index" + APART["keep_in"],
    "dist2_keep": WHO + ": d_out_dist2" + APART["keep_in"],
    "weight_keep": WHO + ": d_out_weight" + APART["keep_in"],
    "index_rows": WHO + ": d_out_index" + APART["rows"],
    "dist2_rows": WHO + ": d_out_dist2" + APART["rows"],
    "weight_rows": WHO + ": d_out_weight" + APART["rows"],
    "index_centres": WHO + ": d_out_index" + APART["centres"],
    "dist2_centres": WHO + ": d_out_dist2" + APART["centres"],
    "weight_centres": WHO + ": d_out_weight" + APART["centres"],
    "dist2_index": WHO + ": d_out_dist2 overlaps d_out_index" + OWN,
    "weight_index": WHO + ": d_out_weight overlaps d_out_index" + OWN,
    "weight_dist2": WHO + ": d_out_weight overlaps d_out_dist2" + OWN,
}
ACCEPTED = ("clean", "null_out_weight", "null_keep_in", "null_range", "float64", "empty_null_rows_and_outputs", "centre_features_5", "k_1", "k_8",
            "centres_2p31_minus_1", "frame_2p30_rows", "cell_lists_fit", "range_infinite", "keep_in_behind_index", "index_behind_rows",
            "index_behind_centres", "weight_behind_dist2")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_centres", "null_out_index", "null_out_dist2", "bad_dtype", "no_frames", "negative_rows", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_centre_features_2"),
    "centre_features": ("centre_features_2", "centre_features_6", "centre_features_2_and_centres_0"),
    "centres": ("centres_0", "centres_negative", "centres_0_and_k_0"),
    "k": ("k_0", "k_9", "k_negative", "k_0_and_centres_2p31"),
    "slots": ("centres_2p31", "centres_overflowing", "centres_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_cell_lists_too_large"),
    "cells": ("cell_lists_too_large", "cell_lists_too_large_and_range_nan"),
    "nan": ("range_nan_lo", "range_nan_hi", "range_nan_and_range_reversed"),
    "order": ("range_reversed", "range_lo_is_hi", "range_reversed_and_index_is_keep_in"),
    "index_keep": ("index_is_keep_in", "index_overlaps_keep_in"),
    "dist2_keep": ("dist2_overlaps_keep_in",),
    "weight_keep": ("weight_overlaps_keep_in",),
    "index_rows": ("index_overlaps_rows",),
    "dist2_rows": ("dist2_is_rows",),
    "weight_rows": ("weight_overlaps_rows",),
    "index_centres": ("index_overlaps_centres",),
    "dist2_centres": ("dist2_is_centres",),
    "weight_centres": ("weight_overlaps_centres",),
    "dist2_index": ("dist2_is_index",),
    "weight_index": ("weight_overlaps_index",),
    "weight_dist2": ("weight_is_dist2",),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "nn_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "nn_refusals.cpp"), "-o", str(exe)]
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
    assert "int snowgpu_nearest_centres_device(" in header and "snowgpu_nearest_centres_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_nearest_centres_device") and hasattr(_native.Context, "nearest_centres_device")
    assert "snowgpu_nn.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import nearest, tensors
    assert callable(tensors.nearest_keypoints) and callable(tensors.NearestBatch.empty) and callable(nearest.three_nn)
    for method in ("flat_index", "interpolate", "nearest"):
        assert callable(getattr(tensors.NearestBatch, method))
