"""Point-to-voxel grouping without a GPU: the conditions under which the comparisons of tests/test_gpu_voxelize.py are not vacuous, asserted
on the shared inputs of tests/voxel_reference.py; the cell arithmetic and the table of open cells of csrc/sg_voxel.h, compiled for the host
(tests/host_harness/voxel_cells.cpp, once more under the address and undefined-behaviour sanitizers as a stand-alone program), against
the restatement; and what snowgpu_voxelize_device refuses, in which words (tests/host_harness/voxel_refusals.cpp)."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import voxel_reference as vr
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = vr.DTYPES


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_frame_meets_the_conditions(dtype):
    rows, _, _, (rng, size, T, V) = vr.case("constructed", dtype)
    e = vr.expected("constructed", dtype)
    ok, c = vr.cells(rows, rng, size)
    assert rows.shape == (6000, 5) and (T, V) == (8, 300)
    assert len({tuple(x) for x in c[ok]}) > V and e["voxel_offsets"][1] == V
    per = e["rows_per_voxel"][:V]
    assert (per > T).sum() >= 16 and (per == T).sum() >= 16 and ((per < T) & (per > 0)).sum() >= 16, per
    assert (~ok).sum() >= 16 and np.isnan(rows[:, :3]).any(axis=1).sum() >= 16
    dropped = ok & (e["voxel_of"] < 0)
    assert dropped.sum() >= 16                                   # rows of cells beyond V
    on_face = ok & (rows[:, 0] == np.rint(rows[:, 0]))
    assert on_face.sum() >= 16 and np.array_equal(c[on_face, 0], rows[on_face, 0].astype(np.int64))      # the upper cell's
    assert np.array_equal(e["num_points"][:V], np.minimum(per, T)) and not e["num_points"][V:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("faces", "faces_second"))
def test_face_rows(name, dtype):
    """On lo_j and on an inner face: the upper cell; one ulp below: the lower cell, or out below lo_j (unless the float64
    subtraction of the definition absorbs the ulp); on hi_j and beyond: out -- wherever the quotient is exact, as it is for the unit grid."""
    rows, _, _, (rng, size, _, _) = vr.case(name, dtype)
    ok, c = vr.cells(rows, rng, size)
    n = vr.grid_dims(rng, size)
    assert n == ((40, 40, 4) if name == "faces" else (1408, 1600, 40))
    assert ok.sum() >= 16 and (~ok).sum() >= 6
    seen = {j: set() for j in range(3)}
    for i in range(0, len(rows), 3):                              # triples: one ulp below, on, one ulp above
        j = int(rows[i, 4])
        below, on, above = (float(rows[i + k, j]) for k in range(3))
        assert below < on < above
        if name == "faces":
            k = on - rng[j]
            assert k == int(k)
            k = int(k)
            kb = k if np.float64(below) - rng[j] == k else k - 1      # (the float64 subtraction may absorb the ulp: the definition's answer)
            assert bool(ok[i]) == (0 <= kb < n[j]) and bool(ok[i + 1]) == bool(ok[i + 2]) == (0 <= k < n[j]), (i, k)
            if ok[i]:
                assert c[i, j] == kb
            if ok[i + 1]:
                assert c[i + 1, j] == c[i + 2, j] == k
            seen[j].add(k)
    if name == "faces":
        for j in range(3):
            assert {0, 1, n[j] - 1, n[j]} <= seen[j]
    e = vr.expected(name, dtype)
    assert e["voxel_offsets"][1] == len({tuple(x) for x in c[ok]}) >= 16


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_usable_row_its_own_voxel(dtype):
    rows, _, _, _ = vr.case("own_voxel", dtype)
    e = vr.expected("own_voxel", dtype)
    usable = int(e["usable"].sum())
    assert rows.shape[0] == 4096 and usable == 1302 and e["voxel_offsets"][1] == usable
    assert np.array_equal(e["voxel_of"][e["usable"]], np.arange(usable)) and (e["num_points"][:usable] == 1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_of_frames(dtype):
    rows, offsets, keep, (_, _, T, V) = vr.case("batch", dtype)
    assert np.array_equal(np.diff(offsets), (6000, 0, 1500, 300)) and all(int(o) % 64 for o in offsets[1:])
    assert not keep[offsets[3]:].any() and 0.7 < keep[:offsets[3]].mean() < 0.9
    assert rows[2000:3500].tobytes() == rows[6000:7500].tobytes()      # the same coordinates in two frames
    e, e0 = vr.expected("batch", dtype), vr.expected("batch_nokeep", dtype)
    m, m0 = np.diff(e["voxel_offsets"]), np.diff(e0["voxel_offsets"])
    assert m[0] == V and m[1] == 0 and 16 <= m[2] <= V and m[3] == 0 and m0[3] >= 16
    assert (e["voxel_of"][~keep] == -1).all() and (e["voxel_of"][offsets[3]:] == -1).all()
    a, b = e["voxel_offsets"][2], e["voxel_offsets"][3]
    assert (e["coords"][a:b, 0] == 2).all() and (e["coords"][b:] == -1).all() and not e["voxels"][b:].any()
    assert not np.array_equal(e["voxel_of"], e0["voxel_of"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_voxels_straddle_blocks(dtype):
    """Channel-major order puts the rows of one voxel more than 4096 rows apart; firing order keeps them close.  Same cells either way."""
    spans = {}
    for name in ("straddle", "straddle_firing"):
        e = vr.expected(name, dtype)
        vo, m = e["voxel_of"], int(e["voxel_offsets"][1])
        rows_of = np.flatnonzero(vo >= 0)
        first = np.full(m, len(vo)); last = np.zeros(m, np.int64)
        np.minimum.at(first, vo[rows_of], rows_of)
        np.maximum.at(last, vo[rows_of], rows_of)
        spans[name] = int((last - first).max())
        assert m >= 1000 and (e["rows_per_voxel"][:m] > 32).sum() >= 16
    assert spans["straddle"] > 4096 > spans["straddle_firing"]
    a, b = vr.expected("straddle", dtype), vr.expected("straddle_firing", dtype)
    cells = lambda e: sorted(map(tuple, e["coords"][:e["voxel_offsets"][1]].tolist()))
    assert cells(a) == cells(b) and not np.array_equal(a["coords"], b["coords"])


# ---- csrc/sg_voxel.h on the host --------------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra,
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "voxel_cells.cpp"),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("voxel"), "voxel_cells")


@pytest.fixture(scope="module")
def harness_sanitized(tmp_path_factory):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    return _compile(tmp_path_factory.mktemp("voxel_san"), "voxel_cells_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _run(exe, mode, rows, rng, size, tmp_path, tag, seed=None):
    fi, fo = tmp_path / f"{tag}.in", tmp_path / f"{tag}.out"
    np.ascontiguousarray(np.asarray(rows)[:, :3], np.float64).tofile(fi)
    cmd = [str(exe), mode, *(repr(float(v)) for v in rng), *(repr(float(v)) for v in size), str(fi), str(fo)] + ([str(seed)] if seed is not None else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.fromfile(fo, np.int32), r.stdout.split()


def _check_against_restatement(exe, tmp_path, names, seeds):
    for dtype in DTYPES:
        for name in names:
            rows, offsets, _, (rng, size, _, _) = vr.case(name, dtype)
            ok, c = vr.cells(rows, rng, size)
            n = vr.grid_dims(rng, size)
            key = np.where(ok, (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0], -1)
            got, words = _run(exe, "cells", rows, rng, size, tmp_path, f"{name}_{dtype}")
            assert words == ["dims", *map(str, n)] and np.array_equal(got, key), (name, dtype)
            # one frame's table, fed in a scrambled order: the smallest row of every cell
            first = {}
            for i in np.flatnonzero(ok):
                first.setdefault(int(key[i]), int(i))
            want = np.array([first[int(k)] if k >= 0 else -1 for k in key], np.int32)
            for seed in seeds:
                got, words = _run(exe, "table", rows, rng, size, tmp_path, f"{name}_{dtype}_t", seed)
                assert np.array_equal(got, want), (name, dtype, seed)
                assert int(words[3]) == len(first) and int(words[1]) >= 2 * len(rows) and int(words[1]) & (int(words[1]) - 1) == 0


def test_host_cells_and_table_equal_the_restatement(harness, tmp_path):
    _check_against_restatement(harness, tmp_path, vr.CASES, (1, 2, 3))


def test_host_cells_and_table_under_sanitizers(harness_sanitized, tmp_path):
    _check_against_restatement(harness_sanitized, tmp_path, ("constructed", "faces_second", "own_voxel"), (5,))


def test_host_grid_domain(harness, tmp_path):
    rows = vr.case("faces", "float64")[0]
    for rng, size in (((0, 0, 0, 1, 1, 1), (1, 1, 0)), ((0, 0, 0, 0.25, 1, 1), (1, 1, 1)), ((0, 0, 0, 2147483647, 1, 1), (1, 1, 1))):
        fi = tmp_path / "d.in"
        np.ascontiguousarray(rows[:, :3], np.float64).tofile(fi)
        r = subprocess.run([str(harness), "cells", *(repr(float(v)) for v in rng), *(repr(float(v)) for v in size), str(fi), str(tmp_path / "d.out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 3, (rng, size)


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_voxelize_device"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "features": WHO + ": n_features must be 3, 4 or 5: the columns of a row that a voxel stores",
    "least_1": WHO + ": max_points and max_voxels must be at least 1",
    "size": WHO + ": every voxel size must be positive and finite",
    "axis": WHO + ": the range must be finite and hold at least one voxel on every axis (llround((hi - lo) / size) >= 1)",
    "cells": WHO + ": the grid has more than 2^31 - 2 cells; a cell's index is kept in 31 bits",
    "slots": WHO + ": n_frames * max_voxels exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "overlap": WHO + ": d_out_voxel_of overlaps d_keep_in; the keep-in bytes of other rows are read while it is written: pass a buffer apart from it",
}
OK_4_4_2 = ("clean", "null_out_voxel_of", "null_keep_in", "float64", "empty_null_buffers", "features_3", "features_5", "points_1", "voxels_1",
            "frames_times_voxels_2p31_minus_1", "frame_2p30_rows", "voxel_of_behind_keep_in", "keep_in_behind_voxel_of", "coords_are_num_points")
OK_OTHER = {"axis_half_cell": "1 4 2", "cells_2p31_minus_2": "2147483646 1 1", "cells_2p31_minus_2_as_product": "46341 46339 1"}
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_range", "null_size", "null_out_voxels", "null_out_coords", "null_out_num_points",
             "null_out_voxel_offsets", "bad_dtype", "no_frames", "negative_rows", "empty_null_voxel_offsets", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_features_2"),
    "features": ("features_2", "features_6", "features_2_and_points_0"),
    "least_1": ("points_0", "voxels_0", "voxels_negative", "points_0_and_size_zero"),
    "size": ("size_zero", "size_negative", "size_inf", "size_nan", "size_zero_and_axis_without_cell"),
    "axis": ("axis_without_cell", "range_reversed", "range_inf", "range_nan", "range_reversed_and_cells_1e30"),
    "cells": ("cells_2p31_minus_1", "cells_product_too_large", "cells_1e30", "cells_1e30_and_frames_times_voxels_2p31"),
    "slots": ("frames_times_voxels_2p31", "frames_times_voxels_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_voxel_of_is_keep_in"),
    "overlap": ("voxel_of_is_keep_in", "voxel_of_overlaps_keep_in"),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "voxel_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "voxel_refusals.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split("|", 1) for ln in r.stdout.splitlines())
    want = {case: "0|OK|4 4 2" for case in OK_4_4_2}
    want.update({case: "0|OK|" + dims for case, dims in OK_OTHER.items()})
    for key, cases in REFUSED.items():
        want.update({case: "1|" + MESSAGES[key] + "|0 0 0" for case in cases})
    assert got == want


def test_the_entry_is_declared_and_bound():
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_voxelize_device(" in header and "snowgpu_voxelize_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_voxelize_device")
    assert "snowgpu_voxel.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
