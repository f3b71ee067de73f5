"""RoI-aware voxel pooling without a GPU: the restatement (tests/roiaware_reference.py) against tests/roipool_reference.py where the two
overlap; the conditions under which the comparisons of tests/test_gpu_roiaware.py are not vacuous, asserted on the shared inputs; what
snowgpu_roi_voxel_pool_device refuses, in which words (tests/host_harness/roiaware_refusals.cpp); csrc/sg_roiaware.h's voxel function on
the host against the NumPy rule (tests/host_harness/roiaware_voxel.cpp); and that the entry is declared and bound."""
import itertools
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import roiaware_reference as ra
import roipool_reference as rr
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
R = ra.ROI


def _lists(c, f, m, grid, P=8192, ew=(0.0, 0.0, 0.0), keep=None):
    a, b = (int(v) for v in c["offsets"][f:f + 2])
    at, vox = ra.roi_lists(c["rows"][a:b], c["rois"][f, m], c["pose"][f, m], grid, P, ew, None if keep is None else keep[a:b])
    return a + at, vox


# ---- the restatement against roipool_reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("small_grid", "double_one", "capacity"))
def test_restatement_agrees_with_roipool_reference(name):
    """roi_count is the point pooling's count, and the voxel lists of a roi are a partition of its first P members, each in row order."""
    dtype, out_size, T, Cf, P, masked, ew = ra.SETTINGS[name]
    c = ra.case(dtype)
    e = ra.pool_setting(name, T=128)                                       # (above every voxel's count but the big roi's: checked below)
    S = 1100
    point = rr.roi_point_pool(c["rows"], c["rois"], c["pose"], S, 3, ew, c["keep"] if masked else None, c["offsets"])
    assert np.array_equal(e["roi_count"], point["count"]) and point["count"].max() < S and e["pose"].tobytes() == point["pose"].tobytes()
    assert np.array_equal(e["count"].sum(axis=-1), np.minimum(point["count"], P))
    F, M = c["rois"].shape[:2]
    checked = 0
    for f in range(F):
        for m in range(M):
            if (e["count"][f, m] > 128).any():
                continue
            idx = e["index"][f, m]
            union = np.sort(idx[idx >= 0])
            assert np.array_equal(union, point["index"][f, m, :min(point["count"][f, m], P)])
            assert all((np.diff(row[row >= 0]) > 0).all() for row in idx) and np.array_equal((idx >= 0).sum(axis=-1), e["count"][f, m])
            checked += len(union) > 0
    assert checked > 50


def test_the_restatement_on_a_case_by_hand():
    rois = np.array([[[0, 0, 0, 4, 2, 2, 0, 1], [0, 0, 0, 0, 2, 2, 0, 1]]], np.float64)
    rows = np.array([[-1.5, -0.5, -0.5, 0, 0], [1.5, 0.5, 0.5, 0, 0], [-0.5, -0.9, -1.0, 0, 0], [0.0, 0.0, 0.0, 0, 0], [1.9, 0.9, 1.0, 0, 0], [3, 0, 0, 0, 0]], np.float64)
    feats = np.array([[1.0], [2.0], [7.0], [np.nan], [2.0], [100.0]], np.float32)
    e = ra.roi_voxel_pool(rows, rois, rr.br.numpy_pose(rois), (2, 1, 2), 2, 64, feats)
    assert e["roi_count"].tolist() == [[5, 0]] and e["count"][0, 0].tolist() == [2, 0, 0, 3] and not e["count"][0, 1].any()
    assert e["index"][0, 0].tolist() == [[0, 2], [-1, -1], [-1, -1], [1, 3]]                # the third member of the last voxel is not pooled
    assert e["max"][0, 0, :, 0].tolist() == [7.0, 0.0, 0.0, 2.0] and e["argmax"][0, 0, :, 0].tolist() == [2, -1, -1, 1]
    assert e["avg"][0, 0, 0, 0] == 4.0 and np.isnan(e["avg"][0, 0, 3, 0]) and e["avg"][0, 0, 1, 0] == 0.0


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
def test_shapes_of_the_shared_input():
    c = ra.case("float32")
    n = np.diff(c["offsets"])
    assert n.tolist() == [901, 0, 602] and n[0] > ra.RUN and c["rois"].shape == (3, ra.M, 8) and ra.M > 64 and 1400 < n.sum() < 1600
    assert set(c["features"]) == {1, 5, 8, 65} and {s[1] for s in ra.SETTINGS.values()} == {(2, 3, 4), 12}
    assert {s[2] for s in ra.SETTINGS.values()} == {1, 4} and {s[3] for s in ra.SETTINGS.values()} == {1, 5, 8, 65, None} and ra.SETTINGS["capacity"][4] == 64


@pytest.mark.parametrize("dtype", ra.DTYPES)
@pytest.mark.parametrize("grid", ra.GRIDS)
def test_rows_on_planes_faces_and_in_the_margin(grid, dtype):
    """In exact arithmetic: the planes roi has pose (1, 0) and dyadic centre and sizes, so lx, ly, sz and every quotient below are exact."""
    c = ra.case(dtype)
    m = R["planes"]
    cx, cy, cz, dx, dy, dz = (Fraction(float(v)) for v in c["rois"][0, m, :6])
    assert c["pose"][0, m].tolist() == [1.0, 0.0]
    at, vox = _lists(c, 0, m, grid)
    voxel = dict(zip(at.tolist(), vox.tolist()))
    on_plane, clamped = set(), set()
    for name, i in ra.PLANE_AT.items():
        assert i in voxel, name                                            # a member
        x, y, z = (Fraction(float(v)) for v in c["rows"][i, :3])
        u = [(x - cx + dx / 2) / (dx / grid[0]), (y - cy + dy / 2) / (dy / grid[1]), (z - cz + dz / 2) / (dz / grid[2])]
        want = [min(max(v.numerator // v.denominator, 0), g - 1) for v, g in zip(u, grid)]
        assert voxel[i] == (want[0] * grid[1] + want[1]) * grid[2] + want[2], name
        for axis, (v, g) in enumerate(zip(u, grid)):
            if v.denominator == 1 and 0 < v < g:
                on_plane.add(axis)                                         # exactly on an interior plane: the upper voxel
            if v < 0:
                clamped.add((axis, "low"))
            if v >= g:
                clamped.add((axis, "high"))
    assert on_plane == {0, 1, 2}
    assert clamped == {(0, "low"), (0, "high"), (1, "low"), (1, "high"), (2, "high")}      # (the lower z face is u = 0 itself)
    z_bottom = c["rows"][ra.PLANE_AT["z_bottom"], 2]
    assert Fraction(float(z_bottom)) == cz - dz / 2 and Fraction(float(c["rows"][ra.PLANE_AT["z_top"], 2])) == cz + dz / 2
    beyond = Fraction(float(c["rows"][ra.PLANE_AT["x_beyond"], 0])) - cx
    assert dx / 2 < beyond < dx / 2 + Fraction(1, 100000)


@pytest.mark.parametrize("name", ("small_grid", "twelve", "double_one", "double_small"))
def test_voxels_at_and_above_the_cap(name):
    T = ra.SETTINGS[name][2]
    e = ra.expected(name)
    assert (e["count"] == T).any() and (e["count"] == T + 1).any() and (e["count"] > 3 * T).any() and (e["count"] == 0).any()
    full = e["count"] > T
    assert (e["index"][full] >= 0).all() and (e["index"][e["count"] == 0] == -1).all()


def test_chunks_and_seams():
    """A voxel whose members all lie in one 64-member chunk of its roi's list, and one whose members span several chunks and a run seam."""
    c = ra.case("float32")
    at, vox = _lists(c, 0, R["big"], (2, 3, 4), keep=c["keep"])
    assert len(at) > 4 * 64
    pos = np.arange(len(at)) // 64
    spans = [(len(set(pos[vox == g].tolist())), len(set(((at[vox == g] - int(c["offsets"][0])) // ra.RUN).tolist()))) for g in np.unique(vox)]
    assert any(chunks >= 3 and runs == 2 for chunks, runs in spans)
    one_chunk = 0
    for m in range(ra.FIRST_RANDOM, ra.FIRST_ZERO):
        at, vox = _lists(c, 0, m, (2, 3, 4), keep=c["keep"])
        one_chunk += len(at) <= 64 and any((vox == g).sum() >= 2 for g in np.unique(vox))
    assert one_chunk >= 10
    at, vox = _lists(c, 0, R["hand"], (12, 12, 12), keep=c["keep"])        # the hand voxel `order`: three rows on both sides of the seam
    assert at.tolist() == sorted(i for v in ra.HAND_AT.values() for i in v) and len(set((np.array(ra.HAND_AT["order"]) // ra.RUN).tolist())) == 2


def test_the_capacity_drops_a_tail_that_counts():
    whole, capped = ra.expected("small_grid"), ra.expected("capacity")
    free = ra.pool_setting("capacity", P=8192)
    big = R["big"]
    assert (free["roi_count"][:, big] > 64)[[0, 2]].all() and np.array_equal(capped["roi_count"], free["roi_count"])
    assert (capped["count"][0, big] != free["count"][0, big]).any() and capped["count"][0, big].sum() == 64
    assert not np.array_equal(capped["max"][0, big], free["max"][0, big]) and whole["roi_count"][0, big] < free["roi_count"][0, big]       # (the mask)
    small = free["roi_count"] <= 64
    assert small.sum() > 100 and np.array_equal(capped["count"][small], free["count"][small])


def test_overlap_absent_empty_unusable_and_masked():
    c = ra.case("float32")
    e, free = ra.expected("small_grid"), ra.pool_setting("small_grid", keep=None)
    a, _ = _lists(c, 0, R["planes"], (2, 3, 4))
    b, _ = _lists(c, 0, R["lapping"], (2, 3, 4))
    big, _ = _lists(c, 0, R["big"], (2, 3, 4))
    assert len(set(a.tolist()) & set(b.tolist())) >= 10 and set(a.tolist()) <= set(big.tolist())        # rois share rows
    present = rr.present(c["rois"], c["pose"])
    assert not present[:, ra.FIRST_ZERO:].any() and not present[:, R["nan"]].any() and present[:, :R["nan"]].all()
    assert not e["roi_count"][~present].any() and not e["count"][~present].any() and not e["pose"][~present].any() and (e["argmax"][~present] == -1).all()
    assert present[:, R["empty"]].all() and not e["roi_count"][:, R["empty"]].any()                     # present, no member
    assert not e["roi_count"][1].any() and e["pose"][1].any()                                           # the empty frame
    bad = ~rr.br.usable_rows(c["rows"])
    assert bad.sum() == 3 and c["keep"][bad].all() and not set(np.flatnonzero(bad).tolist()) & set(free["index"].reshape(-1).tolist())
    assert (free["roi_count"] >= e["roi_count"]).all() and free["roi_count"].sum() > e["roi_count"].sum() + 50
    dropped = set(free["index"].reshape(-1).tolist()) - set(e["index"].reshape(-1).tolist())
    assert len(dropped) > 20 and not c["keep"][sorted(dropped)].any()


@pytest.mark.parametrize("name", ("small_grid", "twelve"))
def test_the_hand_voxels(name):
    """Equal maxima, an all-NaN voxel, a -inf winner, and three values whose float32 sum is the row-order one in no other order."""
    dtype, out_size, T, Cf, P, masked, ew = ra.SETTINGS[name]
    c, e = ra.case(dtype), ra.expected(name)
    grid = ra.grid3(out_size)
    assert T == 4
    at, vox = _lists(c, 0, R["hand"], grid, keep=c["keep"])
    where = dict(zip(at.tolist(), vox.tolist()))
    got = {}
    for key, rows in ra.HAND_AT.items():
        g = {where[i] for i in rows}
        assert len(g) == 1 and e["count"][0, R["hand"], g.copy().pop()] == len(rows), key               # the voxel holds these rows alone
        g = g.pop()
        assert e["index"][0, R["hand"], g, :len(rows)].tolist() == list(rows)
        got[key] = tuple(e[k][0, R["hand"], g] for k in ("max", "argmax", "avg"))
    assert len({where[ra.HAND_AT[k][0]] for k in ra.HAND_AT}) == 4
    mx, am, av = got["equal"]
    assert (mx == 5.0).all() and (am == ra.HAND_AT["equal"][1]).all() and (av == np.float32(13.0 / 4)).all()
    mx, am, av = got["nan"]
    assert (mx == 0.0).all() and (am == -1).all() and np.isnan(av).all()
    mx, am, av = got["neginf"]
    assert np.isneginf(mx).all() and (am == ra.HAND_AT["neginf"][0]).all() and np.isnan(av).all()
    mx, am, av = got["order"]
    values = [np.float32(v) for v in ra.HAND["order"][1]]
    in_order = np.float32(np.float32(np.float32(0) + values[0]) + values[1]) + values[2]
    assert (av == np.float32(in_order / np.float32(3))).all() and (mx == np.float32(1e8)).all() and (am == ra.HAND_AT["order"][0]).all()
    for perm in itertools.permutations(range(3)):
        total = np.float32(np.float32(values[perm[0]] + values[perm[1]]) + values[perm[2]])
        assert (total == in_order) == (perm[2] == 2), perm                 # (IEEE addition commutes: only the first pair can swap unseen)
    ties = 0                                                               # equal maxima among the random features: the first row wins
    idx, feats = e["index"], c["features"][Cf]
    for f, m, g in zip(*np.nonzero(e["count"] >= 2)):
        pooled = idx[f, m, g][idx[f, m, g] >= 0]
        col = feats[pooled, 0]
        if (col == col.max()).sum() >= 2:
            ties += 1
            assert e["argmax"][f, m, g, 0] == pooled[np.argmax(col)]
    assert ties >= 10


# ---- csrc/sg_roiaware.h on the host -------------------------------------------------------------------------------------------------------------
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


def _triples():
    """(values n x 6, grids n x 3): random members of random rois, members on voxel planes and faces and in the margin, and degenerate sizes."""
    rng = np.random.default_rng(6200)
    n = 20000
    sizes = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 3)))
    grids = rng.integers(1, 17, (n, 3)).astype(np.int32)
    local = rng.uniform(-0.5, 0.5, (n, 3)) * sizes
    on = rng.integers(0, 17, (n, 3))                                       # a multiple of the voxel's edge from the lower face, computed as the rule does
    planes = np.subtract(np.multiply(np.minimum(on, grids), np.divide(sizes, grids)), np.multiply(sizes, 0.5))
    local = np.where(rng.uniform(0, 1, (n, 3)) < 0.3, planes, local)
    local = np.where(rng.uniform(0, 1, (n, 3)) < 0.1, np.nextafter(local, rng.choice([-np.inf, np.inf], (n, 3))), local)
    margin = rng.uniform(0, 1, (n, 3)) < 0.05
    local = np.where(margin, np.sign(local) * (sizes * 0.5 + rng.uniform(0, 1e-5, (n, 3))), local)
    values = np.column_stack((local, sizes))
    edge = [(0.0, 0.0, 0.0, 5e-324, 5e-324, 5e-324), (1e-5, -1e-5, 0.0, 5e-324, 1e-320, 1e-310), (np.nan, 0.0, 0.0, 1.0, 1.0, 1.0), (np.inf, -np.inf, 0.0, 1.0, 1.0, 1.0),
            (3.0, 1.5, 0.75, 6.0, 3.0, 1.5), (-3.0, -1.5, -0.75, 6.0, 3.0, 1.5), (1e6, 1e6, 1e6, 1e6, 1e6, 1e6)]
    values = np.vstack((values, np.repeat(np.array(edge), 3, axis=0)))
    grids = np.vstack((grids, np.tile(np.array([[1, 1, 1], [16, 16, 16], [2, 3, 4]], np.int32), (len(edge), 1))))
    return np.ascontiguousarray(values), np.ascontiguousarray(grids)


@pytest.mark.parametrize("sanitized", (False, True), ids=("plain", "asan_ubsan"))
def test_the_voxel_function_on_the_host_is_the_numpy_rule(tmp_path, sanitized):
    exe = _compile(tmp_path, "roiaware_voxel.cpp", "roiaware_voxel", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all") if sanitized else ())
    values, grids = _triples()
    values.tofile(tmp_path / "values.f64")
    grids.tofile(tmp_path / "grids.i32")
    r = subprocess.run([str(exe), str(len(values)), str(tmp_path / "values.f64"), str(tmp_path / "grids.i32"), str(tmp_path / "out.i32")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["voxel", str(len(values))], (r.stdout, r.stderr[-2000:])
    got = np.fromfile(tmp_path / "out.i32", np.int32)
    want = np.array([ra.voxel_ids(v[0:1], v[1:2], v[2:3], v[3:6], tuple(g))[0] for v, g in zip(values, grids.tolist())])
    assert np.array_equal(got, want)
    per = [np.array([ra.axis_index(v[j:j + 1], v[3 + j], g[j])[0] for v, g in zip(values, grids.tolist())]) for j in range(3)]
    low, high = sum((p == 0).sum() for p in per), sum((p == grids[:, j] - 1).sum() for j, p in enumerate(per))
    assert low > 3000 and high > 3000 and len(np.unique(got)) > 1000       # both clamps and the interior are reached


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_roi_voxel_pool_device"
APART = "; the mask, the rows, the rois, the pose and the features are read while the voxels are written: pass a buffer apart from them"
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "rois": WHO + ": n_rois must lie in 1 .. 512",
    "roi_features": WHO + ": roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first",
    "extra_width": WHO + ": every component of extra_width must be finite and lie in 0 .. 100",
    "out_size": WHO + ": every component of out_size must lie in 1 .. 16",
    "points": WHO + ": max_points must lie in 1 .. 128",
    "capacity": WHO + ": roi_capacity must lie in 64 .. 65536",
    "pool": WHO + ": d_out_max, d_out_argmax and d_out_avg need d_features; there is nothing to pool",
    "channels": WHO + ": feature_channels must lie in 1 .. 256",
    "elements": WHO + ": n_frames * n_rois * the voxels of a roi * max(max_points, feature_channels) exceeds 2^31 - 1; split the batch",
    "list": WHO + ": n_frames * n_rois * roi_capacity exceeds 2^31 - 1; split the batch or lower the capacity",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "runs": WHO + ": n_frames * n_rois * the 512-row runs of the longest frame exceeds 2^31 - 1; split the batch",
}
PAIRS = {"roi_count:keep_in": ("roi_count_is_keep_in",), "count:keep_in": ("count_overlaps_keep_in",), "index:rows": ("index_overlaps_rows",),
         "max:rois": ("max_is_rois",), "argmax:pose_in": ("argmax_overlaps_pose_in",), "avg:features": ("avg_is_features",),
         "max:features": ("max_overlaps_features",), "pose:pose_in": ("pose_is_pose_in",)}
OUTS = {"count:roi_count": ("count_is_roi_count",), "index:count": ("index_overlaps_count",), "max:index": ("max_overlaps_index",),
        "argmax:max": ("argmax_is_max",), "avg:argmax": ("avg_overlaps_argmax",), "pose:avg": ("pose_overlaps_avg",), "pose:roi_count": ("pose_overlaps_roi_count",)}
MESSAGES.update({k: f"{WHO}: d_out_{k.split(':')[0]} overlaps d_{k.split(':')[1]}{APART}" for k in PAIRS})
MESSAGES.update({k: f"{WHO}: d_out_{k.split(':')[0]} overlaps d_out_{k.split(':')[1]}{OWN}" for k in OUTS})
ACCEPTED = ("clean", "null_out_index", "null_out_max", "null_out_argmax", "null_out_avg", "null_out_pose", "null_pose_in", "null_keep_in", "null_extra_width",
            "no_features_no_pool", "float64", "empty_null_rows", "empty_null_features", "rois_1", "rois_512", "roi_features_7", "roi_features_10", "extra_width_100", "out_size_1",
            "out_size_16", "points_1", "points_128", "capacity_65536", "channels_1", "channels_256", "elements_below_2p31", "list_below_2p31", "frame_2p30_rows",
            "runs_below_2p31", "keep_in_behind_count", "index_behind_rows", "max_behind_features", "count_behind_roi_count", "avg_behind_argmax")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_rois", "null_out_size", "null_out_roi_count", "null_out_count", "bad_dtype", "no_frames", "negative_rows", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_rois_0"),
    "rois": ("rois_0", "rois_513", "rois_negative", "rois_0_and_roi_features_6"),
    "roi_features": ("roi_features_6", "roi_features_11", "roi_features_6_and_extra_width_nan"),
    "extra_width": ("extra_width_negative", "extra_width_above_100", "extra_width_nan", "extra_width_inf", "extra_width_nan_and_out_size_0"),
    "out_size": ("out_size_0", "out_size_17", "out_size_negative", "out_size_0_and_points_0"),
    "points": ("points_0", "points_129", "points_0_and_capacity_63"),
    "capacity": ("capacity_63", "capacity_65537", "capacity_63_and_no_features_max"),
    "pool": ("no_features_max", "no_features_argmax", "no_features_avg", "no_features_max_and_channels_0"),
    "channels": ("channels_0", "channels_257", "channels_257_and_elements_above_2p31"),
    "elements": ("elements_above_2p31", "elements_by_channels", "elements_overflowing", "elements_above_2p31_and_list_above_2p31"),
    "list": ("list_above_2p31", "list_above_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_runs_above_2p31"),
    "runs": ("runs_above_2p31", "runs_above_2p31_and_roi_count_is_rows"),
    **PAIRS, **OUTS,
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "roiaware_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "roiaware_refusals.cpp"), "-o", str(exe)]
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
    assert "int snowgpu_roi_voxel_pool_device(" in header and "snowgpu_roi_voxel_pool_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_roi_voxel_pool_device") and hasattr(_native.Context, "roi_voxel_pool_device")
    assert "snowgpu_roiaware.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import roiaware, stages, tensors
    assert tensors.roi_voxel_pool is stages.roi_voxel_pool and tensors.RoiVoxelBatch is stages.RoiVoxelBatch and callable(roiaware.roiaware_pool3d)
    assert callable(tensors.RoiVoxelBatch.empty) and isinstance(tensors.RoiVoxelBatch.nonempty, property)
    for method in ("max_features", "avg_features", "as_grid"):
        assert callable(getattr(tensors.RoiVoxelBatch, method))
