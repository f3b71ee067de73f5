"""Points in 3D boxes without a GPU: the conditions under which the comparisons of tests/test_gpu_boxes.py are not vacuous, asserted on the
shared inputs of tests/box_reference.py; csrc/sg_box.h compiled for the host (tests/host_harness/box_cells.cpp) -- the footprint of a box
against more than a million confirmed (row, box) pairs, and whole frames through the filing and the walk against the restatement, byte
for byte -- once more under the address and undefined-behaviour sanitizers as a stand-alone program; what
snowgpu_points_in_boxes_device refuses, in which words (tests/host_harness/box_refusals.cpp); and that the entry is declared and bound."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import box_reference as br
from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
DTYPES = br.DTYPES
FRAME = br.FRAME


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_edge_row_is_on_the_side_its_name_says(dtype):
    """In exact arithmetic: the face box is centred on the origin with heading 0, so lx = x, ly = y and sz = z are the rows' own values."""
    from fractions import Fraction
    rows, offsets, keep, boxes, pose = br.case("constructed", dtype)
    sp, e = br.special(dtype), br.expected("constructed", dtype)
    box = boxes[FRAME["faces"], 0].astype(np.float64)
    assert box[:3].tolist() == [0, 0, 0] and box[6] == 0 and pose[FRAME["faces"], 0].tolist() == [1.0, 0.0]
    hx, hy = (Fraction(float(np.add(np.multiply(box[j], 0.5), br.MARGIN))) for j in (3, 4))      # the definition's rounded operand
    hz = Fraction(float(box[5])) / 2
    t = rows.dtype.type
    for name, i in sp.items():
        if not isinstance(i, int):
            continue
        x, y, z = (Fraction(float(v)) for v in rows[i, :3])
        inside = abs(z) <= hz and abs(x) < hx and abs(y) < hy
        assert inside == name.endswith("_in") and (e["box_of"][i] == 0) == inside and keep[i], name
    assert Fraction(float(rows[sp["top_in"], 2])) == hz and Fraction(float(rows[sp["bottom_in"], 2])) == -hz
    assert rows[sp["top_out"], 2] == np.nextafter(t(0.75), t(1)) and rows[sp["bottom_out"], 2] == np.nextafter(t(-0.75), t(-1))
    for axis, (name, h) in enumerate((("x", hx), ("y", hy))):
        out, inn = rows[sp[name + "_out"], axis], rows[sp[name + "_in"], axis]
        assert Fraction(float(out)) >= h > Fraction(float(inn)) and inn == np.nextafter(out, t(0)) and rows[sp["-" + name + "_out"], axis] == -out
        if dtype == "float64":
            assert Fraction(float(out)) == h                                          # exactly on the face
    assert (br.cells(box[:2]) == 32).all() and ((box[:2] + br.SENSOR) / br.EDGE % 1 == 0).all()      # the box is centred on a cell corner


@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_batch_meets_the_conditions(dtype):
    rows, offsets, keep, boxes, pose = br.case("constructed", dtype)
    sp = br.special(dtype)
    e, free = br.expected("constructed", dtype), br.expected("constructed", dtype, given=False)
    assert np.diff(offsets).tolist() == list(br.COUNTS) and boxes.shape == (7, br.CONSTRUCTED_B, 8)
    ok = br.present(boxes, pose)
    frame = np.repeat(np.arange(7), np.diff(offsets))
    # headings: the named ones, each box with a row; the thin box at 45 degrees crosses several cells and holds the rows along it only
    f = FRAME["headings"]
    assert [float(v) for v in boxes[f, :8, 6]] == [float(rows.dtype.type(h)) for h in br.HEADINGS] and (e["count"][f, :8] > 0).all()
    thin = boxes[f, 9].astype(np.float64)
    assert thin[3] == rows.dtype.type(0.05) and thin[4] == 6 and abs(thin[6] - np.pi / 4) < 1e-7
    a, b = sp["thin_along"]
    assert (e["box_of"][a:b] == 9).all() and len({(int(br.cells(x)), int(br.cells(y))) for x, y in rows[a:b, :2]}) >= 3 and e["count"][f, 9] == b - a
    a, b = sp["thin_beside"]
    assert (e["box_of"][a:b] == -1).all()
    # overlap: the smallest number wins and both count, whichever of the two is the containing box
    f = FRAME["overlap"]
    sl = slice(int(offsets[f]), int(offsets[f + 1]))
    inside = br.frame_matrices(rows[sl, :3].astype(np.float64), boxes[f], pose[f])[3] & br.usable_rows(rows[sl], keep[sl])[:, None]
    assert (inside[:, 1] & inside[:, 4]).sum() >= 3 and (inside[:, 1] & inside[:, 6]).sum() >= 3 and (inside[:, 2] & inside[:, 8]).sum() >= 3
    assert (e["box_of"][sl][inside[:, 1] & inside[:, 4]] == 1).all() and (e["box_of"][sl][inside[:, 2] & inside[:, 8]] == 2).all()
    assert (inside[:, 4] <= inside[:, 1]).all() and (inside[:, 2] <= inside[:, 8]).all()          # nested
    assert e["count"][f].sum() > (e["box_of"][sl] >= 0).sum() and e["count"][f, 4] == inside[:, 4].sum() > 0
    # equal boxes at equal places in neighbouring frames, rows only in the second
    a, b = FRAME["all_rows"], FRAME["extremes"]
    assert boxes[a, 0].tobytes() == boxes[b, 0].tobytes() and e["count"][a, 0] == 0 and e["count"][b, 0] >= 10
    # absent boxes: every kind; a frame whose boxes are all absent; the given pose (2, 0) against the computed one
    f = FRAME["absent"]
    assert not ok[f].any() and not e["count"][f].any() and e["box_of"][offsets[f]] == -1
    kinds = boxes[f].astype(np.float64)
    assert not kinds[0].any() and np.isnan(kinds[1, 0]) and kinds[2, 3] == 0 and kinds[3, 3] < 0 and np.isinf(kinds[4, 6]) and kinds[5, 0] > br.BOUND
    assert pose[f, 6].tolist() == [2.0, 0.0] and free["box_of"][offsets[f]] == 6 and free["count"][f].tolist() == [0] * 6 + [1] + [0] * 5
    assert np.isnan(kinds[7, 5]) and kinds[8, 4] > br.BOUND and kinds[9, 6] < -br.BOUND and np.isinf(kinds[10, 2])
    assert ok[FRAME["no_row"]].sum() == 1 and not e["count"][FRAME["no_row"]].any()
    # extremes
    f = FRAME["all_rows"]
    sl = slice(int(offsets[f]), int(offsets[f + 1]))
    assert e["count"][f, 7] == 257 and (e["box_of"][sl] == 7).all() and (np.abs(rows[sl, :2]) > br.SENSOR).any(axis=1).sum() >= 20
    f = FRAME["extremes"]
    sl = slice(int(offsets[f]), int(offsets[f + 1]))
    small = boxes[f, 2].astype(np.float64)
    assert max(small[3:5]) < br.EDGE / 4 and ((small[:2] + br.SENSOR) / br.EDGE % 1 == 0).all() and e["count"][f, 2] >= 5
    assert np.abs(boxes[f, 3, :2]).min() > br.SENSOR and e["count"][f, 3] >= 5 and abs(boxes[f, 5, 0]) == 9e5 and e["count"][f, 5] >= 5 and e["count"][f, 6] >= 5
    assert ok[f, 11] and e["count"][f, 11] == 0
    a, b = sp["unusable"]
    bad = rows[a:b, :3].astype(np.float64)
    assert np.isnan(bad[0, 0]) and np.isinf(bad[1, 1]) and np.isinf(bad[2, 2]) and (np.abs(bad[3:]) > br.BOUND).any(axis=1).all() and keep[a:b].all()
    assert (e["box_of"][a:b] == -1).all() and not br.usable_rows(rows[a:b]).any()
    # a keep mask that removes rows inside boxes
    unmasked = br.points_in_boxes(rows, boxes, pose, None, offsets)
    assert ((unmasked["box_of"] >= 0) & ~keep).sum() >= 10 and (e["box_of"][~keep] == -1).all() and unmasked["count"].sum() > e["count"].sum()
    assert not e["local"][e["box_of"] < 0].any() and np.abs(e["local"][e["box_of"] >= 0]).sum(axis=1).all()
    assert set(np.unique(frame[e["box_of"] >= 0]).tolist()) == {2, 3, 4, 5, 6}


@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_words_and_the_random_case(dtype):
    for B in br.WORDS:
        rows, offsets, keep, boxes, pose = br.case(f"words{B}", dtype)
        e = br.expected(f"words{B}", dtype)
        assert boxes.shape == (2, B, 7) and br.present(boxes, pose).all()
        assert set(np.unique(e["box_of"]).tolist()) == {-1, B - 1} and (e["count"][:, B - 1] >= 15).all() and not e["count"][:, :B - 1].any()
    rows, offsets, keep, boxes, pose = br.case("random", dtype)
    e = br.expected("random", dtype)
    ok = br.present(boxes, pose)
    assert boxes.shape == (2, br.RANDOM_B, 10) and 1900 < min(np.diff(offsets)) and 0.2 < (~ok).mean() < 0.3
    per_row = np.zeros(len(rows), np.int64)
    for f in range(2):
        sl = slice(int(offsets[f]), int(offsets[f + 1]))
        per_row[sl] = br.frame_matrices(rows[sl, :3].astype(np.float64), boxes[f], pose[f])[3].sum(axis=1)
    assert (per_row == 0).sum() > 1000 and (per_row == 1).sum() > 100 and (per_row >= 2).sum() > 30
    assert (ok & (e["count"] == 0)).sum() >= 2 and ok[:, 38].all() and not e["count"][:, 38].any()
    assert e["count"].sum() == per_row.sum() and ((e["box_of"] >= 0) == (per_row > 0)).all()


def test_the_restatement_on_a_case_by_hand():
    boxes = np.array([[[0, 0, 0, 4, 2, 2, np.pi / 2, 3], [0, 0, 0, 10, 10, 10, 0, 1]]], np.float64)
    rows = np.array([[0.5, 1.9, 0.0, 0, 0], [1.5, 0, 0, 0, 0], [0, 0, 5.0, 0, 0], [0, 0, 5.1, 0, 0]], np.float64)
    e = br.points_in_boxes(rows, boxes, br.numpy_pose(boxes))
    assert e["box_of"].tolist() == [0, 1, 1, -1] and e["count"].tolist() == [[1, 3]]
    assert np.allclose(e["local"], [[1.9, -0.5, 0], [1.5, 0, 0], [0, 0, 5], [0, 0, 0]], atol=1e-15)


# ---- csrc/sg_box.h on the host ----------------------------------------------------------------------------------------------------------------
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
    return _compile(tmp_path_factory.mktemp("box"), "box_cells.cpp", "box_cells")


def _walk(exe, tmp_path, rows, keep, boxes, pose, dtype, given):
    fi, fk, fb, fp, fo = (tmp_path / f"w.{s}" for s in ("in", "keep", "boxes", "pose", "out"))
    np.ascontiguousarray(np.asarray(rows)[:, :3], np.float64).tofile(fi)
    (np.ones(len(rows), np.uint8) if keep is None else np.asarray(keep).astype(np.uint8)).tofile(fk)
    np.ascontiguousarray(np.asarray(boxes)[:, :7], np.float64).tofile(fb)
    np.ascontiguousarray(pose, np.float64).tofile(fp)
    B = len(boxes)
    r = subprocess.run([str(exe), "walk", str(DTYPES.index(dtype)), str(B), str(int(given)), str(fi), str(fk), str(fb), str(fp), str(fo)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    n, t = len(rows), np.dtype(dtype)
    raw = fo.read_bytes()
    assert len(raw) == n * 4 + B * 4 + n * 3 * t.itemsize + B * 16
    return dict(box_of=np.frombuffer(raw, np.int32, n), count=np.frombuffer(raw, np.int32, B, n * 4),
                local=np.frombuffer(raw, t, n * 3, (n + B) * 4).reshape(n, 3), pose=np.frombuffer(raw, np.float64, B * 2, (n + B) * 4 + n * 3 * t.itemsize).reshape(B, 2))


def _walk_case(exe, tmp_path, name, dtype, given):
    rows, offsets, keep, boxes, pose = br.case(name, dtype)
    want = br.expected(name, dtype)
    for f, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        got = _walk(exe, tmp_path, rows[a:b], None if keep is None else keep[a:b], boxes[f], pose[f], dtype, given)
        if given:
            assert got["pose"].tobytes() == br.used_pose(boxes[f], pose[f]).tobytes(), (name, dtype, f)
            ref = {k: (v[f] if k == "count" else v[a:b]) for k, v in want.items()}
        else:                                              # the host library's cos / sin: the restatement is fed the pose that was used
            ref = br.points_in_boxes(rows[a:b], boxes[f][None], got["pose"][None].copy(), None if keep is None else keep[a:b])
            ref["count"] = ref["count"][0]
        for field in ("box_of", "count", "local"):
            assert got[field].tobytes() == ref[field].tobytes(), (name, dtype, f, given, field)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_walk_equals_the_restatement(harness, tmp_path, dtype):
    for name in br.CASES:
        _walk_case(harness, tmp_path, name, dtype, True)
    for name in ("constructed", "random"):
        _walk_case(harness, tmp_path, name, dtype, False)


def test_no_member_outside_the_footprint(harness):
    r = subprocess.run([str(harness), "cover", "1", "1200000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    word, pairs, boxes = r.stdout.split()
    assert word == "cover" and int(pairs) >= 1_000_000 and int(boxes) > 10_000


def test_harness_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    exe = _compile(tmp_path, "box_cells.cpp", "box_cells_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([str(exe), "cover", "2", "100000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.split()[0] == "cover" and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-2000:]
    _walk_case(exe, tmp_path, "constructed", "float32", True)
    _walk_case(exe, tmp_path, "words256", "float64", True)
    _walk_case(exe, tmp_path, "words65", "float32", False)


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_points_in_boxes_device"
APART = {"keep_in": " overlaps d_keep_in; the mask is read while the labels are written: pass a buffer apart from it",
         "rows": " overlaps d_rows; the rows are read while the labels are written: pass a buffer apart from them",
         "boxes": " overlaps d_boxes; the boxes are read while the labels are written: pass a buffer apart from them",
         "pose_in": " overlaps d_pose_in; the pose is read while the labels are written: pass a buffer apart from it"}
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "boxes": WHO + ": n_boxes must lie in 1 .. 256",
    "box_features": WHO + ": box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first",
    "slots": WHO + ": n_frames * n_boxes exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
}
OUTPUTS = ("box_of", "count", "local", "pose")
MESSAGES.update({f"{o}_{i}": f"{WHO}: d_out_{o}{APART[i]}" for o in OUTPUTS for i in APART})
MESSAGES.update({f"{o}_{p}": f"{WHO}: d_out_{o} overlaps d_out_{p}{OWN}" for j, o in enumerate(OUTPUTS) for p in OUTPUTS[:j]})
ACCEPTED = ("clean", "null_out_count", "null_out_local", "null_out_pose", "null_pose_in", "null_keep_in", "float64", "empty_null_rows_and_box_of",
            "boxes_1", "boxes_256", "box_features_7", "box_features_10", "slots_2p31_minus_256", "frame_2p30_rows", "keep_in_behind_box_of",
            "box_of_behind_rows", "box_of_behind_boxes", "box_of_behind_pose_in", "count_behind_box_of")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_boxes", "null_out_box_of", "bad_dtype", "no_frames", "negative_rows", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_boxes_0"),
    "boxes": ("boxes_0", "boxes_257", "boxes_negative", "boxes_0_and_box_features_6"),
    "box_features": ("box_features_6", "box_features_11", "box_features_6_and_slots_2p31"),
    "slots": ("slots_2p31", "slots_overflowing", "slots_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_box_of_is_keep_in"),
    "box_of_keep_in": ("box_of_is_keep_in", "box_of_overlaps_keep_in"),
    "count_keep_in": ("count_overlaps_keep_in",),
    "local_keep_in": ("local_overlaps_keep_in",),
    "pose_keep_in": ("pose_overlaps_keep_in",),
    "box_of_rows": ("box_of_overlaps_rows",),
    "count_rows": ("count_is_rows",),
    "local_rows": ("local_is_rows",),
    "pose_rows": ("pose_overlaps_rows",),
    "box_of_boxes": ("box_of_overlaps_boxes",),
    "count_boxes": ("count_is_boxes",),
    "local_boxes": ("local_overlaps_boxes",),
    "pose_boxes": ("pose_overlaps_boxes",),
    "box_of_pose_in": ("box_of_overlaps_pose_in",),
    "count_pose_in": ("count_is_pose_in",),
    "local_pose_in": ("local_overlaps_pose_in",),
    "pose_pose_in": ("pose_is_pose_in",),
    "count_box_of": ("count_is_box_of",),
    "local_box_of": ("local_overlaps_box_of",),
    "local_count": ("local_overlaps_count",),
    "pose_box_of": ("pose_overlaps_box_of",),
    "pose_count": ("pose_overlaps_count",),
    "pose_local": ("pose_is_local",),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "box_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "box_refusals.cpp"), "-o", str(exe)]
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
    assert "int snowgpu_points_in_boxes_device(" in header and "snowgpu_points_in_boxes_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_points_in_boxes_device") and hasattr(_native.Context, "points_in_boxes_device")
    assert "snowgpu_box.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import boxes, tensors
    assert callable(tensors.points_in_boxes) and callable(tensors.BoxLabelBatch.empty) and callable(boxes.points_in_boxes)
    for method in ("flat_index", "labels", "keep_boxes", "rows_in"):
        assert callable(getattr(tensors.BoxLabelBatch, method))
