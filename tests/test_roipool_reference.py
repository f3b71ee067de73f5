"""RoI point pooling without a GPU: the restatement (tests/roipool_reference.py) against tests/box_reference.py where the two overlap; the
conditions under which the comparisons of tests/test_gpu_roipool.py are not vacuous, asserted on the shared inputs; what
snowgpu_roi_point_pool_device refuses, in which words (tests/host_harness/roipool_refusals.cpp); and that the entry is declared and bound."""
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import box_reference as br
import roipool_reference as rr
from conftest import ROOT

DTYPES = rr.DTYPES


# ---- the restatement against box_reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("constructed", "random"))
def test_restatement_agrees_with_box_reference(name, dtype):
    """With ew = 0: count is box_reference's count, and the smallest roi that has a row among its members is the row's box_of."""
    rows, offsets, keep, boxes, pose = br.case(name, dtype)
    e = br.expected(name, dtype)
    S = 1100                                                               # above every count: index holds all members
    got = rr.roi_point_pool(rows, boxes, pose, S, 3, (0.0, 0.0, 0.0), keep, offsets)
    assert np.array_equal(got["count"], e["count"]) and got["count"].max() < S and got["count"].max() > 20
    assert got["pose"].tobytes() == br.used_pose(boxes, pose).tobytes()
    first = np.full(len(rows), -1, np.int32)
    F, M = boxes.shape[:2]
    for f in range(F):
        for m in reversed(range(M)):
            first[got["index"][f, m, :got["count"][f, m]]] = m
    assert np.array_equal(first, e["box_of"])
    for f, m in zip(*np.nonzero(got["count"])):                            # local is box_reference's wherever the roi is the row's box
        at = got["index"][f, m, :got["count"][f, m]]
        own = e["box_of"][at] == m
        assert got["local"][f, m, :len(at)][own].tobytes() == e["local"][at[own]].tobytes()
        assert (np.diff(at) > 0).all() and got["points"][f, m, :len(at)].tobytes() == np.ascontiguousarray(rows[at, :3]).tobytes()


def test_the_restatement_on_a_case_by_hand():
    rois = np.array([[[0, 0, 0, 4, 2, 2, np.pi / 2, 3], [0, 0, 0, 10, 10, 10, 0, 1], [0, 0, 0, 0, 2, 2, 0, 1]]], np.float64)
    rows = np.array([[0.5, 1.9, 0.0, 7, 0], [1.5, 0, 0, 8, 0], [0, 0, 5.0, 9, 0], [0, 0, 5.1, 10, 0], [0.0, 2.2, 0, 11, 0]], np.float64)
    e = rr.roi_point_pool(rows, rois, br.numpy_pose(rois), 4, 4)
    assert e["count"].tolist() == [[1, 4, 0]] and e["index"].tolist() == [[[0, 0, 0, 0], [0, 1, 2, 4], [-1] * 4]]
    assert e["points"][0, 1, :, 3].tolist() == [7, 8, 9, 11] and not e["points"][0, 2].any() and not e["pose"][0, 2].any()
    assert np.allclose(e["local"][0, 0, 0], [1.9, -0.5, 0], atol=1e-15)
    wide = rr.roi_point_pool(rows, rois, br.numpy_pose(rois), 3, 3, (0.5, 0.0, 0.25))
    assert wide["count"].tolist() == [[2, 5, 0]] and wide["index"][0, 0].tolist() == [0, 4, 0] and wide["index"][0, 1].tolist() == [0, 1, 2]


# ---- the shared inputs meet the conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", (1, 100, 512))
def test_counts_around_the_samples(S, dtype):
    c, e = rr.case(f"counts{S}", dtype), rr.expected(f"counts{S}", dtype)
    targets = list(rr.count_targets(S))
    assert c["S"] == S and e["count"][0].tolist() == targets + [S] and e["count"][1].tolist() == [t + 3 for t in targets] + [S + 3]
    assert e["count"].max() > 3 * S and (e["index"][0, 0] == -1).all() and not e["points"][0, 0].any()
    assert e["index"][0, 3].tobytes() == e["index"][0, 6].tobytes() and e["local"][0, 3].tobytes() == e["local"][0, 6].tobytes()      # twins
    if S > 1:
        one, short = e["index"][0, 1], e["index"][0, 2]
        assert (one == one[0]).all() and short[S - 1] == short[0] and len(set(short[:S - 1].tolist())) == S - 1
        spread = (e["index"][0, 4] - int(c["offsets"][0])) // rr.RUN                      # the first S of S + 1 members: across the runs
        assert (np.diff(e["index"][0, 5]) > 0).all() and (np.diff(e["index"][0, 4]) > 0).all() and len(set(spread.tolist())) >= 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_seams(dtype):
    c, e = rr.case("seams", dtype), rr.expected("seams", dtype)
    off, R = c["offsets"], rr.SEAM_ROI
    n = np.diff(off)
    assert n.tolist() == [1000, 0, 1345, 1700] and n[3] >= 3 * rr.RUN + 1 and all(o % 64 for o in off[1:]) and off[1] % rr.RUN
    a = int(off[3])
    assert e["count"][3, R["ends"]] == 2 and e["index"][3, R["ends"], :2].tolist() == [a, a + 1699]
    for name, k in (("first63", 63), ("first64", 64), ("first65", 65)):
        assert e["count"][3, R[name]] == k and e["index"][3, R[name], :k].tolist() == list(range(a + 1, a + 1 + k))
    assert e["count"][:, R["all"]].tolist() == n.tolist()                                  # every row of its own frame and no other
    assert (e["index"][1] == -1).all() and not e["count"][1].any() and e["pose"][1].any()   # the empty frame: present rois, no member
    for f in (0, 2, 3):
        assert e["index"][f, R["all"]].tolist() == list(range(int(off[f]), int(off[f]) + 100))
        assert 50 < e["count"][f, R["cluster"]] < n[f] // 3
    assert not e["count"][:3, :4].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", rr.OVERLAP_M)
def test_overlap(M, dtype):
    c, e = rr.case(f"overlap{M}", dtype), rr.expected(f"overlap{M}", dtype)
    assert c["rois"].shape == (2, M, 7) and rr.present(c["rois"], c["pose"]).all()
    assert (e["index"][0, :, 0] == 0).all()                                                # row 0 lies in every roi of frame 0
    assert e["index"][:, 0].tobytes() == e["index"][:, M - 1].tobytes() and e["points"][:, 0].tobytes() == e["points"][:, M - 1].tobytes()
    assert (e["count"] >= 10).all()
    if M > 1:
        assert len({e["index"][0, m].tobytes() for m in range(M)}) > M // 2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("faces", "faces_ew"))
def test_face_rows_are_on_the_side_their_name_says(name, dtype):
    """In exact arithmetic: FACE_ROI is centred on the origin under the pose (1, 0), so lx = x, ly = y and sz = z are the rows' own values."""
    c, e = rr.case(name, dtype), rr.expected(name, dtype)
    sp, tag = c["special"], "ew:" if name == "faces_ew" else ""
    big = rr.enlarged(c["rois"][0, 0], c["ew"])
    hx, hy = (Fraction(float(np.add(np.multiply(big[j], 0.5), br.MARGIN))) for j in (3, 4))
    hz = Fraction(float(big[5])) / 2
    members = set(e["index"][0, 0, :min(e["count"][0, 0], c["S"])].tolist())
    assert e["count"][0, 0] <= c["S"] and c["pose"][0].tolist() == [[1.0, 0.0], [1.0, 0.0]]
    for key, i in sp.items():
        if not isinstance(i, int) or key.startswith("ew:") != bool(tag):
            continue
        x, y, z = (Fraction(float(v)) for v in c["rows"][i, :3])
        inside = abs(z) <= hz and abs(x) < hx and abs(y) < hy
        assert inside == key.endswith("_in") and (i in members) == inside, key
    assert Fraction(float(c["rows"][sp[tag + "top_in"], 2])) == hz and Fraction(float(c["rows"][sp[tag + "bottom_in"], 2])) == -hz
    if dtype == "float64":
        assert Fraction(float(c["rows"][sp[tag + "x_out"], 0])) == hx and Fraction(float(c["rows"][sp[tag + "-y_out"], 1])) == -hy
        assert c["rows"][sp[tag + "x_in"], 0] == np.nextafter(c["rows"][sp[tag + "x_out"], 0], 0.0)
    a, b = sp["only_ew"]
    assert e["count"][0, 1] == (b - a if tag else 0) and (not tag or e["index"][0, 1, :b - a].tolist() == list(range(a, b)))
    assert (c["rows"][:, :3].astype(np.float64) * 2.0 ** 30 % 1 == 0).all() or dtype == "float64"    # dyadic but for the float64 face values


@pytest.mark.parametrize("dtype", DTYPES)
def test_absent_things(dtype):
    c, e = rr.case("absent", dtype), rr.expected("absent", dtype)
    A = rr.ABSENT
    ok = rr.present(c["rois"], c["pose"], c["ew"])[0]
    assert ok.tolist() == [k in ("good", "far", "edge") for k in A]
    assert br.present(rr.enlarged(c["rois"], c["ew"]), c["pose"])[0, [A["zero"], A["dx0"], A["dz_negative"]]].all()      # absent by the original sizes alone
    assert not e["count"][0, ~ok].any() and (e["index"][0, ~ok] == -1).all() and not e["pose"][0, ~ok].any()
    free = rr.pool_case(c, keep=None)
    dropped = sorted(set(free["index"][0, A["good"]].tolist()) - set(e["index"][0, A["good"]].tolist()))
    assert 40 <= e["count"][0, A["good"]] < free["count"][0, A["good"]] and len(dropped) >= 10 and not c["keep"][dropped].all()
    bad = ~br.usable_rows(c["rows"])
    assert bad[[1, 5, 9]].all() and c["keep"][[1, 5, 9]].all() and not set(np.flatnonzero(bad).tolist()) & set(free["index"].reshape(-1).tolist())
    assert e["count"][0, A["far"]] >= 10 and np.abs(c["rois"][0, A["far"], :2]).min() > br.SENSOR
    a = 90
    assert e["index"][0, A["edge"], :3].tolist() == [a, a + 2, a + 3] and e["count"][0, A["edge"]] == 3 and c["rows"][a + 1, 0] == 1e6 + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_headings_case(dtype):
    c, e = rr.case("headings", dtype), rr.expected("headings", dtype)
    plain = rr.pool_case(c, ew=(0.0, 0.0, 0.0))
    assert (e["count"] >= plain["count"]).all() and e["count"].sum() > plain["count"].sum() + 20 and (e["count"] > c["S"]).any()
    assert 0.2 < (e["count"] == 0).mean() < 0.5 and len(np.unique(c["rois"][..., 6])) > 50


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_roi_point_pool_device"
APART = "; the mask, the rows, the rois and the pose are read while the pool is written: pass a buffer apart from them"
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "rows": "batch too large: split it below 2^31 rows",
    "rois": WHO + ": n_rois must lie in 1 .. 512",
    "roi_features": WHO + ": roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first",
    "samples": WHO + ": n_samples must lie in 1 .. 2048",
    "features": WHO + ": num_features must be 3, 4 or 5: the columns of a row that a roi stores",
    "extra_width": WHO + ": every component of extra_width must be finite and lie in 0 .. 100",
    "elements": WHO + ": n_frames * n_rois * n_samples * max(num_features, 3) exceeds 2^31 - 1; split the batch",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "runs": WHO + ": n_frames * n_rois * the 512-row runs of the longest frame exceeds 2^31 - 1; split the batch",
}
PAIRS = {"index_keep_in": ("index_is_keep_in", "index_overlaps_keep_in"), "count_rows": ("count_overlaps_rows",), "points_rois": ("points_is_rois",),
         "local_pose_in": ("local_overlaps_pose_in",), "pose_pose_in": ("pose_is_pose_in",), "pose_rows": ("pose_overlaps_rows",)}
OUTS = {"count_index": ("count_is_index",), "points_index": ("points_overlaps_index",), "points_count": ("points_overlaps_count",),
        "local_points": ("local_is_points",), "pose_local": ("pose_overlaps_local",), "pose_count": ("pose_overlaps_count",)}
MESSAGES.update({k: f"{WHO}: d_out_{k.split('_', 1)[0]} overlaps d_{k.split('_', 1)[1]}{APART}" for k in PAIRS})
MESSAGES.update({k: f"{WHO}: d_out_{k.split('_')[0]} overlaps d_out_{k.split('_')[1]}{OWN}" for k in OUTS})
ACCEPTED = ("clean", "null_out_points", "null_out_local", "null_out_pose", "null_pose_in", "null_keep_in", "null_extra_width", "float64", "empty_null_rows",
            "rois_1", "rois_512", "roi_features_7", "roi_features_10", "samples_1", "samples_2048", "features_3", "features_5", "extra_width_100",
            "elements_below_2p31", "frame_2p30_rows", "runs_below_2p31", "keep_in_behind_index", "count_behind_rows", "count_behind_index",
            "local_behind_points")
REFUSED = {
    "null": ("null_frame_offsets", "null_rows", "null_rois", "null_out_index", "null_out_count", "bad_dtype", "no_frames", "negative_rows", "null_and_rows_2p31"),
    "rows": ("rows_2p31", "rows_2p31_and_rois_0"),
    "rois": ("rois_0", "rois_513", "rois_negative", "rois_0_and_roi_features_6"),
    "roi_features": ("roi_features_6", "roi_features_11", "roi_features_6_and_samples_0"),
    "samples": ("samples_0", "samples_2049", "samples_0_and_features_2"),
    "features": ("features_2", "features_6", "features_2_and_extra_width_nan"),
    "extra_width": ("extra_width_negative", "extra_width_above_100", "extra_width_nan", "extra_width_inf", "extra_width_nan_and_elements_above_2p31"),
    "elements": ("elements_above_2p31", "elements_overflowing", "elements_above_2p31_and_frame_2p30_plus_1_rows"),
    "frame": ("frame_2p30_plus_1_rows", "frame_2p30_plus_1_rows_and_runs_above_2p31"),
    "runs": ("runs_above_2p31", "runs_above_2p31_and_index_is_rows"),
    **PAIRS, **OUTS,
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "roipool_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "roipool_refusals.cpp"), "-o", str(exe)]
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
    assert "int snowgpu_roi_point_pool_device(" in header and "snowgpu_roi_point_pool_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_roi_point_pool_device") and hasattr(_native.Context, "roi_point_pool_device")
    assert "snowgpu_roipool.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import roipool, stages, tensors
    assert tensors.roi_point_pool is stages.roi_point_pool and tensors.RoiPointBatch is stages.RoiPointBatch and callable(roipool.roipoint_pool3d)
    assert callable(tensors.RoiPointBatch.empty) and isinstance(tensors.RoiPointBatch.empty_flag, property)
    for method in ("gather", "labels"):
        assert callable(getattr(tensors.RoiPointBatch, method))
