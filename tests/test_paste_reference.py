"""The object paste without a GPU: the restatement (tests/paste_reference.py) on a case worked by hand; the conditions that keep the GPU
comparisons from being vacuous, asserted on the shared cases; csrc/sg_paste.h compiled for the host (tests/host_harness/paste_sweep.cpp)
against the restatement, byte for byte, and once under sanitizers; what snowgpu_paste_objects_device refuses, in which words and in which
order (tests/host_harness/paste_refusals.cpp); and that the entry is declared and bound."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import box_reference as br
import paste_reference as pr
import roipool_reference as rp

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
S = pr.STATE_SLOT


def test_the_restatement_on_a_case_by_hand():
    """One frame of 8 rows, rows 1, 4, 5 and 7 absent; one gt of class 1 at (10, 0); SAMPLE_GROUPS (2, 1).  Class 1 lacks one object and
    has one in the bank, of 2 points, at (0, 0): slot 0 is pasted into rows 1 and 4, slot 1 is inactive.  Class 2 has one object of 3 points
    at (1, 0) that overlaps the pasted one: state 3.  Row 0 at (0.5, 0, 0) lies in the pasted box and is removed; row 2 at (3, 0, 0) does
    not; row 4's input bytes -- inside the box, but absent -- are never tested and are overwritten."""
    dt = np.float32
    bank = pr.make_bank(np.array([[0.1, 0.1, 0, 9, 1], [-0.1, 0.2, 0, 8, 2], [1, 0, 0, 7, 3], [1.1, 0, 0, 6, 4], [0.9, 0, 0, 5, 5]], dt), [0, 2, 5],
                        np.array([[0, 0, 0, 4, 2, 1.5, 0, 1], [1, 0, 0, 4, 2, 1.5, 0, 2]], dt))
    rows = np.array([[0.5, 0, 0, 1, 0], [np.nan] * 5, [3, 0, 0, 1, 0], [20, 0, 0, 1, 0], [0.2, 0, 0, 1, 0], [np.inf] * 5, [-1.5, 0.9, 0.75, 1, 0], [0, 0, 0, 0, 0]], dt)
    keep = np.array([1, 0, 1, 1, 0, 0, 1, 0], bool)
    gt = np.array([[[10, 0, 0, 4, 2, 1.5, 0, 1]]], dt)
    e = pr.paste_objects(rows, [0, 8], keep, gt, br.numpy_pose(gt), bank, (2, 1), seed=5, step=9)
    assert e["object"].tolist() == [[0, -1, 1]] and e["state"].tolist() == [[pr.PASTED, pr.INACTIVE, pr.HIT_PASTED]]
    assert e["count"].tolist() == [[1, 2, 2, 4]]                      # rows 0 and 6 (on the z face, inside x and y) are removed
    assert e["keep"].tolist() == [False, True, True, True, True, False, False, False]
    assert e["source"].tolist() == [-1, 1, -1, -1, 1, -1, -1, -1]
    assert e["rows"][1].tobytes() == bank["points"][0].tobytes() and e["rows"][4].tobytes() == bank["points"][1].tobytes()
    assert e["rows"][[0, 2, 3, 5, 6, 7]].tobytes() == rows[[0, 2, 3, 5, 6, 7]].tobytes()
    assert e["gt_boxes"][0].tolist() == [gt[0, 0].tolist(), bank["boxes"][0].tolist(), [0.0] * 8, [0.0] * 8]
    assert e["pose"][0].tolist() == [[1.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 0.0]]


def test_words_are_the_weather_draws_positions():
    """r_q is word q % 4 of block (step, frame, tag + q / 4): step in the index, the frame in the group."""
    from seeded_reference import philox4x32_10
    w = pr.words(11, (1 << 40) + 3, 2, 7)
    assert w[:4] == philox4x32_10(11, (1 << 40) + 3, 2, 0x50415354) and w[4:] == philox4x32_10(11, (1 << 40) + 3, 2, 0x50415355)[:3]


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_every_state_and_every_edge_occurs(dtype):
    c, e = pr.case("states", dtype), pr.expected("states", dtype)
    st, P = e["state"][0].tolist(), pr.STATE_POINTS
    assert set(st) == set(range(6))                                   # every state 0 .. 5
    assert [st[S["first"]], st[S["twin"]], st[S["twin2"]]] == [1, 3, 3]                # the duplicate draw
    assert e["object"][0, S["first"]] == e["object"][0, S["twin"]] == e["object"][0, S["twin2"]] == 0
    assert st[S["full"]] == st[S["full2"]] == 0 and pr.class_counts(c["gt_boxes"][0], c["pose"][0])[1] == 2 == c["groups"][1]      # n_c <= cnt_c
    assert st[S["no_bank"]] == 0 and c["bank"]["class_offsets"][5] == c["bank"]["class_offsets"][6] and c["groups"][4] == 1        # an empty bank range
    assert st[S["on_gt"]] == 2 and st[S["absent"]] == 5
    # the edge toucher: area exactly 0 against the gt it touches, pasted
    trace = {}
    obj = e["object"][0].tolist()
    free = int((~c["keep"][:c["offsets"][1]]).sum())
    pr.sweep_frame(obj, c["bank"], c["gt_boxes"][0], c["pose"][0], free, trace)
    q = S["touching"]
    box = c["bank"]["boxes"][obj[q]].astype(np.float64)
    assert st[q] == 1 and trace[q][0] == 0.0 and box[0] - box[3] / 2 == pr.GT0[0] + pr.GT0[3] / 2
    assert max(trace[S["on_gt"]]) > 0.0
    # exactly free_left, and one more
    points = np.diff(c["bank"]["offsets"])
    assert st[S["exact"]] == 1 and points[obj[S["exact"]]] == free - P["A"] - P["E"] and st[S["one_more"]] == 4 and points[obj[S["one_more"]]] == 1
    assert e["count"][0].tolist()[:2] == [3, free] and e["count"][0, 3] == free
    # frame 1: no gt, class 2 active, unused free slots
    assert not br.present(c["gt_boxes"][1], c["pose"][1]).any() and e["object"][1, S["full"]] in (1, 2) and e["state"][1, S["full"]] == 4
    assert e["state"][1, S["first"]] == 1 and 0 < e["count"][1, 1] < e["count"][1, 3] == 25


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_removed_rows_on_the_faces_and_by_the_extra_width(dtype):
    c, e = pr.case("states", dtype), pr.expected("states", dtype)
    sp, keep = c["special"], e["keep"]
    assert c["ew"] == rp.EW
    for name in ("ew:top_in", "ew:bottom_in", "ew:x_in", "ew:-x_in", "ew:y_in", "ew:-y_in", "top_in", "x_in"):
        assert c["keep"][sp[name]] and not keep[sp[name]], name      # a z face of the enlarged box; within its 1e-5 margin; well inside
    for name in ("ew:top_out", "ew:bottom_out", "ew:x_out", "ew:-x_out", "ew:y_out", "ew:-y_out"):
        assert keep[sp[name]], name
    x_in = float(c["rows"][sp["ew:x_in"], 0])
    assert (4.0 + rp.EW[0]) / 2 < x_in < (4.0 + rp.EW[0]) / 2 + br.MARGIN                                    # inside by the margin alone
    assert float(c["rows"][sp["ew:top_in"], 2]) == (1.5 + rp.EW[2]) / 2                                      # exactly on the face
    without = pr.expected_of(c, ew=(0.0, 0.0, 0.0))
    for i in sp["only_ew"]:
        assert not keep[i] and without["keep"][i], i                 # removed only thanks to the extra width
    assert keep[sp["unusable"]]                                      # beyond 1e6: not usable, never removed
    assert e["count"][0, 2] == int((c["keep"] & ~keep)[:c["offsets"][1]].sum()) > without["count"][0, 2] > 0
    # bytes stay, absent rows inside a pasted box are not touched unless filled
    gone = c["keep"] & ~keep
    assert e["rows"][gone].tobytes() == c["rows"][gone].tobytes()
    untouched = ~c["keep"] & (e["source"] < 0)
    assert untouched.any() and not keep[untouched].any() and e["rows"][untouched].tobytes() == c["rows"][untouched].tobytes()


@pytest.mark.parametrize("dtype", pr.DTYPES)
def test_shapes_of_the_other_cases(dtype):
    for name, Q, B in (("q1", 1, 1), ("q63", 63, 65), ("q64", 64, 192)):
        c, e = pr.case(name, dtype), pr.expected(name, dtype)
        assert sum(c["groups"]) == Q and c["gt_boxes"].shape[1] == B and e["gt_boxes"].shape[1] == B + Q
        assert (e["state"] == 1).any(), name
    e = pr.expected("q63", dtype)
    assert {2, 3}.issubset(set(e["state"].ravel().tolist())) and (e["count"][:, 2] > 0).any()
    assert {0, 1}.issubset(set(pr.expected("q64", dtype)["state"].ravel().tolist()))
    c, e = pr.case("lengths", dtype), pr.expected("lengths", dtype)
    assert tuple(np.diff(c["offsets"])) == pr.LENGTHS and (e["count"][3:, 0] > 0).all() and e["count"][0].tolist()[1:] == [0, 0, 0]
    # the straddle: each object where the docstring says
    c, e = pr.case("straddle", dtype), pr.expected("straddle", dtype)
    B = c["gt_boxes"].shape[1]
    assert e["state"][0].tolist() == [1, 1, 1]
    assert np.flatnonzero(e["source"][:1537] == B).tolist() == list(range(58, 66))
    assert np.flatnonzero(e["source"][:1537] == B + 1).tolist() == [66, 67] + list(range(505, 521)) + [1525, 1526]
    assert np.flatnonzero(e["source"][:1537] == B + 2).tolist() == list(range(1527, 1537))
    assert e["count"][1, 3] == 40 and (e["source"][1537:1537 + 38] >= 0).all() and e["source"][1537 + 38] == -1
    # 0, 64 and 600 points; a frame without a free slot
    c, e = pr.case("big", dtype), pr.expected("big", dtype)
    assert tuple(np.diff(c["bank"]["offsets"])) == pr.BIG_POINTS == (0, 64, 600)
    assert e["state"].tolist() == [[1, 1, 1], [1, 4, 4], [1, 1, 4]] and e["count"][1, [0, 1, 3]].tolist() == [1, 0, 0] and e["count"][0, 1] == 664


def test_step_seed_and_frame_change_the_draws():
    c = pr.case("q63", "float32")
    base = pr.expected("q63", "float32")["object"]
    assert not np.array_equal(pr.expected_of(c, step=c["step"] + 1)["object"], base)
    assert not np.array_equal(pr.expected_of(c, seed=c["seed"] + 1)["object"], base)
    assert not np.array_equal(pr.expected_of(c, frames=(1, 0))["object"], base)
    assert np.array_equal(pr.expected_of(c)["object"], base)


# ---- csrc/sg_paste.h on the host ----------------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra, "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "paste_sweep.cpp"), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("paste_sweep"), "paste_sweep")


def _sweep(exe, tmp, c):
    """object, state, base and the rows pasted of the harness on case c."""
    gt, bank = c["gt_boxes"], c["bank"]
    F, B, Cb = gt.shape
    Q, O = sum(c["groups"]), len(bank["boxes"])
    present = np.ones(len(c["rows"]), bool) if c["keep"] is None else c["keep"]
    free = np.array([int((~present[a:b]).sum()) for a, b in zip(c["offsets"][:-1], c["offsets"][1:])], np.int32)
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    with open(fin, "wb") as fp:
        for a in (gt, c["pose"], free, bank["offsets"], bank["boxes"], bank["pose"], bank["class_offsets"]):
            fp.write(np.ascontiguousarray(a).tobytes())
    args = [0 if gt.dtype == np.float32 else 1, F, B, Cb, O, c["seed"], c["step"], fin, fout, len(c["groups"]), *c["groups"]]
    r = subprocess.run([str(exe), *(str(a) for a in args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(fout, np.int32)
    assert len(raw) == 3 * F * Q + F
    return raw[:F * Q].reshape(F, Q), raw[F * Q:2 * F * Q].reshape(F, Q), raw[2 * F * Q:3 * F * Q].reshape(F, Q), raw[3 * F * Q:], free


def _held_to_the_restatement(exe, tmp, name, dtype):
    c, e = pr.case(name, dtype), pr.expected(name, dtype)
    obj, state, base, n_rows, free = _sweep(exe, tmp, c)
    assert obj.tobytes() == e["object"].tobytes() and state.tobytes() == e["state"].tobytes(), (name, dtype)
    assert n_rows.tobytes() == np.ascontiguousarray(e["count"][:, 1]).tobytes()
    for f in range(len(free)):
        _, want = pr.sweep_frame(e["object"][f].tolist(), c["bank"], c["gt_boxes"][f], c["pose"][f], int(free[f]))
        assert base[f].tolist() == want, (name, dtype, f)


@pytest.mark.parametrize("dtype", pr.DTYPES)
@pytest.mark.parametrize("name", pr.CASE_NAMES)
def test_the_header_on_the_host_equals_the_restatement(sweep, tmp_path, name, dtype):
    _held_to_the_restatement(sweep, tmp_path, name, dtype)


def test_the_header_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan -- host code only, a stand-alone program: the records, the conflict words and the
    sweep stay inside their arrays at Q = 64 with B = 192 and on the state case."""
    exe = _compile(tmp_path, "paste_sweep_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name, dtype in (("q64", "float64"), ("states", "float32"), ("q1", "float32")):
        _held_to_the_restatement(exe, tmp_path, name, dtype)


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_paste_objects_device"
APART = "; the mask, the rows, the gt boxes, the pose, the bank and the step are read while the batch is written: pass a buffer apart from them"
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "slots": WHO + ": the sample groups must add up to 1 .. 64 slots",
    "classes": WHO + ": n_classes must lie in 1 .. 16",
    "gt": WHO + ": n_gt must be at least 1 and n_gt plus the slots at most 256",
    "gt_features": WHO + ": gt_features must lie in 8 .. 10: cx, cy, cz, dx, dy, dz, heading, class first",
    "group": WHO + ": a sample group is negative",
    "extra_width": WHO + ": every component of extra_width must be finite and lie in 0 .. 100",
    "elements": WHO + ": n_frames * (n_gt + slots) * gt_features exceeds 2^31 - 1; split the batch",
    "rows": "batch too large: split it below 2^31 rows",
    "bank": WHO + ": the bank must stay below 2^31 points and objects",
    "frame": WHO + ": a frame of more than 2^30 rows; split it",
    "step": WHO + ": d_step is NULL; one uint64 in device memory",
}
ORDER = tuple(MESSAGES)              # the order of the checks: a call wrong in two ways gets the earlier message
DOUBLY = ("null_gt_boxes_and_slots_0", "slots_65_and_classes_17", "classes_17_and_gt_0", "gt_0_and_gt_features_7", "gt_features_7_and_group_negative",
          "group_negative_and_extra_width_nan", "extra_width_nan_and_elements_at_2p31", "elements_at_2p31_and_rows_at_2p31", "rows_at_2p31_and_bank_points_at_2p31",
          "bank_points_at_2p31_and_frame_above_2p30", "frame_above_2p30_and_null_step", "null_step_and_out_rows_is_rows")
PAIRS = {("rows", "rows"): ("out_rows_is_rows", "out_rows_overlaps_rows"), ("keep", "keep_in"): ("out_keep_is_keep_in",), ("gt_boxes", "gt_boxes"): ("out_gt_boxes_is_gt_boxes",),
         ("object", "frame_offsets"): ("object_overlaps_frame_off",), ("state", "bank_offsets"): ("state_is_bank_off",),
         ("source", "bank_points"): ("source_overlaps_bank_points",), ("count", "bank_boxes"): ("count_is_bank_boxes",), ("count", "class_offsets"): ("count_is_class_off",),
         ("count", "step"): ("count_is_step",), ("pose", "pose_in"): ("pose_is_pose_in",), ("pose", "bank_pose"): ("pose_is_bank_pose",)}
OUTS = {("keep", "rows"): ("out_keep_is_out_rows",), ("state", "object"): ("state_is_object",), ("source", "state"): ("source_overlaps_state",),
        ("count", "gt_boxes"): ("count_is_out_gt_boxes",), ("pose", "count"): ("pose_is_count",)}
ACCEPTED = ("clean", "null_pose_in", "null_keep_in", "null_out_source", "null_out_pose", "null_extra_width", "no_rows_needs_no_row_buffers", "bank_without_points",
            "float64", "slots_1", "slots_64", "classes_16", "gt_1", "gt_252", "gt_features_10", "a_group_beyond_nc_is_not_read", "extra_width_100",
            "elements_below_2p31", "frame_of_2p30", "out_rows_behind_rows", "out_keep_behind_keep_in", "source_behind_bank_points", "out_keep_behind_out_rows")
REFUSED = {
    "null": ("null_frame_off", "null_rows", "null_gt_boxes", "null_bank_points", "null_bank_off", "null_bank_boxes", "null_bank_pose", "null_class_off", "null_groups",
             "null_out_rows", "null_out_keep", "null_out_gt_boxes", "null_out_object", "null_out_state", "null_out_count", "bad_dtype", "no_frames", "rows_negative",
             "null_gt_boxes_and_slots_0"),
    "slots": ("slots_0", "slots_65", "classes_0", "classes_negative_with_slots", "slots_65_and_classes_17"),
    "classes": ("classes_17", "classes_17_and_gt_0"),
    "gt": ("gt_0", "gt_253", "gt_0_and_gt_features_7"),
    "gt_features": ("gt_features_7", "gt_features_11", "gt_features_7_and_group_negative"),
    "group": ("group_negative", "group_negative_and_extra_width_nan"),
    "extra_width": ("extra_width_negative", "extra_width_above_100", "extra_width_nan", "extra_width_inf", "extra_width_nan_and_elements_at_2p31"),
    "elements": ("elements_at_2p31", "elements_at_2p31_and_rows_at_2p31"),
    "rows": ("rows_at_2p31", "rows_at_2p31_and_bank_points_at_2p31"),
    "bank": ("bank_points_at_2p31", "bank_objects_at_2p31", "bank_points_at_2p31_and_frame_above_2p30"),
    "frame": ("frame_above_2p30", "frame_above_2p30_and_null_step"),
    "step": ("null_step", "null_step_and_out_rows_is_rows"),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "paste_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "paste_refusals.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split("|", 1) for ln in r.stdout.splitlines())
    want = {case: "0|OK" for case in ACCEPTED}
    for key, cases in REFUSED.items():
        want.update({case: "1|" + MESSAGES[key] for case in cases})
    for (out, inp), cases in PAIRS.items():
        want.update({case: f"1|{WHO}: d_out_{out} overlaps d_{inp}{APART}" for case in cases})
    for (out, other), cases in OUTS.items():
        want.update({case: f"1|{WHO}: d_out_{out} overlaps d_out_{other}{OWN}" for case in cases})
    assert got == want
    assert set(MESSAGES) == set(REFUSED)              # every message is reached
    # the order: the checks stand in sg_check_paste_args in the order of MESSAGES, the overlaps behind them -- every "<first>_and_<second>"
    # case of the harness is wrong in two ways, of checks next to each other, and is filed above under the earlier one
    for key, later, case in zip(ORDER, ORDER[1:] + (None,), DOUBLY):
        first, second = case.split("_and_")
        assert first in REFUSED[key] and case in REFUSED[key], case
        assert second in REFUSED[later] if later else any(second in cases for cases in PAIRS.values()), case


def test_the_entry_is_declared_and_bound():
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_paste_objects_device(" in header and "snowgpu_paste_objects_device" in _native.EXPORTS
    assert "NOT CHECKED against" in header.split("GROUND-TRUTH OBJECT PASTE")[1].split("*/")[0] and "NOT pcdet's all-pairs rejection" in header
    assert hasattr(_native.lib(), "snowgpu_paste_objects_device") and hasattr(_native.Context, "paste_objects_device")
    assert "snowgpu_paste.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import paste, stages, tensors
    assert tensors.paste_objects is stages.paste_objects and tensors.PasteBatch is stages.PasteBatch and tensors.ObjectBank is stages.ObjectBank
    assert callable(paste.build_bank) and callable(paste.paste_objects) and tuple(paste.FIELDS) == tuple(pr.FIELDS)
