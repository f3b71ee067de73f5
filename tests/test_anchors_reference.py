"""Anchor target assignment without a GPU: the conditions under which the comparisons of tests/test_gpu_anchors.py are not vacuous,
asserted on the shared cases of tests/anchors_reference.py; csrc/sg_anchors.h compiled for the host (tests/host_harness/anchors_walk.cpp)
against the restatement, byte for byte; what snowgpu_assign_anchors_device refuses, in which words and in which order
(tests/host_harness/anchors_refusals.cpp); the layout of anchor_grid; and that the entry is declared and bound."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import anchors_reference as ar
from conftest import ROOT
from lidar_snow_sim_amd.stages import AnchorTargetBatch, assign_anchors  # noqa: F401  (the stage all of this is about: without it nothing here runs)

DTYPES = ar.DTYPES
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---- the shared cases meet the conditions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_by_hand(dtype):
    """a0 on g0: 1.  a1 one metre off: 3 x 2 / (8 + 8 - 6) = 0.6 = matched: positive.  a2 1.5 m off: 5 / 11, between the thresholds and not
    g0's best: ignored.  a3 two metres off g1: 4 / 12, below unmatched but g1's best: forced.  a4 (class 2) a quarter off g2:
    0.75 / 1.25 = 0.6.  a5 meets nothing: background."""
    e = ar.expected("by_hand", dtype)
    assert e["label"].tolist() == [[1, 1, -1, 1, 2, 0]] and e["gt_index"].tolist() == [[0, 0, -1, 1, 2, -1]]
    assert e["count"].tolist() == [[4, 1, 1]] and e["gt_count"].tolist() == [[2, 1, 1]]
    assert e["iou"].dtype == np.dtype(dtype) and e["iou"][0].tolist() == [np.dtype(dtype).type(v) for v in (1.0, 0.6, 5 / 11, 4 / 12, 0.6, 0.0)]
    assert e["forced"].tolist() == [[True, False, False, True, True, False]] and e["best"][0, 1] == 0.6


@pytest.mark.parametrize("dtype", DTYPES)
def test_thresholds(dtype):
    """The two judged anchors sit at 0.5 and 0.25 exactly and are no gt's best: every comparison of the label rule is met from either side."""
    seen = set()
    for i, name in enumerate(ar.THRESHOLD_NAMES):
        c, e = ar.case(name, dtype), ar.expected(name, dtype)
        (m,), (u,) = c["matched"], c["unmatched"]
        assert (m, u) == ar.THRESHOLD_SETTINGS[i] and 0 < u <= m <= 1
        assert e["best"][0].tolist() == [0.5, 1.0, 0.25, 1.0] and e["forced"][0].tolist() == [False, True, False, True]
        for a, v in ((ar.P_HALF, 0.5), (ar.P_QUARTER, 0.25)):
            want = 1 if v >= m else (0 if v < u else -1)
            assert e["label"][0, a] == want
            seen.add((v, np.sign(m - v), np.sign(u - v), want))
        assert e["label"][0, [ar.Q_HALF, ar.Q_QUARTER]].tolist() == [1, 1]
    for v in (0.5, 0.25):                                      # matched below, at and above the overlap; unmatched likewise
        assert {s[1] for s in seen if s[0] == v} == {-1, 0, 1} and {s[2] for s in seen if s[0] == v} == {-1, 0, 1}
        assert {s[3] for s in seen if s[0] == v} == {1, 0, -1}
    assert (0.5, 1, 0, -1) in seen and (0.5, 1, 1, 0) in seen and (0.25, 0, 0, 1) in seen and (0.25, 1, 0, -1) in seen


@pytest.mark.parametrize("dtype", DTYPES)
def test_headings(dtype):
    c, e = ar.case("headings", dtype), ar.expected("headings", dtype)
    hs = ar.heading_values()
    t = np.dtype(dtype).type
    assert len(hs) == 30 and np.signbit(hs[-1]) and hs[-1] == 0 and np.signbit(c["gt_boxes"][0, 2 * 29, 6])
    for base in (np.pi / 4, -np.pi / 4, 3 * np.pi / 4, 5 * np.pi / 4):
        d, s = np.float64(base), np.float32(base)
        assert {float(d), float(np.nextafter(d, np.inf)), float(np.nextafter(d, -np.inf)), float(s), float(np.nextafter(s, np.float32(np.inf))),
                float(np.nextafter(s, np.float32(-np.inf)))} <= set(hs)
    kept = swapped = 0
    for i, h in enumerate(hs):
        h = float(t(h))                                        # the heading the case holds
        turn = abs(h - np.floor(h / np.pi + 0.5) * np.pi)
        swap = not turn < np.pi / 4
        for row in (0, 2):                                     # the gt turns; the anchor turns
            first, second = e["best"][0, 4 * i + row], e["best"][0, 4 * i + row + 1]
            assert first == (4 / 12 if swap else 1.0) and second == (4 / 11 if swap else 7 / 8), (i, h, row)
            assert e["label"][0, 4 * i + row] == (0 if swap else 1) and e["label"][0, 4 * i + row + 1] == 1
        kept, swapped = kept + (not swap), swapped + swap
    assert kept >= 8 and swapped >= 8
    # a step across pi / 4 changes the answer, in the format of the case
    near = [float(t(v)) for v in hs[:6]]
    turns = [abs(v - np.floor(v / np.pi + 0.5) * np.pi) < np.pi / 4 for v in near]
    assert True in turns and False in turns
    assert abs(1e5 - np.floor(1e5 / np.pi + 0.5) * np.pi) < np.pi / 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_forced(dtype):
    e = ar.expected("forced", dtype)
    A, G = ar.FORCED, ar.FORCED_GT
    label, arg, best, forced, top = e["label"][0], e["gt_index"][0], e["best"][0], e["forced"][0], e["top"][0]
    # below unmatched but the gt's best: positive
    assert 0 < best[A["low"]] == top[G["low"]] == 2 / 14 < 0.45 and forced[A["low"]] and label[A["low"]] == 1 and arg[A["low"]] == G["low"]
    # two anchors at the same overlap of one gt: both forced
    assert best[A["tie_a"]] == best[A["tie_b"]] == top[G["tie"]] == 5 / 11 < 0.6 and forced[A["tie_a"]] and forced[A["tie_b"]]
    assert label[[A["tie_a"], A["tie_b"]]].tolist() == [1, 1] and e["gt_count"][0, G["tie"]] == 2
    # a gt that meets no anchor
    assert top[G["nothing"]] == 0 and e["gt_count"][0, G["nothing"]] == 0 and not (arg == G["nothing"]).any()
    # the quirk: forced by one gt, assigned its own arg -- and positive only because it was forced
    q = A["quirk"]
    assert top[G["quirk_forcing"]] == 2 / 14 and forced[q] and best[q] == 5 / 11 < 0.6 and top[G["quirk_own"]] == 1.0
    assert label[q] == 1 and arg[q] == G["quirk_own"] and e["gt_count"][0, G["quirk_forcing"]] == 0 and e["gt_count"][0, G["quirk_own"]] == 2
    # two bit-equal gts: the smaller number
    assert arg[A["twin"]] == G["twin_a"] < G["twin_b"] and e["gt_count"][0, G["twin_b"]] == 0 and top[G["twin_a"]] == top[G["twin_b"]] > 0
    # ties across waves and workgroups
    far = [A["far_a"], A["far_b"], A["far_c"]]
    assert far[1] // 64 != far[0] // 64 and far[1] // 256 == far[0] // 256 and far[2] - far[0] > 1024
    assert forced[far].all() and (best[far] == top[G["far"]]).all() and top[G["far"]] == 5 / 11 and e["gt_count"][0, G["far"]] == 3
    # a gt of another class on an anchor takes no part; the filler is background
    assert e["gt_count"][0, G["other_class"]] == 0 and top[G["other_class"]] == 0
    assert e["count"][0].tolist() == [9, A["n"] - 9, 0] and (label[20:60] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_absent(dtype):
    c, e = ar.case("absent", dtype), ar.expected("absent", dtype)
    gone = sorted(ar.ABSENT_ANCHORS.values())
    assert not e["anchor_ok"][gone].any() and e["anchor_ok"].sum() == 20 - 3
    for f in range(3):
        assert (e["label"][f, gone] == -1).all() and (e["gt_index"][f, gone] == -1).all() and not e["iou"][f, gone].any()
        assert e["count"][f].sum() == 17
    cls0 = ar.gt_class(c["gt_boxes"][0], 3)
    assert cls0.tolist() == [0] * 9 + [1, 1, 1, 1, 2]
    # every absent gt of frame 0 lies on an anchor it would win, every absent anchor under a gt it would win
    assert e["gt_count"][0].tolist() == [0] * 12 + [1, 1] and e["count"][0].tolist() == [2, 15, 0]
    assert e["label"][0, [1, 2, 6, 7, 8]].tolist() == [0] * 5 and e["label"][0, 9] == 1 and e["label"][0, 12] == 2
    assert (e["label"][0, 16:] == 0).all()                     # class 3 has no gt in frame 0: all background
    # a frame without any gt: all background
    assert e["count"][1].tolist() == [0, 17, 0] and not e["gt_count"][1].any() and not e["iou"][1].any()
    assert e["count"][2].tolist() == [3, 14, 0] and e["label"][2, [0, 13, 18]].tolist() == [1, 2, 3]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ar.GRID_NAMES)
def test_grid(name, dtype):
    c, e = ar.case(name, dtype), ar.expected(name, dtype)
    F, B = c["gt_boxes"].shape[:2]
    assert c["anchors"].shape == (3300, 7) and 3300 % 64 and 3300 % 256 and F == 3 and f"grid_b{B}" == name
    for f in range(F):
        label = e["label"][f]
        assert (label > 0).any() and (label == 0).any() and (label == -1).any() and e["forced"][f].any()
        assert (e["forced"][f] & (e["best"][f] < 0.5)).any()                                    # someone is positive only because forced
        assert e["count"][f].sum() == 3300 and e["gt_count"][f].sum() == e["count"][f, 0]
    if B >= 64:
        assert {1, 2, 3} <= set(e["label"].reshape(-1).tolist())


def test_the_cases_the_gpu_tests_run():
    assert {"by_hand", "headings", "forced", "absent"} <= set(ar.CASE_NAMES) and len(ar.THRESHOLD_NAMES) == len(ar.THRESHOLD_SETTINGS) >= 9
    assert sorted(int(n[6:]) for n in ar.GRID_NAMES) == [1, 64, 65, 256]


# ---- the layout of anchor_grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align_center", (False, True))
def test_anchor_grid_layout(align_center):
    import torch
    from lidar_snow_sim_amd.stages import anchor_grid
    anchors, cls = anchor_grid(ar.GRID_RANGE, ar.GRID_N, ar.GRID_SIZES, ar.GRID_ROTATIONS, ar.GRID_BOTTOMS, align_center=align_center, dtype=torch.float64,
                               device="cpu")
    want, want_cls = ar.grid_anchors(align_center)
    assert anchors.dtype == torch.float64 and cls.dtype == torch.int32 and anchors.is_contiguous()
    assert anchors.numpy().tobytes() == want.tobytes() and cls.numpy().tobytes() == want_cls.tobytes()
    nx, ny = ar.GRID_N
    lo, hi = ar.GRID_RANGE[:3], ar.GRID_RANGE[3:]
    NC, R = 3, 2
    for (y, x, c, r) in ((0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0), (3, 7, 2, 1), (ny - 1, nx - 1, NC - 1, R - 1)):
        a = ((y * nx + x) * NC + c) * R + r
        cx = lo[0] + (x + 0.5) * ((hi[0] - lo[0]) / nx) if align_center else lo[0] + x * ((hi[0] - lo[0]) / (nx - 1))
        cy = lo[1] + (y + 0.5) * ((hi[1] - lo[1]) / ny) if align_center else lo[1] + y * ((hi[1] - lo[1]) / (ny - 1))
        size = ar.GRID_SIZES[c]
        assert anchors[a].tolist() == [cx, cy, ar.GRID_BOTTOMS[c] + size[2] / 2, *size, ar.GRID_ROTATIONS[r]] and int(cls[a]) == c + 1
    single = anchor_grid(ar.GRID_RANGE, ar.GRID_N, ar.GRID_SIZES, ar.GRID_ROTATIONS, ar.GRID_BOTTOMS, align_center=align_center, device="cpu")[0]
    assert single.dtype == torch.float32 and torch.equal(single, anchors.float())
    with pytest.raises(ValueError, match="one .dx, dy, dz. per class"):
        anchor_grid(ar.GRID_RANGE, ar.GRID_N, ar.GRID_SIZES, ar.GRID_ROTATIONS, ar.GRID_BOTTOMS[:2], device="cpu")


# ---- csrc/sg_anchors.h on the host --------------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra, "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "anchors_walk.cpp"), "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("anchors"), "anchors_walk")


def _walk(exe, tmp_path, c):
    """The outputs of the harness on case c, as a dict of arrays shaped like the restatement's."""
    A, Ca = c["anchors"].shape
    F, B, Cg = c["gt_boxes"].shape
    dt = c["anchors"].dtype
    fin, fout = tmp_path / "case.in", tmp_path / "case.out"
    with open(fin, "wb") as fp:
        for a in (c["anchors"], c["anchor_class"], c["gt_boxes"]):
            fp.write(np.ascontiguousarray(a).tobytes())
    args = [int(dt == np.float64), F, A, B, Ca, Cg, len(c["matched"]), *(repr(v) for v in c["matched"]), *(repr(v) for v in c["unmatched"])]
    r = subprocess.run([str(exe), *(str(a) for a in args), str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    shapes = dict(label=((F, A), np.int32), gt_index=((F, A), np.int32), count=((F, 3), np.int32), gt_count=((F, B), np.int32), iou=((F, A), dt))
    blob, at, got = fout.read_bytes(), 0, {}
    for name in ar.FIELDS:
        shape, kind = shapes[name]
        n = int(np.prod(shape)) * np.dtype(kind).itemsize
        got[name] = np.frombuffer(blob[at:at + n], kind).reshape(shape)
        at += n
    assert at == len(blob)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ar.CASE_NAMES)
def test_the_header_on_the_host_equals_the_restatement(walk, tmp_path, name, dtype):
    c, e = ar.case(name, dtype), ar.expected(name, dtype)
    got = _walk(walk, tmp_path, c)
    for field in ar.FIELDS:
        assert got[field].tobytes() == e[field].tobytes(), field


def test_the_header_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan -- host code only, a stand-alone program: the records and the words stay inside
    their arrays at B = 256 and with every kind of absent box."""
    exe = _compile(tmp_path, "anchors_walk_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    for name, dtype in (("grid_b256", "float64"), ("absent", "float32"), ("forced", "float32")):
        c, e = ar.case(name, dtype), ar.expected(name, dtype)
        got = _walk(exe, tmp_path, c)
        for field in ar.FIELDS:
            assert got[field].tobytes() == e[field].tobytes(), (name, dtype, field)


# ---- the refusal walk -------------------------------------------------------------------------------------------------------------------------
WHO = "snowgpu_assign_anchors_device"
APART = "; the anchors, their classes and the gt boxes are read while the targets are written: pass a buffer apart from them"
OWN = "; every output needs memory of its own"
MESSAGES = {
    "null": WHO + ": null pointer or bad dtype",
    "anchors": WHO + ": n_anchors must be at least 1",
    "gt": WHO + ": n_gt must lie in 1 .. 256",
    "anchor_features": WHO + ": anchor_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first",
    "gt_features": WHO + ": gt_features must lie in 8 .. 10: cx, cy, cz, dx, dy, dz, heading, class first",
    "classes": WHO + ": n_classes must lie in 1 .. 16",
    "thresholds": WHO + ": every class needs 0 < unmatched <= matched <= 1",
    "elements": WHO + ": n_frames * n_anchors exceeds 2^31 - 1; split the batch",
}
ORDER = tuple(MESSAGES)              # the order of the checks: a call wrong in two ways gets the earlier message
DOUBLY = ("null_anchors_and_anchors_0", "anchors_0_and_gt_0", "gt_0_and_anchor_features_6", "anchor_features_6_and_gt_features_7", "gt_features_7_and_classes_0",
          "classes_17_and_unmatched_0", "unmatched_0_and_elements_at_2p31", "elements_at_2p31_and_label_is_anchors")              # one per check and the one behind it
PAIRS = {("label", "anchors"): ("label_is_anchors", "label_overlaps_anchors"), ("gt_index", "anchor_class"): ("gt_index_is_anchor_class",),
         ("count", "gt_boxes"): ("count_overlaps_gt_boxes",), ("gt_count", "gt_boxes"): ("gt_count_is_gt_boxes",), ("iou", "anchor_class"): ("iou_overlaps_anchor_class",)}
OUTS = {("gt_index", "label"): ("gt_index_is_label",), ("count", "label"): ("count_overlaps_label",), ("gt_count", "count"): ("gt_count_is_count",),
        ("iou", "gt_count"): ("iou_overlaps_gt_count",), ("iou", "gt_index"): ("iou_is_gt_index",)}
ACCEPTED = ("clean", "null_out_iou", "float64", "anchors_1", "gt_1", "gt_256", "anchor_features_10", "gt_features_10", "classes_1", "classes_16",
            "unmatched_equals_matched", "matched_1", "a_class_beyond_nc_is_not_read", "elements_at_2p31_minus_1", "label_behind_anchors",
            "iou_behind_anchor_class", "count_behind_label")
REFUSED = {
    "null": ("null_anchors", "null_anchor_class", "null_gt_boxes", "null_matched", "null_unmatched", "null_out_label", "null_out_gt_index", "null_out_count",
             "null_out_gt_count", "bad_dtype", "no_frames", "null_anchors_and_anchors_0"),
    "anchors": ("anchors_0", "anchors_negative", "anchors_0_and_gt_0"),
    "gt": ("gt_0", "gt_257", "gt_0_and_anchor_features_6"),
    "anchor_features": ("anchor_features_6", "anchor_features_11", "anchor_features_6_and_gt_features_7"),
    "gt_features": ("gt_features_7", "gt_features_11", "gt_features_7_and_classes_0"),
    "classes": ("classes_0", "classes_17", "classes_17_and_unmatched_0"),
    "thresholds": ("unmatched_0", "unmatched_negative", "unmatched_above_matched", "matched_above_1", "matched_nan", "unmatched_nan", "unmatched_0_and_elements_at_2p31"),
    "elements": ("elements_at_2p31", "elements_overflowing", "elements_at_2p31_and_label_is_anchors"),
}


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "anchors_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "anchors_refusals.cpp"), "-o", str(exe)]
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
    # the order: the checks stand in sg_check_anchors_args in the order of MESSAGES, the overlaps behind them -- every "<first>_and_<second>"
    # case of the harness is wrong in two ways, of checks next to each other, and is filed above under the earlier one
    for key, later, case in zip(ORDER, ORDER[1:] + (None,), DOUBLY):
        first, second = case.split("_and_")
        assert first in REFUSED[key] and case in REFUSED[key], case
        assert second in REFUSED[later] if later else any(second in cases for cases in PAIRS.values()), case


def test_the_entry_is_declared_and_bound():
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    assert "int snowgpu_assign_anchors_device(" in header and "snowgpu_assign_anchors_device" in _native.EXPORTS
    assert hasattr(_native.lib(), "snowgpu_assign_anchors_device") and hasattr(_native.Context, "assign_anchors_device")
    assert "snowgpu_anchors.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import anchors, stages, tensors
    assert tensors.assign_anchors is stages.assign_anchors and tensors.AnchorTargetBatch is stages.AnchorTargetBatch and tensors.anchor_grid is stages.anchor_grid
    assert callable(anchors.assign_targets) and tuple(anchors.FIELDS) == tuple(ar.FIELDS)
    assert callable(tensors.AnchorTargetBatch.empty) and isinstance(tensors.AnchorTargetBatch.positive, property)
    assert all(callable(getattr(tensors.AnchorTargetBatch, n)) for n in ("matched", "reg_weights", "cls_weights"))
