"""No GPU: the conditions that keep the comparisons of tests/test_gpu_iou.py from being vacuous.  The NumPy restatement of rotated box IoU
and NMS (tests/iou_reference.py) on analytic cases; against an independent method (edge intersections, contained corners, an angular sort)
on every shared case, within the tolerance derived there, with every NMS and best decision further from its threshold and its runner-up
than that tolerance, so that the independent method gives the same index lists; what each case must contain; csrc/sg_iou.h compiled for
the host (tests/host_harness/iou_clip.cpp) on millions of adversarial pairs and byte for byte against the restatement; the refusals of
both entries; and (5) the adversarial families and exact ties the device meets in tests/test_gpu_iou.py: the host build equal to the
restatement on every designed and incidental pair, the independent method within the pair's own TOL_AREA, what each must contain."""
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import iou_reference as ir

ROOT = Path(__file__).resolve().parent.parent
HIPCC = "/opt/rocm/bin/hipcc"
TOL_A, TOL_I = ir.case_tol_area(), ir.case_tol_iou()


def _box(cx, cy, dx, dy, h, cz=0.0, dz=2.0):
    return np.array([[cx, cy, cz, dx, dy, dz, h]], np.float64)


def _area(a, b, method=ir.clip_area):
    return float(method(a, ir.numpy_pose(a), b, ir.numpy_pose(b))[0])


# ---- 1. analytic cases ------------------------------------------------------------------------------------------------------------------------
def test_the_tolerance_is_what_the_derivation_says():
    assert 1.0e-11 < TOL_A < 1.1e-11 and TOL_I == 2 * TOL_A / 4.5 + 8 * ir.EPS and TOL_I < 5e-12


def test_axis_aligned_overlap_is_the_product_of_interval_overlaps_exactly():
    rng = np.random.default_rng(5)
    n = 400
    a = np.column_stack((rng.integers(-40, 40, n) / 4, rng.integers(-40, 40, n) / 4, np.zeros(n), rng.integers(1, 24, n) / 2, rng.integers(1, 24, n) / 2, np.ones(n), np.zeros(n)))
    b = np.column_stack((rng.integers(-40, 40, n) / 4, rng.integers(-40, 40, n) / 4, np.zeros(n), rng.integers(1, 24, n) / 2, rng.integers(1, 24, n) / 2, np.ones(n), np.zeros(n)))
    ox = np.maximum(np.minimum(a[:, 0] + a[:, 3] / 2, b[:, 0] + b[:, 3] / 2) - np.maximum(a[:, 0] - a[:, 3] / 2, b[:, 0] - b[:, 3] / 2), 0)
    oy = np.maximum(np.minimum(a[:, 1] + a[:, 4] / 2, b[:, 1] + b[:, 4] / 2) - np.maximum(a[:, 1] - a[:, 4] / 2, b[:, 1] - b[:, 4] / 2), 0)
    got = ir.clip_area(a, ir.numpy_pose(a), b, ir.numpy_pose(b))                  # (quarters and halves: every operation is exact)
    assert np.array_equal(got, ox * oy) and (got > 0).sum() > 50 and (got == 0).sum() > 50


def test_analytic_cases():
    sq = _box(0, 0, 2, 2, 0)
    for method in (ir.clip_area, ir.area_independent):
        assert abs(_area(sq, _box(0, 0, 2, 2, math.pi / 4), method) - 8 * (math.sqrt(2) - 1)) <= TOL_A
        assert abs(_area(_box(0, 0, 2, 2, math.pi / 4), sq, method) - 8 * (math.sqrt(2) - 1)) <= TOL_A
        assert _area(sq, _box(5, 0, 2, 2, 0.3), method) == 0.0 and _area(sq, _box(1.5, 1.9, 1, 1, math.pi / 4), method) == 0.0       # disjoint
        assert abs(_area(_box(0.2, -0.1, 1, 0.5, 0.7), sq, method) - 0.5) <= TOL_A and abs(_area(sq, _box(0.2, -0.1, 1, 0.5, 0.7), method) - 0.5) <= TOL_A
        assert abs(_area(sq, sq, method) - 4.0) <= TOL_A
        assert _area(sq, _box(2, 0, 2, 2, 0), method) <= TOL_A and _area(sq, _box(2, 2, 2, 2, 0), method) <= TOL_A                   # a shared edge, a shared corner
        assert _area(sq, _box(1 + math.sqrt(0.5), 0, 1, 1, math.pi / 4), method) <= TOL_A                                            # a corner on an edge
    a, b = _box(0, 0, 4, 2, 0, cz=0.0, dz=2.0), _box(1, 0, 4, 2, 0, cz=1.5, dz=2.0)
    ok = np.ones(1, bool)
    assert ir.pair_iou(a, ir.numpy_pose(a), ok, b, ir.numpy_pose(b), ok, "bev")[0] == 6.0 / 10.0
    assert ir.pair_iou(a, ir.numpy_pose(a), ok, b, ir.numpy_pose(b), ok, "3d")[0] == 3.0 / 29.0                                      # h = 0.5: 3 / (16 + 16 - 3)
    far = _box(1, 0, 4, 2, 0, cz=5.0)
    assert ir.pair_iou(a, ir.numpy_pose(a), ok, far, ir.numpy_pose(far), ok, "3d")[0] == 0.0
    assert ir.pair_iou(a, ir.numpy_pose(a), ok, far, ir.numpy_pose(far), ~ok, "bev")[0] == 0.0                                       # an absent box


def test_the_loop_and_the_vectors_agree():
    rng = np.random.default_rng(6)
    n = 600
    a = ir.clustered(rng, n, 40)[:, :7]
    b = a.copy()
    b[:, :2] += rng.normal(0, 1.5, (n, 2))
    b[:, 6] += rng.normal(0, 0.5, n)
    b[:60] = a[:60]
    b[60:120, 6] = np.nextafter(a[60:120, 6], 9.0)
    b[120:180, 6] += math.pi / 2
    pa, pb = ir.numpy_pose(a), ir.numpy_pose(b)
    vec, most = ir.clip_area(a, pa, b, pb, return_most=True)
    assert vec.tobytes() == np.array([ir.area_scalar(a[i], pa[i], b[i], pb[i]) for i in range(n)]).tobytes() and (vec > 0).sum() > 200
    assert 8 <= most.max() <= 19                                      # (equal boxes: more vertices than geometry has, fewer than the slots)
    ind = ir.area_independent(a, pa, b, pb)
    assert np.abs(ind - np.array([ir.area_independent_one(a[i], pa[i], b[i], pb[i]) for i in range(n)])).max() <= TOL_A
    assert np.abs(ind - vec).max() <= TOL_A


# ---- 2. the shared cases: the independent method, the margins, the content -------------------------------------------------------------------
def _frame_trace(c, f):
    trace = []
    kept = ir.nms_frame(c["boxes"][f], c["scores"][f], c["pose"][f], c["iou_thresh"], c["post_max"], c["score_thresh"], c["mode"], trace=trace)
    return kept, trace


def _find_chain(c, f, limit=256):
    """(A, B, C): A kept and suppresses B; B alone would suppress the later C; C is kept.  Among the first `limit` ranked candidates."""
    boxes, pose, th = c["boxes"][f], c["pose"][f], c["iou_thresh"]
    order = ir.ranking(boxes, c["scores"][f], pose, c["score_thresh"])[:limit]
    kept = set(ir.nms_frame(boxes, c["scores"][f], pose, th, c["post_max"], c["score_thresh"], c["mode"]).tolist())
    b, n = boxes[:, :7].astype(np.float64), len(order)
    jj, ii = np.tril_indices(n, -1)
    ok = np.ones(len(jj), bool)
    v = np.zeros((n, n))
    v[jj, ii] = ir.pair_iou(b[order[jj]], pose[order[jj]], ok, b[order[ii]], pose[order[ii]], ok, c["mode"])
    for rb in range(n):
        if order[rb] in kept:
            continue
        sup = [ra for ra in range(rb) if order[ra] in kept and v[rb, ra] > th]
        later = [rc for rc in range(rb + 1, n) if order[rc] in kept and v[rc, rb] > th]
        if sup and later:
            return int(order[sup[0]]), int(order[rb]), int(order[later[0]])
    return None


@pytest.mark.parametrize("dtype", ir.DTYPES)
@pytest.mark.parametrize("name", ir.NMS_CASES)
def test_nms_cases(name, dtype):
    c, e = ir.nms_case(name, dtype), ir.nms_expected(name, dtype)
    other = ir.nms(c["boxes"], c["scores"], c["pose"], c["iou_thresh"], c["post_max"], c["score_thresh"], c["mode"], area=ir.area_independent)
    for k in e:
        assert e[k].tobytes() == other[k].tobytes(), (name, dtype, k)          # the same lists by the independent method, nothing left out
    b = c["boxes"][..., :7].astype(np.float64)
    pres = ir.present(c["boxes"], c["pose"])
    assert np.abs(b[pres][:, :2]).max() <= 50 and (b[pres][:, 3] <= 6).all() and (b[pres][:, 4] <= 3).all() and (b[pres][:, 3] * b[pres][:, 4]).min() >= ir.CASE_AMIN
    for f in range(len(b)):
        kept, trace = _frame_trace(c, f)
        assert np.array_equal(kept, e["index"][f, :e["count"][f]])
        decided = np.concatenate(trace) if trace else np.zeros(0)
        if decided.size:                                                       # every decision keeps its distance from the threshold
            assert np.abs(decided - c["iou_thresh"]).min() > TOL_I, (name, dtype, f)
        cand = len(ir.ranking(c["boxes"][f], c["scores"][f], c["pose"][f], c["score_thresh"]))
        if cand >= 60:
            assert 1 < len(kept) < cand and _find_chain(c, f) is not None, (name, dtype, f, len(kept), cand)
    assert (e["kept"].sum(axis=1) == e["count"]).all() and (e["index"] >= 0).sum() == e["count"].sum()


@pytest.mark.parametrize("dtype", ir.DTYPES)
@pytest.mark.parametrize("name", ir.NMS_CASES)
def test_the_blocked_walk_equals_the_plain_walk(name, dtype):
    """nms_frame() walks the ranking in blocks, as the device's sweep does; here it is held to the definition's own walk, one candidate
    at a time, on every case and frame -- a mistake in the block logic that both shared would show here."""
    c, e = ir.nms_case(name, dtype), ir.nms_expected(name, dtype)
    for f in range(len(c["boxes"])):
        plain = ir.nms_frame_plain(c["boxes"][f], c["scores"][f], c["pose"][f], c["iou_thresh"], c["post_max"], c["score_thresh"], c["mode"])
        assert np.array_equal(plain, e["index"][f, :e["count"][f]]), (name, dtype, f)
    if name == "b129":                                                         # and where post_max cuts inside a block, and at 1
        for post_max in (1, 5, 70):
            want = ir.nms(c["boxes"], c["scores"], c["pose"], c["iou_thresh"], post_max)
            plain = ir.nms_frame_plain(c["boxes"][0], c["scores"][0], c["pose"][0], c["iou_thresh"], post_max)
            assert np.array_equal(plain, want["index"][0, :want["count"][0]])


def test_what_the_nms_cases_contain():
    natural = {n: ir.nms(*(ir.nms_case(n)[k] for k in ("boxes", "scores", "pose", "iou_thresh")), ir.nms_case(n)["boxes"].shape[1])["count"] for n in ("b64", "mixed")}
    assert natural["b64"][0] > ir.nms_case("b64")["post_max"] == ir.nms_expected("b64")["count"][0]           # post_max cuts here
    assert (ir.nms_expected("mixed")["count"] < ir.nms_case("mixed")["post_max"]).all()                        # and not here
    assert ir.nms_expected("b1")["index"].tolist() == [[0]] and ir.nms_expected("b2")["index"].tolist() == [[int(np.argmax(ir.nms_case("b2")["scores"][0])), -1]]
    e = ir.nms_expected("chain")                                               # A suppresses B; B alone would suppress C; C and the loner are kept
    assert e["index"].tolist() == [[0, 2, 3, -1]] and _find_chain(ir.nms_case("chain"), 0) == (0, 1, 2)
    for dtype in ir.DTYPES:
        c, e = ir.nms_case("mixed", dtype), ir.nms_expected("mixed", dtype)
        s, pres = c["scores"], ir.present(c["boxes"], c["pose"])
        assert np.isnan(s[0, 40]) and not e["kept"][0, 40] and np.isinf(s[0, 41]) and e["index"][0, 0] == 41
        assert not pres[1].any() and e["count"][1] == 0 and (e["index"][1] == -1).all() and not e["boxes"][1].any()
        assert not pres[0, 5] and not pres[0, 6] and not e["kept"][0, [5, 6]].any()
        assert ((s[0] < ir.SCORE_CUT) & pres[0]).sum() >= 3 and not e["kept"][0][s[0] < ir.SCORE_CUT].any()
        assert np.signbit(s[0, 30]) and s[0, 30] == s[0, 31] and len(set(s[2, :60].tolist())) <= 11
        order = ir.ranking(c["boxes"][0], s[0], c["pose"][0], c["score_thresh"])
        at = [int(np.flatnonzero(order == k)[0]) for k in (20, 21, 22, 23)]
        assert at == list(range(at[0], at[0] + 4))                             # equal scores: ascending box numbers
        assert e["kept"][0, 8] + e["kept"][0, 9] <= 1                          # of two equal boxes at most one stays
    big = ir.nms_expected("b4160")
    assert big["count"][0] > 64 and ir.nms_expected("b9216")["count"][0] > 20


@pytest.mark.parametrize("dtype", ir.DTYPES)
@pytest.mark.parametrize("mode", ir.MODES)
@pytest.mark.parametrize("name", ir.IOU_CASES)
def test_iou_cases(name, mode, dtype):
    c, e = ir.iou_case(name, dtype), ir.iou_expected(name, dtype, mode)
    other = ir.boxes_iou(c["a"], c["b"], c["pose_a"], c["pose_b"], mode, area=ir.area_independent)
    assert np.abs(other["iou64"] - e["iou64"]).max() <= TOL_I
    assert np.array_equal(other["best"], e["best"]), (name, mode, dtype)       # the same partners by the independent method, no row left out
    v = e["iou64"]
    bb = c["b"][..., :7]
    for f in range(3):
        for m in range(v.shape[1]):
            k = e["best"][f, m]
            if k < 0:
                assert not v[f, m].any() and not other["iou64"][f, m].any()
                continue
            rivals = ~(bb[f] == bb[f, k]).all(axis=1)                          # (an equal box gives an equal value by either method: the smallest number wins)
            assert v[f, m, k] > TOL_I and (not rivals.any() or v[f, m, k] - v[f, m, rivals].max() > TOL_I), (name, mode, dtype, f, m)
    pa, pb = ir.present(c["a"], c["pose_a"]), ir.present(c["b"], c["pose_b"])
    assert pb[0].all() and not pb[2].any() and not e["iou64"][2].any() and (e["best"][2] == -1).all()
    if v.shape[2] >= 2:
        assert 0 < pb[1].sum() < pb[0].sum() and e["best"][0, 1] == 0 and v[0, 1, 0] == v[0, 1, 1] > 0.5          # the tie: the smallest number
    if v.shape[1] >= 63:
        assert not pa[1].all() and (e["best"] >= 0).sum() > 20
        bev = ir.iou_expected(name, dtype, "bev")["iou64"]
        assert ((bev > 0) & (ir.iou_expected(name, dtype, "3d")["iou64"] == 0)).sum() >= 3                         # apart in z only


# ---- 3. csrc/sg_iou.h on the host -------------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra=()):
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    exe = tmp / name
    cmd = [HIPCC, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-w", *extra,
           "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"), "-I", str(ROOT / "include"), str(ROOT / "tests" / "host_harness" / "iou_clip.cpp"),
           "-o", str(exe), "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("iou"), "iou_clip")


def _fixed_pairs():
    """A fixed few thousand pairs (a, pose a, b, pose b): clustered, equal, 1 ulp apart, right angles, shared faces, absent ones, and one
    under a pose that is not NumPy's."""
    rng = np.random.default_rng(7)
    n = 4000
    a = ir.clustered(rng, n, 250)[:, :7]
    b = a.copy()
    b[:, :2] += rng.normal(0, 1.5, (n, 2))
    b[:, 6] += rng.normal(0, 0.5, n)
    b[:200] = a[:200]
    b[200:400, 6] = np.nextafter(a[200:400, 6], 9.0)
    a[400:600, 6] = np.round(a[400:600, 6] / (math.pi / 2)) * (math.pi / 2)
    b[400:600] = a[400:600]
    b[400:600, 6] += math.pi / 2
    b[600:800] = a[600:800]
    b[600:800, 0] += a[600:800, 3] * np.cos(a[600:800, 6])
    b[600:800, 1] += a[600:800, 3] * np.sin(a[600:800, 6])
    a[800:820] = 0.0
    b[820:840, 3] = -1.0
    a[840:860, 0] = np.nan
    pa, pb = ir.numpy_pose(a), ir.numpy_pose(b)
    pa[860:880] = 2.0, 0.0                                            # not a rotation: absent
    pb[880:900] *= 1.0 + 4e-7                                         # within the pose tolerance: used as it is
    return a, pa, b, pb


def test_host_clip_equals_the_restatement_byte_for_byte(harness, tmp_path):
    a, pa, b, pb = _fixed_pairs()
    n = len(a)
    np.ascontiguousarray(np.concatenate((a, pa, b, pb), axis=1)).tofile(tmp_path / "in")
    r = subprocess.run([str(harness), "areas", str(n), str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(tmp_path / "out", np.float64).reshape(n, 3)
    oka, okb = ir.present(a, pa), ir.present(b, pb)
    assert (~oka).sum() == 60 and (~okb).sum() == 20 and okb[880:900].all()
    both = oka & okb
    area = np.zeros(n)
    area[both] = ir.clip_area(a[both], pa[both], b[both], pb[both])
    assert got[:, 0].tobytes() == area.tobytes() and (area > 0).sum() > 1500 and (area == 0).sum() > 500
    for k, mode in ((1, "bev"), (2, "3d")):
        assert got[:, k].tobytes() == ir.pair_iou(a, pa, oka, b, pb, okb, mode).tobytes(), mode
    assert not got[~both].any()


def test_millions_of_adversarial_pairs(harness):
    r = subprocess.run([str(harness), "stress", "1", "4000000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    word, pairs, most, excess, asym = r.stdout.split()
    print("clip on the host:", r.stdout.strip())
    assert word == "stress" and int(pairs) >= 3_900_000 and 8 < int(most) <= 19 and float(excess) <= 1.0 and float(asym) <= 1.0


def test_harness_under_sanitizers(tmp_path):
    """The same program under AddressSanitizer and UBSan: host code only, a stand-alone program."""
    exe = _compile(tmp_path, "iou_clip_san", ("-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([str(exe), "stress", "2", "200000"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.split()[0] == "stress" and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-2000:]


# ---- 4. the refusals, the declarations ------------------------------------------------------------------------------------------------------
IOU, NMS = "snowgpu_boxes_iou_device", "snowgpu_nms_device"
FEATS = ": box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first"
REFUSALS = {
    "iou_clean": "0|OK", "iou_best_only": "0|OK", "iou_m_9216": "0|OK", "iou_same_set": "0|OK", "iou_slots_2p31_minus_1": "0|OK",
    "iou_null_a": f"1|{IOU}: null pointer or bad dtype", "iou_dtype_2": f"1|{IOU}: null pointer or bad dtype", "iou_no_frames": f"1|{IOU}: null pointer or bad dtype",
    "iou_mode_2": f"1|{IOU}: mode must be 0 (BEV) or 1 (3D)", "iou_no_output": f"1|{IOU}: no output: pass d_out_iou, d_out_best or d_out_best_iou",
    "iou_m_0": f"1|{IOU}: the boxes per frame must lie in 1 .. 9216 on either side", "iou_b_9217": f"1|{IOU}: the boxes per frame must lie in 1 .. 9216 on either side",
    "iou_feats_6": f"1|{IOU}{FEATS}", "iou_feats_11": f"1|{IOU}{FEATS}", "iou_slots_2p31": f"1|{IOU}: n_frames * M * B exceeds 2^31 - 1; split the batch",
    "iou_out_is_boxes_b": f"1|{IOU}: d_out_iou overlaps d_boxes_b; the boxes and poses are read while the overlaps are written: pass a buffer apart from them",
    "iou_best_is_iou": f"1|{IOU}: d_out_best overlaps d_out_iou; every output needs memory of its own",
    "nms_clean": "0|OK", "nms_bare": "0|OK", "nms_b_9216": "0|OK", "nms_post_max_b": "0|OK", "nms_minus_inf": "0|OK",
    "nms_null_scores": f"1|{NMS}: null pointer or bad dtype", "nms_null_index": f"1|{NMS}: null pointer or bad dtype", "nms_null_count": f"1|{NMS}: null pointer or bad dtype",
    "nms_mode_m1": f"1|{NMS}: mode must be 0 (BEV) or 1 (3D)", "nms_b_0": f"1|{NMS}: n_boxes must lie in 1 .. 9216", "nms_b_9217": f"1|{NMS}: n_boxes must lie in 1 .. 9216",
    "nms_feats_6": f"1|{NMS}{FEATS}", "nms_feats_11": f"1|{NMS}{FEATS}", "nms_post_max_0": f"1|{NMS}: post_max must lie in 1 .. n_boxes",
    "nms_post_max_b_plus_1": f"1|{NMS}: post_max must lie in 1 .. n_boxes", "nms_nan_iou_thresh": f"1|{NMS}: a threshold is NaN", "nms_nan_score_thresh": f"1|{NMS}: a threshold is NaN",
    "nms_slots_2p31": f"1|{NMS}: n_frames * n_boxes exceeds 2^31 - 1; split the batch",
    "nms_boxes_out_is_boxes": f"1|{NMS}: d_out_boxes overlaps d_boxes; the boxes, scores and pose are read while the keep list is written: pass a buffer apart from them",
    "nms_kept_overlaps_index": f"1|{NMS}: d_out_kept overlaps d_out_index; every output needs memory of its own",
}
# a call wrong in two ways, of checks that stand next to each other, gets the earlier check's message: "<first>_and_<second>"
REFUSALS.update({case: REFUSALS[first] for first, case in (
    ("iou_null_a", "iou_null_a_and_mode_2"), ("iou_mode_2", "iou_mode_2_and_no_output"), ("iou_no_output", "iou_no_output_and_m_0"),
    ("iou_m_0", "iou_m_0_and_feats_6"), ("iou_feats_6", "iou_feats_6_and_slots_2p31"), ("iou_slots_2p31", "iou_slots_2p31_and_out_is_boxes_b"),
    ("nms_null_scores", "nms_null_scores_and_mode_m1"), ("nms_mode_m1", "nms_mode_m1_and_b_0"), ("nms_b_0", "nms_b_0_and_feats_6"),
    ("nms_feats_6", "nms_feats_6_and_post_max_0"), ("nms_post_max_0", "nms_post_max_0_and_nan_iou_thresh"),
    ("nms_nan_iou_thresh", "nms_nan_iou_thresh_and_slots_2p31"), ("nms_slots_2p31", "nms_slots_2p31_and_boxes_out_is_boxes"))})


def test_refusal_walk(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or HIPCC
    exe = tmp_path / "iou_refusals"
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "lidar_snow_sim_amd" / "csrc"),
           str(ROOT / "tests" / "host_harness" / "iou_refusals.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert dict(ln.split("|", 1) for ln in r.stdout.splitlines()) == REFUSALS


def test_the_entries_are_declared_and_bound():
    from lidar_snow_sim_amd import _native
    header = (ROOT / "include" / "snowgpu.h").read_text()
    for name in (IOU, NMS):
        assert f"int {name}(" in header and name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert hasattr(_native.Context, "boxes_iou_device") and hasattr(_native.Context, "nms_device")
    assert "snowgpu_iou.hip" in __import__("lidar_snow_sim_amd.build", fromlist=["SOURCES"]).SOURCES
    from lidar_snow_sim_amd import iou, tensors
    assert callable(tensors.boxes_iou) and callable(tensors.nms) and callable(tensors.IouBatch.empty) and callable(tensors.NmsBatch.empty)
    assert callable(iou.boxes_iou_bev) and callable(iou.boxes_iou3d) and callable(iou.nms)


# ---- 5. the adversarial families and the exact ties of tests/test_gpu_iou.py -------------------------------------------------------------------
def _all_pairs(c, k):
    """Every pair of frame k of a family case: a, pose a, b, pose b (16 900, ...) float64, and which are the designed ones."""
    n = ir.FAMILY_N
    mi, bi = (x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij"))
    return ir._f64(c["a"][k][mi]), c["pose_a"][k][mi], ir._f64(c["b"][k][bi]), c["pose_b"][k][bi], mi == bi


@pytest.mark.parametrize("dtype", ir.DTYPES)
def test_host_clip_equals_the_restatement_on_every_family(harness, tmp_path, dtype):
    """csrc/sg_iou.h on the host, under the given pose, on the designed and the incidental pairs of every family: area, BEV and 3D IoU equal
    the restatement's byte for byte, so the expected values of the device tests are the definition's."""
    c = ir.family_case(dtype)
    assert c["a"].dtype == np.dtype(dtype) and ir.present(c["a"], c["pose_a"]).all() and ir.present(c["b"], c["pose_b"]).all()
    rows, areas = [], []
    for k in range(len(ir.FAMILIES)):
        a, pa, b, pb, _ = _all_pairs(c, k)
        rows.append(np.concatenate((a, pa, b, pb), axis=1))
        areas.append(ir.clip_area(a, pa, b, pb))
    rows = np.ascontiguousarray(np.concatenate(rows))
    n = len(rows)
    rows.tofile(tmp_path / "in")
    r = subprocess.run([str(harness), "areas", str(n), str(tmp_path / "in"), str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(tmp_path / "out", np.float64).reshape(len(ir.FAMILIES), -1, 3)
    for k, name in enumerate(ir.FAMILIES):
        assert got[k, :, 0].tobytes() == areas[k].tobytes(), (name, dtype, "area", int((got[k, :, 0] != areas[k]).sum()))
        for col, mode in ((1, "bev"), (2, "3d")):
            want = ir.family_expected(dtype, mode)["iou64"][k].reshape(-1)
            assert got[k, :, col].tobytes() == want.tobytes(), (name, dtype, mode, int((got[k, :, col] != want).sum()))


@pytest.mark.parametrize("dtype", ir.DTYPES)
@pytest.mark.parametrize("name", ir.FAMILIES)
def test_the_independent_method_on_every_family(name, dtype):
    """Within TOL_AREA(R, L) of the PAIR (the bound the harness's stress mode uses), every designed and incidental pair; the independent
    method with the pair's vertex error as slack (iou_reference.area_independent says why the families need it)."""
    a, pa, b, pb, _ = _all_pairs(ir.family_case(dtype), ir.FAMILIES.index(name))
    L = np.maximum(np.hypot(a[:, 3], a[:, 4]), np.hypot(b[:, 3], b[:, 4]))
    R = np.maximum(np.abs(a[:, :2]).max(axis=1), np.abs(b[:, :2]).max(axis=1)) + L
    err = np.abs(ir.clip_area(a, pa, b, pb) - ir.area_independent(a, pa, b, pb, slack=32 * ir.EPS * R))
    assert (err <= ir.tol_area(R, L)).all(), (name, dtype, float((err / ir.tol_area(R, L)).max()))


@pytest.mark.parametrize("dtype", ir.DTYPES)
def test_what_the_families_contain(dtype):
    """What keeps the device comparison from being vacuous, by the restatement alone, over the DESIGNED pairs of each family."""
    c = ir.family_case(dtype)
    s = {name: ir.designed_stats(c["a"][k], c["b"][k]) for k, name in enumerate(ir.FAMILIES)}
    assert c["a"].shape == (10, 130, 7) and c["b"].shape == (10, 130, 9)
    assert (s["equal"]["most"] > 8).sum() >= 3 and (c["a"][0] == c["b"][0, :, :7]).all()
    assert (c["a"][0, :10, 6] == 0).all() and np.array_equal(s["equal"]["area"][:10], (c["a"][0, :10, 3] * c["a"][0, :10, 4]).astype(np.float64))   # dyadic: exact
    for name in ("right_angle", "one_ulp", "sliver"):
        assert (s[name]["area"] > 0).sum() >= 40, name
    for name in ir.BOUNDARY_FAMILIES:                                  # pairs whose area `<` for `<=` in the clip would change (rarer in float32: what 12 000 draws gave)
        k = ir.FAMILIES.index(name)
        least = 8 if name in ("equal", "right_angle") else 10 if dtype == "float64" else 0
        assert ir.boundary_decides(c["a"][k], c["b"][k]).sum() >= least, name
    T = np.dtype(dtype).type
    ha, hb = c["a"][2, :, 6], c["b"][2, :, 6]
    assert (hb != ha).all() and ((np.nextafter(ha, T(10)) == hb) | (np.nextafter(ha, T(-10)) == hb)).all()                  # 1 ulp of T
    assert (s["shared_face"]["area"] == 0).sum() >= 20 and (s["shared_face"]["area"] > 0).sum() >= 20
    for u, clamp in (("u_bev", ir.EPS_BEV), ("u_3d", ir.EPS_3D)):
        assert (s["clamped"][u] <= clamp).sum() >= 50 and (s["clamped"][u] > clamp).sum() >= 10, u
        assert ((s["clamped"][u] <= clamp) & (s["clamped"][u] > clamp / 10) & (s["clamped"]["area"] > 0)).sum() >= 10, u    # a clamp ten times smaller would show
    z = s["z_sliver"]
    assert ((z["bev"] > 0) & (z["i3d"] > 0)).sum() >= 20 and ((z["bev"] > 0) & (z["i3d"] == 0)).sum() >= 20
    a, b = ir._f64(c["a"][8]), ir._f64(c["b"][8])
    d = np.minimum(a[:, 2] + a[:, 5] * 0.5, b[:, 2] + b[:, 5] * 0.5) - np.maximum(a[:, 2] - a[:, 5] * 0.5, b[:, 2] - b[:, 5] * 0.5)
    assert ((d > 0) & (d <= 1e-9)).sum() >= 20 and ((d <= 0) & (d >= -1e-9)).sum() >= 20                                   # heights that meet, and miss, by a sliver
    for mode in ir.MODES:
        e = ir.family_expected(dtype, mode)
        assert e["iou"].dtype == np.dtype(dtype) and (e["best"] >= 0).sum() > 1000 and np.isfinite(e["iou64"]).all()
        if dtype == "float32":
            v = e["iou"][ir.FAMILIES.index("clamped")]
            assert ((v != 0) & (np.abs(v) < ir.F32_TINY)).sum() >= 4 and ((np.diag(v) != 0) & (np.abs(np.diag(v)) < ir.F32_TINY)).sum() >= 4, mode
        p = ir.pairs_expected(ir.family_pairs(c), mode)                                                                    # the one-pair frames say what the diagonals say
        diag = np.stack([np.diag(e["iou"][k]) for k in range(len(ir.FAMILIES))]).reshape(-1)
        assert p["iou"].reshape(-1).tobytes() == diag.tobytes() and (p["best"] == 0).sum() > 600 and (p["best"] == -1).sum() > 100


@pytest.mark.parametrize("dtype", ir.DTYPES)
def test_what_the_tie_cases_contain(dtype):
    c = ir.best_tie_case(dtype)
    for mode in ir.MODES:
        e = ir.boxes_iou(c["a"], c["b"], c["pose_a"], c["pose_b"], mode)
        for f in range(2):
            for g, group in enumerate(ir.BEST_TIE_GROUPS):
                v = e["iou64"][f, g]
                assert len({v[k].tobytes() for k in group}) == 1 and v[group[0]] == v.max() > 0.3, (mode, f, group)            # equal bytes, and the largest
                assert e["best"][f, g] == min(group) and (v == v.max()).sum() == len(group)
            assert e["best"][f, 3] == -1 and not e["iou64"][f, 3].any()
    assert {k // 64 for k in ir.BEST_TIE_GROUPS[0]} == {0, 1, 2} and len({k % 64 for k in ir.BEST_TIE_GROUPS[0]}) == 1
    assert ir.BEST_TIE_GROUPS[2][1] % 64 < ir.BEST_TIE_GROUPS[2][0] % 64
    # rank ties: all kept, in the order score, then number; ties across 255 | 256, 1023 | 1024, 2047 | 2048 and at (5, 1029)
    c, e = ir.tie_case("rank_ties", dtype), ir.tie_expected("rank_ties", dtype)
    B = c["boxes"].shape[1]
    s = c["scores"][0]
    assert B == 2100 and e["count"][0] == B and np.array_equal(e["index"][0], ir.ranking(c["boxes"][0], s, c["pose"][0]))
    assert np.array_equal(e["index"][0], np.lexsort((np.arange(B), -s.astype(np.float64))))
    rank = np.argsort(e["index"][0])
    for group in ir.RANK_TIES:
        assert len(set(s[list(group)].tolist())) == 1 and (s == s[group[0]]).sum() == len(group)
        assert rank[list(group)].tolist() == list(range(rank[group[0]], rank[group[0]] + len(group)))
    assert len(set(s.tolist())) == B - sum(len(g) - 1 for g in ir.RANK_TIES)
    # suppression at equality
    for name, value in (("equal_bev", 6.0 / 10.0), ("equal_3d", 9.0 / 23.0)):
        c = ir.tie_case(name, dtype)
        n = ir.EQ_PAIRS
        b, ok = ir._f64(c["boxes"][0]), np.ones(n, bool)
        v = ir.pair_iou(b[n:], c["pose"][0, n:], ok, b[:n], c["pose"][0, :n], ok, c["mode"])
        assert c["iou_thresh"] == value and len({x.tobytes() for x in v}) == 1 and v[0] == value                              # the same bits for every pair
        order = ir.ranking(c["boxes"][0], c["scores"][0], c["pose"][0])
        assert np.array_equal(order[:n], np.arange(n)) and not np.array_equal(order[n:], np.arange(n, 2 * n))
        counts = {word: int(ir.tie_expected(name, dtype, t)["count"][0]) for word, t in ir.tie_thresholds(c)}
        assert counts == dict(at=2 * n, below=n, above=2 * n)
        assert np.array_equal(ir.tie_expected(name, dtype, ir.tie_thresholds(c)[1][1])["index"][0, :n], np.arange(n))
    # stacks
    c, e = ir.tie_case("stack", dtype), ir.tie_expected("stack", dtype)
    assert len(np.unique(c["boxes"][0, :, 6])) == 3 and len(np.unique(c["boxes"][0, :, :6], axis=0)) == 1 and len(set(c["scores"][0].tolist())) == ir.FAMILY_N
    assert e["count"][0] == 1 and e["index"][0, 0] == np.argmax(c["scores"][0])
    cut, e2 = ir.tie_case("stack_cut", dtype), ir.tie_expected("stack_cut", dtype)
    assert (cut["scores"][0] >= cut["score_thresh"]).sum() == ir.FAMILY_N // 2 and e2["count"][0] == 1 and e2["index"][0, 0] == np.argmax(cut["scores"][0])
    for name in ir.TIE_CASES:                                                                                               # the blocked walk is the plain walk here too
        c = ir.tie_case(name, dtype)
        for _, t in (ir.tie_thresholds(c) if name.startswith("equal") else (("", c["iou_thresh"]),)):
            if name == "rank_ties":
                continue                                                                                                   # (all kept: shown above)
            plain = ir.nms_frame_plain(c["boxes"][0], c["scores"][0], c["pose"][0], t, c["post_max"], c["score_thresh"], c["mode"])
            e = ir.tie_expected(name, dtype, t)
            assert np.array_equal(plain, e["index"][0, :e["count"][0]]), (name, t)
