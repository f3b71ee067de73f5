"""-m gpu: rotated box IoU and NMS on the device (tensors.boxes_iou, tensors.nms, lidar_snow_sim_amd.iou, snowgpu_boxes_iou_device,
snowgpu_nms_device; csrc/snowgpu_iou.hip, csrc/sg_iou.h) against the NumPy restatement of their definition (tests/iou_reference.py, whose
inputs tests/test_iou_reference.py holds to the conditions that keep these comparisons from being vacuous).  The restatement takes the pose
as an input and everything behind the pose is separately rounded float64 arithmetic in the definition's order: every output is compared
byte for byte, for both dtypes, with no element left out -- under a given pose, and under the pose the device computed, which
points_in_boxes returns (the same device library, the same rule of presence).

Beside the shared cases, which keep every decision away from its threshold on purpose, the device meets the hard inputs (2a, 2b):
the ten adversarial families of iou_reference.family_case -- the eight adversarial kinds of tests/host_harness/iou_clip.cpp (equal
boxes, right angles, headings 1 ulp apart, shared faces, slivers, coordinates to 1e6, 1 cm to 100 m, boxes a few ulps wide), z_sliver
(heights that meet or miss by 1 ulp of T or 1e-15 .. 1e-10 of dz) and clamped (unions on both sides of 1e-8 m^2 and 1e-6 m^3, overlaps
whose IoU is a float32 subnormal) --, each built in the dtype under test, one frame of 130 x 130 per family with the designed partners
on the diagonal, and the 1300 designed pairs again as M = B = 1 frames; IoUs that tie for best across the 64-wide tiles of the b side;
equal scores across the groups and tiles of k_nms_rank; iou_thresh equal to an IoU the call computes, and the doubles beside it; stacks
of one box.  tests/test_iou_reference.py holds the host build of sg_iou.h equal to the restatement on every one of these pairs, and the
inputs to what they must contain.

Measured on an MI355X: float32-subnormal IoUs COME BACK AS SUBNORMALS -- the (T)v store does not flush them: of the 10 x 130 x 130 float32
IoUs of the family call 729 (BEV) and 498 (3D) are subnormal in the definition and the same 729 and 498 on the device, equal bytes.
Nothing differed between device and restatement on any new input, so neither the kernels nor the restatement changed.

That the new tests bite.  Each one-line variant changes a comparison or a constant only.  Header variants of csrc/sg_iou.h, on the host
harness (no GPU; both fail test_iou_reference.py::test_host_clip_equals_the_restatement_on_every_family[float32, float64]; in brackets
the DESIGNED pairs of 130 per family whose area or IoU changes, float32 / float64 frame):
  - a boundary point is outside (`dp < h`): equal [16 / 17], right_angle [10 / 16], one_ulp [0 / 16], shared_face [1 / 17] -- the
    changes are last bits of float64: rounded to float32 none survives, so on the device the float64 frames decide it;
  - both union clamps ten times smaller (1e-9, 1e-7): clamped [111 / 111] and 2667 of its 16 900 pairs, collapsed [120 / 82];
  - a height overlap of at most 1e-9 counts as none: z_sliver [22 / 56].
Kernel variants of csrc/snowgpu_iou.hip, each built apart from the tree and run once against this file on the same device:
  - k_iou_pairs `v > best_v || (v == best_v && v > 0.0)`: test_best_among_equal_ious_across_tiles[float32, float64], nothing else
    (the tie of the shared cases sits in two lanes of one tile);
  - k_nms_sweep `>=` for `>` in both tests: test_suppression_at_equality[equal_bev, equal_3d x float32, float64] (count 70 at
    equality where 140 are kept), no test of before;
  - k_nms_rank `i < j` for `t0 + i < j`: test_rank_ties_across_tiles_and_groups[float32, float64] -- and the b4160 and b9216 cases
    of before, because behind the first tile that form also counts a candidate before itself; built with `order` zero-filled and its
    store guarded, so that the colliding ranks stayed inside the buffers;
  - SG_IOU_CAP 8 for 20 (tried, not required to fail): all 131 tests pass, the 8 / 6 designed equal pairs that emit more than 8
    vertices included -- the dropped vertices coincide with kept ones to within rounding, on the device as on the host."""
import re

import numpy as np
import pytest
import torch

import box_reference as br
import iou_reference as ir

pytestmark = pytest.mark.gpu

DTYPES = ir.DTYPES
IOU_FIELDS = ("iou", "best", "best_iou")
NMS_FIELDS = ("index", "count", "boxes", "scores", "kept")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _iou(*args, **kw):
    from lidar_snow_sim_amd.tensors import boxes_iou
    return boxes_iou(*args, **kw)


def _nms(*args, **kw):
    from lidar_snow_sim_amd.tensors import nms
    return nms(*args, **kw)


def _same(got, want, what, fields):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _device_pose(boxes):
    """The (cos, sin) the device library gives for the headings of `boxes` (..., Cb), (0, 0) for an absent box: points_in_boxes returns the
    pose it used; the boxes go through it 256 at a time, one row per frame."""
    from lidar_snow_sim_amd.tensors import DeviceBatch, points_in_boxes
    flat = np.asarray(boxes).reshape(-1, boxes.shape[-1])
    G = (len(flat) + 255) // 256
    padded = np.zeros((G * 256, flat.shape[1]), flat.dtype)
    padded[:len(flat)] = flat
    rows = DeviceBatch(_t(np.zeros((G, 5), flat.dtype)), np.arange(G + 1, dtype=np.int64))
    pose = points_in_boxes(rows, _t(padded.reshape(G, 256, -1)), return_count=False, return_pose=True).pose.cpu().numpy()
    return np.ascontiguousarray(pose.reshape(-1, 2)[:len(flat)].reshape(boxes.shape[:-1] + (2,)))


def _run_nms(c, pose="given", **kw):
    args = dict(post_max=c["post_max"], score_thresh=c["score_thresh"], mode=c["mode"], pose=_t(c["pose"]) if pose == "given" else None,
                return_scores=True, return_kept=True)
    args.update(kw)
    return _nms(_t(c["boxes"]), _t(c["scores"]), c["iou_thresh"], **args)


def _want_nms(c, pose=None, **kw):
    a = dict(c, **kw)
    return ir.nms(a["boxes"], a["scores"], a["pose"] if pose is None else pose, a["iou_thresh"], a["post_max"], a["score_thresh"], a["mode"])


# ---- 1. the IoU matrix and the best partner ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ir.IOU_CASES)
def test_iou_cases_under_a_given_pose(name, dtype):
    c = ir.iou_case(name, dtype)
    a, b, pa, pb = _t(c["a"]), _t(c["b"]), _t(c["pose_a"]), _t(c["pose_b"])
    for mode in ir.MODES:
        _same(_iou(a, b, mode=mode, pose_a=pa, pose_b=pb, return_best=True), ir.iou_expected(name, dtype, mode), (name, dtype, mode), IOU_FIELDS)
    want = ir.iou_expected(name, dtype, "3d")
    alone = _iou(a, b, pose_a=pa, pose_b=pb, return_iou=False, return_best=True)
    assert alone.iou is None
    _same(alone, want, (name, dtype, "best alone"), IOU_FIELDS[1:])
    alone = _iou(a, b, pose_a=pa, pose_b=pb)
    assert alone.best is None and alone.best_iou is None
    _same(alone, want, (name, dtype, "iou alone"), IOU_FIELDS[:1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ir.IOU_CASES)
def test_iou_cases_under_the_device_pose(name, dtype):
    c = ir.iou_case(name, dtype)
    pa, pb = _device_pose(c["a"]), _device_pose(c["b"])
    assert np.abs(pa - br.used_pose(c["a"], c["pose_a"])).max() < 1e-15 and np.array_equal(pb != 0, br.used_pose(c["b"], c["pose_b"]) != 0)
    for mode in ir.MODES:
        _same(_iou(_t(c["a"]), _t(c["b"]), mode=mode, return_best=True), ir.boxes_iou(c["a"], c["b"], pa, pb, mode), (name, dtype, mode), IOU_FIELDS)


# ---- 2. NMS ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ir.NMS_CASES)
def test_nms_cases_under_a_given_pose(name, dtype):
    c = ir.nms_case(name, dtype)
    got = _run_nms(c)
    _same(got, ir.nms_expected(name, dtype), (name, dtype), NMS_FIELDS)
    index, kept = got.index.cpu().numpy(), got.kept.cpu().numpy()
    for f in range(len(index)):                                        # return_kept says what index says
        assert np.array_equal(np.flatnonzero(kept[f]), np.sort(index[f][index[f] >= 0]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ir.NMS_CASES)
def test_nms_cases_under_the_device_pose(name, dtype):
    c = ir.nms_case(name, dtype)
    pose = _device_pose(c["boxes"])
    _same(_run_nms(c, pose=None), _want_nms(c, pose), (name, dtype), NMS_FIELDS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_post_max_and_modes(dtype):
    """post_max = 1, the number kept without a limit, and B; both modes; three frames of different content in one call."""
    for name in ("b129", "mixed"):
        c = ir.nms_case(name, dtype)
        B = c["boxes"].shape[1]
        free = _want_nms(c, post_max=B)
        natural = int(free["count"].max())
        assert 1 < natural < B
        for mode in ir.MODES:
            for post_max in (1, natural, B):
                _same(_run_nms(c, post_max=post_max, mode=mode), _want_nms(c, post_max=post_max, mode=mode), (name, dtype, mode, post_max), NMS_FIELDS)
    bare = _run_nms(c, return_boxes=False, return_scores=False, return_kept=False)
    assert bare.boxes is None and bare.scores is None and bare.kept is None
    _same(bare, ir.nms_expected("mixed", dtype), dtype, NMS_FIELDS[:2])
    c = ir.nms_case("b129", dtype)                                     # a threshold above every IoU: all are kept; below every IoU: the first box suppresses all
    assert _nms(_t(c["boxes"]), _t(c["scores"]), 2.0, post_max=129, pose=_t(c["pose"])).count.tolist() == [129]
    assert _nms(_t(c["boxes"]), _t(c["scores"]), -1.0, post_max=129, pose=_t(c["pose"])).count.tolist() == [1]


# ---- 2a. the adversarial families: the kinds of the host harness, z_sliver and clamped ---------------------------------------------------------
def _subnormals(x):
    return int(((x != 0) & (np.abs(x) < ir.F32_TINY)).sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_families_under_a_given_pose(dtype):
    """One frame per family, 130 x 130 (two full tiles of b and a partial one), designed partners on the diagonal; both modes."""
    c = ir.family_case(dtype)
    a, b, pa, pb = _t(c["a"]), _t(c["b"]), _t(c["pose_a"]), _t(c["pose_b"])
    for mode in ir.MODES:
        got, want = _iou(a, b, mode=mode, pose_a=pa, pose_b=pb, return_best=True), ir.family_expected(dtype, mode)
        if dtype == "float32":
            print(f"float32 subnormal IoUs, {mode}: the device returns {_subnormals(got.iou.cpu().numpy())}, the definition has {_subnormals(want['iou'])}")
        _same(got, want, (dtype, mode), IOU_FIELDS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_families_under_the_device_pose(dtype):
    c = ir.family_case(dtype)
    pa, pb = _device_pose(c["a"]), _device_pose(c["b"])
    assert np.array_equal(pa.any(axis=-1), ir.present(c["a"], c["pose_a"])) and np.array_equal(pb.any(axis=-1), ir.present(c["b"], c["pose_b"]))
    for mode in ir.MODES:
        _same(_iou(_t(c["a"]), _t(c["b"]), mode=mode, return_best=True), ir.boxes_iou(c["a"], c["b"], pa, pb, mode), (dtype, mode), IOU_FIELDS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_pairs_one_per_frame(dtype):
    """The 1300 designed pairs as frames of M = B = 1: one lane of one wave per frame, a tile with one record."""
    p = ir.family_pairs(ir.family_case(dtype))
    for mode in ir.MODES:
        got = _iou(_t(p["a"]), _t(p["b"]), mode=mode, pose_a=_t(p["pose_a"]), pose_b=_t(p["pose_b"]), return_best=True)
        _same(got, ir.pairs_expected(p, mode), (dtype, mode, "given pose"), IOU_FIELDS)
    q = dict(p, pose_a=_device_pose(p["a"]), pose_b=_device_pose(p["b"]))
    _same(_iou(_t(p["a"]), _t(p["b"]), mode="3d", return_best=True), ir.pairs_expected(q, "3d"), (dtype, "device pose"), IOU_FIELDS)


# ---- 2b. exact ties and thresholds at equality ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_best_among_equal_ious_across_tiles(dtype):
    """Equal b boxes in one lane of three tiles, in a later tile, and in a later tile and a smaller lane: best is the smallest number."""
    c = ir.best_tie_case(dtype)
    for mode in ir.MODES:
        got = _iou(_t(c["a"]), _t(c["b"]), mode=mode, pose_a=_t(c["pose_a"]), pose_b=_t(c["pose_b"]), return_best=True)
        assert got.best.cpu().numpy()[:, :3].tolist() == [[min(g) for g in ir.BEST_TIE_GROUPS]] * 2
        _same(got, ir.boxes_iou(c["a"], c["b"], c["pose_a"], c["pose_b"], mode), (dtype, mode), IOU_FIELDS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_ties_across_tiles_and_groups(dtype):
    """2100 disjoint boxes, all kept: the kept order is the ranking, equal scores in ascending numbers across 255 | 256, 1023 | 1024,
    2047 | 2048 and at (5, 1029)."""
    c = ir.tie_case("rank_ties", dtype)
    got = _run_nms(c)
    _same(got, ir.tie_expected("rank_ties", dtype), dtype, NMS_FIELDS)
    assert got.count.tolist() == [2100] and sorted(got.index.cpu().numpy()[0].tolist()) == list(range(2100))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("equal_bev", "equal_3d"))
def test_suppression_at_equality(name, dtype):
    """iou_thresh equal to the IoU of every partner with its box: nothing is suppressed (the test is >); the double below: every partner is,
    against a box kept in an earlier block and against one of its own block; the double above: nothing."""
    c = ir.tie_case(name, dtype)
    n = ir.EQ_PAIRS
    for (word, t), count in zip(ir.tie_thresholds(c), (2 * n, n, 2 * n)):
        got = _run_nms(c, pose="given") if word == "at" else _nms(_t(c["boxes"]), _t(c["scores"]), t, post_max=c["post_max"], mode=c["mode"], pose=_t(c["pose"]),
                                                               return_scores=True, return_kept=True)
        assert got.count.tolist() == [count], (name, dtype, word, got.count.tolist())
        _same(got, ir.tie_expected(name, dtype, t), (name, dtype, word), NMS_FIELDS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stacks_of_one_box(dtype):
    """130 copies of one box, some turned by 1 ulp: one is kept, the best scored; the same with score_thresh at the median."""
    for name in ("stack", "stack_cut"):
        c = ir.tie_case(name, dtype)
        for pose in ("given", None):
            got = _run_nms(c, pose=pose)
            assert got.count.tolist() == [1] and got.index[0, 0].item() == int(np.argmax(c["scores"][0]))
            _same(got, ir.tie_expected(name, dtype) if pose else _want_nms(c, _device_pose(c["boxes"])), (name, dtype, pose), NMS_FIELDS)


# ---- 3. buffers, runs, streams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written_in_place(dtype):
    from lidar_snow_sim_amd.tensors import IouBatch, NmsBatch
    td = getattr(torch, dtype)
    for name in ("mixed", "b65"):
        c = ir.nms_case(name, dtype)
        F, B, Cb = c["boxes"].shape
        out = NmsBatch.empty(F, B, c["post_max"], Cb, td, with_scores=True, with_kept=True)
        for f in NMS_FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        assert _run_nms(c, out=out) is out
        _same(out, ir.nms_expected(name, dtype), (name, dtype), NMS_FIELDS)
    c = ir.iou_case("m65b129", dtype)
    out = IouBatch.empty(3, 65, 129, td, with_best=True)
    for f in IOU_FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x7f)
    assert _iou(_t(c["a"]), _t(c["b"]), pose_a=_t(c["pose_a"]), pose_b=_t(c["pose_b"]), out=out, return_best=True) is out
    _same(out, ir.iou_expected("m65b129", dtype, "3d"), dtype, IOU_FIELDS)


def test_two_calls_and_two_streams_give_identical_bytes():
    c = ir.nms_case("b4160")
    runs = [_run_nms(c), _run_nms(c)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())                      # (one engine slot: its record scratch is shared, so the calls are ordered)
    with torch.cuda.stream(side):
        runs.append(_run_nms(c))
    side.synchronize()
    for f in NMS_FIELDS:
        for other in runs[1:]:
            assert getattr(runs[0], f).data_ptr() != getattr(other, f).data_ptr() and torch.equal(getattr(runs[0], f).view(torch.uint8), getattr(other, f).view(torch.uint8)), f
    _same(runs[2], ir.nms_expected("b4160"), "side stream", NMS_FIELDS)
    c = ir.iou_case("m3b9216")
    args = (_t(c["a"]), _t(c["b"]))
    kw = dict(pose_a=_t(c["pose_a"]), pose_b=_t(c["pose_b"]), return_best=True)
    runs = [_iou(*args, **kw), _iou(*args, **kw)]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(_iou(*args, **kw))
    side.synchronize()
    for f in IOU_FIELDS:
        for other in runs[1:]:
            assert torch.equal(getattr(runs[0], f).view(torch.uint8), getattr(other, f).view(torch.uint8)), f
    _same(runs[2], ir.iou_expected("m3b9216", "float32", "3d"), "side stream", IOU_FIELDS)


# ---- 4. one graph: nms -> proposal-centric keypoints -> points in the kept boxes -> roi-to-gt IoU ------------------------------------------------
def test_graph_capture():
    """One capture after a warm-up, replayed on boxes, scores and gt rewritten in place, every output filled with 0x7f before: each
    replay equals the restatements composed -- NMS, then fps_sectors_reference and box_reference on the kept boxes, then the IoU of the
    kept boxes with gt.  The kept boxes' pose is the device's (points_in_boxes returns it); the given poses are NumPy's."""
    import fps_sectors_reference as sr
    from lidar_snow_sim_amd.tensors import BoxLabelBatch, DeviceBatch, IouBatch, KeypointBatch, NmsBatch, points_in_boxes, sample_keypoints
    F, n, B, P, G, K, S = 2, 2500, 96, 24, 12, 48, 4
    rng = np.random.default_rng(4300)
    inputs = []
    for _ in range(2):
        boxes = np.stack([ir.clustered(rng, B, 10) for _ in range(F)]).astype(np.float32)
        scores = rng.uniform(0.05, 1.0, (F, B)).astype(np.float32)
        gt = np.stack([ir.clustered(rng, G, G, Cb=8, spread=0.0) for _ in range(F)]).astype(np.float32)
        gt[:, :G - 2, :7] = boxes[:, 3:3 + G - 2, :7] + np.float32(0.3) * rng.normal(0, 1, (F, G - 2, 7)).astype(np.float32) * np.array([1, 1, 0.2, 0, 0, 0, 0.3], np.float32)
        gt[:, G - 1] = 0.0
        inputs.append((boxes, scores, gt))
    frames = []
    for f in range(F):                                                     # rows about the proposals of both inputs
        at = np.concatenate((inputs[0][0][f, :, :3], inputs[1][0][f, :, :3]))[rng.integers(0, 2 * B, n)]
        frames.append(np.column_stack((at + rng.normal(0, 1.5, (n, 3)) * np.array([1, 1, 0.4]), rng.integers(1, 255, n), rng.integers(0, 64, n))))
    cloud = np.concatenate(frames).astype(np.float32)
    offsets = np.arange(F + 1, dtype=np.int64) * n
    rows = DeviceBatch(_t(cloud), offsets)
    boxes, scores, gt = (_t(x) for x in inputs[0])
    pose = _t(ir.numpy_pose(inputs[0][0]))
    pose_gt = _t(ir.numpy_pose(inputs[0][2]))
    nb_out = NmsBatch.empty(F, B, P, 8, torch.float32, with_scores=True, with_kept=True)
    kp_out = KeypointBatch.empty(F, K, 4, torch.float32, sectors=S)
    lb_out = BoxLabelBatch.empty(offsets, P, torch.float32, with_pose=True)
    io_out = IouBatch.empty(F, P, G, torch.float32, with_best=True)
    s = torch.cuda.Stream()

    def chain():
        nb = _nms(boxes, scores, 0.45, post_max=P, score_thresh=0.1, pose=pose, out=nb_out, return_scores=True, return_kept=True)
        kp = sample_keypoints(rows, K, sectors=S, rois=nb.boxes, out=kp_out)
        lb = points_in_boxes(rows, nb.boxes, out=lb_out, return_pose=True)
        return nb, kp, lb, _iou(nb.boxes, gt, pose_b=pose_gt, out=io_out, return_best=True)

    outputs = ([getattr(nb_out, f) for f in NMS_FIELDS] + [kp_out.index, kp_out.points, kp_out.usable, lb_out.box_of, lb_out.count, lb_out.pose] +
               [getattr(io_out, f) for f in IOU_FIELDS])
    with torch.cuda.stream(s):
        chain()                                                            # warm-up: the captured calls allocate nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = chain()
        assert got[0] is nb_out and got[1] is kp_out and got[2] is lb_out and got[3] is io_out
        snaps = []
        for k in (1, 0):
            for dst, src in zip((boxes, scores, gt), inputs[k]):
                dst.copy_(_t(src))
            pose.copy_(_t(ir.numpy_pose(inputs[k][0])))
            pose_gt.copy_(_t(ir.numpy_pose(inputs[k][2])))
            for t in outputs:
                t.view(torch.uint8).fill_(0x7f)
            g.replay()
            snaps.append((k, [t.clone() for t in outputs]))
        s.synchronize()
    names = NMS_FIELDS + ("kp_index", "kp_points", "kp_usable", "box_of", "box_count", "box_pose") + IOU_FIELDS
    counts = []
    for k, snap in snaps:
        got = dict(zip(names, (t.cpu().numpy() for t in snap)))
        b, sc, g_ = inputs[k]
        want = ir.nms(b, sc, ir.numpy_pose(b), 0.45, P, 0.1, "bev")
        counts.append(want["count"].tolist())
        assert (want["count"] > 2).all() and (want["count"] < P).any()
        for f in NMS_FIELDS:
            assert got[f].tobytes() == want[f].tobytes(), (k, f)
        kp = sr.fps_sectors(cloud, K, S, None, 4, None, offsets, rois=want["boxes"], roi_margin=1.6)
        assert (kp["usable"] >= K).all() and (kp["usable"] < n).all()
        for f in ("index", "points", "usable"):
            assert got["kp_" + f].tobytes() == kp[f].tobytes(), (k, "keypoints", f)
        used = got["box_pose"]
        assert np.array_equal(used.any(axis=-1), ir.present(want["boxes"], ir.numpy_pose(want["boxes"])))
        lb = br.points_in_boxes(cloud, want["boxes"], used, None, offsets)
        assert got["box_of"].tobytes() == lb["box_of"].tobytes() and got["box_count"].tobytes() == lb["count"].tobytes() and (lb["box_of"] >= 0).sum() > 100
        io = ir.boxes_iou(want["boxes"], g_, used, ir.numpy_pose(g_), "3d")
        assert (io["best"] >= 0).sum() >= 4 and (io["best"] == -1).sum() >= 1
        for f in IOU_FIELDS:
            assert got[f].tobytes() == io[f].tobytes(), (k, f)
    assert counts[0] != counts[1]


# ---- 5. the NumPy entries ---------------------------------------------------------------------------------------------------------------------
def test_numpy_entries():
    from lidar_snow_sim_amd import iou
    for dtype in DTYPES:
        c = ir.iou_case("m63b65", dtype)
        for fn, mode in ((iou.boxes_iou_bev, "bev"), (iou.boxes_iou3d, "3d")):
            got = fn(c["a"][1], c["b"][1])
            assert got.dtype == c["a"].dtype and got.tobytes() == ir.iou_expected("m63b65", dtype, mode)["iou"][1].tobytes()
        c, e = ir.nms_case("b129", dtype), ir.nms_expected("b129", dtype)
        keep = iou.nms(c["boxes"][0], c["scores"][0], c["iou_thresh"])
        assert keep.dtype == np.int32 and np.array_equal(keep, e["index"][0, :e["count"][0]])
        assert np.array_equal(iou.nms(c["boxes"][0], c["scores"][0], c["iou_thresh"], post_max=5), e["index"][0, :5])
    with pytest.raises(ValueError):
        iou.boxes_iou_bev(c["boxes"][0][:, :6], c["boxes"][0])
    with pytest.raises(ValueError):
        iou.nms(c["boxes"][0], c["scores"][0][:5], 0.5)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import IouBatch, NmsBatch
    c = ir.nms_case("mixed")
    bx, sc, ps = _t(c["boxes"]), _t(c["scores"]), _t(c["pose"])
    F, B, Cb = c["boxes"].shape
    wide = _t(np.concatenate((c["boxes"], c["boxes"]), axis=2))
    for kw, words in ((dict(boxes=bx.double()), "scores must be a contiguous"), (dict(boxes=bx.cpu()), "boxes must be a contiguous"), (dict(boxes=bx[0]), "boxes must be a contiguous"),
                      (dict(boxes=wide[:, :, :8]), "boxes must be a contiguous"), (dict(boxes=bx[:, :, :6].contiguous()), "box_features must lie in 7 .. 10"),
                      (dict(boxes=wide[:, :, :11].contiguous()), "box_features must lie in 7 .. 10"), (dict(boxes=_t(np.zeros((1, 9217, 7), np.float32))), "boxes per frame must lie in 1 .. 9216"),
                      (dict(scores=sc[:, :5].contiguous()), "scores must be a contiguous"), (dict(scores=sc.double()), "scores must be a contiguous"),
                      (dict(post_max=0), "post_max must be an integer in 1 .. B"), (dict(post_max=B + 1), "post_max must be an integer in 1 .. B"), (dict(post_max=2.5), "post_max must be"),
                      (dict(mode="aligned"), "mode must be 'bev' or '3d'"), (dict(iou_thresh=float("nan")), "a threshold is NaN"), (dict(score_thresh=float("nan")), "a threshold is NaN"),
                      (dict(pose=ps.float()), "pose must be a contiguous"), (dict(pose=ps[:, :5].contiguous()), "pose must be a contiguous"),
                      (dict(out=NmsBatch.empty(F, B, 9, Cb)), "out must be a NmsBatch whose index"), (dict(out=NmsBatch.empty(F, B, 10, 7)), "out must be a NmsBatch whose boxes"),
                      (dict(out=NmsBatch.empty(F, B, 10, Cb), return_kept=True), "out must be a NmsBatch whose kept")):
        args = dict(boxes=bx, scores=sc, iou_thresh=0.5, post_max=10, pose=ps)
        args.update(kw)
        with pytest.raises(ValueError, match=words.replace("..", r"\.\.")):
            _nms(args.pop("boxes"), args.pop("scores"), args.pop("iou_thresh"), **args)
    g = _t(ir.iou_case("m63b65")["b"])
    for kw, words in ((dict(b=g[:2].contiguous()), "boxes_b must have the frames"), (dict(b=g.double()), "boxes_b must have the frames"), (dict(a=c["boxes"]), "boxes_a must be a contiguous"),
                      (dict(mode="2d"), "mode must be"), (dict(return_iou=False), "nothing to compute"), (dict(pose_a=ps[:, :3].contiguous()), "pose_a must be a contiguous"),
                      (dict(out=IouBatch.empty(F, B, 64)), "out must be a IouBatch whose iou"), (dict(out=IouBatch.empty(F, B, 65), return_best=True), "out must be a IouBatch whose best")):
        args = dict(a=bx, b=g)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            _iou(args.pop("a"), args.pop("b"), **args)
    # the C entries refuse on their own, at every edge of the domain
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    out = NmsBatch.empty(F, B, 10, Cb, with_scores=True, with_kept=True)
    io = IouBatch.empty(F, B, 65, with_best=True)

    def call_nms(n_frames=F, n_boxes=B, feats=Cb, dtype=0, mode=0, iou_thresh=0.5, score_thresh=0.0, post_max=10, boxes=bx.data_ptr(), scores=sc.data_ptr(),
                 index=out.index.data_ptr(), count=out.count.data_ptr(), kboxes=out.boxes.data_ptr(), kept=out.kept.data_ptr()):
        ctx.nms_device(n_frames, n_boxes, boxes, feats, scores, dtype, mode, iou_thresh, score_thresh, post_max, ps.data_ptr(), index, count, kboxes,
                       out.scores.data_ptr(), kept)

    def call_iou(n_frames=F, n_a=B, n_b=65, fa=Cb, fb=9, dtype=0, mode=1, a=bx.data_ptr(), iou=io.iou.data_ptr(), best=io.best.data_ptr(), best_iou=io.best_iou.data_ptr()):
        ctx.boxes_iou_device(n_frames, n_a, a, fa, n_b, g.data_ptr(), fb, dtype, mode, 0, 0, iou, best, best_iou)

    who = "snowgpu_nms_device: "
    for kw, words in ((dict(n_boxes=0), "n_boxes must lie in 1 .. 9216"), (dict(n_boxes=9217), "n_boxes must lie in 1 .. 9216"), (dict(feats=6), "box_features must lie in 7 .. 10"),
                      (dict(feats=11), "box_features must lie in 7 .. 10"), (dict(post_max=0), "post_max must lie in 1 .. n_boxes"), (dict(post_max=B + 1), "post_max must lie in 1 .. n_boxes"),
                      (dict(mode=2), "mode must be 0"), (dict(dtype=2), "null pointer or bad dtype"), (dict(n_frames=0), "null pointer or bad dtype"), (dict(scores=0), "null pointer or bad dtype"),
                      (dict(index=0), "null pointer or bad dtype"), (dict(count=0), "null pointer or bad dtype"), (dict(iou_thresh=float("nan")), "a threshold is NaN"),
                      (dict(score_thresh=float("nan")), "a threshold is NaN"), (dict(n_frames=2 ** 20, n_boxes=2048), "n_frames \\* n_boxes exceeds"),
                      (dict(kboxes=bx.data_ptr()), "d_out_boxes overlaps d_boxes"), (dict(kept=sc.data_ptr() + 4), "d_out_kept overlaps d_scores"),
                      (dict(kept=out.index.data_ptr()), "d_out_kept overlaps d_out_index; every output needs memory of its own")):
        with pytest.raises(ValueError, match=who + words.replace("..", r"\.\.")):
            call_nms(**kw)
    who = "snowgpu_boxes_iou_device: "
    for kw, words in ((dict(n_a=0), "the boxes per frame must lie in 1 .. 9216"), (dict(n_b=9217), "the boxes per frame must lie in 1 .. 9216"), (dict(fa=6), "box_features must lie in 7 .. 10"),
                      (dict(fb=11), "box_features must lie in 7 .. 10"), (dict(mode=-1), "mode must be 0"), (dict(dtype=3), "null pointer or bad dtype"), (dict(a=0), "null pointer or bad dtype"),
                      (dict(iou=0, best=0, best_iou=0), "no output"), (dict(n_frames=2 ** 15, n_a=256, n_b=256), "n_frames \\* M \\* B exceeds"),
                      (dict(iou=g.data_ptr()), "d_out_iou overlaps d_boxes_b"), (dict(best_iou=io.best.data_ptr()), "d_out_best_iou overlaps d_out_best; every output needs memory of its own")):
        with pytest.raises(ValueError, match=who + words.replace("..", r"\.\.")):
            call_iou(**kw)
    call_nms(kboxes=0, kept=0)                                         # the nullable outputs may be null
    torch.cuda.synchronize()
    want = ir.nms(c["boxes"], c["scores"], c["pose"], 0.5, 10, 0.0, "bev")
    assert out.index.cpu().numpy().tobytes() == want["index"].tobytes() and out.count.cpu().numpy().tobytes() == want["count"].tobytes()


# ---- every refusal of the Python boundary word for word, and which of two faults is reported -----------------------------------------------------
def _pin_boxes(n=2, features=7, dtype=torch.float32, frames=2):
    return torch.ones((frames, n, features), dtype=dtype, device="cuda:0")


def _pin_pose(dtype=torch.float64):
    return torch.ones((2, 2, 2), dtype=dtype, device="cuda:0")


def _iou_out(*args, **kw):
    from lidar_snow_sim_amd.tensors import IouBatch
    return IouBatch.empty(2, *args, **kw)


def _nms_out(*args, **kw):
    from lidar_snow_sim_amd.tensors import NmsBatch
    return NmsBatch.empty(2, 2, *args, **kw)


SET_WORDS = "boxes_iou: %s must be a contiguous (frames, B, 7 .. 10) float32 or float64 CUDA tensor"
LIKE_WORDS = "boxes_iou: boxes_b must have the frames, the dtype and the device of the other boxes"
IOU_OUT_WORDS = "boxes_iou: out must be a IouBatch whose %s tensor on the device of the boxes"
PINNED_IOU = (
    ("boxes_a on the host", lambda: dict(boxes_a=np.ones((2, 2, 7), np.float32)), SET_WORDS % "boxes_a"),
    ("boxes_b of two dimensions", lambda: dict(boxes_b=_pin_boxes()[0]), SET_WORDS % "boxes_b"),
    ("boxes_b of another dtype", lambda: dict(boxes_b=_pin_boxes(dtype=torch.float64)), LIKE_WORDS),
    ("boxes_b of other frames", lambda: dict(boxes_b=_pin_boxes(frames=3)), LIKE_WORDS),
    ("no box a", lambda: dict(boxes_a=_pin_boxes(0)), "boxes_iou: the boxes per frame must lie in 1 .. 9216, the frames be at least 1 (boxes_a)"),
    ("9217 boxes b", lambda: dict(boxes_b=_pin_boxes(9217)), "boxes_iou: the boxes per frame must lie in 1 .. 9216, the frames be at least 1 (boxes_b)"),
    ("boxes_b of 11 columns", lambda: dict(boxes_b=_pin_boxes(features=11)), "boxes_iou: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes_b)"),
    ("mode", lambda: dict(mode="2d"), "boxes_iou: mode must be 'bev' or '3d'"),
    ("nothing asked for", lambda: dict(return_iou=False), "boxes_iou: nothing to compute: return_iou or return_best"),
    ("2^31 pairs", lambda: dict(boxes_a=torch.empty((26, 9216, 7), device="cuda:0"), boxes_b=torch.empty((26, 9216, 7), device="cuda:0")),
     "boxes_iou: frames * M * B exceeds 2^31 - 1; split the batch"),
    ("pose_a of float32", lambda: dict(pose_a=_pin_pose(torch.float32)), "boxes_iou: pose_a must be a contiguous (2, 2, 2) float64 tensor (cos, sin) on the device of the boxes"),
    ("pose_b of another shape", lambda: dict(pose_b=_pin_pose()[:, :1].contiguous()), "boxes_iou: pose_b must be a contiguous (2, 2, 2) float64 tensor (cos, sin) on the device of the boxes"),
    ("out of another shape", lambda: dict(out=_iou_out(2, 3)), IOU_OUT_WORDS % "iou is a contiguous (2, 2, 2) torch.float32"),
    ("out of another kind", lambda: dict(out=object()), IOU_OUT_WORDS % "iou is a contiguous (2, 2, 2) torch.float32"),
    ("out without best", lambda: dict(out=_iou_out(2, 2), return_best=True), IOU_OUT_WORDS % "best is a contiguous (2, 2) torch.int32"),
    # two faults: the earlier step of the call reports
    ("boxes_a before boxes_b", lambda: dict(boxes_a=_pin_boxes(features=6), boxes_b=_pin_boxes(features=6)),
     "boxes_iou: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes_a)"),
    ("the boxes before the mode", lambda: dict(boxes_b=_pin_boxes(features=11), mode="2d"), "boxes_iou: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes_b)"),
    ("the mode before the outputs", lambda: dict(mode="2d", return_iou=False), "boxes_iou: mode must be 'bev' or '3d'"),
    ("the outputs before the pose", lambda: dict(return_iou=False, pose_a=_pin_pose(torch.float32)), "boxes_iou: nothing to compute: return_iou or return_best"),
    ("the pose before out", lambda: dict(pose_a=_pin_pose(torch.float32), out=object()), "boxes_iou: pose_a must be a contiguous (2, 2, 2) float64 tensor (cos, sin) on the device of the boxes"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED_IOU], ids=[c[0] for c in PINNED_IOU])
def test_every_refusal_of_boxes_iou_word_for_word(overrides, words):
    args = dict(boxes_a=_pin_boxes(), boxes_b=_pin_boxes())
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        _iou(args.pop("boxes_a"), args.pop("boxes_b"), **args)


SCORE_WORDS = "nms: scores must be a contiguous (2, 2) tensor in the boxes' dtype on their device"
NMS_OUT_WORDS = "nms: out must be a NmsBatch whose %s tensor on the device of the boxes"
PINNED_NMS = (
    ("boxes on the host", lambda: dict(boxes=np.ones((2, 2, 7), np.float32)), "nms: boxes must be a contiguous (frames, B, 7 .. 10) float32 or float64 CUDA tensor"),
    ("no box", lambda: dict(boxes=_pin_boxes(0)), "nms: the boxes per frame must lie in 1 .. 9216, the frames be at least 1 (boxes)"),
    ("boxes of 6 columns", lambda: dict(boxes=_pin_boxes(features=6)), "nms: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes)"),
    ("scores of another dtype", lambda: dict(scores=torch.ones((2, 2), dtype=torch.float64, device="cuda:0")), SCORE_WORDS),
    ("scores of another shape", lambda: dict(scores=torch.ones((2, 3), device="cuda:0")), SCORE_WORDS),
    ("mode", lambda: dict(mode="aligned"), "nms: mode must be 'bev' or '3d'"),
    ("post_max 1.5", lambda: dict(post_max=1.5), "nms: post_max must be an integer in 1 .. B"),
    ("post_max True", lambda: dict(post_max=True), "nms: post_max must be an integer in 1 .. B"),
    ("post_max 3", lambda: dict(post_max=3), "nms: post_max must be an integer in 1 .. B"),
    ("iou_thresh NaN", lambda: dict(iou_thresh=float("nan")), "nms: a threshold is NaN"),
    ("score_thresh NaN", lambda: dict(score_thresh=float("nan")), "nms: a threshold is NaN"),
    ("pose of float32", lambda: dict(pose=_pin_pose(torch.float32)), "nms: pose must be a contiguous (2, 2, 2) float64 tensor (cos, sin) on the device of the boxes"),
    ("out of another length", lambda: dict(out=_nms_out(1)), NMS_OUT_WORDS % "index is a contiguous (2, 2) torch.int32"),
    ("out of another kind", lambda: dict(out=object()), NMS_OUT_WORDS % "index is a contiguous (2, 2) torch.int32"),
    ("out of other columns", lambda: dict(out=_nms_out(2, 8)), NMS_OUT_WORDS % "boxes is a contiguous (2, 2, 7) torch.float32"),
    ("out without scores", lambda: dict(out=_nms_out(2), return_scores=True), NMS_OUT_WORDS % "scores is a contiguous (2, 2) torch.float32"),
    ("out without kept", lambda: dict(out=_nms_out(2), return_kept=True), NMS_OUT_WORDS % "kept is a contiguous (2, 2) torch.uint8"),
    # two faults: the earlier step of the call reports
    ("the boxes before the scores", lambda: dict(boxes=_pin_boxes(features=6), scores=torch.ones((2, 3), device="cuda:0")),
     "nms: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes)"),
    ("the scores before the mode", lambda: dict(scores=torch.ones((2, 3), device="cuda:0"), mode="aligned"), SCORE_WORDS),
    ("the mode before post_max", lambda: dict(mode="aligned", post_max=1.5), "nms: mode must be 'bev' or '3d'"),
    ("post_max before a threshold", lambda: dict(post_max=1.5, iou_thresh=float("nan")), "nms: post_max must be an integer in 1 .. B"),
    ("a threshold before the pose", lambda: dict(iou_thresh=float("nan"), pose=_pin_pose(torch.float32)), "nms: a threshold is NaN"),
    ("the pose before out", lambda: dict(pose=_pin_pose(torch.float32), out=object()), "nms: pose must be a contiguous (2, 2, 2) float64 tensor (cos, sin) on the device of the boxes"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED_NMS], ids=[c[0] for c in PINNED_NMS])
def test_every_refusal_of_nms_word_for_word(overrides, words):
    args = dict(boxes=_pin_boxes(), scores=torch.ones((2, 2), device="cuda:0"), iou_thresh=0.5, post_max=2)
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        _nms(args.pop("boxes"), args.pop("scores"), args.pop("iou_thresh"), **args)
