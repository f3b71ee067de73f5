"""-m gpu: proposal target sampling on the device (tensors.sample_rois, targets.sample_rois, snowgpu_sample_rois_device;
csrc/snowgpu_targets.hip, csrc/sg_targets.h) against the restatement of its definition (tests/targets_reference.py, whose cases
tests/test_targets_reference.py holds to the conditions that keep these comparisons from being vacuous).  The restatement takes the pose
as an input; the draws are Philox words in Python integers and everything behind the pose is separately rounded float64 arithmetic in the
definition's order: every output is compared byte for byte, for both dtypes, with no element left out -- under a given pose, and under
the pose the device computed and returned."""
import numpy as np
import pytest
import torch

import targets_reference as tr
from lidar_snow_sim_amd.tensors import sample_rois  # noqa: F401  (the stage under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

DTYPES = tr.DTYPES
FIELDS = tr.FIELDS


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _step(v):
    return torch.tensor([int(v)], dtype=torch.int64, device="cuda")


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _run(c, pose="given", step=None, **kw):
    from lidar_snow_sim_amd.tensors import sample_rois
    args = dict(c["cfg"], step=_step(c["step"]) if step is None else step, seed=c["seed"], pose=_t(c["pose"]) if pose == "given" else None,
                return_local=True, return_pose=True)
    args.update(kw)
    return sample_rois(_t(c["rois"]), _t(c["gt_boxes"]), (_t(c["overlap"]), _t(c["assignment"])), **args)


# ---- 1. the shared cases under their given pose -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", tr.CASE_NAMES)
def test_cases_under_a_given_pose(name, dtype):
    """M in 1, 2, 63, 64, 65, 129, 9216; S in 1, 4, 5, 128, 1024; B in 1, 65; fg_ratio 0 and 1; both score types; the branches spread over
    the frames of one batch; the walk of 1024 steps."""
    got = _run(tr.case(name, dtype))
    _same(got, tr.expected(name, dtype), (name, dtype))
    assert torch.equal(got.valid, got.index >= 0)


def test_the_shapes_the_cases_cover():
    sizes = [(tr.case(n, "float32")["rois"].shape[1], tr.case(n, "float32")["cfg"]["roi_per_image"], tr.case(n, "float32")["gt_boxes"].shape[1],
              tr.case(n, "float32")["rois"].shape[0]) for n in tr.CASE_NAMES]
    assert {1, 2, 63, 64, 65, 129, 9216} <= {s[0] for s in sizes} and {1, 4, 5, 128, 1024} <= {s[1] for s in sizes} and {1, 65} <= {s[2] for s in sizes}
    assert max(s[3] for s in sizes) <= 6
    kinds = {(tr.case(n, "float32")["cfg"]["cls_score_type"], tr.case(n, "float32")["cfg"]["fg_ratio"]) for n in tr.CASE_NAMES}
    assert {k for k, _ in kinds} == {"roi_iou", "cls"} and {0.0, 1.0} <= {r for _, r in kinds}


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_other_score_type_on_the_thresholds(dtype):
    c = tr.case("edges", dtype)
    c = dict(c, cfg={**c["cfg"], "cls_score_type": "cls"})
    _same(_run(c), tr.expected_of(c), ("edges, cls", dtype))


# ---- 2. the device pose -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("branches", "headings", "m129"))
def test_cases_under_the_device_pose(name, dtype):
    """The stage returns the pose of every PICK (F, S, 2), not of every roi: the restatement is fed NumPy's pose with the returned pose
    in the place of every picked roi.  A roi that was not picked only had its presence decided by its pose, and the pose tolerance of 1e-6
    is ten orders above the difference of two float64 cosines."""
    c = tr.case(name, dtype)
    got = _run(c, pose=None)
    used, index = got.pose.cpu().numpy(), got.index.cpu().numpy()
    pose = np.array(c["pose"])
    for f, k in zip(*np.nonzero(index >= 0)):
        assert np.allclose(used[f, k], c["pose"][f, index[f, k]], rtol=0, atol=1e-15)
        pose[f, index[f, k]] = used[f, k]
    assert not used[index < 0].any() and (index >= 0).any()
    _same(got, tr.expected_of(c, pose=pose), (name, dtype, "device pose"))


# ---- 3. no clearing, repeatable ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_is_fully_written_and_calls_repeat(dtype):
    from lidar_snow_sim_amd.tensors import RoiTargetBatch
    c = tr.case("branches", dtype)
    F, _, Cb = c["rois"].shape
    out = RoiTargetBatch.empty(F, c["cfg"]["roi_per_image"], Cb, c["gt_boxes"].shape[2], getattr(torch, dtype), with_pose=True, with_local=True)
    snaps = []
    for _ in range(2):
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x5A)
        got = _run(c, out=out)
        assert got is out
        snaps.append([getattr(out, f).clone() for f in FIELDS])
        _same(out, tr.expected("branches", dtype), ("out=", dtype))
    for a, b in zip(*snaps):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_fields_that_were_not_asked_for_an_nms_batch_and_an_iou_batch():
    from lidar_snow_sim_amd.tensors import IouBatch, NmsBatch, sample_rois
    c, e = tr.case("m64", "float32"), tr.expected("m64", "float32")
    F, M = c["rois"].shape[:2]
    nb = NmsBatch(torch.zeros((F, M), dtype=torch.int32).cuda(), torch.zeros(F, dtype=torch.int32).cuda(), _t(c["rois"]))
    ib = IouBatch(None, _t(c["assignment"]), _t(c["overlap"]))
    got = sample_rois(nb, _t(c["gt_boxes"]), ib, step=_step(c["step"]), seed=c["seed"], pose=_t(c["pose"]), **c["cfg"])
    assert got.pose is None and got.gt_local is None
    _same(got, e, "bare", FIELDS[:9])
    scores = torch.arange(F * M, dtype=torch.float32, device="cuda").view(F, M) + 1
    index = torch.from_numpy(e["index"]).cuda().long()
    assert torch.equal(got.gather(scores), torch.gather(scores, 1, index)) and got.gather(torch.stack((scores, -scores), -1)).shape == (F, 128, 2)
    blank = _run(tr.case("branches", "float32"))
    f = tr.BRANCH_FRAMES["nothing"]
    labels = torch.ones(tr.case("branches", "float32")["rois"].shape[:2], dtype=torch.int64, device="cuda")
    assert (blank.gather(labels, fill=-7)[f] == -7).all() and (blank.gather(labels)[f] == 0).all() and not blank.valid[f].any()


def test_the_host_array_mirror():
    from lidar_snow_sim_amd import targets
    c, e = tr.case("m129", "float64"), tr.expected("m129", "float64")
    got = targets.sample_rois(c["rois"][0], c["gt_boxes"][0], c["overlap"][0], c["assignment"][0], step=c["step"], seed=c["seed"], **c["cfg"])
    for name in FIELDS:
        assert got[name].tobytes() == e[name][0].tobytes(), name


# ---- 4. the counter: step, seed and the frame's position -------------------------------------------------------------------------------------
def test_a_frame_of_a_batch_is_a_one_frame_call_only_at_position_0():
    """The counter holds the frame's position in the batch: frame 0 of a batch equals the one-frame call on its data, frame f > 0 does
    not -- it equals the restatement keyed by f."""
    c = tr.case("branches", "float32")
    whole = _run(c)
    f = tr.BRANCH_FRAMES["few_fg"]
    for g in (0, f):
        one = dict(c, **{k: v[g:g + 1] for k, v in c.items() if isinstance(v, np.ndarray)})
        alone = _run(one)
        _same(alone, tr.expected_of(one), ("one frame", g))
        assert torch.equal(alone.index[0], whole.index[g]) == (g == 0)
    assert whole.index[f].cpu().numpy().tolist() == tr.expected_of(dict(c, **{k: v[f:f + 1] for k, v in c.items() if isinstance(v, np.ndarray)}), frames=[f])["index"][0].tolist()


def test_step_and_seed_change_the_picks():
    c = tr.case("m129", "float32")
    base = _run(c)
    for changed in (dict(step=c["step"] + 1), dict(step=c["step"] + (1 << 32)), dict(seed=c["seed"] + 1), dict(seed=c["seed"] + (1 << 32))):
        d = dict(c, **changed)
        got = _run(d)
        _same(got, tr.expected_of(d), changed)
        assert not torch.equal(got.index, base.index)


# ---- 5. one graph -----------------------------------------------------------------------------------------------------------------------------
def test_sample_rois_and_step_in_one_graph():
    """sample_rois and step += 1 captured once on one stream and replayed three times: the replays equal three eager calls at steps
    s, s + 1, s + 2 -- and the restatement at those steps -- and differ from one another."""
    from lidar_snow_sim_amd.tensors import RoiTargetBatch, sample_rois
    c = tr.case("branches", "float32")
    F, _, Cb = c["rois"].shape
    rois, gt, ov, assign, pose = (_t(c[k]) for k in ("rois", "gt_boxes", "overlap", "assignment", "pose"))
    s0 = c["step"]
    eager = []
    for k in range(3):
        eager.append(sample_rois(rois, gt, (ov, assign), step=_step(s0 + k), seed=c["seed"], pose=pose, return_local=True, return_pose=True, **c["cfg"]))
    s = torch.cuda.Stream()
    out = RoiTargetBatch.empty(F, c["cfg"]["roi_per_image"], Cb, c["gt_boxes"].shape[2], torch.float32, with_pose=True, with_local=True)
    step = _step(s0 - 1)

    def call():
        sample_rois(rois, gt, (ov, assign), step=step, seed=c["seed"], pose=pose, out=out, return_local=True, return_pose=True, **c["cfg"])
        step.add_(1)

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        call()                                                            # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        got = []
        for k in range(3):                                                # no host read between the replays
            g.replay()
            got.append({n: getattr(out, n).clone() for n in FIELDS})
        s.synchronize()
    assert int(step[0]) == s0 + 3
    for k in range(3):
        for n in FIELDS:
            assert torch.equal(got[k][n].view(torch.uint8), getattr(eager[k], n).view(torch.uint8)), (k, n)
        want = tr.expected_of(c, step=s0 + k)
        assert got[k]["index"].cpu().numpy().tobytes() == want["index"].tobytes()
    assert not torch.equal(got[0]["index"], got[1]["index"]) and not torch.equal(got[1]["index"], got[2]["index"]) and not torch.equal(got[0]["index"], got[2]["index"])


# ---- 6. what Python refuses -------------------------------------------------------------------------------------------------------------------
def test_python_refusals_in_the_stages_order():
    from lidar_snow_sim_amd.tensors import RoiTargetBatch, sample_rois
    c = tr.case("m63", "float32")
    rois, gt, ov, assign = (_t(c[k]) for k in ("rois", "gt_boxes", "overlap", "assignment"))
    step = _step(0)

    def refused(words, *args, **kw):
        kw.setdefault("step", step)
        with pytest.raises(ValueError, match=words):
            sample_rois(*args, **kw)

    refused("roi_per_image must be an integer", rois, gt, (ov, assign), roi_per_image=4.5)
    refused("must be finite", rois, gt, (ov, assign), cls_fg_thresh=float("nan"))
    refused("cls_score_type must be", rois, gt, (ov, assign), cls_score_type="iou")
    refused("rois must be a contiguous", rois.cpu(), gt, (ov, assign))
    refused("gt_boxes must have the frames, the dtype and the device", rois, gt.double(), (ov, assign))
    refused("an IouBatch or a pair", rois, gt, ov)
    refused("max_overlaps must be a contiguous", rois, gt, (ov.double(), assign))
    refused("gt_assignment must be a contiguous", rois, gt, (ov, assign.long()))
    refused("step must be a one-element int64", rois, gt, (ov, assign), step=torch.zeros(1, dtype=torch.int32, device="cuda"))
    refused("roi_per_image must lie in 1 .. 1024", rois, gt, (ov, assign), roi_per_image=1025)
    refused("fg_per_image must lie in 0 .. roi_per_image", rois, gt, (ov, assign), fg_ratio=1.5)
    refused("pose must be a contiguous", rois, gt, (ov, assign), pose=torch.zeros((2, 63, 2), device="cuda"))
    refused("out must be a RoiTargetBatch whose index", rois, gt, (ov, assign), out=RoiTargetBatch.empty(2, 64, 8, 8))
    # wrong in two ways: the earlier check speaks
    refused("roi_per_image must be an integer", rois.cpu(), gt, (ov, assign), roi_per_image=4.5)
    refused("cls_score_type must be", rois, gt, (ov.double(), assign), cls_score_type="iou")
    refused("rois must be a contiguous", rois.cpu(), gt, (ov, assign), roi_per_image=1025)
    refused("max_overlaps must be a contiguous", rois, gt, (ov.double(), assign), out=RoiTargetBatch.empty(2, 64, 8, 8))
    refused("roi_per_image must lie in 1 .. 1024", rois, gt, (ov, assign), roi_per_image=0, pose=torch.zeros((2, 63, 2), device="cuda"))
    # what only the entry refuses comes back in the entry's words
    refused("snowgpu_sample_rois_device: cls_fg_thresh must be above cls_bg_thresh", rois, gt, (ov, assign), cls_fg_thresh=0.2)
    refused("snowgpu_sample_rois_device: hard_bg_ratio must lie in 0 .. 1", rois, gt, (ov, assign), hard_bg_ratio=1.5)
    out = RoiTargetBatch.empty(2, 128, 8, 8)
    out.roi_iou = out.cls_label
    refused("d_out_cls_label overlaps d_out_roi_iou; every output needs memory of its own", rois, gt, (ov, assign), out=out)
