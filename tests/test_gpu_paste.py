"""-m gpu: ground-truth object paste on the device (tensors.paste_objects, tensors.ObjectBank, paste.paste_objects, paste.build_bank,
snowgpu_paste_objects_device; csrc/snowgpu_paste.hip, csrc/sg_paste.h) against the restatement of its definition
(tests/paste_reference.py, whose cases tests/test_paste_reference.py holds to the conditions that keep these comparisons from being
vacuous).  The restatement takes the poses as inputs; the draws are Philox words in Python integers and everything behind the pose is
separately rounded float64 arithmetic in the definition's order: every output is compared byte for byte, for both dtypes, with no element
left out -- under given poses, and under the pose the device computed and returned."""
import numpy as np
import pytest
import torch

import box_reference as br
import paste_reference as pr
from lidar_snow_sim_amd.tensors import paste_objects  # noqa: F401  (the stage under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

DTYPES = pr.DTYPES
FIELDS = pr.FIELDS


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _step(v):
    return torch.tensor([int(v)], dtype=torch.int64, device="cuda")


def _bank(b, pose="given"):
    from lidar_snow_sim_amd.tensors import ObjectBank
    return ObjectBank(_t(b["points"]), b["offsets"], _t(b["boxes"]), _t(b["pose"]) if pose == "given" else None)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy() if not isinstance(got, dict) else got[name]
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _run(c, pose="given", step=None, bank=None, **kw):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    args = dict(step=_step(c["step"]) if step is None else step, seed=c["seed"], keep=None if c["keep"] is None else _t(c["keep"]),
                remove_extra_width=c["ew"], pose=_t(c["pose"]) if pose == "given" else None, return_source=True, return_pose=True)
    args.update(kw)
    return paste_objects(DeviceBatch(_t(c["rows"]), c["offsets"]), _t(c["gt_boxes"]), _bank(c["bank"]) if bank is None else bank, c["groups"], **args)


# ---- 1. the shared cases under their given poses ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", pr.CASE_NAMES)
def test_cases_under_given_poses(name, dtype):
    """Q in 1, 3, 11, 12, 63, 64; B in 1, 3, 4, 5, 65, 192; frames of 0, 1, 511, 512, 513 and 1537 rows in one batch; free slots over a lane
    border, a run border and a frame's last row; objects of 0, 64 and 600 points; a frame without a free slot; NaN in absent slots."""
    got = _run(pr.case(name, dtype))
    e = pr.expected(name, dtype)
    _same(got, e, (name, dtype))
    assert torch.equal(got.pasted, got.state == 1)
    cls = got.labels().cpu().numpy()
    B = pr.case(name, dtype)["gt_boxes"].shape[1]
    frame = np.repeat(np.arange(len(e["count"])), np.diff(pr.case(name, dtype)["offsets"]))
    want = np.where(e["source"] >= 0, e["gt_boxes"][frame, np.maximum(e["source"], 0), 7], 0)
    assert cls.tobytes() == want.astype(cls.dtype).tobytes() and (e["source"].max() < B or (cls != 0).any())


def test_the_shapes_the_cases_cover():
    sizes = [(sum(pr.case(n, "float32")["groups"]), pr.case(n, "float32")["gt_boxes"].shape[1], pr.case(n, "float32")["gt_boxes"].shape[0],
              int(np.diff(pr.case(n, "float32")["offsets"]).max()), len(pr.case(n, "float32")["bank"]["boxes"]), int(np.diff(pr.case(n, "float32")["bank"]["offsets"]).max()))
             for n in pr.CASE_NAMES]
    assert {1, 63, 64} <= {s[0] for s in sizes} and {1, 65, 192} <= {s[1] for s in sizes}
    assert max(s[2] for s in sizes) <= 6 and max(s[3] for s in sizes) <= 1600 and max(s[4] for s in sizes) <= 40 and max(s[5] for s in sizes) <= 700
    assert any(np.isnan(pr.case(n, "float32")["rows"][~pr.case(n, "float32")["keep"]]).any() for n in pr.CASE_NAMES)


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_a_mask_and_without_a_gt(dtype):
    """keep=None: every row is present, no slot is free -- only the object of 0 points is pasted, and it still clears its place.  All gts
    absent: every class lacks its whole group."""
    c = dict(pr.case("big", dtype), keep=None)
    e = pr.expected_of(c)
    _same(_run(c), e, ("keep=None", dtype))
    assert e["state"].tolist() == [[1, 4, 4]] * 3 and not e["count"][:, 3].any()
    c = pr.case("q63", dtype)
    c = dict(c, gt_boxes=np.zeros_like(c["gt_boxes"]), pose=br.numpy_pose(np.zeros_like(c["gt_boxes"])))
    e = pr.expected_of(c)
    _same(_run(c), e, ("no gt", dtype))
    assert (e["object"] >= 0).all() and not (e["state"] == 2).any() and (e["state"] == 1).any()


# ---- 2. the device pose -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("states", "q63"))
def test_cases_under_the_device_pose(name, dtype):
    """pose=None and a bank without a pose: the gts' pose comes back in `pose` (rows 0 .. B - 1, (0, 0) for absent gts, which NumPy's pose
    leaves absent just as well), the bank's is its `pose` tensor; both are fed to the restatement."""
    c = pr.case(name, dtype)
    bank = _bank(c["bank"], pose=None)
    got = _run(c, pose=None, bank=bank)
    B = c["gt_boxes"].shape[1]
    used = got.pose.cpu().numpy()[:, :B]
    ok = br.present(c["gt_boxes"], c["pose"])
    assert ok.any() and np.allclose(used[ok], c["pose"][ok], rtol=0, atol=1e-15) and not used[~ok].any()
    bank_pose = bank.pose.cpu().numpy()
    assert np.allclose(bank_pose, c["bank"]["pose"], rtol=0, atol=1e-15)
    other = dict(c["bank"], pose=bank_pose)
    _same(got, pr.expected_of(c, pose=np.where(ok[..., None], used, c["pose"]), bank=other), (name, dtype, "device pose"))


# ---- 3. no clearing, repeatable ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_is_fully_written_and_calls_repeat(dtype):
    from lidar_snow_sim_amd.tensors import PasteBatch
    c = pr.case("states", dtype)
    out = PasteBatch.empty(c["offsets"], c["gt_boxes"].shape[1], sum(c["groups"]), c["gt_boxes"].shape[2], getattr(torch, dtype), with_pose=True)
    bank = _bank(c["bank"])
    snaps = []
    for _ in range(2):
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0xFF)
        got = _run(c, out=out, bank=bank)
        assert got is out
        snaps.append([getattr(out, f).clone() for f in FIELDS])
        _same(out, pr.expected("states", dtype), ("out=", dtype))
    for a, b in zip(*snaps):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    bare = _run(c, bank=bank, return_source=False, return_pose=False)
    assert bare.source is None and bare.pose is None
    _same(bare, pr.expected("states", dtype), "bare", FIELDS[:5] + ("count",))


# ---- 4. the counter: step, seed and the frame's position -------------------------------------------------------------------------------------
def test_step_seed_and_position_change_the_draws():
    c = pr.case("q63", "float32")
    bank = _bank(c["bank"])
    base = _run(c, bank=bank)
    again = _run(c, bank=bank)
    for f in FIELDS:
        assert torch.equal(getattr(base, f).view(torch.uint8), getattr(again, f).view(torch.uint8)), f
    for changed in (dict(step=c["step"] + 1), dict(step=c["step"] + (1 << 32)), dict(seed=c["seed"] + 1), dict(seed=c["seed"] + (1 << 32))):
        d = dict(c, **changed)
        got = _run(d, bank=bank)
        _same(got, pr.expected_of(d), changed)
        assert not torch.equal(got.object, base.object)
    # frame 1 alone is frame 0 of its call: another draw than at position 1
    a, b = int(c["offsets"][1]), int(c["offsets"][2])
    one = dict(c, rows=c["rows"][a:b], keep=c["keep"][a:b], offsets=np.array([0, b - a], np.int64), gt_boxes=c["gt_boxes"][1:], pose=c["pose"][1:])
    alone = _run(one, bank=bank)
    _same(alone, pr.expected_of(one), "one frame")
    assert not torch.equal(alone.object[0], base.object[1])
    assert base.object[1].cpu().numpy().tolist() == pr.expected_of(one, frames=[1])["object"][0].tolist()


# ---- 5. one graph -----------------------------------------------------------------------------------------------------------------------------
def test_paste_objects_and_step_in_one_graph():
    """paste_objects and step += 1 captured once on a side stream after one warm-up and replayed three times: every replay equals the
    restatement at its step, and they differ from one another."""
    from lidar_snow_sim_amd.tensors import DeviceBatch, PasteBatch
    c = pr.case("q63", "float32")
    batch, gt, keep, pose, bank = DeviceBatch(_t(c["rows"]), c["offsets"]), _t(c["gt_boxes"]), _t(c["keep"]), _t(c["pose"]), _bank(c["bank"])
    out = PasteBatch.empty(c["offsets"], c["gt_boxes"].shape[1], sum(c["groups"]), c["gt_boxes"].shape[2], torch.float32, with_pose=True)
    s0 = c["step"]
    step = _step(s0 - 1)

    def call():
        paste_objects(batch, gt, bank, c["groups"], step=step, seed=c["seed"], keep=keep, remove_extra_width=c["ew"], pose=pose, out=out, return_pose=True)
        step.add_(1)

    s = torch.cuda.Stream()
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
        _same({n: v.cpu().numpy() for n, v in got[k].items()}, pr.expected_of(c, step=s0 + k), ("replay", k))
    assert not torch.equal(got[0]["object"], got[1]["object"]) and not torch.equal(got[1]["object"], got[2]["object"])


# ---- 6. the NumPy mirror and the bank builder --------------------------------------------------------------------------------------------------
def test_the_host_array_mirror_and_build_bank():
    from lidar_snow_sim_amd import paste
    c = pr.case("states", "float64")
    a, b = int(c["offsets"][0]), int(c["offsets"][1])
    one = dict(c, rows=c["rows"][a:b], keep=c["keep"][a:b], offsets=np.array([0, b - a], np.int64), gt_boxes=c["gt_boxes"][:1], pose=c["pose"][:1])
    e = pr.expected_of(one)
    got = paste.paste_objects(one["rows"], one["keep"], one["gt_boxes"][0], _bank(c["bank"]), c["groups"], seed=c["seed"], step=c["step"], remove_extra_width=c["ew"])
    for name in FIELDS:
        want = e[name][0] if name in ("gt_boxes", "object", "state", "count", "pose") else e[name]
        assert got[name].tobytes() == want.tobytes(), name
    # a bank cropped from a small frame: two cars and a pedestrian, a box with too few rows, a zero row and a class that is no whole number
    rng = np.random.default_rng(7500)
    boxes = np.array([[5, 0, 0, 4, 2, 1.5, 0.3, 2], [-6, 4, 0, 0.8, 0.8, 1.8, 0, 1], [0, -8, 0, 4, 2, 1.5, -1, 2], [20, 20, 0, 4, 2, 1.5, 0, 3], [0] * 8,
                      [-20, -20, 0, 4, 2, 1.5, 0, 1.5]], np.float32)
    counts = (30, 12, 7, 3, 0, 9)
    parts = [pr._points_in(rng, bx, n, np.float32) for bx, n in zip(boxes, counts) if n]
    frame = np.concatenate(parts + [np.column_stack((rng.uniform(40, 50, (50, 2)), np.zeros(50), np.ones(50), np.zeros(50))).astype(np.float32)])
    frame = frame[rng.permutation(len(frame))]
    bank = paste.build_bank([frame], [boxes], min_points=5)
    assert bank.n_objects == 3 and bank.classes.tolist() == [1, 2, 2] and np.diff(bank.offsets.cpu().numpy()).tolist() == [12, 30, 7]
    assert bank.class_offsets.cpu().numpy().tolist() == [0, 0, 1] + [3] * 15
    assert bank.boxes.cpu().numpy().tobytes() == boxes[[1, 0, 2]].tobytes()
    inside = br.frame_matrices(frame[:, :3].astype(np.float64), boxes[:1], br.numpy_pose(boxes[:1]))[3][:, 0]
    assert bank.points.cpu().numpy()[12:42].tobytes() == frame[inside].tobytes()            # rows in frame order, positions kept
    with pytest.raises(ValueError, match="ascending"):
        from lidar_snow_sim_amd.tensors import ObjectBank
        ObjectBank(bank.points, bank.offsets, _t(boxes[[0, 1, 2]]))


# ---- 7. what Python refuses -------------------------------------------------------------------------------------------------------------------
def test_python_refusals_in_the_stages_order():
    from lidar_snow_sim_amd.tensors import DeviceBatch, PasteBatch
    c = pr.case("q1", "float32")
    rows, gt, keep, bank = _t(c["rows"]), _t(c["gt_boxes"]), _t(c["keep"]), _bank(c["bank"])
    batch, step, groups = DeviceBatch(rows, c["offsets"]), _step(0), c["groups"]

    def refused(words, *args, **kw):
        kw.setdefault("step", step)
        with pytest.raises(ValueError, match=words):
            paste_objects(*args, **kw)

    refused("torch CUDA tensors or an aligned result", c["rows"], gt, bank, groups)
    refused(r"sample_groups\[1\] must be an integer", batch, gt, bank, (0, 1.5))
    refused("remove_extra_width is a number or three", batch, gt, bank, groups, remove_extra_width=(0.1, -0.1, 0.0))
    refused("keep must have one element per row", batch, gt, bank, groups, keep=keep[:-1])
    refused("gt_boxes must be a contiguous", batch, gt.double(), bank, groups)
    refused("bank must be an ObjectBank", batch, gt, c["bank"], groups)
    refused("step must be a one-element int64", batch, gt, bank, groups, step=torch.zeros(1, dtype=torch.int32, device="cuda"))
    refused("must add up to 1 .. 64 slots", batch, gt, bank, (0, 0))
    refused("must add up to 1 .. 64 slots", batch, gt, bank, (40, 25))
    refused("n_classes must lie in 1 .. 16", batch, gt, bank, (1,) + (0,) * 16)
    refused("n_gt plus the slots at most 256", batch, _t(np.zeros((2, 200, 8), np.float32)), bank, (30, 30))
    refused("gt_features must lie in 8 .. 10", batch, _t(np.zeros((2, 1, 7), np.float32)), bank, groups)
    refused("a sample group is negative", batch, gt, bank, (3, -1))
    refused("pose must be a contiguous", batch, gt, bank, groups, pose=torch.zeros((2, 2, 2), device="cuda"))
    refused("out must be a PasteBatch whose rows", batch, gt, bank, groups, out=PasteBatch.empty(c["offsets"][:2], 1, 1))
    # wrong in two ways: the earlier check speaks
    refused(r"sample_groups\[1\] must be an integer", batch, gt.double(), bank, (0, 1.5))
    refused("remove_extra_width is a number or three", batch, gt, bank, (0, 0), remove_extra_width=200.0)
    refused("gt_boxes must be a contiguous", batch, gt.double(), bank, (0, 0))
    refused("must add up to 1 .. 64 slots", batch, gt, bank, (0,) * 17)
    refused("a sample group is negative", batch, gt, bank, (3, -1), pose=torch.zeros((2, 2, 2), device="cuda"))
    # what only the entry refuses comes back in the entry's words
    out = PasteBatch.empty(c["offsets"], 1, 1)
    out.rows = rows
    refused("snowgpu_paste_objects_device: d_out_rows overlaps d_rows", batch, gt, bank, groups, out=out)
    out = PasteBatch.empty(c["offsets"], 1, 1)
    out.state = out.object
    refused("d_out_state overlaps d_out_object; every output needs memory of its own", batch, gt, bank, groups, out=out)
