"""-m gpu: anchor target assignment on the device (tensors.assign_anchors, anchors.assign_targets, snowgpu_assign_anchors_device;
csrc/snowgpu_anchors.hip, csrc/sg_anchors.h) against the restatement of its definition (tests/anchors_reference.py, whose cases
tests/test_anchors_reference.py holds to the conditions that keep these comparisons from being vacuous).  Everything is separately rounded
float64 arithmetic without a transcendental function, integer counts and a maximum: every output is compared byte for byte, for both
dtypes, with no element left out."""
import numpy as np
import pytest
import torch

import anchors_reference as ar
from lidar_snow_sim_amd.stages import AnchorTargetBatch, assign_anchors  # noqa: F401  (the stage under test: without it nothing here runs)

pytestmark = pytest.mark.gpu

DTYPES = ar.DTYPES
FIELDS = ar.FIELDS


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _run(c, **kw):
    kw.setdefault("return_iou", True)
    return assign_anchors(_t(c["anchors"]), _t(c["anchor_class"]), _t(c["gt_boxes"]), c["matched"], c["unmatched"], **kw)


# ---- 1. the shared cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ar.CASE_NAMES)
def test_cases(name, dtype):
    """A in 4, 6, 20, 120, 1600, 3300 (no multiple of 64 or 256 among the last two); B in 1, 2, 3, 9, 14, 60, 64, 65, 256; F in 1, 3."""
    got = _run(ar.case(name, dtype))
    _same(got, ar.expected(name, dtype), (name, dtype))
    assert torch.equal(got.positive, got.label > 0)


def test_the_shapes_the_cases_cover():
    shapes = [(ar.case(n, "float32")["anchors"].shape[0], ar.case(n, "float32")["gt_boxes"].shape[1], ar.case(n, "float32")["gt_boxes"].shape[0]) for n in ar.CASE_NAMES]
    assert {4, 6, 20, 120, 1600, 3300} <= {s[0] for s in shapes} and {1, 2, 3, 9, 14, 60, 64, 65, 256} <= {s[1] for s in shapes} and {1, 3} <= {s[2] for s in shapes}


@pytest.mark.parametrize("dtype", DTYPES)
def test_wider_rows_are_read_by_their_stride(dtype):
    """Anchors of 10 columns and gts of 10: the columns behind the heading and behind the class are not read."""
    c = ar.case("grid_b65", dtype)
    rng = np.random.default_rng(9)
    anchors = np.concatenate((c["anchors"], rng.normal(size=(c["anchors"].shape[0], 3)).astype(dtype)), axis=1)
    gt = np.concatenate((c["gt_boxes"], rng.normal(size=c["gt_boxes"].shape[:2] + (2,)).astype(dtype)), axis=2)
    _same(_run(dict(c, anchors=anchors, gt_boxes=gt)), ar.expected("grid_b65", dtype), ("wide", dtype))


def test_more_frames_than_the_grid_has_rows():
    """F = 65 537 > 65 535: the frames lie on grid.y, so a workgroup takes more than one frame -- the only size at which the kernels' frame
    loop turns twice.  Four anchors, two gts; the frames are one of three kinds (the `thresholds` gts, no gt, the two gts swapped), the
    kinds of the last three frames among them, so the expected outputs are the restatement's on the three kinds, gathered."""
    c = ar.case("thresholds_4", "float32")
    kinds = np.stack((c["gt_boxes"][0], np.zeros_like(c["gt_boxes"][0]), c["gt_boxes"][0][::-1]))
    e = ar.expected_of(dict(c, gt_boxes=kinds))
    F = 65537
    kind = (np.arange(F) % 3).astype(np.int64)
    kind[-3:] = (2, 1, 2)
    got = _run(dict(c, gt_boxes=kinds[kind]))
    assert e["gt_index"][:, ar.Q_HALF].tolist() == [0, -1, 1] and e["count"].tolist() != [e["count"][0].tolist()] * 3
    _same(got, {name: e[name][kind] for name in FIELDS}, "65537 frames")


# ---- 2. no clearing, repeatable, streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_is_fully_written_and_calls_repeat(dtype):
    c = ar.case("grid_b64", dtype)
    F, B = c["gt_boxes"].shape[:2]
    out = AnchorTargetBatch.empty(F, c["anchors"].shape[0], B, getattr(torch, dtype), with_iou=True)
    snaps = []
    for _ in range(2):
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x5A)
        got = _run(c, out=out)
        assert got is out
        snaps.append([getattr(out, f).clone() for f in FIELDS])
        _same(out, ar.expected("grid_b64", dtype), ("out=", dtype))
    for a, b in zip(*snaps):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_iou_on_request_only():
    c, e = ar.case("absent", "float32"), ar.expected("absent", "float32")
    got = _run(c, return_iou=False)
    assert got.iou is None
    _same(got, e, "without iou", FIELDS[:4])
    out = AnchorTargetBatch.empty(3, 20, 14, torch.float32, with_iou=True)
    out.iou.fill_(7)
    bare = _run(c, out=out, return_iou=False)
    assert bare.iou is None and bare.label is out.label and (out.iou == 7).all()        # a field that was not asked for is left alone
    _same(bare, e, "out= without iou", FIELDS[:4])


def test_a_side_stream_and_the_default_stream():
    c, e = ar.case("grid_b256", "float32"), ar.expected("grid_b256", "float32")
    args = [_t(c[k]) for k in ("anchors", "anchor_class", "gt_boxes")]
    torch.cuda.synchronize()
    on_default = assign_anchors(*args, c["matched"], c["unmatched"], return_iou=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        on_side = assign_anchors(*args, c["matched"], c["unmatched"], return_iou=True, slot=1)
    s.synchronize()
    _same(on_default, e, "default stream")
    _same(on_side, e, "side stream")


# ---- 3. the NumPy call shape and the helpers ---------------------------------------------------------------------------------------------------
def test_the_host_array_mirror():
    from lidar_snow_sim_amd import anchors
    for name, dtype in (("forced", "float64"), ("by_hand", "float32")):
        c, e = ar.case(name, dtype), ar.expected(name, dtype)
        got = anchors.assign_targets(c["anchors"], c["anchor_class"], c["gt_boxes"][0], c["matched"], c["unmatched"])
        for field in FIELDS:
            assert got[field].dtype == e[field].dtype and got[field].tobytes() == e[field][0].tobytes(), (name, field)


def test_helpers_against_their_indexing():
    c, e = ar.case("grid_b65", "float32"), ar.expected("grid_b65", "float32")
    got = _run(c)
    gt = c["gt_boxes"]
    F, A = e["label"].shape
    matched = np.zeros((F, A, gt.shape[2]), np.float32)
    for f in range(F):
        for a in np.flatnonzero(e["label"][f] > 0):
            matched[f, a] = gt[f, e["gt_index"][f, a]]
    assert got.matched(_t(gt)).cpu().numpy().tobytes() == matched.tobytes() and matched.any()
    assert np.array_equal(got.positive.cpu().numpy(), e["label"] > 0)
    n = np.maximum(e["count"][:, 0] + e["count"][:, 1], 1).astype(np.float32)
    want = np.where(e["label"] > 0, np.float32(1) / n[:, None], np.float32(0)).astype(np.float32)
    assert got.reg_weights().cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(got.reg_weights(norm_by_num_examples=False).cpu().numpy(), (e["label"] > 0).astype(np.float32))
    assert np.array_equal(got.cls_weights().cpu().numpy(), (e["label"] >= 0).astype(np.float32)) and (e["label"] < 0).any()
    with pytest.raises(ValueError, match="matched: gt_boxes must be"):
        got.matched(_t(gt[:, :64]))


def test_anchor_grid_on_the_device():
    from lidar_snow_sim_amd.tensors import anchor_grid
    anchors, cls = anchor_grid(ar.GRID_RANGE, ar.GRID_N, ar.GRID_SIZES, ar.GRID_ROTATIONS, ar.GRID_BOTTOMS, dtype=torch.float64)
    want, want_cls = ar.grid_anchors()
    assert anchors.is_cuda and anchors.cpu().numpy().tobytes() == want.tobytes() and cls.cpu().numpy().tobytes() == want_cls.tobytes()
    c = ar.case("grid_b64", "float64")
    got = assign_anchors(anchors, cls, _t(c["gt_boxes"]), return_iou=True)               # the defaults are KITTI's three classes
    _same(got, ar.expected("grid_b64", "float64"), "anchor_grid")


# ---- 4. one graph -----------------------------------------------------------------------------------------------------------------------------
def _scene(seed, c, n):
    """n rows per frame, most of them inside the frame's gts (a gt holds none, a few or many), and a keep mask."""
    rng = np.random.default_rng(seed)
    gt = np.array(c["gt_boxes"])
    for f in range(gt.shape[0]):
        gt[f] = gt[f, rng.permutation(gt.shape[1])]
    F, B = gt.shape[:2]
    rows = np.zeros((F * n, 5), np.float32)
    for f in range(F):
        g = gt[f, rng.integers(0, B // 2, n)]                             # only the first half of the gts gets rows
        rows[f * n:(f + 1) * n, :3] = g[:, :3] + rng.uniform(-0.3, 0.3, (n, 3)) * g[:, 3:6]
    rows[:, 3], rows[:, 4] = rng.integers(1, 255, F * n), rng.integers(0, 64, F * n)
    return rows, rng.uniform(0, 1, F * n) < 0.8, gt


def test_keep_boxes_assign_and_matched_in_one_graph():
    """points_in_boxes(res, gt).keep_boxes(5) -> the gts zeroed by that mask -> assign_anchors(out=) -> .matched(), captured once and replayed
    after rows, keep mask and gt boxes were rewritten in place: each replay equals the eager chain on the same inputs, and the restatement
    on the gts that chain kept."""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import AlignedResult, BoxLabelBatch, points_in_boxes
    c = ar.case("grid_b64", "float32")
    F, B, n = 3, 64, 1500
    offsets = np.arange(F + 1, dtype=np.int64) * n
    anchors, cls = _t(c["anchors"]), _t(c["anchor_class"])
    A = anchors.shape[0]
    scenes = [_scene(40 + k, c, n) for k in range(3)]
    eng = engine.get_engine(torch.cuda.current_device(), 0)
    z = torch.zeros(1, dtype=torch.int64).cuda()
    rows, keep, gt = _t(scenes[0][0]), _t(scenes[0][1]), _t(scenes[0][2])
    live = torch.empty_like(gt)

    def chain(res, labels, out):
        lab = points_in_boxes(res, gt, out=labels)
        live.copy_(gt * lab.keep_boxes(5)[..., None].to(gt.dtype))
        at = assign_anchors(anchors, cls, live, out=out, return_iou=True)
        return at, at.matched(live)

    eager = []
    for r, k, g in scenes:
        rows.copy_(_t(r)); keep.copy_(_t(k)); gt.copy_(_t(g))
        res = AlignedResult(eng.ctx, rows, keep, z, z, z, offsets, torch.cuda.current_stream())
        at, m = chain(res, None, None)
        eager.append(({f: getattr(at, f).clone() for f in FIELDS}, m.clone(), live.clone()))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        res = AlignedResult(eng.ctx, rows, keep, z, z, z, offsets, s)
        labels, out = BoxLabelBatch.empty(offsets, B, torch.float32), AnchorTargetBatch.empty(F, A, B, torch.float32, with_iou=True)
        chain(res, labels, out)                                            # warm-up: the captured calls allocate no scratch
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            at, m = chain(res, labels, out)
        assert at is out
        got = []
        for r, k, b in scenes:                                             # no host read between the replays
            rows.copy_(_t(r)); keep.copy_(_t(k)); gt.copy_(_t(b))
            for f in FIELDS:
                getattr(out, f).view(torch.uint8).fill_(0x5A)
            g.replay()
            got.append(({f: getattr(out, f).clone() for f in FIELDS}, m.clone(), live.clone()))
        s.synchronize()
    for k in range(3):
        for f in FIELDS:
            assert torch.equal(got[k][0][f].view(torch.uint8), eager[k][0][f].view(torch.uint8)), (k, f)
        assert torch.equal(got[k][1].view(torch.uint8), eager[k][1].view(torch.uint8)) and torch.equal(got[k][2].view(torch.uint8), eager[k][2].view(torch.uint8))
        kept = got[k][2].cpu().numpy()
        present = (kept[..., 3] > 0)
        assert present.any(axis=1).all() and (~present & (scenes[k][2][..., 3] > 0)).any()      # the mask keeps some gts and drops some
        want = ar.assign(c["anchors"], c["anchor_class"], kept)
        for f in FIELDS:
            assert got[k][0][f].cpu().numpy().tobytes() == want[f].tobytes(), (k, f)
        assert (want["label"] > 0).any(axis=1).all() and got[k][1].any()
    assert not torch.equal(got[0][0]["label"], got[1][0]["label"]) and not torch.equal(got[1][0]["label"], got[2][0]["label"])


# ---- 5. what Python refuses -------------------------------------------------------------------------------------------------------------------
def test_python_refusals_in_the_stages_order():
    c = ar.case("absent", "float32")
    anchors, cls, gt = _t(c["anchors"]), _t(c["anchor_class"]), _t(c["gt_boxes"])

    def refused(words, *args, **kw):
        with pytest.raises(ValueError, match=words):
            assign_anchors(*args, **kw)

    refused("matched and unmatched hold one number per class", anchors, cls, gt, (0.6, 0.5), (0.45,))
    refused("matched and unmatched hold one number per class", anchors, cls, gt, 0.6, 0.45)
    refused("anchors must be a contiguous", anchors.cpu(), cls, gt)
    refused("anchors must be a contiguous", anchors[None], cls, gt)
    refused("anchor_class must be a contiguous", anchors, cls.long(), gt)
    refused("anchor_class must be a contiguous", anchors, cls[:-1], gt)
    refused("gt_boxes must be a contiguous", anchors, cls, gt.double())
    refused("gt_boxes must be a contiguous", anchors, cls, gt[0])
    refused("n_gt must lie in 1 .. 256", anchors, cls, torch.zeros((1, 257, 8), device="cuda"))
    refused("out must be a AnchorTargetBatch whose label", anchors, cls, gt, out=AnchorTargetBatch.empty(3, 21, 14))
    refused("out must be a AnchorTargetBatch whose iou", anchors, cls, gt, out=AnchorTargetBatch.empty(3, 20, 14), return_iou=True)
    # wrong in two ways: the earlier check speaks
    refused("anchors must be a contiguous", anchors.cpu(), cls.long(), gt)
    refused("gt_boxes must be a contiguous", anchors, cls, gt.double(), out=AnchorTargetBatch.empty(3, 21, 14))
    # what only the entry refuses comes back in the entry's words
    refused("snowgpu_assign_anchors_device: every class needs 0 < unmatched <= matched <= 1", anchors, cls, gt, (0.6, 0.5, 0.5), (0.45, 0.55, 0.35))
    refused("snowgpu_assign_anchors_device: n_classes must lie in 1 .. 16", anchors, cls, gt, (0.6,) * 17, (0.45,) * 17)
    refused("snowgpu_assign_anchors_device: gt_features must lie in 8 .. 10", anchors, cls, gt[..., :7].contiguous())
    refused("snowgpu_assign_anchors_device: anchor_features must lie in 7 .. 10", anchors[:, :6].contiguous(), cls, gt)
    out = AnchorTargetBatch.empty(3, 20, 14)
    out.gt_index = out.label
    refused("d_out_gt_index overlaps d_out_label; every output needs memory of its own", anchors, cls, gt, out=out)
