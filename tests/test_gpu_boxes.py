"""-m gpu: points in 3D boxes on the device (tensors.points_in_boxes, boxes.points_in_boxes, snowgpu_points_in_boxes_device;
csrc/snowgpu_box.hip, csrc/sg_box.h) against the brute-force NumPy restatement of its definition (tests/box_reference.py, whose inputs
tests/test_box_reference.py holds to the conditions that keep these comparisons from being vacuous).  The restatement takes the pose as an
input and everything behind the pose is separately rounded float64 arithmetic in the definition's order: box_of, count and local are
compared byte for byte, for both dtypes, with no row and no box left out.  The device library's cos / sin is compared on its own."""
import re

import numpy as np
import pytest
import torch

import box_reference as br

pytestmark = pytest.mark.gpu

DTYPES = br.DTYPES
FIELDS = ("box_of", "count", "local")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _frames(rows, offsets):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(rows), offsets)


def _pib(*args, **kw):
    from lidar_snow_sim_amd.tensors import points_in_boxes
    return points_in_boxes(*args, **kw)


def _run_case(name, dtype, given, **kw):
    rows, offsets, keep, boxes, pose = br.case(name, dtype)
    kw.setdefault("return_local", True)
    kw.setdefault("return_pose", True)
    return _pib(_frames(rows, offsets), _t(boxes), pose=_t(pose) if given else None, keep=None if keep is None else _t(keep), **kw)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


# ---- 1. the restatement under the pose the device used ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", br.CASES)
def test_shared_inputs_equal_the_restatement_fed_the_returned_pose(name, dtype):
    rows, offsets, keep, boxes, _ = br.case(name, dtype)
    got = _run_case(name, dtype, False)
    used = got.pose.cpu().numpy()
    ok = br.present(boxes, br.numpy_pose(boxes))
    assert used.dtype == np.float64 and used.shape == boxes.shape[:2] + (2,) and not used[~ok].any() and (np.abs((used[ok] ** 2).sum(-1) - 1) < 1e-12).all()
    _same(got, br.points_in_boxes(rows, boxes, used, keep, offsets), (name, dtype))
    assert got.n_boxes == boxes.shape[1] and np.array_equal(got.offsets, offsets)


# ---- 2. a given pose ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", br.CASES)
def test_given_pose(name, dtype):
    """NumPy's pose given (in the constructed batch one box under (2, 0): absent): every output is the restatement's, byte for byte."""
    rows, offsets, keep, boxes, pose = br.case(name, dtype)
    got = _run_case(name, dtype, True)
    _same(got, br.expected(name, dtype), (name, dtype))
    assert got.pose.cpu().numpy().tobytes() == br.used_pose(boxes, pose).tobytes()


# ---- 3. the device library's cos / sin ------------------------------------------------------------------------------------------------------------
def test_device_pose():
    """cos / sin of the heading in float64 from the device library against the correctly rounded values.  No bound for float64 sin / cos is
    documented in the ROCm installation, so this is OpenCL's conformance bound: 4 ulp.  The reference is glibc's cosl / sinl on the
    80-bit format (np.longdouble, 64 bits of precision: 2^-11 ulp of a double -- the headings are doubles, so the argument is exact); on
    a host without that format it is NumPy's float64 cos / sin, which glibc holds within 1 ulp, and the bound is 4 + 1 ulp.  Exactly
    (1, 0) at heading 0.  Seen on one MI355X: 0.704 ulp at most, 1.0 ulp from NumPy's values."""
    rng = np.random.default_rng(77)
    h = np.concatenate((list(br.HEADINGS), [0.0, -0.0, np.pi / 4, 1e-300, 1e6, -1e6, 999999.5], rng.uniform(-np.pi, np.pi, 96), rng.uniform(-100, 100, 77),
                        rng.uniform(-1e6, 1e6, 68)))
    assert len(h) == 256
    boxes = np.zeros((1, 256, 7))
    boxes[0, :, 3:6] = 1.0
    boxes[0, :, 6] = h
    got = _pib(_t(np.zeros((4, 5))), _t(boxes), return_pose=True).pose.cpu().numpy()[0]
    assert got[h == 0].tolist() == [[1.0, 0.0]] * int((h == 0).sum()) and (h == 0).sum() >= 3
    extended = np.finfo(np.longdouble).nmant >= 63
    hl = h.astype(np.longdouble)
    true = np.stack((np.cos(hl), np.sin(hl)), axis=-1)
    ulp = np.spacing(np.abs(true.astype(np.float64))).astype(np.longdouble)
    err = np.abs(got.astype(np.longdouble) - true) / ulp
    against_numpy = np.abs(got - br.numpy_pose(boxes)[0]) / np.spacing(np.abs(true.astype(np.float64)))
    print("device pose: largest error %.3f ulp, largest difference from NumPy %.3f ulp" % (float(err.max()), float(against_numpy.max())))
    assert float(err.max()) <= (4.0 if extended else 5.0), (float(err.max()), h[np.unravel_index(int(err.argmax()), err.shape)[0]])


# ---- 4. behind the aligned snowfall call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_synthetic_sweep_behind_the_aligned_call(tables, dtype):
    """One synthetic sweep through augment_batch(layout='aligned'); boxes centred on kept rows.  The aligned result goes in as it is, and
    calling with res.keep equals calling on the compacted rows, at their indices."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import augment_batch
    tl = [tables["t"][i % 4] for i in range(64)]
    plane, bd = (np.array([0.0, 0.0, -1.0]), -1.7), float(np.degrees(3e-3))
    frame = np.ascontiguousarray(synthetic_sweep(64, 128, seed=1900, intensity="lambert").astype(dtype))
    res = augment_batch([_t(frame)], "unused", bd, particles=tl, orders=[list(np.random.default_rng(3).permutation(64))], planes=[plane], layout="aligned",
                        sync=False)
    res.wait()
    rows, keep = res.rows.cpu().numpy(), res.keep.cpu().numpy().astype(bool)
    rng = np.random.default_rng(11)
    kept = np.flatnonzero(keep & br.usable_rows(rows))
    assert 2000 < len(kept) < len(rows)
    B = 24
    boxes = np.zeros((1, B, 8), rows.dtype)
    at = rng.choice(kept, B, replace=False)
    boxes[0, :, :3] = rows[at, :3]
    boxes[0, :, 3:6] = np.column_stack((rng.uniform(3.5, 5, B), rng.uniform(1.6, 2.1, B), rng.uniform(1.4, 2, B)))
    boxes[0, :, 6] = rng.uniform(-np.pi, np.pi, B)
    boxes[0, 5] = 0                                                  # padding
    pose = br.numpy_pose(boxes)
    got = _pib(res, _t(boxes), pose=_t(pose), return_local=True)
    want = br.points_in_boxes(rows, boxes, pose, keep)
    _same(got, want, dtype)
    assert (want["box_of"][at[np.arange(B) != 5]] >= 0).all() and (want["box_of"][~keep] == -1).all() and want["count"][0, 5] == 0
    assert (want["count"][0, np.arange(B) != 5] >= 1).all() and (want["box_of"] >= 0).sum() > B
    compact = _pib(_t(rows[keep]), _t(boxes), pose=_t(pose), return_local=True)
    assert compact.box_of.cpu().numpy().tobytes() == want["box_of"][keep].tobytes() and compact.local.cpu().numpy().tobytes() == want["local"][keep].tobytes()
    assert compact.count.cpu().numpy().tobytes() == want["count"].tobytes()
    with_mask = _pib(_t(rows), _t(boxes), pose=_t(pose), keep=res.keep, return_local=True)
    _same(with_mask, want, (dtype, "keep="))


# ---- 5. the ways back -----------------------------------------------------------------------------------------------------------------------------
def test_ways_back():
    from lidar_snow_sim_amd.tensors import dror_keep, sample_keypoints
    rows, offsets, keep, boxes, pose = br.case("random", "float32")
    got = _run_case("random", "float32", True)
    want = br.expected("random", "float32")
    F, B = boxes.shape[:2]
    frame = np.repeat(np.arange(F), np.diff(offsets))
    flat = np.where(want["box_of"] >= 0, want["box_of"] + frame * B, -1)
    assert np.array_equal(got.flat_index().cpu().numpy(), flat) and got.flat_index().dtype == torch.int64
    cls = boxes[:, :, 7].astype(np.int64)
    labels = got.labels(_t(cls)).cpu().numpy()
    assert np.array_equal(labels, np.where(flat >= 0, cls.reshape(-1)[np.maximum(flat, 0)], 0)) and set(np.unique(labels).tolist()) == {0, 1, 2, 3}
    wide = got.labels(_t(boxes[:, :, 7:10]), background=-7).cpu().numpy()
    assert wide.shape == (len(rows), 3) and np.array_equal(wide, np.where((flat >= 0)[:, None], boxes.reshape(F * B, -1)[np.maximum(flat, 0), 7:10], -7))
    for m in (1, 5, 40):
        kb = got.keep_boxes(m).cpu().numpy()
        assert kb.dtype == bool and np.array_equal(kb, want["count"] >= m)
    assert int(got.keep_boxes().sum()) < int(br.present(boxes, pose).sum())                      # an empty present box is filtered out
    assert np.array_equal(got.rows_in().cpu().numpy(), want["box_of"] >= 0)
    pick = np.random.default_rng(2).random((F, B)) < 0.5
    assert np.array_equal(got.rows_in(_t(pick)).cpu().numpy(), (flat >= 0) & pick.reshape(-1)[np.maximum(flat, 0)])
    for bad in (dict(min_points=0), dict(min_points=1.5)):
        with pytest.raises(ValueError, match="min_points must be an integer of at least 1"):
            got.keep_boxes(**bad)
    with pytest.raises(ValueError, match="per_box must be a"):
        got.labels(_t(cls[:, :5]))
    with pytest.raises(ValueError, match="box_mask must be a"):
        got.rows_in(_t(cls))
    # labels of keypoints: box_of at their indices; the objects' rows as a keep mask of the outlier filter
    one = _t(rows[:offsets[1]])
    kp = sample_keypoints(one, 128)
    single = _pib(one, _t(boxes[:1]), pose=_t(pose[:1]))
    index = kp.index[0].long()
    assert np.array_equal(single.box_of[index].cpu().numpy(), want["box_of"][:offsets[1]][kp.index[0].cpu().numpy()])
    inside = single.rows_in()
    kept = dror_keep(one, keep=inside).cpu().numpy().astype(bool)
    assert kept.shape == (offsets[1],) and not kept[~inside.cpu().numpy()].any() and kept.any()


# ---- 6. buffers, runs and graphs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written_in_place(dtype):
    from lidar_snow_sim_amd.tensors import BoxLabelBatch
    for name in ("constructed", "words65"):
        rows, offsets, _, boxes, pose = br.case(name, dtype)
        out = BoxLabelBatch.empty(offsets, boxes.shape[1], getattr(torch, dtype), with_local=True, with_pose=True)
        for f in FIELDS + ("pose",):
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        got = _run_case(name, dtype, True, out=out)
        assert got is out
        _same(out, br.expected(name, dtype), (name, dtype))
        assert out.pose.cpu().numpy().tobytes() == br.used_pose(boxes, pose).tobytes()
    bare = _run_case("random", dtype, True, return_count=False, return_local=False, return_pose=False)
    assert bare.count is None and bare.local is None and bare.pose is None
    _same(bare, br.expected("random", dtype), dtype, FIELDS[:1])
    # a batch without a row: the counts are zeroed and the pose is written
    boxes = br.case("random", dtype)[3]
    out = BoxLabelBatch.empty(np.array([0, 0, 0]), boxes.shape[1], getattr(torch, dtype), with_local=True, with_pose=True)
    out.count.fill_(9)
    out.pose.fill_(9.0)
    none = _pib(_frames(np.zeros((0, 5), dtype), np.array([0, 0, 0], np.int64)), _t(boxes), out=out, return_local=True, return_pose=True)
    assert tuple(none.box_of.shape) == (0,) and tuple(none.local.shape) == (0, 3) and not none.count.any()
    assert none.pose.cpu().numpy()[~br.present(boxes, br.numpy_pose(boxes))].any() == False and (none.pose.cpu().numpy() != 9.0).all()


def test_two_calls_give_identical_bytes():
    for name in ("constructed", "words256", "random"):
        a, b = _run_case(name, "float32", False), _run_case(name, "float32", False)
        for f in FIELDS + ("pose",):
            assert getattr(a, f).data_ptr() != getattr(b, f).data_ptr() and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), (name, f)


def test_graph_capture():
    """One capture after a warm-up, replayed on changed rows and boxes in the same tensors: the scratch and every output are rewritten by
    the captured sequence itself.  A linear graph."""
    from lidar_snow_sim_amd.tensors import BoxLabelBatch
    rows0, offsets, _, boxes0, pose0 = br.case("random", "float32")
    n = int(offsets[1])
    assert offsets[2] - offsets[1] < n                                 # (the second draw is padded with rows of the first)
    inputs = [(rows0[:n], boxes0[:1], pose0[:1]), (np.vstack((rows0[offsets[1]:], rows0[:n - (offsets[2] - offsets[1])])), boxes0[1:], pose0[1:])]
    want = [br.points_in_boxes(r, b, p) for r, b, p in inputs]
    assert not np.array_equal(want[0]["box_of"], want[1]["box_of"])
    s = torch.cuda.Stream()
    rows, boxes, pose = (_t(a) for a in inputs[0])
    out = BoxLabelBatch.empty(n, boxes.shape[1], torch.float32, with_local=True)
    with torch.cuda.stream(s):
        _pib(rows, boxes, pose=pose, out=out, return_local=True)       # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = _pib(rows, boxes, pose=pose, out=out, return_local=True)
        assert got is out
        snaps = []
        for k in (1, 0, 1):
            for dst, src in zip((rows, boxes, pose), inputs[k]):
                dst.copy_(_t(src))
            for f in FIELDS:
                getattr(out, f).view(torch.uint8).fill_(0x7f)
            g.replay()
            snaps.append((k, {f: getattr(out, f).clone() for f in FIELDS}))
        s.synchronize()
    for k, snap in snaps:
        for f in FIELDS:
            assert snap[f].cpu().numpy().tobytes() == want[k][f].tobytes(), (k, f)


# ---- 7. the NumPy entry -----------------------------------------------------------------------------------------------------------------------
def test_numpy_entry():
    from lidar_snow_sim_amd.boxes import points_in_boxes
    for dtype in DTYPES:
        rows, offsets, _, boxes, _ = br.case("random", dtype)
        a, b = int(offsets[1]), int(offsets[2])
        want = br.points_in_boxes(rows[a:b], boxes[1:], br.numpy_pose(boxes[1:]))
        for cols in (5, 3):
            box_of, count, local = points_in_boxes(rows[a:b, :cols], boxes[1], return_local=True)
            assert box_of.dtype == np.int32 and count.dtype == np.int32 and local.dtype == rows.dtype and count.shape == (boxes.shape[1],)
            assert np.array_equal(box_of, want["box_of"]) and np.array_equal(count, want["count"][0]) and local.tobytes() == want["local"].tobytes()
        box_of, count = points_in_boxes(rows[a:b], boxes[1][:, :7])
        assert np.array_equal(box_of, want["box_of"]) and np.array_equal(count, want["count"][0])
    with pytest.raises(ValueError):
        points_in_boxes(rows[:, :2], boxes[0])
    with pytest.raises(ValueError):
        points_in_boxes(rows, boxes[0][:, :6])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import BoxLabelBatch
    rows, offsets, _, boxes, pose = br.case("random")
    pc, bx, ps, n = _frames(rows, offsets), _t(boxes), _t(pose), len(rows)
    F, B = boxes.shape[:2]
    wide = _t(np.concatenate((boxes, boxes), axis=2))
    many = _t(np.zeros((F, 257, 7), np.float32))
    for kw, words in ((dict(boxes=bx.double()), "boxes must be a contiguous"), (dict(boxes=bx.cpu()), "boxes must be a contiguous"),
                      (dict(boxes=bx[0]), "boxes must be a contiguous"), (dict(boxes=bx[:1]), "boxes must be a contiguous"),
                      (dict(boxes=wide[:, :, :8]), "boxes must be a contiguous"),                       # not contiguous
                      (dict(boxes=bx[:, :, :6].contiguous()), "box_features must lie in 7 .. 10.*boxes"),
                      (dict(boxes=wide[:, :, :11].contiguous()), "box_features must lie in 7 .. 10.*boxes"),
                      (dict(boxes=many), "n_boxes must lie in 1 .. 256.*boxes"), (dict(boxes=bx[:, :0].contiguous()), "n_boxes must lie in 1 .. 256.*boxes"),
                      (dict(pose=ps.float()), "pose must be a contiguous"), (dict(pose=ps[:, :5].contiguous()), "pose must be a contiguous"),
                      (dict(pose=pose), "pose must be a contiguous")):
        args = dict(boxes=bx, pose=ps)
        args.update(kw)
        with pytest.raises(ValueError, match=words.replace("..", r"\.\.")):
            _pib(pc, args.pop("boxes"), **args)
    with pytest.raises(ValueError, match="torch CUDA tensors"):
        _pib(rows, bx)
    with pytest.raises(ValueError):
        _pib(pc, bx, keep=torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError, match="out must be a BoxLabelBatch whose box_of"):
        _pib(pc, bx, out=BoxLabelBatch.empty(n - 1, B))
    with pytest.raises(ValueError, match="out must be a BoxLabelBatch whose count"):
        _pib(pc, bx, out=BoxLabelBatch.empty(offsets, B + 1))
    with pytest.raises(ValueError, match="out must be a BoxLabelBatch whose local"):
        _pib(pc, bx, out=BoxLabelBatch.empty(offsets, B, torch.float64, with_local=True), return_local=True)
    with pytest.raises(ValueError, match="out must be a BoxLabelBatch whose pose"):
        _pib(pc, bx, out=BoxLabelBatch.empty(offsets, B), return_pose=True)
    # the C entry refuses on its own: the domain, the overlaps, and a null output; the nullable ones may be null
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    arena = torch.zeros(bx.numel() + 3 * n, device="cuda:0")          # the boxes with 12 n bytes of their own allocation behind them: a d_out_local put
    bx = arena[:bx.numel()].view(bx.shape).copy_(bx)                  # on their last value reaches no other tensor, wherever the allocator placed the rest
    d_rows, off = _t(rows), _t(offsets)
    out = BoxLabelBatch.empty(offsets, B, with_local=True, with_pose=True)
    mask = torch.ones(n + 65536, dtype=torch.uint8, device="cuda:0")
    head = (F, n, int(np.diff(offsets).max()), off.data_ptr(), d_rows.data_ptr(), 0)
    p = dict(box_of=out.box_of.data_ptr(), count=out.count.data_ptr(), local=out.local.data_ptr(), pose=out.pose.data_ptr())

    def call(n_boxes=B, feats=10, pose_in=ps.data_ptr(), keep=0, **outs):
        q = dict(p, **outs)
        ctx.points_in_boxes_device(*head, n_boxes, bx.data_ptr(), feats, pose_in, keep, q["box_of"], q["count"], q["local"], q["pose"])

    who = "snowgpu_points_in_boxes_device: "
    for kw, words in ((dict(n_boxes=0), who + "n_boxes must lie in 1 .. 256"), (dict(n_boxes=257), who + "n_boxes must lie in 1 .. 256"),
                      (dict(feats=6), who + "box_features must lie in 7 .. 10"), (dict(feats=11), who + "box_features must lie in 7 .. 10"),
                      (dict(box_of=0), who + "null pointer or bad dtype"),
                      (dict(keep=mask.data_ptr(), box_of=mask.data_ptr() + 8), who + "d_out_box_of overlaps d_keep_in"),
                      (dict(count=d_rows.data_ptr()), who + "d_out_count overlaps d_rows"),
                      (dict(local=bx.data_ptr() + 4 * (F * B * 10 - 1)), who + "d_out_local overlaps d_boxes"),
                      (dict(pose=ps.data_ptr()), who + "d_out_pose overlaps d_pose_in"),
                      (dict(count=out.box_of.data_ptr()), who + "d_out_count overlaps d_out_box_of; every output needs memory of its own"),
                      (dict(pose=out.local.data_ptr()), who + "d_out_pose overlaps d_out_local; every output needs memory of its own")):
        with pytest.raises(ValueError, match=words.replace("..", r"\.\.")):
            call(**kw)
    want = br.expected("random", "float32")
    out.box_of.fill_(9)
    call(count=0, local=0, pose=0)
    torch.cuda.synchronize()
    assert np.array_equal(out.box_of.cpu().numpy(), want["box_of"])


# ---- every refusal of the Python boundary word for word, and which of two faults is reported -----------------------------------------------------
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _pin_boxes(n=2, features=7, dtype=torch.float32):
    return torch.ones((2, n, features), dtype=dtype, device="cuda:0")


def _label_out(rows=128, **kw):
    from lidar_snow_sim_amd.tensors import BoxLabelBatch
    return BoxLabelBatch.empty(np.array([0, rows // 2, rows]), 2, **kw)


HOST_WORDS = "points_in_boxes: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.boxes.points_in_boxes)"
BOX_WORDS = "points_in_boxes: boxes must be a contiguous (frames, B, 7 .. 10) tensor in the rows' dtype on their device"
POSE_WORDS = "points_in_boxes: pose must be a contiguous (2, 2, 2) float64 tensor (cos, sin) on the device of the rows"
KEEP_WORDS = "keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)"
OUT_WORDS = "points_in_boxes: out must be a BoxLabelBatch whose %s tensor on the device of the rows"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)), HOST_WORDS),
    ("boxes of another dtype", lambda: dict(boxes=_pin_boxes(dtype=torch.float64)), BOX_WORDS),
    ("boxes of one frame", lambda: dict(boxes=_pin_boxes()[:1]), BOX_WORDS),
    ("257 boxes", lambda: dict(boxes=_pin_boxes(257)), "points_in_boxes: n_boxes must lie in 1 .. 256 (boxes)"),
    ("no box", lambda: dict(boxes=_pin_boxes(0)), "points_in_boxes: n_boxes must lie in 1 .. 256 (boxes)"),
    ("boxes of 6 columns", lambda: dict(boxes=_pin_boxes(features=6)), "points_in_boxes: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes)"),
    ("pose of float32", lambda: dict(pose=torch.ones((2, 2, 2), device="cuda:0")), POSE_WORDS),
    ("out for other rows", lambda: dict(out=_label_out(126)), OUT_WORDS % "box_of is a contiguous (128,) torch.int32"),
    ("out of another kind", lambda: dict(out=object()), OUT_WORDS % "box_of is a contiguous (128,) torch.int32"),
    ("out without count", lambda: dict(out=_label_out(with_count=False)), OUT_WORDS % "count is a contiguous (2, 2) torch.int32"),
    ("out without local", lambda: dict(out=_label_out(), return_local=True), OUT_WORDS % "local is a contiguous (128, 3) torch.float32"),
    ("out without pose", lambda: dict(out=_label_out(), return_pose=True), OUT_WORDS % "pose is a contiguous (2, 2, 2) torch.float64"),
    # two faults: the earlier step of the call reports
    ("host rows before the boxes", lambda: dict(frames=np.zeros((4, 5), np.float32), boxes=_pin_boxes(features=6)), HOST_WORDS),
    ("the device before the boxes", lambda: dict(device=1, boxes=_pin_boxes(features=6)), "the tensors live on cuda:0, device=1 was asked for"),
    ("keep before the boxes", lambda: dict(keep=torch.ones(127, dtype=torch.bool, device="cuda:0"), boxes=_pin_boxes(features=6)), KEEP_WORDS),
    ("the boxes before the pose", lambda: dict(boxes=_pin_boxes(features=6), pose=torch.ones((2, 2, 2), device="cuda:0")),
     "points_in_boxes: box_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (boxes)"),
    ("the pose before out", lambda: dict(pose=torch.ones((2, 2, 2), device="cuda:0"), out=object()), POSE_WORDS),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    from lidar_snow_sim_amd.tensors import points_in_boxes
    args = dict(frames=_pin_batch(), boxes=_pin_boxes())
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        points_in_boxes(**args)
