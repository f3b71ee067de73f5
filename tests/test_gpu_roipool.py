"""-m gpu: RoI point pooling on the device (tensors.roi_point_pool, roipool.roipoint_pool3d, snowgpu_roi_point_pool_device;
csrc/snowgpu_roipool.hip, csrc/sg_roipool.h) against the NumPy restatement of its definition (tests/roipool_reference.py, whose inputs
tests/test_roipool_reference.py holds to the conditions that keep these comparisons from being vacuous).  The restatement takes the pose
as an input and everything behind the pose is separately rounded float64 arithmetic in the definition's order: every output is compared
byte for byte, for both dtypes, with no element left out -- under a given pose, and under the pose the device computed and returned."""
import re

import numpy as np
import pytest
import torch

import iou_reference as ir
import roipool_reference as rr

pytestmark = pytest.mark.gpu

DTYPES = rr.DTYPES
FIELDS = ("index", "count", "points", "local", "pose")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _pool(*args, **kw):
    from lidar_snow_sim_amd.tensors import roi_point_pool
    return roi_point_pool(*args, **kw)


def _batch(c):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(c["rows"]), np.array(c["offsets"]))                 # (copies: the shared inputs are read-only)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, len(bad), "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _run(c, pose="given", **kw):
    args = dict(extra_width=c["ew"], pose=_t(c["pose"]) if pose == "given" else None, keep=None if c["keep"] is None else _t(c["keep"]),
                num_features=c["C"], return_local=True, return_pose=True)
    args.update(kw)
    return _pool(_batch(c), _t(c["rois"]), c["S"], **args)


# ---- 1. the shared cases under their given pose: counts around S, the seams, overlap, faces, absent things ------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", rr.CASES)
def test_cases_under_a_given_pose(name, dtype):
    c = rr.case(name, dtype)
    got = _run(c)
    _same(got, rr.expected(name, dtype), (name, dtype))
    assert torch.equal(got.empty_flag, got.count == 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_are_not_clipped_and_the_fill_wraps(dtype):
    """Stated on the device's own output: count beyond S, and slot j of a roi of fewer members is slot j mod count."""
    for S in (1, 100, 512):
        c = rr.case(f"counts{S}", dtype)
        got = _run(c)
        count, index = got.count.cpu().numpy(), got.index.cpu().numpy()
        assert count[0].tolist() == list(rr.count_targets(S)) + [S] and count.max() > 3 * S
        for f, m in zip(*np.nonzero((count > 0) & (count < S))):
            assert np.array_equal(index[f, m], index[f, m, np.arange(S) % count[f, m]]) and (np.diff(index[f, m, :count[f, m]]) > 0).all()
        assert (index[count == 0] == -1).all()


# ---- 2. headings through the device pose -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("headings", "seams", "absent"))
def test_cases_under_the_device_pose(name, dtype):
    c = rr.case(name, dtype)
    got = _run(c, pose=None)
    used = got.pose.cpu().numpy()
    rois = c["rois"]
    numpy_pose = ir.numpy_pose(rois)
    with np.errstate(invalid="ignore"):
        ok = rr.present(rois, numpy_pose, c["ew"])
    assert np.array_equal(used.any(axis=-1), ok) and np.allclose(used[ok], numpy_pose[ok], rtol=0, atol=1e-15)
    _same(got, rr.pool_case(c, pose=used), (name, dtype, "device pose"))


# ---- 3. no clearing ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_is_fully_written_and_calls_repeat(dtype):
    from lidar_snow_sim_amd.tensors import DeviceBatch, RoiPointBatch
    c = rr.case("counts100", dtype)
    F, M = c["rois"].shape[:2]
    out = RoiPointBatch.empty(F, M, c["S"], c["C"], getattr(torch, dtype), with_local=True, with_pose=True)
    snaps = []
    for _ in range(2):
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x5A)
        got = _run(c, out=out)
        assert got is out
        snaps.append([getattr(out, f).clone() for f in FIELDS])
        _same(out, rr.expected("counts100", dtype), ("out=", dtype))
    for a, b in zip(*snaps):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # a batch with no rows still writes -1, zeros and the pose
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x5A)
    empty = DeviceBatch(_t(np.zeros((0, 5), dtype)), np.zeros(F + 1, np.int64))
    got = _pool(empty, _t(c["rois"]), c["S"], pose=_t(c["pose"]), num_features=c["C"], out=out, return_local=True, return_pose=True)
    want = rr.roi_point_pool(np.zeros((0, 5), dtype), c["rois"], c["pose"], c["S"], c["C"], offsets=np.zeros(F + 1, np.int64))
    assert (want["index"] == -1).all() and want["pose"].any()
    _same(got, want, ("no rows", dtype))


def test_fields_that_were_not_asked_for_and_an_nms_batch():
    from lidar_snow_sim_amd.tensors import NmsBatch
    c = rr.case("overlap65", "float32")
    got = _pool(_batch(c), _t(c["rois"]), c["S"], pose=_t(c["pose"]), return_points=False)
    assert got.points is None and got.local is None and got.pose is None
    _same(got, rr.expected("overlap65", "float32"), "bare", ("index", "count"))
    F, M = c["rois"].shape[:2]
    nb = NmsBatch(torch.zeros((F, M), dtype=torch.int32).cuda(), torch.zeros(F, dtype=torch.int32).cuda(), _t(c["rois"]))
    _same(_pool(_batch(c), nb, c["S"], pose=_t(c["pose"]), return_local=True, return_pose=True), rr.expected("overlap65", "float32"), "NmsBatch")


def test_an_aligned_result_brings_its_rows_and_its_keep_mask():
    """An AlignedResult stands where the frames stand: its rows, its offsets, and its keep mask ANDed with the caller's."""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import AlignedResult
    c = rr.case("absent", "float32")
    n = len(c["rows"])
    own = np.arange(n) % 5 != 2
    eng = engine.get_engine(torch.cuda.current_device(), 0)
    z = torch.zeros(1, dtype=torch.int64).cuda()
    res = AlignedResult(eng.ctx, _t(c["rows"]), _t(own), z, z, z, np.array(c["offsets"]), torch.cuda.current_stream())
    for mask in (None, c["keep"]):
        got = _pool(res, _t(c["rois"]), c["S"], extra_width=c["ew"], pose=_t(c["pose"]), keep=None if mask is None else _t(mask), num_features=c["C"],
                    return_local=True, return_pose=True)
        want = rr.pool_case(c, keep=own if mask is None else own & mask)
        assert want["count"].sum() < rr.expected("absent", "float32")["count"].sum() or mask is None
        _same(got, want, ("aligned result", mask is not None))


# ---- 4. one graph: nms -> roi_point_pool -> gather ---------------------------------------------------------------------------------------------
def test_graph_capture():
    """One capture after a warm-up on a side stream, replayed after rows, proposals, scores and the keep mask have been rewritten in place,
    every output filled with 0x7f before: each replay equals the restatements composed -- NMS, then the pooling of the kept boxes under
    the pose the device used, then plain indexing."""
    from lidar_snow_sim_amd.tensors import DeviceBatch, NmsBatch, RoiPointBatch, nms
    F, n, B, P, S, C = 2, 2500, 96, 24, 64, 4
    rng = np.random.default_rng(5600)
    inputs = []
    for _ in range(2):
        boxes = np.stack([ir.clustered(rng, B, 10) for _ in range(F)]).astype(np.float32)
        scores = rng.uniform(0.05, 1.0, (F, B)).astype(np.float32)
        frames = []
        for f in range(F):
            at = boxes[f, rng.integers(0, B, n), :3]
            frames.append(np.column_stack((at + rng.normal(0, 1.5, (n, 3)) * np.array([1, 1, 0.4]), rng.integers(1, 255, n), rng.integers(0, 64, n))))
        inputs.append((boxes, scores, np.concatenate(frames).astype(np.float32), rng.uniform(0, 1, F * n) < 0.8))
    offsets = np.arange(F + 1, dtype=np.int64) * n
    boxes, scores, cloud, keep = (_t(x) for x in inputs[0])
    rows = DeviceBatch(cloud, offsets)
    pose = _t(ir.numpy_pose(inputs[0][0]))
    seg = _t(np.linspace(0.0, 1.0, F * n).astype(np.float32))              # a per-row score, the same for both inputs
    nb_out = NmsBatch.empty(F, B, P, 8, torch.float32)
    rp_out = RoiPointBatch.empty(F, P, S, C, torch.float32, with_local=True, with_pose=True)
    s = torch.cuda.Stream()

    def chain():
        nb = nms(boxes, scores, 0.45, post_max=P, score_thresh=0.1, pose=pose, out=nb_out)
        rp = _pool(rows, nb, S, extra_width=(0.2, 0.2, 0.2), keep=keep, num_features=C, out=rp_out, return_local=True, return_pose=True)
        return nb, rp, rp.gather(seg)

    with torch.cuda.stream(s):
        chain()                                                            # warm-up: the captured calls allocate nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = chain()
        assert got[0] is nb_out and got[1] is rp_out
        outputs = [nb_out.index, nb_out.count, nb_out.boxes] + [getattr(rp_out, f) for f in FIELDS] + [got[2]]
        snaps = []
        for k in (1, 0):
            for dst, src in zip((boxes, scores, cloud, keep), inputs[k]):
                dst.copy_(_t(src))
            pose.copy_(_t(ir.numpy_pose(inputs[k][0])))
            for t in outputs:
                t.view(torch.uint8).fill_(0x7f)
            g.replay()
            snaps.append((k, [t.clone() for t in outputs]))
        s.synchronize()
    names = ("nms_index", "nms_count", "nms_boxes") + FIELDS + ("gathered",)
    counts = []
    for k, snap in snaps:
        got = dict(zip(names, (t.cpu().numpy() for t in snap)))
        b, sc, cl, kp = inputs[k]
        want = ir.nms(b, sc, ir.numpy_pose(b), 0.45, P, 0.1, "bev")
        counts.append(want["count"].tolist())
        assert (want["count"] > 2).all() and (want["count"] < P).any()
        for f in ("index", "count", "boxes"):
            assert got["nms_" + f].tobytes() == want[f].tobytes(), (k, f)
        used = got["pose"]
        assert np.array_equal(used.any(axis=-1), ir.present(want["boxes"], ir.numpy_pose(want["boxes"])))
        rp = rr.roi_point_pool(cl, want["boxes"], used, S, C, (0.2, 0.2, 0.2), kp, offsets)
        assert (rp["count"] > S).any() and ((rp["count"] > 0) & (rp["count"] < S)).any() and (rp["count"] == 0).any()
        for f in FIELDS:
            assert got[f].tobytes() == rp[f].tobytes(), (k, f)
        score = np.linspace(0.0, 1.0, F * n).astype(np.float32)
        assert got["gathered"].tobytes() == np.where(rp["index"] >= 0, score[np.maximum(rp["index"], 0)], np.float32(0)).tobytes(), k
    assert counts[0] != counts[1]


def test_gather_and_labels():
    from lidar_snow_sim_amd.tensors import points_in_boxes
    c, e = rr.case("seams", "float32"), rr.expected("seams", "float32")
    got = _run(c)
    feats = np.arange(len(c["rows"]) * 3, dtype=np.float32).reshape(-1, 3)
    wide = got.gather(_t(feats)).cpu().numpy()
    assert wide.shape == e["index"].shape + (3,) and np.array_equal(wide, np.where((e["index"] >= 0)[..., None], feats[np.maximum(e["index"], 0)], 0))
    lab = points_in_boxes(_batch(c), _t(c["rois"]), pose=_t(c["pose"]))
    box_of = lab.box_of.cpu().numpy()
    assert np.array_equal(got.labels(lab).cpu().numpy(), np.where(e["index"] >= 0, box_of[np.maximum(e["index"], 0)], -1))
    with pytest.raises(ValueError, match="gather: per_row must be"):
        got.gather(feats)
    with pytest.raises(ValueError, match="labels: box_labels must be a BoxLabelBatch"):
        got.labels(lab.box_of)


# ---- 5. the NumPy entry -------------------------------------------------------------------------------------------------------------------------
def test_numpy_entry():
    from lidar_snow_sim_amd.roipool import roipoint_pool3d
    for dtype in DTYPES:
        c = rr.case("seams", dtype)
        a, b = (int(v) for v in c["offsets"][3:5])
        want = rr.roi_point_pool(c["rows"][a:b], c["rois"][3:4], c["pose"][3:4], 100, 5, (0.5, 0.5, 0.5))
        pooled, empty = roipoint_pool3d(c["rows"][a:b], c["rois"][3], 100, 0.5)
        assert pooled.dtype == c["rows"].dtype and pooled.tobytes() == want["points"][0].tobytes()
        assert empty.dtype == np.int32 and np.array_equal(empty, (want["count"][0] == 0).astype(np.int32))
    with pytest.raises(ValueError, match="pc must be N x M"):
        roipoint_pool3d(c["rows"][:, :2], c["rois"][0])
    with pytest.raises(ValueError, match="boxes must be M x 7 .. 10"):
        roipoint_pool3d(c["rows"], c["rois"][0][:, :6])


# ---- 6. what the wrapper refuses, in words -----------------------------------------------------------------------------------------------------
def _pin(dtype=torch.float32, rows=8, M=2, features=7, **kw):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return dict(frames=DeviceBatch(torch.zeros((rows, 5), dtype=dtype).cuda(), np.array([0, rows // 2, rows])),
                rois=torch.zeros((2, M, features), dtype=dtype).cuda(), n_samples=4, **kw)


def _out(**kw):
    from lidar_snow_sim_amd.tensors import RoiPointBatch
    return RoiPointBatch.empty(2, 2, 4, 4, **kw)


ROI_WORDS = "roi_point_pool: rois must be a contiguous (frames, M, 7 .. 10) tensor in the rows' dtype on their device, or an NmsBatch of such boxes"
EW_WORDS = "roi_point_pool: extra_width is a number or three (x, y, z), each finite and in 0 .. 100"
OUT_WORDS = "roi_point_pool: out must be a RoiPointBatch whose %s tensor on the device of the rows"
REFUSALS = [
    ("host rows", lambda: dict(_pin(), frames=np.zeros((8, 5), np.float32)),
     "roi_point_pool: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.roipool.roipoint_pool3d)"),
    ("rois of another dtype", lambda: dict(_pin(), rois=torch.zeros((2, 2, 7), dtype=torch.float64).cuda()), ROI_WORDS),
    ("rois on the host", lambda: dict(_pin(), rois=torch.zeros((2, 2, 7))), ROI_WORDS),
    ("rois not contiguous", lambda: dict(_pin(), rois=torch.zeros((2, 2, 14)).cuda()[:, :, ::2]), ROI_WORDS),
    ("rois of another frame count", lambda: dict(_pin(), rois=torch.zeros((3, 2, 7)).cuda()), ROI_WORDS),
    ("no roi", lambda: _pin(M=0), "roi_point_pool: n_rois must lie in 1 .. 512 (rois)"),
    ("513 rois", lambda: _pin(M=513), "roi_point_pool: n_rois must lie in 1 .. 512 (rois)"),
    ("rois of 6 columns", lambda: _pin(features=6), "roi_point_pool: roi_features must lie in 7 .. 10: cx, cy, cz, dx, dy, dz, heading first (rois)"),
    ("no sample", lambda: dict(_pin(), n_samples=0), "roi_point_pool: n_samples must lie in 1 .. 2048"),
    ("2049 samples", lambda: dict(_pin(), n_samples=2049), "roi_point_pool: n_samples must lie in 1 .. 2048"),
    ("half a sample", lambda: dict(_pin(), n_samples=2.5), "roi_point_pool: n_samples must be an integer"),
    ("6 features", lambda: _pin(num_features=6), "roi_point_pool: num_features must be 3, 4 or 5: the columns of a row that a roi stores"),
    ("a negative extra width", lambda: _pin(extra_width=-0.1), EW_WORDS),
    ("a negative component", lambda: _pin(extra_width=(0.1, -0.1, 0.0)), EW_WORDS),
    ("an extra width above 100", lambda: _pin(extra_width=(0.0, 0.0, 101.0)), EW_WORDS),
    ("an extra width of NaN", lambda: _pin(extra_width=float("nan")), EW_WORDS),
    ("two extra widths", lambda: _pin(extra_width=(0.1, 0.2)), EW_WORDS),
    ("a pose of another shape", lambda: _pin(pose=torch.zeros((2, 3, 2), dtype=torch.float64).cuda()),
     "roi_point_pool: pose must be a contiguous (2, 2, 2) float64 tensor (cos, sin) on the device of the rows"),
    ("out of another kind", lambda: _pin(out=torch.zeros(4).cuda()), OUT_WORDS % "index is a contiguous (2, 2, 4) torch.int32"),
    ("out of another sample count", lambda: dict(_pin(), n_samples=5, out=_out()), OUT_WORDS % "index is a contiguous (2, 2, 5) torch.int32"),
    ("out of another feature count", lambda: _pin(num_features=5, out=_out()), OUT_WORDS % "points is a contiguous (2, 2, 4, 5) torch.float32"),
    ("out without local", lambda: _pin(out=_out(), return_local=True), OUT_WORDS % "local is a contiguous (2, 2, 4, 3) torch.float32"),
    ("out of another dtype", lambda: _pin(out=_out(dtype=torch.float64)), OUT_WORDS % "points is a contiguous (2, 2, 4, 4) torch.float32"),
    ("out without pose", lambda: _pin(out=_out(), return_pose=True), OUT_WORDS % "pose is a contiguous (2, 2, 2) torch.float64"),
]


@pytest.mark.parametrize("what, make, words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_python_refusals(what, make, words):
    args = make()
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        _pool(args.pop("frames"), args.pop("rois"), args.pop("n_samples"), **args)


def test_the_entry_refuses_in_its_own_words():
    """Through the binding, past the wrapper: an output that overlaps the rois."""
    from lidar_snow_sim_amd import engine
    rows, rois = torch.zeros((8, 5)).cuda(), torch.zeros((2, 64, 8)).cuda()
    off = torch.tensor([0, 4, 8], dtype=torch.int64).cuda()
    count = torch.zeros((2, 64), dtype=torch.int32).cuda()
    ctx = engine.get_engine(torch.cuda.current_device(), 0).ctx
    with pytest.raises(ValueError, match="^snowgpu_roi_point_pool_device: d_out_index overlaps d_rois; the mask, the rows, the rois and the pose are read"):
        ctx.roi_point_pool_device(2, 8, 4, off.data_ptr(), rows.data_ptr(), 0, 64, rois.data_ptr(), 8, None, 2, 4, 0, 0, rois.data_ptr(), count.data_ptr(), 0, 0, 0)
    with pytest.raises(ValueError, match="^snowgpu_roi_point_pool_device: every component of extra_width must be finite and lie in 0 .. 100$"):
        ctx.roi_point_pool_device(2, 8, 4, off.data_ptr(), rows.data_ptr(), 0, 64, rois.data_ptr(), 8, (0.0, 200.0, 0.0), 2, 4, 0, 0, rois.data_ptr(),
                                  count.data_ptr(), 0, 0, 0)
