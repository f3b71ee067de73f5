"""-m gpu: the nearest centres of every row on the device (tensors.nearest_keypoints, nearest.three_nn, snowgpu_nearest_centres_device;
csrc/snowgpu_nn.hip, csrc/sg_nn.h) against the brute-force NumPy restatement of its definition (tests/nn_reference.py, whose inputs
tests/test_nn_reference.py holds to the conditions that keep these comparisons from being vacuous).  Indices are integers, distances are
separately rounded operations that the restatement makes in the same order, and the weights are correctly rounded float64 operations in
the definition's order: every comparison is equality of bytes, for both dtypes."""
import re

import numpy as np
import pytest
import torch

import nn_reference as nr

pytestmark = pytest.mark.gpu

DTYPES = nr.DTYPES
FIELDS = ("index", "dist2", "weight")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _frames(rows, offsets):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(rows), offsets)


def _nn(*args, **kw):
    from lidar_snow_sim_amd.tensors import nearest_keypoints
    return nearest_keypoints(*args, **kw)


def _run_case(name, dtype, k=3, **kw):
    rows, offsets, keep, centres, rng = nr.case(name, dtype)
    return _nn(_frames(rows, offsets), _t(centres), k, point_cloud_range=rng, keep=None if keep is None else _t(keep), **kw)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


# ---- 1. the shared inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", nr.CASES)
def test_shared_inputs_equal_the_restatement(name, dtype):
    got = _run_case(name, dtype)
    _same(got, nr.expected(name, dtype, 3), (name, dtype))
    assert got.n_centres == nr.case(name, dtype)[3].shape[1]


# ---- 2. every k -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", range(1, nr.MAX_K + 1))
def test_every_k(k, dtype):
    for name in ("constructed", "batch"):
        _same(_run_case(name, dtype, k), nr.expected(name, dtype, k), (name, k, dtype))


# ---- 3. the number of centres -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_centres", nr.SIZES)
def test_number_of_centres(n_centres, dtype):
    """K = 1, 2, 3 (fewer centres than slots, and exactly as many), 64, and 4096: the largest grid."""
    name = f"sized{n_centres}"
    want = nr.expected(name, dtype, 3)
    _same(_run_case(name, dtype), want, (n_centres, dtype))
    assert ((want["index"] >= 0).sum(axis=1) == min(3, n_centres)).all()
    assert nr.grid(nr.RANGE, n_centres)["budget"] == (nr.MAX_CELLS if n_centres == 4096 else max(nr.MIN_CELLS, n_centres // 2))


# ---- 4. the columns of the centres ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_centre_features(dtype):
    rows, offsets, _, centres, rng = nr.case("batch", dtype)         # centres of 4 columns; now of 3 and of 5
    want = nr.expected("batch", dtype, 3)
    for cq in (3, 5):
        cen = np.ascontiguousarray(np.concatenate((centres, np.full(centres.shape[:2] + (1,), np.nan, centres.dtype)), axis=2)[:, :, :cq])
        _same(_nn(_frames(rows, offsets), _t(cen), 3, point_cloud_range=rng), want, (dtype, cq))


# ---- 5. the chain behind the keypoints ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    return np.ascontiguousarray(synthetic_sweep(64, 320, seed=1700, intensity="lambert"))


@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_synthetic_sweep_and_its_keypoints(sweep, dtype, masked):
    from lidar_snow_sim_amd.tensors import sample_keypoints
    rows = np.ascontiguousarray(sweep.astype(dtype))
    keep = np.random.default_rng(5).random(len(rows)) < 0.6 if masked else None
    d_rows, d_keep = _t(rows), None if keep is None else _t(keep)
    kp = sample_keypoints(d_rows, 256, point_cloud_range=nr.SECOND_RANGE, keep=d_keep)
    got = _nn(d_rows, kp, 3, point_cloud_range=nr.SECOND_RANGE, keep=d_keep)
    points, picked = kp.points.cpu().numpy(), kp.index[0].cpu().numpy().astype(np.int64)
    want = nr.nearest(rows, points, 3, nr.SECOND_RANGE, keep)         # (in blocks of rows)
    assert 15000 < len(rows) < 25000 and (want["index"][:, 0] >= 0).sum() > 3000 and (want["index"][:, 0] < 0).sum() > 1000
    _same(got, want, (dtype, masked))
    # every sampled row finds itself: distance 0, and the first keypoint at its position
    index, dist2 = got.index.cpu().numpy(), got.dist2.cpu().numpy()
    assert len(set(picked.tolist())) == 256 and (dist2[picked, 0] == 0).all()
    first_at = {}
    for j, p in enumerate(points[0, :, :3]):
        first_at.setdefault(p.tobytes(), j)
    assert [int(v) for v in index[picked, 0]] == [first_at[rows[i, :3].tobytes()] for i in picked]
    if masked:
        assert keep[picked].all() and (index[~keep] == -1).all()


# ---- 6. the way back --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_interpolate_and_nearest(dtype):
    rows, offsets, _, centres, rng = nr.case("batch", dtype)
    got = _run_case("batch", dtype)
    want = nr.expected("batch", dtype, 3)
    F, K = centres.shape[:2]
    frame = np.repeat(np.arange(F), np.diff(offsets))
    flat = np.where(want["index"] >= 0, want["index"] + frame[:, None] * K, -1)
    assert np.array_equal(got.flat_index().cpu().numpy(), flat)
    # the keypoints' own coordinates, interpolated: a row that is a keypoint comes back, to the weight's rounding.  Its own slot has
    # u = 1e8, so another slot at distance s weighs at most 1e-8 / s and moves the sum by at most 1e-8 m; the products and sums of the
    # gather are made in the rows' dtype on coordinates below 40 m: 3 * 2 * 40 * 2^-24 = 1.4e-5 m in float32.
    d_cen = _t(centres)
    back = got.interpolate(d_cen[:, :, :3].contiguous()).cpu().numpy()
    on = np.flatnonzero(want["dist2"][:, 0] == 0)
    assert len(on) >= 19 and back.shape == (len(rows), 3) and back.dtype == rows.dtype
    assert np.abs(back[on].astype(np.float64) - rows[on, :3]).max() < (2e-5 if dtype == "float32" else 1e-7)
    gathered = centres.reshape(F * K, -1)[np.maximum(flat, 0), :3].astype(np.float64)
    every = (gathered * want["weight"].astype(np.float64)[:, :, None]).sum(axis=1)
    assert np.abs(back - every).max() < (2e-5 if dtype == "float32" else 1e-12)
    one = got.interpolate(d_cen[:, :, 3].contiguous())                  # (F, K) values
    assert one.shape == (len(rows),) and torch.equal(one, got.interpolate(d_cen[:, :, 3:4].contiguous())[:, 0])
    # Voronoi labelling: a per-keypoint decision becomes a per-row mask
    decision = torch.from_numpy(np.random.default_rng(9).random((F, K)) < 0.5).cuda()
    mask = got.nearest(decision, default=False)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), decision.cpu().numpy().reshape(-1)[flat[:, 0]])
    ids = got.nearest(torch.arange(F * K, device="cuda").reshape(F, K, 1), default=-7)
    assert np.array_equal(ids.cpu().numpy()[:, 0], flat[:, 0])
    none = _run_case("constructed", dtype)
    labels = none.nearest(torch.ones((11, nr.CONSTRUCTED_K), device="cuda"), default=-7).cpu().numpy()
    assert np.array_equal(labels == -7, nr.expected("constructed", dtype, 3)["index"][:, 0] < 0) and (labels == -7).sum() > 60
    assert not none.interpolate(torch.ones((11, nr.CONSTRUCTED_K), device="cuda", dtype=getattr(torch, dtype)))[labels == -7].any()
    with pytest.raises(ValueError, match="values must be a"):
        got.nearest(decision[:, :5])


# ---- 7. buffers, runs and graphs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written_in_place(dtype):
    from lidar_snow_sim_amd.tensors import NearestBatch
    for name in ("constructed", "beyond"):
        _, offsets, _, centres, _ = nr.case(name, dtype)
        out = NearestBatch.empty(offsets, centres.shape[1], 3, getattr(torch, dtype))
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        got = _run_case(name, dtype, out=out)
        assert got is out
        _same(out, nr.expected(name, dtype, 3), (name, dtype))
    bare = _run_case("batch", dtype, return_weights=False)
    assert bare.weight is None
    _same(bare, nr.expected("batch", dtype, 3), dtype, FIELDS[:2])
    none = _nn(_t(np.zeros((0, 5), dtype)), _t(np.zeros((1, 5, 3), dtype)), 3)          # a batch without a row
    assert tuple(none.index.shape) == (0, 3) and tuple(none.weight.shape) == (0, 3)


def test_two_calls_give_identical_bytes():
    for name in ("constructed", "cluster", "batch"):
        a, b = _run_case(name, "float32", 8), _run_case(name, "float32", 8)
        for f in FIELDS:
            assert getattr(a, f).data_ptr() != getattr(b, f).data_ptr() and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), (name, f)


def test_graph_capture():
    """One capture after a warm-up, replayed three times on changed rows and centres in the same tensors: the scratch and every output are
    rewritten by the captured sequence itself.  A linear graph."""
    from lidar_snow_sim_amd.tensors import NearestBatch
    n, K = 3000, 64
    inputs = [(r, np.ascontiguousarray(c[:, :K])) for r, c in (nr.sized_case(K + extra, "float32", n) for extra in (0, 1))]      # two draws
    want = [nr.nearest(r, c, 3, nr.RANGE) for r, c in inputs]
    assert not np.array_equal(want[0]["index"], want[1]["index"])
    s = torch.cuda.Stream()
    rows, cen = _t(inputs[0][0]), _t(inputs[0][1])
    out = NearestBatch.empty(n, K, 3, torch.float32)
    with torch.cuda.stream(s):
        _nn(rows, cen, 3, point_cloud_range=nr.RANGE, out=out)            # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = _nn(rows, cen, 3, point_cloud_range=nr.RANGE, out=out)
        assert got is out
        snaps = []
        for k in (1, 0, 1):
            rows.copy_(_t(inputs[k][0]))
            cen.copy_(_t(inputs[k][1]))
            for f in FIELDS:
                getattr(out, f).view(torch.uint8).fill_(0x7f)
            g.replay()
            snaps.append((k, {f: getattr(out, f).clone() for f in FIELDS}))
        s.synchronize()
    for k, snap in snaps:
        for f in FIELDS:
            assert snap[f].cpu().numpy().tobytes() == want[k][f].tobytes(), (k, f)


# ---- 8. the NumPy entry -----------------------------------------------------------------------------------------------------------------------
def test_numpy_entry():
    from lidar_snow_sim_amd.nearest import three_nn
    for dtype in DTYPES:
        rows, _, _, centres, rng = nr.case("corner", dtype)
        want = nr.expected("corner", dtype, 3)
        for cols in (5, 3):
            dist2, index, weight = three_nn(rows[:, :cols], centres[0], point_cloud_range=rng)
            assert index.dtype == np.int32 and dist2.dtype == rows.dtype and weight.dtype == rows.dtype
            assert np.array_equal(index, want["index"]) and dist2.tobytes() == want["dist2"].tobytes() and weight.tobytes() == want["weight"].tobytes()
        dist2, index = three_nn(rows, centres[0], 1, rng, return_weights=False)
        assert np.array_equal(index, nr.expected("corner", dtype, 1)["index"]) and dist2.shape == (len(rows), 1)
    with pytest.raises(ValueError):
        three_nn(rows[:, :2], centres[0])
    with pytest.raises(ValueError):
        three_nn(rows, centres[0][:, :2])


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import NearestBatch
    rows, offsets, keep, centres, rng = nr.case("batch")
    pc, cen, n = _frames(rows, offsets), _t(centres), len(rows)
    wide = _t(np.concatenate((centres, centres), axis=2))
    for kw, words in ((dict(k=0), "k must lie in 1 .. 8"), (dict(k=9), "k must lie in 1 .. 8"), (dict(k=2.5), "k must be an integer"),
                      (dict(centres=cen.double()), "centres must be a KeypointBatch or a contiguous"),
                      (dict(centres=cen.cpu()), "centres must be a KeypointBatch or a contiguous"),
                      (dict(centres=cen[0]), "centres must be a KeypointBatch or a contiguous"),
                      (dict(centres=cen[:4]), "centres must be a KeypointBatch or a contiguous"),
                      (dict(centres=wide[:, :, :4]), "centres must be a KeypointBatch or a contiguous"),          # not contiguous
                      (dict(centres=cen[:, :, :2].contiguous()), "centre_features must be 3, 4 or 5.*centres"),
                      (dict(centres=wide[:, :, :6].contiguous()), "centre_features must be 3, 4 or 5.*centres"),
                      (dict(centres=cen[:, :0].contiguous()), "n_centres must be at least 1.*centres"),
                      (dict(point_cloud_range=(0, 0, float("nan"), 1, 1, 1)), "snowgpu_nearest_centres_device: a bound of the range is NaN"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 0, 1)), "snowgpu_nearest_centres_device: the range needs lo < hi on every axis"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 1)), "point_cloud_range holds 6 numbers")):
        args = dict(centres=cen, k=3, point_cloud_range=rng)
        args.update(kw)
        with pytest.raises(ValueError, match=words.replace("..", r"\.\.")):
            _nn(pc, args.pop("centres"), args.pop("k"), **args)
    with pytest.raises(ValueError, match="torch CUDA tensors"):
        _nn(rows, cen, 3)
    with pytest.raises(ValueError):
        _nn(pc, cen, 3, keep=torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError, match="out must be a NearestBatch whose index"):
        _nn(pc, cen, 3, out=NearestBatch.empty(offsets, 64, 4))
    with pytest.raises(ValueError, match="out must be a NearestBatch whose index"):
        _nn(pc, cen, 3, out=NearestBatch.empty(n - 1, 64, 3))
    with pytest.raises(ValueError, match="out must be a NearestBatch whose dist2"):
        _nn(pc, cen, 3, out=NearestBatch.empty(offsets, 64, 3, torch.float64))
    with pytest.raises(ValueError, match="out must be a NearestBatch whose weight"):
        _nn(pc, cen, 3, out=NearestBatch.empty(offsets, 64, 3, with_weights=False))
    # the C entry refuses on its own: the overlaps, and a null output; the nullable output may be null
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    arena = torch.zeros(cen.numel() + 3 * n, device="cuda:0")         # the centres with 12 n bytes of their own allocation behind them: a d_out_weight put
    cen = arena[:cen.numel()].view(cen.shape).copy_(cen)              # on their last value reaches no other tensor, wherever the allocator placed the rest
    d_rows, off = _t(rows), _t(offsets)
    out = NearestBatch.empty(offsets, 64, 3)
    mask = torch.ones(n + 65536, dtype=torch.uint8, device="cuda:0")
    args = (len(offsets) - 1, n, int(np.diff(offsets).max()), off.data_ptr(), d_rows.data_ptr(), 0, rng, 64, cen.data_ptr(), 4, 3)
    with pytest.raises(ValueError, match="d_out_index overlaps d_keep_in"):
        ctx.nearest_centres_device(*args, mask.data_ptr(), mask.data_ptr() + 8, out.dist2.data_ptr(), out.weight.data_ptr())
    with pytest.raises(ValueError, match="d_out_dist2 overlaps d_rows"):
        ctx.nearest_centres_device(*args, 0, out.index.data_ptr(), d_rows.data_ptr(), out.weight.data_ptr())
    with pytest.raises(ValueError, match="d_out_weight overlaps d_centres"):
        ctx.nearest_centres_device(*args, 0, out.index.data_ptr(), out.dist2.data_ptr(), cen.data_ptr() + 4 * (5 * 64 * 4 - 1))
    with pytest.raises(ValueError, match="d_out_weight overlaps d_out_dist2; every output needs memory of its own"):
        ctx.nearest_centres_device(*args, 0, out.index.data_ptr(), out.dist2.data_ptr(), out.dist2.data_ptr())
    with pytest.raises(ValueError, match="null pointer or bad dtype"):
        ctx.nearest_centres_device(*args, 0, 0, out.dist2.data_ptr(), out.weight.data_ptr())
    with pytest.raises(ValueError, match="k must lie in 1 .. 8".replace("..", r"\.\.")):
        ctx.nearest_centres_device(*args[:-1], 9, 0, out.index.data_ptr(), out.dist2.data_ptr(), 0)
    want = nr.expected("batch", "float32", 3)
    out.index.fill_(9)
    ctx.nearest_centres_device(*args, 0, out.index.data_ptr(), out.dist2.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(out.index.cpu().numpy(), want["index"]) and out.dist2.cpu().numpy().tobytes() == want["dist2"].tobytes()


# ---- every refusal of the Python boundary word for word, and which of two faults is reported -----------------------------------------------------
# (the one refusal left out, n_frames * n_centres beyond 2^31 - 1, needs centres of 24 GiB)
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _centres(n=8, features=3, dtype=torch.float32):
    return torch.empty((2, n, features), dtype=dtype, device="cuda:0")


def _nearest_out(*args, **kw):
    from lidar_snow_sim_amd.tensors import NearestBatch
    return NearestBatch.empty(np.array([0, 64, 128]), 8, *args, **kw)


HOST_WORDS = "nearest_keypoints: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.nearest.three_nn)"
CENTRE_WORDS = "nearest_keypoints: centres must be a KeypointBatch or a contiguous (frames, K, 3 .. 5) tensor in the rows' dtype on their device"
KEEP_WORDS = "keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)"
OUT_WORDS = "nearest_keypoints: out must be a NearestBatch whose %s tensor on the device of the rows"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)), HOST_WORDS),
    ("k 2.5", lambda: dict(k=2.5), "nearest_keypoints: k must be an integer"),
    ("k True", lambda: dict(k=True), "nearest_keypoints: k must be an integer"),
    ("k 9", lambda: dict(k=9), "nearest_keypoints: k must lie in 1 .. 8"),
    ("range of 5", lambda: dict(point_cloud_range=(0, 0, 0, 4, 4)), "nearest_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)"),
    ("centres of another dtype", lambda: dict(centres=_centres(dtype=torch.float64)), CENTRE_WORDS),
    ("centres of 6 columns", lambda: dict(centres=_centres(features=6)), "nearest_keypoints: centre_features must be 3, 4 or 5: x, y, z first (centres)"),
    ("no centre", lambda: dict(centres=_centres(0)), "nearest_keypoints: n_centres must be at least 1 (centres)"),
    ("out of another k", lambda: dict(out=_nearest_out(2)), OUT_WORDS % "index is a contiguous (128, 3) torch.int32"),
    ("out of another kind", lambda: dict(out=object()), OUT_WORDS % "index is a contiguous (128, 3) torch.int32"),
    ("out of another dtype", lambda: dict(out=_nearest_out(3, torch.float64)), OUT_WORDS % "dist2 is a contiguous (128, 3) torch.float32"),
    ("out without weights", lambda: dict(out=_nearest_out(3, with_weights=False)), OUT_WORDS % "weight is a contiguous (128, 3) torch.float32"),
    # two faults: the earlier step of the call reports
    ("host rows before k", lambda: dict(frames=np.zeros((4, 5), np.float32), k=2.5), HOST_WORDS),
    ("k before the range", lambda: dict(k=9, point_cloud_range=(0, 0, 0, 4, 4)), "nearest_keypoints: k must lie in 1 .. 8"),
    ("the range before the device", lambda: dict(point_cloud_range=(0, 0, 0, 4, 4), device=1), "nearest_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)"),
    ("the device before the centres", lambda: dict(device=1, centres=_centres(dtype=torch.float64)), "the tensors live on cuda:0, device=1 was asked for"),
    ("keep before the centres", lambda: dict(keep=torch.ones(127, dtype=torch.bool, device="cuda:0"), centres=_centres(dtype=torch.float64)), KEEP_WORDS),
    ("the centres before out", lambda: dict(centres=_centres(features=6), out=object()), "nearest_keypoints: centre_features must be 3, 4 or 5: x, y, z first (centres)"),
    ("k before out", lambda: dict(k=2.5, out=object()), "nearest_keypoints: k must be an integer"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    from lidar_snow_sim_amd.tensors import nearest_keypoints
    args = dict(frames=_pin_batch(), centres=_centres(), k=3)
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        nearest_keypoints(**args)


def test_the_wrapper_refuses_a_short_range_word_for_word():
    from lidar_snow_sim_amd import engine
    with pytest.raises(ValueError, match="^" + re.escape("snowgpu_nearest_centres_device: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)") + "$"):
        engine.get_engine(0).ctx.nearest_centres_device(2, 128, 64, 0, 0, 0, (0, 0, 0, 4, 4), 8, 0, 3, 3, 0, 0, 0, 0)
