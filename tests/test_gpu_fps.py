"""-m gpu: farthest point sampling on the device (tensors.sample_keypoints, fps.farthest_point_sample, snowgpu_fps_device;
csrc/snowgpu_fps.hip, csrc/sg_fps.h) against the sequential NumPy restatement of its definition (tests/fps_reference.py, whose inputs
tests/test_fps_reference.py holds to the conditions that keep these comparisons from being vacuous).  The outputs are integers, copied
bits and separately rounded sums that the restatement makes in the same order: every comparison is equality."""
import re

import numpy as np
import pytest
import torch

import fps_reference as fr
from lidar_snow_sim_amd.fps import TIER_ROWS

pytestmark = pytest.mark.gpu

DTYPES = fr.DTYPES
FIELDS = ("index", "points", "dist", "usable")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _frames(rows, offsets):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(rows), offsets)


def _sample(*args, **kw):
    from lidar_snow_sim_amd.tensors import sample_keypoints
    return sample_keypoints(*args, **kw)


def _run_case(name, dtype, num_features=4, n_samples=None, **kw):
    rows, offsets, keep, (rng, K) = fr.case(name, dtype)
    return _sample(_frames(rows, offsets), K if n_samples is None else n_samples, point_cloud_range=rng, keep=None if keep is None else _t(keep),
                   num_features=num_features, return_dist=True, **kw)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():      # (bytes: NaN columns and -0.0 are copied as they are)
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


def _one_cloud(n_rows, dtype, K):
    return _sample(_t(fr.cloud_case(n_rows, dtype)), K, point_cloud_range=fr.RANGE, return_dist=True)


# ---- 1. equality against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", fr.CASES)
def test_shared_inputs_equal_the_restatement(name, dtype):
    _same(_run_case(name, dtype), fr.expected(name, dtype), (name, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", (1, 36, 37, 38))
def test_samples_around_the_usable_rows(K, dtype):
    """K = 1, m - 1, m, m + 1 for the frame of m = 37 usable rows."""
    _same(_run_case("fewer37", dtype, n_samples=K), fr.expected("fewer37", dtype, n_samples=K), (K, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_4096_samples_of_5000_rows(dtype):
    _same(_one_cloud(5000, dtype, 4096), fr.cloud_expected(5000, dtype, 4096), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_features", (3, 5))
def test_number_of_features(num_features, dtype):
    for name in ("constructed", "batch"):
        _same(_run_case(name, dtype, num_features=num_features), fr.expected(name, dtype, num_features=num_features), (name, dtype, num_features))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("delta", (-1, 0, 1))
@pytest.mark.parametrize("c", sorted({c for tiers in TIER_ROWS.values() for c in tiers}))
def test_tier_edges(c, delta, dtype):
    """One-frame clouds of c - 1, c and c + 1 usable rows for every capacity c at which the kernel of either dtype takes another path."""
    assert c in TIER_ROWS["float32"] or c in TIER_ROWS["float64"]
    _same(_one_cloud(c + delta, dtype, 96), fr.cloud_expected(c + delta, dtype, 96), (c, delta, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_streamed_frame(dtype):
    """40 000 usable rows: beyond every tier, x, y, z and t stream from scratch."""
    assert 40000 > max(TIER_ROWS[dtype]) + 4
    _same(_one_cloud(40000, dtype, 256), fr.cloud_expected(40000, dtype, 256), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frame_of_the_lds_tier(dtype):
    """Between the register tiers and the streamed path: the running minima in LDS, many steps per lane."""
    n = TIER_ROWS[dtype][2] - 1001
    assert n > TIER_ROWS[dtype][1] + 4096
    _same(_one_cloud(n, dtype, 256), fr.cloud_expected(n, dtype, 256), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_tiers_mixed_in_one_call(dtype):
    """A frame of the first register tier, a streamed frame, an empty frame, a frame of the second register tier and one of the LDS tier
    in one batch."""
    t0, t1, t2 = TIER_ROWS[dtype]
    sizes = (t0 - 700, t2 + 900, 0, t1 - 300, t1 + 500)
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    rows = fr.cloud_case(int(offsets[-1]), dtype, 9)
    want = fr.fps(rows, 64, fr.RANGE, 4, None, offsets)
    assert want["usable"].tolist() == list(sizes)
    _same(_sample(_frames(rows, offsets), 64, point_cloud_range=fr.RANGE, return_dist=True), want, dtype)


# ---- 2. every element is written --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written(dtype):
    from lidar_snow_sim_amd.tensors import KeypointBatch
    for name in ("batch", "fewer37", "fewer0"):
        _, offsets, _, (_, K) = fr.case(name, dtype)
        out = KeypointBatch.empty(len(offsets) - 1, K, 4, getattr(torch, dtype), with_dist=True)
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        got = _run_case(name, dtype, out=out)
        assert got is out
        _same(out, fr.expected(name, dtype), (name, dtype))


# ---- 3. the input mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_keep_equals_the_compacted_frames(dtype):
    rows, offsets, keep, (rng, K) = fr.case("batch", dtype)
    masked = _run_case("batch", dtype)
    parts = [_t(rows[a:b][keep[a:b]]) for a, b in zip(offsets[:-1], offsets[1:])]
    compact = _sample(parts, K, point_cloud_range=rng, return_dist=True)
    for f in FIELDS[1:]:
        assert torch.equal(getattr(masked, f).view(torch.uint8), getattr(compact, f).view(torch.uint8)), f
    back = np.flatnonzero(keep)                                          # compacted row -> row of the batch
    ci = compact.index.cpu().numpy()
    assert np.array_equal(masked.index.cpu().numpy(), np.where(ci >= 0, back[np.maximum(ci, 0)], -1)) and (ci[0] >= 0).all()
    # the mask as uint8, as a list per frame, and on an F x N x 5 tensor whose padding is NaN
    m8 = _sample(_frames(rows, offsets), K, point_cloud_range=rng, keep=_t(keep.astype(np.uint8)), return_dist=True)
    ml = _sample(_frames(rows, offsets), K, point_cloud_range=rng, keep=[_t(keep[a:b]) for a, b in zip(offsets[:-1], offsets[1:])], return_dist=True)
    for other in (m8, ml):
        assert all(torch.equal(getattr(masked, f).view(torch.uint8), getattr(other, f).view(torch.uint8)) for f in FIELDS)
    sizes = (1000, 1500, 37)
    batch = np.full((3, 1500, 5), np.nan, rows.dtype)
    for f, n in enumerate(sizes):
        batch[f, :n] = rows[f * 13:f * 13 + n]
    pad = np.arange(1500)[None, :] < np.array(sizes)[:, None]
    want = fr.fps(batch.reshape(-1, 5), K, rng, 4, pad.reshape(-1), np.arange(4) * 1500)
    assert want["usable"].tolist() == list(sizes)
    _same(_sample(_t(batch), K, point_cloud_range=rng, keep=_t(pad), return_dist=True), want, "padded")
    _same(_sample(_t(batch), K, point_cloud_range=rng, return_dist=True), want, "padded, no mask")      # NaN rows are unusable anyway


# ---- 4. the chain -----------------------------------------------------------------------------------------------------------------------------
def test_chain_behind_the_aligned_snowfall(tables):
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import augment_batch
    tl = [tables["t"][i % 4] for i in range(64)]
    plane, bd = (np.array([0.0, 0.0, -1.0]), -1.7), float(np.degrees(3e-3))
    frames = [np.ascontiguousarray(synthetic_sweep(64, 128, seed=1600 + k, intensity="lambert")) for k in range(2)]
    orders = [list(np.random.default_rng(3 + k).permutation(64)) for k in range(2)]
    res = augment_batch([_t(f) for f in frames], "unused", bd, particles=tl, orders=orders, planes=[plane, plane], layout="aligned", sync=False)
    got = _sample(res, 128, point_cloud_range=fr.SECOND_RANGE, return_dist=True)
    res.wait()
    rows, rk = res.rows.cpu().numpy(), res.keep.cpu().numpy()
    assert 500 < rk.sum() < len(rk) - 100 and int((rows[rk][:, 4] == 2).sum()) > 5      # rows were removed, and rows were scattered
    kept_off = np.concatenate(([0], np.cumsum([rk[a:b].sum() for a, b in zip(res.offsets[:-1], res.offsets[1:])])))
    want = fr.fps(rows[rk], 128, fr.SECOND_RANGE, 4, None, kept_off)
    assert (want["usable"] >= 128).all()
    _same(got, want, "chain", FIELDS[1:])
    assert np.array_equal(got.index.cpu().numpy(), np.flatnonzero(rk)[want["index"]])
    assert torch.equal(got.points, res.rows[got.index.long()][:, :, :4])                 # rows[index] gathers


# ---- 5. run to run ----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    for name in ("batch", "lattice"):
        a, b = _run_case(name, "float32"), _run_case(name, "float32")
        for f in FIELDS:
            assert getattr(a, f).data_ptr() != getattr(b, f).data_ptr() and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), (name, f)


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture():
    """sample_keypoints(..., out=batch) captured on one stream after a warm-up and replayed on other rows in the same tensor: the scratch
    and every output are rewritten by the captured sequence itself."""
    from lidar_snow_sim_amd.tensors import KeypointBatch
    n, K = 9000, 80                                                      # (the second resident tier of float32)
    clouds = [fr.cloud_case(n, "float32", seed) for seed in (0, 1)]
    want = [fr.cloud_expected(n, "float32", K, seed) for seed in (0, 1)]
    assert not np.array_equal(want[0]["index"], want[1]["index"])
    s = torch.cuda.Stream()
    rows = _t(clouds[0])
    out = KeypointBatch.empty(1, K, 4, torch.float32, with_dist=True)
    with torch.cuda.stream(s):
        _sample(rows, K, point_cloud_range=fr.RANGE, out=out, return_dist=True)      # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = _sample(rows, K, point_cloud_range=fr.RANGE, out=out, return_dist=True)
        assert got is out
        snaps = []
        for k in (1, 0, 1):
            rows.copy_(_t(clouds[k]))
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
    from lidar_snow_sim_amd.fps import farthest_point_sample
    for dtype in DTYPES:
        rows, _, _, (rng, K) = fr.case("lattice", dtype)
        for cols, C in ((5, None), (4, None), (3, None), (5, 4)):
            want = fr.expected("lattice", dtype, num_features=C or cols)
            index, points = farthest_point_sample(rows[:, :cols], K, num_features=C)
            assert index.dtype == np.int32 and points.dtype == rows.dtype
            assert np.array_equal(index, want["index"][0]) and points.tobytes() == want["points"][0].tobytes()
    rows, _, keep, (rng, K) = fr.case("constructed", "float64")
    want = fr.fps(rows, K, rng)
    index, points = farthest_point_sample(rows, K, rng, num_features=4)
    assert np.array_equal(index, want["index"][0]) and points.tobytes() == want["points"][0].tobytes()
    with pytest.raises(ValueError):
        farthest_point_sample(rows[:, :2], K)
    with pytest.raises(ValueError):
        farthest_point_sample(rows[:, :3], K, num_features=4)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import KeypointBatch
    rows, _, _, (rng, K) = fr.case("fewer37")
    pc, n = _t(rows), len(rows)
    who = "snowgpu_fps_device"
    for kw, words in ((dict(num_features=2), "n_features must be 3, 4 or 5"), (dict(num_features=6), "n_features must be 3, 4 or 5"),
                      (dict(n_samples=0), "n_samples must be at least 1"), (dict(n_samples=2 ** 31), "exceeds 2\\^31 - 1"),
                      (dict(point_cloud_range=(0, 0, float("nan"), 1, 1, 1)), who + ": a bound of the range is NaN"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 0, 1)), who + ": the range needs lo < hi on every axis"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 1)), "6 numbers"), (dict(n_samples=2.5), "integer")):
        args = dict(n_samples=K, point_cloud_range=rng)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            _sample(pc, **args)
    with pytest.raises(ValueError, match="torch CUDA tensors"):
        _sample(rows, K)
    with pytest.raises(ValueError):
        _sample(pc, K, keep=torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError):
        _sample(pc, K, keep=np.ones(n, bool))
    with pytest.raises(ValueError, match="out must be a KeypointBatch whose dist"):
        _sample(pc, K, out=KeypointBatch.empty(1, K), return_dist=True)
    with pytest.raises(ValueError, match="out must be a KeypointBatch whose index"):
        _sample(pc, K, out=KeypointBatch.empty(1, K + 1))
    with pytest.raises(ValueError, match="out must be a KeypointBatch whose points"):
        _sample(pc, K, out=KeypointBatch.empty(1, K, dtype=torch.float64))
    # infinite bounds and no range are accepted, and agree
    inf = float("inf")
    a, b = _sample(pc, K, point_cloud_range=(-inf, -inf, -inf, inf, inf, inf), return_dist=True), _sample(pc, K, return_dist=True)
    assert all(torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)) for f in FIELDS) and int(a.usable[0]) == 37
    # the C entry refuses on its own: the overlaps, and a null output; the nullable outputs may be null
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    off = _t(np.array([0, n], np.int64))
    out = KeypointBatch.empty(1, K, with_dist=True)
    keep = torch.ones(n + 64, dtype=torch.uint8, device="cuda:0")
    args = (1, n, n, off.data_ptr(), pc.data_ptr(), 0, rng, K, 4)
    with pytest.raises(ValueError, match="d_out_index overlaps d_keep_in"):
        ctx.fps_device(*args, keep.data_ptr(), keep.data_ptr() + 8, out.points.data_ptr(), out.dist.data_ptr(), out.usable.data_ptr())
    with pytest.raises(ValueError, match="d_out_points overlaps d_rows"):
        ctx.fps_device(*args, keep.data_ptr(), out.index.data_ptr(), pc.data_ptr(), out.dist.data_ptr(), out.usable.data_ptr())
    with pytest.raises(ValueError, match="d_out_dist overlaps d_rows"):
        ctx.fps_device(*args, 0, out.index.data_ptr(), out.points.data_ptr(), pc.data_ptr() + 4 * (5 * n - 1), out.usable.data_ptr())
    with pytest.raises(ValueError, match="null pointer or bad dtype"):
        ctx.fps_device(*args, 0, 0, out.points.data_ptr(), out.dist.data_ptr(), out.usable.data_ptr())
    with pytest.raises(ValueError, match="null pointer or bad dtype"):
        ctx.fps_device(*args, 0, out.index.data_ptr(), out.points.data_ptr(), out.dist.data_ptr(), 0)
    want = fr.expected("fewer37")
    out.index.fill_(9)
    out.usable.fill_(9)
    ctx.fps_device(*args, 0, out.index.data_ptr(), 0, 0, out.usable.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.index.cpu().numpy(), want["index"]) and out.usable.tolist() == [37]
    # an empty batch: usable 0, index -1, points 0, dist -1
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x7f)
    ctx.fps_device(1, 0, 0, off.data_ptr(), 0, 0, None, K, 4, 0, out.index.data_ptr(), out.points.data_ptr(), out.dist.data_ptr(), out.usable.data_ptr())
    torch.cuda.synchronize()
    assert out.usable.tolist() == [0] and bool((out.index == -1).all()) and not out.points.any() and bool((out.dist == -1).all())
    empty = _sample(pc[:0], K, return_dist=True)
    assert empty.usable.tolist() == [0] and bool((empty.index == -1).all()) and not empty.points.any() and bool((empty.dist == -1).all())
    assert empty.index.shape == (1, K) and empty.points.shape == (1, K, 4)


# ---- every refusal of the Python boundary word for word, and which of two faults is reported -----------------------------------------------------
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _short_keep():
    return torch.ones(127, dtype=torch.bool, device="cuda:0")


def _keypoint_out(*args, **kw):
    from lidar_snow_sim_amd.tensors import KeypointBatch
    return KeypointBatch.empty(2, *args, **kw)


HOST_WORDS = "sample_keypoints: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.fps.farthest_point_sample)"
KEEP_WORDS = "keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)"
DEVICE_WORDS = "the tensors live on cuda:0, device=1 was asked for"
OUT_WORDS = "sample_keypoints: out must be a KeypointBatch whose %s tensor on the device of the rows"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)), HOST_WORDS),
    ("n_samples 2.5", lambda: dict(n_samples=2.5), "sample_keypoints: n_samples must be an integer"),
    ("num_features True", lambda: dict(num_features=True), "sample_keypoints: num_features must be an integer"),
    ("range of 5", lambda: dict(point_cloud_range=(0, 0, 0, 4, 4)), "sample_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)"),
    ("num_features 2", lambda: dict(num_features=2), "sample_keypoints: n_features must be 3, 4 or 5: the columns of a row that a keypoint carries"),
    ("n_samples 0", lambda: dict(n_samples=0), "sample_keypoints: n_samples must be at least 1"),
    ("n_samples 2^31", lambda: dict(n_samples=2 ** 31), "sample_keypoints: n_frames * n_samples exceeds 2^31 - 1; split the batch"),
    ("out of another shape", lambda: dict(out=_keypoint_out(9)), OUT_WORDS % "index is a contiguous (2, 8) torch.int32"),
    ("out of another kind", lambda: dict(out=object()), OUT_WORDS % "index is a contiguous (2, 8) torch.int32"),
    ("out of another dtype", lambda: dict(out=_keypoint_out(8, dtype=torch.float64)), OUT_WORDS % "points is a contiguous (2, 8, 4) torch.float32"),
    ("out without dist", lambda: dict(out=_keypoint_out(8), return_dist=True), OUT_WORDS % "dist is a contiguous (2, 8) torch.float32"),
    # two faults: the earlier step of the call reports
    ("host rows before a count", lambda: dict(frames=np.zeros((4, 5), np.float32), n_samples=2.5), HOST_WORDS),
    ("a count before out", lambda: dict(n_samples=2.5, out=object()), "sample_keypoints: n_samples must be an integer"),
    ("the range before the device", lambda: dict(point_cloud_range=(0, 0, 0, 4, 4), device=1), "sample_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)"),
    ("the device before the domain", lambda: dict(device=1, n_samples=0), DEVICE_WORDS),
    ("keep before the domain", lambda: dict(keep=_short_keep(), num_features=2), KEEP_WORDS),
    ("the domain before out", lambda: dict(n_samples=0, out=object()), "sample_keypoints: n_samples must be at least 1"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    from lidar_snow_sim_amd.tensors import sample_keypoints
    args = dict(frames=_pin_batch(), n_samples=8)
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        sample_keypoints(**args)


def test_the_wrapper_refuses_a_short_range_word_for_word():
    from lidar_snow_sim_amd import engine
    with pytest.raises(ValueError, match="^" + re.escape("snowgpu_fps_device: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)") + "$"):
        engine.get_engine(0).ctx.fps_device(2, 128, 64, 0, 0, 0, (0, 0, 0, 4, 4), 8, 4, 0, 0, 0, 0, 0)
