"""-m gpu: sectorized, proposal-centric keypoint sampling on the device (tensors.sample_keypoints with sectors / rois,
fps.sectorized_sample, snowgpu_fps_sectors_device; csrc/snowgpu_fps.hip, csrc/sg_fps_sectors.h) against the NumPy restatement of its
definition (tests/fps_sectors_reference.py, whose inputs tests/test_fps_sectors_reference.py holds to the conditions that keep these
comparisons from being vacuous).  The outputs are integers, copied bits and separately rounded sums that the restatement makes in the
same order: every comparison is equality of bytes."""
import re

import numpy as np
import pytest
import torch

import fps_reference as fr
import fps_sectors_reference as sr

pytestmark = pytest.mark.gpu

DTYPES = sr.DTYPES
PLAIN = ("index", "points", "dist", "usable")
FIELDS = PLAIN + ("sector_offsets", "sector_count", "sector_of")
BD = float(np.degrees(3e-3))


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _frames(rows, offsets):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(rows), offsets)


def _sample(*args, **kw):
    from lidar_snow_sim_amd.tensors import sample_keypoints
    return sample_keypoints(*args, **kw)


def _run_case(name, dtype, S, **kw):
    rows, offsets, keep, rois, (rng, K, margin) = sr.case(name, dtype)
    return _sample(_frames(rows, offsets), K, point_cloud_range=rng, keep=None if keep is None else _t(keep), return_dist=True, sectors=S,
                   rois=None if rois is None else _t(rois), roi_margin=margin, return_sector_of=True, **kw)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = (got[name] if isinstance(got, dict) else getattr(got, name)).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():      # (bytes: NaN columns and -0.0 are copied as they are)
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


# ---- 1. every tier of the walk inside one grid ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_tiers(dtype):
    """Three frames, S = 2, K = 24: sectors of c and c + 1 rows at the edge between the register tier and the LDS tier, of c - 1 and
    c + 1 rows around the first register tier's capacity and around the LDS tier's (the streamed walk: the largest case)."""
    rows, offsets, sizes, want = sr.tier_case(dtype)
    assert want["sector_count"].tolist() == [list(s) for s in sizes]
    _same(_sample(_frames(rows, offsets), 24, point_cloud_range=fr.RANGE, return_dist=True, sectors=2, return_sector_of=True), want, dtype)


# ---- 2. the constructed frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", sr.SECTORS)
@pytest.mark.parametrize("name", sr.CASES)
def test_constructed_frames_equal_the_restatement(name, S, dtype):
    _same(_run_case(name, dtype, S), sr.expected(name, dtype, S), (name, S, dtype))


# ---- 3. a batch ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("batch", "batch_rois"))
def test_batch_of_frames(name, dtype):
    """Frames of 6000, 0, 1500 and 300 rows at offsets that are no multiples of 64, a keep mask that removes one frame whole; with rois on
    frames 0 and 2 only."""
    rows, offsets, keep, rois, _ = sr.case(name, dtype)
    assert np.array_equal(np.diff(offsets), (6000, 0, 1500, 300)) and all(int(o) % 64 for o in offsets[1:]) and not keep[offsets[3]:].any()
    for S, C in ((6, 4), (16, 5), (1, 3)):
        want = sr.expected(name, dtype, S, C)
        assert want["usable"][0] > 48 and want["usable"][1] == 0 and want["usable"][3] == 0
        _same(_run_case(name, dtype, S, num_features=C), want, (name, S, C, dtype))
    if rois is not None:
        assert 0 < sr.expected(name, dtype, 6)["usable"][2] < 1500 and not rois[[1, 3]].any()


# ---- 4. identity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_sector_without_rois_equals_the_plain_sampler(dtype):
    for name in ("batch", "constructed", "fewer37", "fewer1", "fewer0", "lattice"):
        rows, offsets, keep, (rng, K) = fr.case(name, dtype)
        kw = dict(point_cloud_range=rng, keep=None if keep is None else _t(keep), return_dist=True)
        plain, one = _sample(_frames(rows, offsets), K, **kw), _sample(_frames(rows, offsets), K, sectors=1, **kw)
        for f in PLAIN:
            assert torch.equal(getattr(plain, f).view(torch.uint8), getattr(one, f).view(torch.uint8)), (name, f)
        assert plain.sector_offsets is None and one.sector_offsets.shape == (len(offsets) - 1, 2)
        assert torch.equal(one.sector_count[:, 0], one.usable) and torch.equal(one.sector_offsets[:, 1], one.usable.clamp(max=K))


# ---- 5. out= and the optional outputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written(dtype):
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import KeypointBatch
    for name, S in (("roi", 6), ("quota", 4), ("batch_rois", 16)):
        rows, offsets, _, _, (_, K, _) = sr.case(name, dtype)
        out = KeypointBatch.empty(len(offsets) - 1, K, 4, getattr(torch, dtype), with_dist=True, sectors=S, with_sector_of=len(rows))
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        got = _run_case(name, dtype, S, out=out)
        assert got is out
        _same(out, sr.expected(name, dtype, S), (name, dtype))
    # the C entry: d_out_reach2, and the nullable outputs null
    rows, offsets, _, rois, (_, K, margin) = sr.case("roi", dtype)
    want = sr.expected("roi", dtype, 6)
    ctx = engine.get_engine(0).ctx
    pc, d_rois, off = _t(rows), _t(rois), _t(offsets)
    out = KeypointBatch.empty(2, K, 4, getattr(torch, dtype), with_dist=True, sectors=6, with_sector_of=len(rows))
    reach2 = torch.empty((2, 6), dtype=torch.float64, device="cuda")
    for t in [getattr(out, f) for f in FIELDS] + [reach2]:
        t.view(torch.uint8).fill_(0x7f)
    args = (2, len(rows), 1500, off.data_ptr(), pc.data_ptr(), DTYPES.index(dtype), None, K, 4, 0, 6, d_rois.data_ptr(), 6, 8, margin)
    ctx.fps_sectors_device(*args, out.index.data_ptr(), out.points.data_ptr(), out.dist.data_ptr(), out.usable.data_ptr(), out.sector_offsets.data_ptr(),
                           out.sector_count.data_ptr(), out.sector_of.data_ptr(), reach2.data_ptr())
    torch.cuda.synchronize()
    _same(out, want, ("entry", dtype))
    assert reach2.cpu().numpy().tobytes() == want["reach2"].tobytes()
    for f in ("index", "usable", "sector_offsets", "sector_count"):
        getattr(out, f).view(torch.uint8).fill_(0x7f)
    ctx.fps_sectors_device(*args, out.index.data_ptr(), 0, 0, out.usable.data_ptr(), out.sector_offsets.data_ptr(), out.sector_count.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    _same(out, want, ("entry, nullable outputs null", dtype), ("index", "usable", "sector_offsets", "sector_count"))
    # an empty batch
    for t in [getattr(out, f) for f in FIELDS] + [reach2]:
        t.view(torch.uint8).fill_(0x7f)
    ctx.fps_sectors_device(2, 0, 0, _t(np.zeros(3, np.int64)).data_ptr(), 0, DTYPES.index(dtype), None, K, 4, 0, 6, d_rois.data_ptr(), 6, 8, margin,
                           out.index.data_ptr(), out.points.data_ptr(), out.dist.data_ptr(), out.usable.data_ptr(), out.sector_offsets.data_ptr(),
                           out.sector_count.data_ptr(), 0, reach2.data_ptr())
    torch.cuda.synchronize()
    assert not out.usable.any() and bool((out.index == -1).all()) and not out.points.any() and bool((out.dist == -1).all())
    assert not out.sector_offsets.any() and not out.sector_count.any() and reach2.cpu().numpy().tobytes() == want["reach2"].tobytes()


# ---- 6. run to run ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes_and_the_scratch_may_grow_between():
    a, b = _run_case("batch_rois", "float32", 6), _run_case("batch_rois", "float32", 6)
    for f in FIELDS:
        assert getattr(a, f).data_ptr() != getattr(b, f).data_ptr() and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), f
    rows, offsets, _, want = sr.tier_case("float64")                              # another size and dtype: the scratch grows
    _same(_sample(_frames(rows, offsets), 24, point_cloud_range=fr.RANGE, return_dist=True, sectors=2, return_sector_of=True), want, "grown")
    _same(_run_case("batch_rois", "float32", 6), sr.expected("batch_rois", "float32", 6), "after the growth")
    _same(_run_case("edges", "float32", 16), sr.expected("edges", "float32", 16), "after the growth, edges")


# ---- 7. graph capture -----------------------------------------------------------------------------------------------------------------------------
def test_graph_capture(tables):
    """Aligned snowfall -> sectorized keypoints (under the result's keep mask) -> ball_query captured as one graph on one stream after a
    warm-up and replayed three times on changing input, every output filled with 0x7f before: each replay equals the restatements of the
    two stages composed on the snowfall's own result of that replay."""
    import ball_reference as br
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import DeviceBatch, KeypointBatch, NeighbourBatch, ball_query
    eng = engine.get_engine(0)
    dev = torch.device("cuda:0")
    tl = [tables["t"][i % 4] for i in range(64)]
    F, n, K, S, pairs = 2, 64 * 128, 96, 6, ((0.8, 1.6), (16, 16))
    inputs = [torch.from_numpy(np.concatenate([synthetic_sweep(64, 128, seed=s0 + f, intensity="lambert") for f in range(F)])).to(dev) for s0 in (1700, 1720)]
    rows = inputs[0].clone()
    offsets = np.arange(F + 1, dtype=np.int64) * n
    off = torch.from_numpy(offsets).to(dev)
    tids = torch.tensor([eng.table_ids_from_arrays(tl, list(range(64))) for _ in range(F)], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    out, keep = torch.empty_like(rows), torch.zeros(F * n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    kp_out = KeypointBatch.empty(F, K, 4, torch.float32, with_dist=True, sectors=S, with_sector_of=F * n)
    nb_out = NeighbourBatch.empty(F, K, pairs[1], 4, torch.float32, with_points=True)
    s = torch.cuda.Stream()

    def chain():
        eng.ctx.augment_batch_device_aligned(F, F * n, n, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), BD, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)
        batch = DeviceBatch(out, offsets)
        kp = _sample(batch, K, point_cloud_range=fr.SECOND_RANGE, keep=keep, sectors=S, out=kp_out, return_dist=True, return_sector_of=True)
        return kp, ball_query(batch, kp, pairs[0], pairs[1], point_cloud_range=fr.SECOND_RANGE, keep=keep, out=nb_out, return_points=True)

    outputs = [getattr(kp_out, f) for f in FIELDS] + [nb_out.index, nb_out.count, nb_out.points]
    with torch.cuda.stream(s):
        chain()                                                            # warm-up: the captured calls allocate nothing
        s.synchronize()
        assert int(status[0]) == 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            kp, nb = chain()
        assert kp is kp_out and nb is nb_out
        snaps = []
        for k in (1, 0, 1):                                                # no host read between the replays
            rows.copy_(inputs[k])
            for t in outputs + [out, keep]:
                t.view(torch.uint8).fill_(0x7f)
            g.replay()
            snaps.append((out.clone(), keep.clone(), {f: getattr(kp_out, f).clone() for f in FIELDS}, dict(index=nb_out.index.clone(), count=nb_out.count.clone(), points=nb_out.points.clone())))
        s.synchronize()
    kept = []
    for r, m, kp_snap, nb_snap in snaps:
        r, m = r.cpu().numpy(), m.cpu().numpy()
        kept.append(int(m.sum()))
        want = sr.fps_sectors(r, K, S, fr.SECOND_RANGE, 4, m, offsets)
        assert (want["usable"] >= K).all() and (want["sector_count"] > 0).sum() >= 2 * F
        _same(kp_snap, want, "graph, keypoints")
        _same(nb_snap, br.ball_query(r, want["points"], pairs[0], pairs[1], fr.SECOND_RANGE, 4, m, offsets), "graph, ball query", ("index", "count", "points"))
    assert kept[0] == kept[2] != kept[1] and 0 < kept[0] < F * n           # rows were removed, and the input changed between the replays
    assert not torch.equal(snaps[0][2]["index"], snaps[1][2]["index"]) and torch.equal(snaps[0][2]["index"], snaps[2][2]["index"])


# ---- 8. the NumPy entry ---------------------------------------------------------------------------------------------------------------------------
def test_numpy_entry():
    from lidar_snow_sim_amd.fps import sectorized_sample
    for dtype in DTYPES:
        rows, _, _, _, (rng, K, _) = sr.case("edges", dtype)
        for cols, S in ((5, 6), (3, 16)):
            want = sr.expected("edges", dtype, S, cols)
            index, points, offsets = sectorized_sample(rows[:, :cols], K, S) if S != 6 else sectorized_sample(rows[:, :cols], K)
            assert index.dtype == np.int32 and points.dtype == rows.dtype and offsets.dtype == np.int32
            assert np.array_equal(index, want["index"][0]) and points.tobytes() == want["points"][0].tobytes() and np.array_equal(offsets, want["sector_offsets"][0])
        rows, offsets, _, rois, (rng, K, margin) = sr.case("roi", dtype)
        want = sr.fps_sectors(rows[:1500], K, 4, None, 4, None, None, rois[:1], margin)
        index, points, so = sectorized_sample(rows[:1500], K, 4, rois[0], margin, num_features=4)
        assert np.array_equal(index, want["index"][0]) and points.tobytes() == want["points"][0].tobytes() and np.array_equal(so, want["sector_offsets"][0])
    with pytest.raises(ValueError):
        sectorized_sample(rows[:, :2], K)
    with pytest.raises(ValueError):
        sectorized_sample(rows, K, rois=rois[0][:, :6])


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import KeypointBatch
    rows, offsets, _, rois, (rng, K, margin) = sr.case("roi")
    pc, d_rois = _frames(rows, offsets), _t(rois)
    who = "snowgpu_fps_sectors_device"
    for kw, words in ((dict(sectors=0), "n_sectors must lie in 1 .. 16"), (dict(sectors=17), "n_sectors must lie in 1 .. 16"), (dict(sectors=2.5), "integer"),
                      (dict(roi_margin=-0.5), who + ": roi_margin must be finite and at least 0"), (dict(roi_margin=float("nan")), who + ": roi_margin"),
                      (dict(rois=d_rois[:, :, :6]), "rois must be a contiguous"), (dict(rois=d_rois[:1]), "rois must be a contiguous"),
                      (dict(rois=d_rois.double()), "rois must be a contiguous"), (dict(rois=rois), "rois must be a contiguous"),
                      (dict(num_features=6), "n_features must be 3, 4 or 5"), (dict(n_samples=0), "n_samples must be at least 1"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 0, 1)), who + ": the range needs lo < hi on every axis")):
        args = dict(n_samples=K, sectors=6, rois=d_rois, roi_margin=margin)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            _sample(pc, **args)
    with pytest.raises(ValueError, match="out must be a KeypointBatch whose sector_offsets"):
        _sample(pc, K, sectors=6, out=KeypointBatch.empty(2, K))
    with pytest.raises(ValueError, match="out must be a KeypointBatch whose sector_count"):
        out = KeypointBatch.empty(2, K, sectors=6)
        out.sector_count = out.sector_count[:, :5].contiguous()
        _sample(pc, K, sectors=6, out=out)
    with pytest.raises(ValueError, match="out must be a KeypointBatch whose sector_of"):
        _sample(pc, K, sectors=6, out=KeypointBatch.empty(2, K, sectors=6), return_sector_of=True)
    # rois alone: one sector
    got = _sample(pc, K, rois=d_rois, roi_margin=margin, return_dist=True, return_sector_of=True)
    _same(got, sr.expected("roi", "float32", 1), "rois alone")


# ---- every refusal of the sectorized call word for word, and which of two faults is reported ---------------------------------------------------
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _keypoint_out(*args, **kw):
    from lidar_snow_sim_amd.tensors import KeypointBatch
    return KeypointBatch.empty(2, *args, **kw)


def _rois(dtype=torch.float32):
    return torch.ones((2, 2, 7), dtype=dtype, device="cuda:0")


HOST_WORDS = "sample_keypoints: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.fps.sectorized_sample)"
ROI_WORDS = "sample_keypoints: rois must be a contiguous (frames, B, 7 .. 10) tensor of the rows' dtype on the device of the rows"
OUT_WORDS = "sample_keypoints: out must be a KeypointBatch whose %s tensor on the device of the rows"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)), HOST_WORDS),
    ("host rows with rois alone", lambda: dict(frames=np.zeros((4, 5), np.float32), sectors=None, rois=_rois()), HOST_WORDS),
    ("n_samples 2.5", lambda: dict(n_samples=2.5), "sample_keypoints: n_samples must be an integer"),
    ("num_features True", lambda: dict(num_features=True), "sample_keypoints: num_features must be an integer"),
    ("sectors 2.5", lambda: dict(sectors=2.5), "sample_keypoints: sectors must be an integer"),
    ("range of 5", lambda: dict(point_cloud_range=(0, 0, 0, 4, 4)), "sample_keypoints: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)"),
    ("num_features 6", lambda: dict(num_features=6), "sample_keypoints: n_features must be 3, 4 or 5: the columns of a row that a keypoint carries"),
    ("n_samples 0", lambda: dict(n_samples=0), "sample_keypoints: n_samples must be at least 1"),
    ("n_samples 2^31", lambda: dict(n_samples=2 ** 31), "sample_keypoints: n_frames * n_samples exceeds 2^31 - 1; split the batch"),
    ("sectors 17", lambda: dict(sectors=17), "sample_keypoints: n_sectors must lie in 1 .. 16"),
    ("sectors 0", lambda: dict(sectors=0), "sample_keypoints: n_sectors must lie in 1 .. 16"),
    ("rois of another dtype", lambda: dict(rois=_rois(torch.float64)), ROI_WORDS),
    ("rois of another frame count", lambda: dict(rois=_rois()[:1]), ROI_WORDS),
    ("out without sectors", lambda: dict(out=_keypoint_out(8)), OUT_WORDS % "sector_offsets is a contiguous (2, 5) torch.int32"),
    ("out of another kind", lambda: dict(out=object()), OUT_WORDS % "index is a contiguous (2, 8) torch.int32"),
    ("out of other sectors", lambda: dict(out=_keypoint_out(8, sectors=5)), OUT_WORDS % "sector_offsets is a contiguous (2, 5) torch.int32"),
    ("out without dist", lambda: dict(out=_keypoint_out(8, sectors=4), return_dist=True), OUT_WORDS % "dist is a contiguous (2, 8) torch.float32"),
    ("out without sector_of", lambda: dict(out=_keypoint_out(8, sectors=4), return_sector_of=True), OUT_WORDS % "sector_of is a contiguous (128,) torch.int8"),
    # two faults: the earlier step of the call reports
    ("a count before out", lambda: dict(sectors=2.5, out=object()), "sample_keypoints: sectors must be an integer"),
    ("the device before the domain", lambda: dict(device=1, sectors=17), "the tensors live on cuda:0, device=1 was asked for"),
    ("the samples before the sectors", lambda: dict(n_samples=0, sectors=17), "sample_keypoints: n_samples must be at least 1"),
    ("the sectors before the rois", lambda: dict(sectors=17, rois=_rois(torch.float64)), "sample_keypoints: n_sectors must lie in 1 .. 16"),
    ("the rois before out", lambda: dict(rois=_rois(torch.float64), out=object()), ROI_WORDS),
    ("dist before sector_of", lambda: dict(out=_keypoint_out(8, sectors=4), return_dist=True, return_sector_of=True), OUT_WORDS % "dist is a contiguous (2, 8) torch.float32"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    from lidar_snow_sim_amd.tensors import sample_keypoints
    args = dict(frames=_pin_batch(), n_samples=8, sectors=4)
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        sample_keypoints(**args)


def test_the_wrapper_refuses_a_short_range_word_for_word():
    from lidar_snow_sim_amd import engine
    with pytest.raises(ValueError, match="^" + re.escape("snowgpu_fps_sectors_device: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)") + "$"):
        engine.get_engine(0).ctx.fps_sectors_device(2, 128, 64, 0, 0, 0, (0, 0, 0, 4, 4), 8, 4, 0, 4, 0, 0, 0, 1.6, 0, 0, 0, 0, 0, 0)
