"""-m gpu: ball-query neighbour groups on the device (tensors.ball_query, ball.ball_query, snowgpu_ball_query_device;
csrc/snowgpu_ball.hip, csrc/sg_ball.h) against the brute-force NumPy restatement of its definition (tests/ball_reference.py, whose inputs
tests/test_ball_reference.py holds to the conditions that keep these comparisons from being vacuous).  The outputs are integers and
copied bits, membership is decided by separately rounded operations that the restatement makes in the same order: every comparison is
equality of bytes."""
import re

import numpy as np
import pytest
import torch

import ball_reference as br

pytestmark = pytest.mark.gpu

DTYPES = br.DTYPES
FIELDS = ("index", "count", "points")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _frames(rows, offsets):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(rows), offsets)


def _query(*args, **kw):
    from lidar_snow_sim_amd.tensors import ball_query
    kw.setdefault("return_points", True)
    return ball_query(*args, **kw)


def _run_case(name, dtype, num_features=4, radii=None, samples=None, **kw):
    rows, offsets, keep, centres, (rng, r, s) = br.case(name, dtype)
    return _query(_frames(rows, offsets), _t(centres), r if radii is None else radii, s if samples is None else samples, point_cloud_range=rng,
                  keep=None if keep is None else _t(keep), num_features=num_features, **kw)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():      # (bytes: NaN columns and -0.0 are copied as they are)
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


# ---- 1. the shared inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("constructed", "batch", "unusable", "absent"))
def test_shared_inputs_equal_the_restatement(name, dtype):
    got = _run_case(name, dtype)
    _same(got, br.expected(name, dtype), (name, dtype))
    assert got.segments == br.case(name, dtype)[4][2]


# ---- 2. samples around the ball's size ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", (1, 16, 39, 40, 41, 64))
def test_samples_around_the_rows_of_a_ball(S, dtype):
    """The balls of n = 5000 rows in one cell (many batches per wave, most of them rejected by the threshold), n = 40 and n = 0."""
    _same(_run_case("cluster", dtype, samples=(S,)), br.expected("cluster", dtype, samples=(S,)), (S, dtype))


# ---- 3. arrival orders ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", (16, 64))
def test_smallest_indices_in_the_first_and_in_the_last_cells(S, dtype):
    want = br.expected("constructed", dtype, samples=(S,))
    got = _run_case("constructed", dtype, samples=(S,))
    for role in ("high_cells_first", "low_cells_first"):
        k = br.ROLE[role]
        assert want["count"][0, k, 0] > 64 and np.array_equal(got.index[0, k].cpu().numpy(), want["index"][0, k]), role
    _same(got, want, (S, dtype))


# ---- 4. grid edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_and_centres_beyond_the_domain(dtype):
    """Border cells, centres 500 m outside the domain, non-finite centres, and cells widened to the budget (r = 0.4 m on 240 m x 240 m)."""
    _same(_run_case("outside", dtype), br.expected("outside", dtype), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("radius", (0.01, 1000.0))
def test_the_smallest_and_the_largest_window(radius, dtype):
    """r = 0.01 m: the cells are widened far beyond the radius.  r = 1000 m: the window is every cell, and count = the usable rows."""
    for name in ("batch", "outside"):
        want = br.expected(name, dtype, radii=(radius,), samples=(16,))
        _same(_run_case(name, dtype, radii=(radius,), samples=(16,)), want, (name, radius, dtype))
        if radius == 1000.0 and name == "batch":
            rows, offsets, _, _, (rng, _, _) = br.case(name, dtype)
            usable = [int(br.usable_rows(rows[a:b], rng).sum()) for a, b in zip(offsets[:-1], offsets[1:])]
            assert usable[3] == 300 and (want["count"][..., 0] == np.array(usable)[:, None]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_frame_of_three_rows(dtype):
    """The minimum cell budget."""
    rows = br.cloud(3, dtype, seed=71, span=1.0)
    centres = np.ascontiguousarray(np.concatenate((rows[:, :3], [[0.5, 0.0, 0.0]])).astype(dtype))[None]
    assert br.cell_budget(3) == br.MIN_CELLS
    for r in (0.05, 0.6, 3.0):
        want = br.ball_query(rows, centres, (r,), (4,), br.RANGE)
        _same(_query(_t(rows), _t(centres), r, 4, point_cloud_range=br.RANGE), want, (r, dtype))
    assert want["count"].reshape(-1).tolist() == [3, 3, 3, 3]


# ---- 5. several radii -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairs", (((0.4, 16), (0.8, 16)), ((1.0, 1), (0.25, 64), (2.5, 64), (0.5, 7))))
def test_several_radii(pairs, dtype):
    radii, samples = tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)
    for name in ("constructed", "batch"):
        got = _run_case(name, dtype, radii=radii, samples=samples)
        _same(got, br.expected(name, dtype, radii=radii, samples=samples), (name, pairs, dtype))
        assert got.segments == samples
        seg = np.concatenate(([0], np.cumsum(samples)))
        for i, (r, s) in enumerate(pairs):
            one = _run_case(name, dtype, radii=(r,), samples=(s,))
            assert torch.equal(got.index[:, :, seg[i]:seg[i + 1]], one.index) and torch.equal(got.count[:, :, i:i + 1], one.count), (name, i)
            assert torch.equal(got.points[:, :, seg[i]:seg[i + 1]].contiguous().view(torch.uint8), one.points.view(torch.uint8)), (name, i)


# ---- 6. the columns ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_features", (3, 5))
def test_number_of_features(num_features, dtype):
    for name in ("constructed", "batch"):
        _same(_run_case(name, dtype, num_features=num_features), br.expected(name, dtype, num_features=num_features), (name, dtype, num_features))
    rows, offsets, _, centres, (rng, r, s) = br.case("batch", dtype)         # centres of 4 columns; now of 3 and of 5
    want = br.expected("batch", dtype)
    for cq in (3, 5):
        cen = np.ascontiguousarray(np.concatenate((centres, np.full(centres.shape[:2] + (1,), np.nan, centres.dtype)), axis=2)[:, :, :cq])
        _same(_query(_frames(rows, offsets), _t(cen), r, s, point_cloud_range=rng), want, (dtype, cq))


# ---- 7. a synthetic sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    return np.ascontiguousarray(synthetic_sweep(64, 512, seed=1700, intensity="lambert"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_synthetic_sweep_around_its_keypoints(sweep, dtype):
    from lidar_snow_sim_amd.tensors import sample_keypoints
    rows = np.ascontiguousarray(sweep.astype(dtype))
    d_rows = _t(rows)
    kp = sample_keypoints(d_rows, 128, point_cloud_range=br.SECOND_RANGE)
    got = _query(d_rows, kp, (0.4, 0.8), (16, 32), point_cloud_range=br.SECOND_RANGE)
    want = br.ball_query(rows, kp.points.cpu().numpy(), (0.4, 0.8), (16, 32), br.SECOND_RANGE)
    assert (want["count"] >= 1).all() and (want["count"][..., 1] > 32).any() and (want["count"][..., 0] < 16).any()
    assert (want["index"][0, :, 0] <= kp.index[0].cpu().numpy()).all()             # a keypoint is in its own ball
    _same(got, want, dtype)


# ---- 8. the input mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_keep_equals_the_compacted_frames(dtype):
    rows, offsets, _, centres, (rng, r, s) = br.case("batch", dtype)
    keep = np.random.default_rng(81).random(len(rows)) < 0.7
    masked = _query(_frames(rows, offsets), _t(centres), r, s, point_cloud_range=rng, keep=_t(keep))
    _same(masked, br.ball_query(rows, centres, r, s, rng, 4, keep, offsets), dtype)
    parts = [_t(rows[a:b][keep[a:b]]) for a, b in zip(offsets[:-1], offsets[1:])]
    compact = _query(parts, _t(centres), r, s, point_cloud_range=rng)
    for f in FIELDS[1:]:
        assert torch.equal(getattr(masked, f).view(torch.uint8), getattr(compact, f).view(torch.uint8)), f
    back = np.flatnonzero(keep)                                          # compacted row -> row of the batch
    ci = compact.index.cpu().numpy()
    assert np.array_equal(masked.index.cpu().numpy(), np.where(ci >= 0, back[np.maximum(ci, 0)], -1)) and (ci >= 0).any()


def _snowfall(tables):
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import augment_batch
    tl = [tables["t"][i % 4] for i in range(64)]
    plane, bd = (np.array([0.0, 0.0, -1.0]), -1.7), float(np.degrees(3e-3))
    frames = [np.ascontiguousarray(synthetic_sweep(64, 128, seed=1600 + k, intensity="lambert")) for k in range(2)]
    orders = [list(np.random.default_rng(3 + k).permutation(64)) for k in range(2)]
    return augment_batch([_t(f) for f in frames], "unused", bd, particles=tl, orders=orders, planes=[plane, plane], layout="aligned", sync=False)


def test_an_aligned_result_equals_its_rows_and_mask(tables):
    res = _snowfall(tables)
    centres = res.rows[torch.tensor([[10, 500, 4000], [8200, 9000, 12000]], device="cuda")][:, :, :3].contiguous()
    a = _query(res, centres, 0.8, 16)
    b = _query(_frames(res.rows.cpu().numpy(), res.offsets), centres, 0.8, 16, keep=res.keep)
    extra = torch.ones_like(res.keep, dtype=torch.bool)
    extra[::3] = False
    c = _query(res, centres, 0.8, 16, keep=extra)
    d = _query(_frames(res.rows.cpu().numpy(), res.offsets), centres, 0.8, 16, keep=res.keep.view(torch.bool) & extra)
    res.wait()
    assert int(a.count.sum()) > int(c.count.sum()) > 0
    for x, y in ((a, b), (c, d)):
        assert all(torch.equal(getattr(x, f).view(torch.uint8), getattr(y, f).view(torch.uint8)) for f in FIELDS)


# ---- 9. every element is written --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written(dtype):
    from lidar_snow_sim_amd.tensors import NeighbourBatch
    for name in ("batch", "unusable", "absent", "outside"):
        _, offsets, _, centres, (_, _, s) = br.case(name, dtype)
        out = NeighbourBatch.empty(len(offsets) - 1, centres.shape[1], s, 4, getattr(torch, dtype), with_points=True)
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        got = _run_case(name, dtype, out=out)
        assert got is out
        _same(out, br.expected(name, dtype), (name, dtype))
    out = NeighbourBatch.empty(1, 5, (2, 3), 4, getattr(torch, dtype), with_points=True)      # a batch without a row: the fill kernel
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x7f)
    _query(_t(np.zeros((0, 5), dtype)), _t(np.zeros((1, 5, 3), dtype)), (0.5, 1.0), (2, 3), out=out)
    assert bool((out.index == -1).all()) and not out.count.any() and not out.points.any()


# ---- 10. run to run ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    for name in ("constructed", "cluster", "batch"):
        a, b = _run_case(name, "float32", samples=(64,)), _run_case(name, "float32", samples=(64,))
        for f in FIELDS:
            assert getattr(a, f).data_ptr() != getattr(b, f).data_ptr() and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), (name, f)


# ---- 11. the chain ----------------------------------------------------------------------------------------------------------------------------
def test_chain_behind_the_aligned_snowfall_and_the_keypoints(tables):
    from lidar_snow_sim_amd.tensors import sample_keypoints
    res = _snowfall(tables)
    kp = sample_keypoints(res, 64, point_cloud_range=br.SECOND_RANGE)
    got = _query(res, kp, (0.4, 0.8), (16, 16), point_cloud_range=br.SECOND_RANGE)
    res.wait()
    rows, rk = res.rows.cpu().numpy(), res.keep.cpu().numpy().astype(bool)
    assert 500 < rk.sum() < len(rk) - 100
    want = br.ball_query(rows, kp.points.cpu().numpy(), (0.4, 0.8), (16, 16), br.SECOND_RANGE, 4, rk, res.offsets)
    assert (want["count"] >= 1).all() and (want["count"][..., 1] > 16).any()
    _same(got, want, "chain")
    sel = got.index.long().clamp(min=0)
    assert torch.equal(got.points, res.rows[sel][..., :4])                         # rows[index] gathers


# ---- 12. graph capture ------------------------------------------------------------------------------------------------------------------------
def test_graph_capture():
    """sample_keypoints + ball_query captured on one stream after a warm-up and replayed on other rows in the same tensor: the scratch and
    every output are rewritten by the captured sequence itself.  A linear graph."""
    from lidar_snow_sim_amd.tensors import KeypointBatch, NeighbourBatch, sample_keypoints
    n, K, pairs = 3000, 48, ((0.4, 0.8), (16, 16))
    clouds = [br.cloud(n, "float32", seed, span=8.0) for seed in (90, 91)]
    want = []
    import fps_reference as fr
    for c in clouds:
        kp = fr.fps(c, K, br.RANGE)
        want.append(br.ball_query(c, kp["points"][:, :, :4], pairs[0], pairs[1], br.RANGE))
    assert not np.array_equal(want[0]["index"], want[1]["index"])
    s = torch.cuda.Stream()
    rows = _t(clouds[0])
    kp_out, out = KeypointBatch.empty(1, K, 4, torch.float32), NeighbourBatch.empty(1, K, pairs[1], 4, torch.float32, with_points=True)

    def chain():
        kp = sample_keypoints(rows, K, point_cloud_range=br.RANGE, out=kp_out)
        return _query(rows, kp, pairs[0], pairs[1], point_cloud_range=br.RANGE, out=out)

    with torch.cuda.stream(s):
        chain()                                                            # warm-up: the captured calls allocate nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = chain()
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


# ---- 13. the NumPy entry ----------------------------------------------------------------------------------------------------------------------
def test_numpy_entry():
    from lidar_snow_sim_amd.ball import ball_query
    for dtype in DTYPES:
        rows, _, _, centres, (rng, r, s) = br.case("constructed", dtype)
        for cols, C in ((5, None), (3, None), (5, 4)):
            want = br.expected("constructed", dtype, num_features=C or cols)
            index, count, points = ball_query(rows[:, :cols], centres[0], r, s, rng, num_features=C, return_points=True)
            assert index.dtype == np.int32 and count.dtype == np.int32 and points.dtype == rows.dtype
            assert np.array_equal(index, want["index"][0]) and np.array_equal(count, want["count"][0]) and points.tobytes() == want["points"][0].tobytes()
        index, count = ball_query(rows, centres[0], 1.0, 16, rng)
        assert np.array_equal(index, want["index"][0]) and np.array_equal(count, want["count"][0])
    with pytest.raises(ValueError):
        ball_query(rows[:, :2], centres[0], 1.0, 16)
    with pytest.raises(ValueError):
        ball_query(rows, centres[0][:, :2], 1.0, 16)
    with pytest.raises(ValueError):
        ball_query(rows[:, :3], centres[0], 1.0, 16, num_features=4)


# ---- 14. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import NeighbourBatch
    rows, _, _, centres, (rng, r, s) = br.case("constructed")
    pc, cen, n = _t(rows), _t(centres), len(rows)
    who = "snowgpu_ball_query_device"
    for kw, words in ((dict(num_features=2), "n_features must be 3, 4 or 5"), (dict(num_features=6), "n_features must be 3, 4 or 5"),
                      (dict(n_neighbours=0), "the samples of a radius must lie in 1 .. 64"), (dict(n_neighbours=65), "the samples of a radius must lie in 1 .. 64"),
                      (dict(radius=0.0), who + ": a radius must be finite, above 0 and at most 1e6"),
                      (dict(radius=float("nan")), who + ": a radius must be finite, above 0 and at most 1e6"),
                      (dict(radius=2e6), who + ": a radius must be finite, above 0 and at most 1e6"),
                      (dict(radius=(1.0, 2.0), n_neighbours=(16,)), "as many radii as sample counts"),
                      (dict(radius=(1.0,) * 5, n_neighbours=(1,) * 5), "n_radii must lie in 1 .. 4"),
                      (dict(centres=cen[:, :, :2].contiguous()), "centre_features must be 3, 4 or 5"),
                      (dict(centres=cen[:, :0].contiguous()), "n_centres must be at least 1"),
                      (dict(centres=cen.double()), "centres must be a KeypointBatch or a contiguous"),
                      (dict(centres=cen[0]), "centres must be a KeypointBatch or a contiguous"),
                      (dict(point_cloud_range=(0, 0, float("nan"), 1, 1, 1)), who + ": a bound of the range is NaN"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 0, 1)), who + ": the range needs lo < hi on every axis"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 1)), "6 numbers"), (dict(n_neighbours=2.5), "integer")):
        args = dict(centres=cen, radius=r, n_neighbours=s, point_cloud_range=rng)
        args.update(kw)
        with pytest.raises(ValueError, match=words.replace("..", r"\.\.")):
            _query(pc, **args)
    with pytest.raises(ValueError, match="torch CUDA tensors"):
        _query(rows, cen, 1.0, 16)
    with pytest.raises(ValueError):
        _query(pc, cen, 1.0, 16, keep=torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError, match="out must be a NeighbourBatch whose points"):
        _query(pc, cen, 1.0, 16, out=NeighbourBatch.empty(1, 24, 16))
    with pytest.raises(ValueError, match="out must be a NeighbourBatch whose index"):
        _query(pc, cen, 1.0, 16, out=NeighbourBatch.empty(1, 24, 17, with_points=True))
    with pytest.raises(ValueError, match="out must be a NeighbourBatch whose count"):
        _query(pc, cen, (1.0, 2.0), (8, 8), out=NeighbourBatch.empty(1, 24, 16, with_points=True))
    # the C entry refuses on its own: the overlaps, and a null output; the nullable output may be null
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    off = _t(np.array([0, n], np.int64))
    out = NeighbourBatch.empty(1, 24, 16, with_points=True)
    keep = torch.ones(n + 4096, dtype=torch.uint8, device="cuda:0")
    args = (1, n, n, off.data_ptr(), pc.data_ptr(), 0, rng, 24, cen.data_ptr(), 3, (1.0,), (16,), 4)
    with pytest.raises(ValueError, match="d_out_index overlaps d_keep_in"):
        ctx.ball_query_device(*args, keep.data_ptr(), keep.data_ptr() + 8, out.count.data_ptr(), out.points.data_ptr())
    with pytest.raises(ValueError, match="d_out_points overlaps d_rows"):
        ctx.ball_query_device(*args, keep.data_ptr(), out.index.data_ptr(), out.count.data_ptr(), pc.data_ptr())
    with pytest.raises(ValueError, match="d_out_count overlaps d_centres"):
        ctx.ball_query_device(*args, 0, out.index.data_ptr(), cen.data_ptr() + 4 * (24 * 3 - 1), out.points.data_ptr())
    with pytest.raises(ValueError, match="null pointer or bad dtype"):
        ctx.ball_query_device(*args, 0, 0, out.count.data_ptr(), out.points.data_ptr())
    with pytest.raises(ValueError, match="null pointer or bad dtype"):
        ctx.ball_query_device(*args, 0, out.index.data_ptr(), 0, out.points.data_ptr())
    want = br.expected("constructed")
    out.index.fill_(9)
    out.count.fill_(9)
    ctx.ball_query_device(*args, 0, out.index.data_ptr(), out.count.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.array_equal(out.index.cpu().numpy(), want["index"]) and np.array_equal(out.count.cpu().numpy(), want["count"])
    no_points = _query(pc, cen, r, s, point_cloud_range=rng, return_points=False)
    assert no_points.points is None and np.array_equal(no_points.index.cpu().numpy(), want["index"])


# ---- every refusal of the Python boundary word for word, and which of two faults is reported -----------------------------------------------------
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _centres(n=8, features=3, dtype=torch.float32):
    return torch.empty((2, n, features), dtype=dtype, device="cuda:0")


def _neighbour_out(*args, **kw):
    from lidar_snow_sim_amd.tensors import NeighbourBatch
    return NeighbourBatch.empty(2, 8, *args, **kw)


HOST_WORDS = "ball_query: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.ball.ball_query)"
CENTRE_WORDS = "ball_query: centres must be a KeypointBatch or a contiguous (frames, K, 3 .. 5) tensor in the rows' dtype on their device"
KEEP_WORDS = "keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)"
OUT_WORDS = "ball_query: out must be a NeighbourBatch whose %s tensor on the device of the rows"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)), HOST_WORDS),
    ("two radii, one count", lambda: dict(radius=(1.0, 2.0)), "ball_query: as many radii as sample counts"),
    ("n_neighbours 2.5", lambda: dict(n_neighbours=2.5), "ball_query: n_neighbours must be an integer"),
    ("num_features True", lambda: dict(num_features=True), "ball_query: num_features must be an integer"),
    ("range of 5", lambda: dict(point_cloud_range=(0, 0, 0, 4, 4)), "ball_query: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)"),
    ("centres of another dtype", lambda: dict(centres=_centres(dtype=torch.float64)), CENTRE_WORDS),
    ("num_features 6", lambda: dict(num_features=6), "ball_query: n_features must be 3, 4 or 5: the columns of a row that a neighbour carries"),
    ("centres of 6 columns", lambda: dict(centres=_centres(features=6)), "ball_query: centre_features must be 3, 4 or 5: x, y, z first"),
    ("no centre", lambda: dict(centres=_centres(0)), "ball_query: n_centres must be at least 1"),
    ("five radii", lambda: dict(radius=(1.0,) * 5, n_neighbours=(4,) * 5), "ball_query: n_radii must lie in 1 .. 4"),
    ("n_neighbours 65", lambda: dict(n_neighbours=65), "ball_query: the samples of a radius must lie in 1 .. 64"),
    ("2^31 slots", lambda: dict(centres=_centres(2 ** 22), radius=(1.0,) * 4, n_neighbours=(64,) * 4),
     "ball_query: n_frames * n_centres * samples exceeds 2^31 - 1; split the batch"),
    ("out of another shape", lambda: dict(out=_neighbour_out(5)), OUT_WORDS % "index is a contiguous (2, 8, 4) torch.int32"),
    ("out of another kind", lambda: dict(out=object()), OUT_WORDS % "index is a contiguous (2, 8, 4) torch.int32"),
    ("out of other radii", lambda: dict(out=_neighbour_out((2, 2))), OUT_WORDS % "count is a contiguous (2, 8, 1) torch.int32"),
    ("out without points", lambda: dict(out=_neighbour_out(4), return_points=True), OUT_WORDS % "points is a contiguous (2, 8, 4, 4) torch.float32"),
    # two faults: the earlier step of the call reports
    ("host rows before the radii", lambda: dict(frames=np.zeros((4, 5), np.float32), radius=(1.0, 2.0)), HOST_WORDS),
    ("the radii before a count", lambda: dict(radius=(1.0, 2.0), num_features=True), "ball_query: as many radii as sample counts"),
    ("a count before out", lambda: dict(n_neighbours=2.5, out=object()), "ball_query: n_neighbours must be an integer"),
    ("the device before the centres", lambda: dict(device=1, centres=_centres(dtype=torch.float64)), "the tensors live on cuda:0, device=1 was asked for"),
    ("keep before the centres", lambda: dict(keep=torch.ones(127, dtype=torch.bool, device="cuda:0"), centres=_centres(dtype=torch.float64)), KEEP_WORDS),
    ("the centres before the domain", lambda: dict(centres=_centres(dtype=torch.float64), num_features=6), CENTRE_WORDS),
    ("the domain before out", lambda: dict(n_neighbours=65, out=object()), "ball_query: the samples of a radius must lie in 1 .. 64"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    from lidar_snow_sim_amd.tensors import ball_query
    args = dict(frames=_pin_batch(), centres=_centres(), radius=1.0, n_neighbours=4)
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        ball_query(**args)


@pytest.mark.parametrize("overrides, words", ((dict(rng=(0, 0, 0, 4, 4)), "snowgpu_ball_query_device: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)"),
                                              (dict(radii=(1.0, 2.0)), "snowgpu_ball_query_device: as many radii as sample counts")), ids=("range of 5", "two radii, one count"))
def test_the_wrapper_refuses_word_for_word(overrides, words):
    from lidar_snow_sim_amd import engine
    args = dict(rng=None, radii=(1.0,))
    args.update(overrides)
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        engine.get_engine(0).ctx.ball_query_device(2, 128, 64, 0, 0, 0, args["rng"], 8, 0, 3, args["radii"], (4,), 4, 0, 0, 0, 0)
