"""-m gpu: the range image on the device (tensors.range_image, RangeImageBatch, range_image.project, snowgpu_range_image_device;
csrc/snowgpu_range.hip, csrc/sg_range.h) against the NumPy restatement of its definition (tests/range_reference.py, whose inputs
tests/test_range_reference.py holds to the conditions that keep these comparisons from being vacuous).  The outputs are integers, copied
bits and one correctly rounded value: every comparison is equality of bytes."""
import re

import numpy as np
import pytest
import torch

import range_reference as rr

pytestmark = pytest.mark.gpu

DTYPES = rr.DTYPES
FIELDS = ("image", "index", "pixel_of", "count")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _frames(rows, offsets):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(rows), offsets)


def _project(*args, **kw):
    from lidar_snow_sim_amd.tensors import range_image
    kw.setdefault("return_count", True)
    return range_image(*args, **kw)


def _run_case(name, dtype, by_ring=False, num_features=4, shape=None, limits=None, **kw):
    c = rr.case(name, dtype)
    H, W = shape or (c["H"], c["W"])
    return _project(_frames(c["rows"], c["offsets"]), H, W, fov_up=c["fov"][0], fov_down=c["fov"][1], ring=_t(c["ring"]) if by_ring else None,
                    range_limits=limits or c["limits"], keep=None if c["keep"] is None else _t(c["keep"]), num_features=num_features, **kw)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != want[name].tobytes():      # (bytes: NaN columns and -0.0 are copied as they are)
            bad = np.flatnonzero((g.view(np.uint8).reshape(g.size, -1) != want[name].view(np.uint8).reshape(g.size, -1)).any(axis=1))
            raise AssertionError((what, name, "first differing elements", bad[:8].tolist(), g.reshape(-1)[bad[:4]], want[name].reshape(-1)[bad[:4]]))


# ---- 1. the shared inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_ring", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", rr.CASES)
def test_shared_inputs_equal_the_restatement(name, dtype, by_ring):
    _same(_run_case(name, dtype, by_ring), rr.expected(name, dtype, by_ring), (name, dtype, by_ring))


@pytest.mark.parametrize("by_ring", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_frame_under_the_default_limits(dtype, by_ring):
    """hi = +inf: the rows beyond 1e6 are taken out by the finite clause alone, the origin by lo = 0."""
    _same(_run_case("constructed", dtype, by_ring, limits=rr.NO_LIMITS), rr.expected("constructed", dtype, by_ring, limits=rr.NO_LIMITS), (dtype, by_ring))


@pytest.mark.parametrize("by_ring", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", rr.SHAPES)
def test_image_shapes(shape, dtype, by_ring):
    """Frames of 37, 37, 0 and 8192 rows; pixel counts that divide no block size; one pixel for everything."""
    _same(_run_case("shapes", dtype, by_ring, shape=shape), rr.expected("shapes", dtype, by_ring, shape=shape), (shape, dtype, by_ring))


# ---- 2. the columns, the count ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("num_features", (3, 5))
def test_number_of_features(num_features, dtype):
    for name, by_ring in (("constructed", False), ("sweep", True)):
        _same(_run_case(name, dtype, by_ring, num_features), rr.expected(name, dtype, by_ring, num_features), (name, dtype, num_features))


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_the_count(dtype):
    for by_ring in (False, True):
        got = _run_case("constructed", dtype, by_ring, return_count=False)
        assert got.count is None
        _same(got, rr.expected("constructed", dtype, by_ring), (dtype, by_ring), FIELDS[:3])


# ---- 3. every element is written --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written(dtype):
    from lidar_snow_sim_amd.tensors import RangeImageBatch
    for name, by_ring in (("shapes", False), ("constructed", True), ("sweep", False)):
        c = rr.case(name, dtype)
        out = RangeImageBatch.empty(len(c["offsets"]) - 1, c["H"], c["W"], len(c["rows"]), 4, getattr(torch, dtype), with_count=True)
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        got = _run_case(name, dtype, by_ring, out=out)
        assert got is out
        _same(out, rr.expected(name, dtype, by_ring), (name, dtype))
    out = RangeImageBatch.empty(2, 3, 5, 0, 4, getattr(torch, dtype), with_count=True)          # a batch without a row
    for f in FIELDS:
        getattr(out, f).view(torch.uint8).fill_(0x7f)
    for ring in (None, torch.zeros(0, dtype=torch.int32, device="cuda")):
        got = _project(_frames(np.zeros((0, 5), dtype), np.zeros(3, np.int64)), 3, 5, ring=ring, out=out)
        assert got is out and bool((out.image == -1).all()) and bool((out.index == -1).all()) and not out.count.any() and out.pixel_of.numel() == 0


# ---- 4. the input mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_dtype", (torch.bool, torch.uint8))
@pytest.mark.parametrize("dtype", DTYPES)
def test_keep_equals_the_compacted_frames(dtype, mask_dtype):
    c = rr.case("sweep", dtype)
    rows, offsets, ring = c["rows"], c["offsets"], c["ring"]
    keep = np.random.default_rng(82).random(len(rows)) < 0.6
    for by_ring in (False, True):
        masked = _project(_frames(rows, offsets), 64, 96, ring=_t(ring) if by_ring else None, keep=_t(keep).to(mask_dtype))
        _same(masked, rr.project(rows, 64, 96, rr.FOV, ring if by_ring else None, rr.NO_LIMITS, 4, keep, offsets), (dtype, by_ring))
        parts = [_t(rows[a:b][keep[a:b]]) for a, b in zip(offsets[:-1], offsets[1:])]
        compact = _project(parts, 64, 96, ring=_t(ring[keep]) if by_ring else None)
        for f in ("image", "count"):
            assert torch.equal(getattr(masked, f).view(torch.uint8), getattr(compact, f).view(torch.uint8)), f
        back = np.flatnonzero(keep)                                          # compacted row -> row of the batch
        ci, po = compact.index.cpu().numpy(), masked.pixel_of.cpu().numpy()
        assert np.array_equal(masked.index.cpu().numpy(), np.where(ci >= 0, back[np.maximum(ci, 0)], -1)) and (ci >= 0).any()
        assert np.array_equal(po[keep], compact.pixel_of.cpu().numpy()) and (po[~keep] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_padded_batch_tensor(dtype):
    """F x Nmax x 5 with NaN padding behind every frame's rows and an F x Nmax mask."""
    c = rr.case("shapes", dtype)
    rows, offsets = c["rows"], c["offsets"]
    lens = np.diff(offsets)
    nmax = int(lens.max()) + 3
    batch = np.full((len(lens), nmax, 5), np.nan, dtype)
    mask = np.zeros((len(lens), nmax), bool)
    for f, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        batch[f, :b - a], mask[f, :b - a] = rows[a:b], True
    got = _project(_t(batch), 5, 67, keep=_t(mask))
    want = rr.expected("shapes", dtype)
    flat = np.flatnonzero(mask.reshape(-1))                                   # row of the compact batch -> row of the padded one
    assert torch.equal(got.image.view(torch.uint8), _t(want["image"]).view(torch.uint8)) and np.array_equal(got.count.cpu().numpy(), want["count"])
    assert np.array_equal(got.index.cpu().numpy(), np.where(want["index"] >= 0, flat[np.maximum(want["index"], 0)], -1))
    po = got.pixel_of.cpu().numpy()
    assert np.array_equal(po[flat], want["pixel_of"]) and (po[~mask.reshape(-1)] == -1).all()
    no_mask = _project(_t(batch), 5, 67)                                      # NaN rows are unusable by themselves
    assert torch.equal(no_mask.index, got.index) and torch.equal(no_mask.pixel_of, got.pixel_of)


# ---- 5. aligned results -----------------------------------------------------------------------------------------------------------------------
def _snowfall(tables):
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import augment_batch
    tl = [tables["t"][i % 4] for i in range(64)]
    plane, bd = (np.array([0.0, 0.0, -1.0]), -1.7), float(np.degrees(3e-3))
    frames = [np.ascontiguousarray(synthetic_sweep(64, 128, seed=1600 + k, intensity="lambert")) for k in range(2)]
    orders = [list(np.random.default_rng(3 + k).permutation(64)) for k in range(2)]
    ring = _t(np.concatenate(frames)[:, 4].astype(np.int32))                   # the INPUT's column 4
    return augment_batch([_t(f) for f in frames], "unused", bd, particles=tl, orders=orders, planes=[plane, plane], layout="aligned", sync=False), ring, frames


def test_an_aligned_result_equals_its_rows_and_mask(tables):
    res, ring, _ = _snowfall(tables)
    a = _project(res, 64, 96, ring=ring)
    b = _project(_frames(res.rows.cpu().numpy(), res.offsets), 64, 96, ring=ring, keep=res.keep)
    extra = torch.ones_like(res.keep, dtype=torch.bool)
    extra[::3] = False
    c = _project(res, 64, 96, keep=extra)
    d = _project(_frames(res.rows.cpu().numpy(), res.offsets), 64, 96, keep=res.keep.view(torch.bool) & extra)
    res.wait()
    assert int(a.count.sum()) > int(c.count.sum()) > 0
    for x, y in ((a, b), (c, d)):
        assert all(torch.equal(getattr(x, f).view(torch.uint8), getattr(y, f).view(torch.uint8)) for f in FIELDS)


def test_chain_behind_the_aligned_snowfall(tables):
    res, ring, frames = _snowfall(tables)
    got = _project(res, 64, 96, ring=ring)
    res.wait()
    rows, rk, src = res.rows.cpu().numpy(), res.keep.cpu().numpy().astype(bool), np.concatenate(frames)
    assert 500 < rk.sum() < len(rk) - 100
    want = rr.project(rows, 64, 96, rr.FOV, ring.cpu().numpy(), rr.NO_LIMITS, 4, rk, res.offsets)
    _same(got, want, "chain")
    # every scattered row that the result kept lies in the image row of its channel
    moved = rk & (rows[:, :3] != src[:, :3]).any(axis=1)
    po = got.pixel_of.cpu().numpy()
    assert moved.sum() >= 10 and (po[moved] >= 0).all()
    assert np.array_equal((po[moved] % (64 * 96)) // 96, src[moved, 4].astype(np.int64))
    sel = got.index.long().clamp(min=0)
    assert torch.equal(torch.where(got.index >= 0, res.rows[sel][..., 3], torch.full_like(got.image[:, 4], -1)), got.image[:, 4])     # rows[index] gathers


# ---- 6. run to run, graph capture ---------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    for name, dtype, by_ring in (("sweep", "float32", False), ("sweep", "float64", True), ("constructed", "float64", False)):
        a, b = _run_case(name, dtype, by_ring), _run_case(name, dtype, by_ring)
        for f in FIELDS:
            assert getattr(a, f).data_ptr() != getattr(b, f).data_ptr() and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), (name, f)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_capture(dtype):
    """range_image captured on one stream after a warm-up and replayed on other rows in the same tensor: the keys and every output are
    rewritten by the captured sequence itself.  A linear graph."""
    from lidar_snow_sim_amd.tensors import RangeImageBatch
    c = rr.case("sweep", dtype)
    clouds = [c["rows"][:8192], c["rows"][8192:]]
    want = [rr.project(x, 64, 96) for x in clouds]
    assert not np.array_equal(want[0]["index"], want[1]["index"])
    s = torch.cuda.Stream()
    rows = _t(clouds[0])
    out = RangeImageBatch.empty(1, 64, 96, 8192, 4, getattr(torch, dtype), with_count=True)
    with torch.cuda.stream(s):
        _project(rows, 64, 96, out=out)                                    # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = _project(rows, 64, 96, out=out)
        assert got is out
        snaps = []
        for k in (1, 0, 1):
            rows.copy_(_t(clouds[k]))
            for f in FIELDS:
                getattr(out, f).view(torch.uint8).fill_(0x7f)
            g.replay()
            snaps.append((k, {f: getattr(out, f).clone() for f in FIELDS}))
        s.synchronize()
    direct = _project(_t(clouds[1]), 64, 96)
    for k, snap in snaps:
        for f in FIELDS:
            assert snap[f].cpu().numpy().tobytes() == want[k][f].tobytes(), (k, f)
            assert k != 1 or torch.equal(snap[f].view(torch.uint8), getattr(direct, f).view(torch.uint8)), f


# ---- 7. the way back --------------------------------------------------------------------------------------------------------------------------
def test_to_rows():
    c = rr.case("shapes", "float32")
    got = _run_case("shapes", "float32")
    po, index = got.pixel_of.cpu().numpy(), got.index.cpu().numpy()
    back = got.to_rows(got.index, fill=-7).cpu().numpy()                     # every row learns who won its pixel
    won = index[index >= 0]
    assert np.array_equal(back[won], won) and (back[po < 0] == -7).all() and np.array_equal(back[po >= 0], index.reshape(-1)[po[po >= 0]])
    assert (po < 0).sum() >= 2 and (back[po >= 0] >= 0).all()
    planes = got.to_rows(got.image, fill=float("nan"))                        # (F, X, H, W) -> (N, X)
    assert planes.shape == (len(po), 5) and bool(torch.isnan(planes[torch.from_numpy(po < 0).cuda()]).all())
    assert torch.equal(planes[torch.from_numpy(won).cuda().long(), 1:], _t(c["rows"])[torch.from_numpy(won).cuda().long(), :4])
    with pytest.raises(ValueError, match="to_rows: values must be"):
        got.to_rows(got.index[0])


def test_a_per_pixel_mask_goes_back_into_the_snowfall(tables):
    """A de-noiser's per-pixel keep map becomes the keep mask of the next aligned call, without a host read."""
    from lidar_snow_sim_amd.tensors import augment_batch
    res, ring, frames = _snowfall(tables)
    img = _project(res, 64, 96, ring=ring)
    verdict = img.image[:, 0] < 30.0                                        # stands for the network: keep what is nearer than 30 m
    keep = img.to_rows(verdict, fill=False)
    assert keep.dtype == torch.bool and keep.shape == res.keep.shape
    tl = [tables["t"][i % 4] for i in range(64)]
    plane, bd = (np.array([0.0, 0.0, -1.0]), -1.7), float(np.degrees(3e-3))
    orders = [list(np.random.default_rng(3 + k).permutation(64)) for k in range(2)]
    again = augment_batch(_frames(res.rows.cpu().numpy(), res.offsets), "unused", bd, particles=tl, orders=orders, planes=[plane, plane], layout="aligned",
                          keep=keep, sync=False)
    again.wait()
    res.wait()
    k, po, v = keep.cpu().numpy(), img.pixel_of.cpu().numpy(), verdict.cpu().numpy().reshape(-1)
    assert np.array_equal(k, np.where(po >= 0, v[np.maximum(po, 0)], False)) and 100 < k.sum() < len(k) - 100
    assert not again.keep.cpu().numpy().astype(bool)[~k].any() and again.keep.cpu().numpy().astype(bool).any()


# ---- 8. the NumPy entry -----------------------------------------------------------------------------------------------------------------------
def test_numpy_entry():
    from lidar_snow_sim_amd.range_image import project
    for dtype in DTYPES:
        c = rr.case("constructed", dtype)
        rows = c["rows"][c["keep"]]
        for cols, C, by_ring in ((5, None, False), (3, None, True), (5, 4, True)):
            ring = c["ring"][c["keep"]] if by_ring else None
            want = rr.project(rows, 64, 96, rr.FOV, ring, c["limits"], C or cols)
            image, index, pixel_of, count = project(rows[:, :cols], 64, 96, ring=ring, range_limits=c["limits"], num_features=C, return_count=True)
            assert image.dtype == rows.dtype and index.dtype == np.int32 and pixel_of.dtype == np.int32 and count.dtype == np.int32
            assert image.tobytes() == want["image"][0].tobytes() and np.array_equal(index, want["index"][0])
            assert np.array_equal(pixel_of, want["pixel_of"]) and np.array_equal(count, want["count"][0])
        assert len(project(rows, 64, 96)) == 3
    with pytest.raises(ValueError):
        project(rows[:, :2], 64, 96)
    with pytest.raises(ValueError):
        project(rows[:, :3], 64, 96, num_features=4)
    with pytest.raises(ValueError):
        project(rows, 64, 96, ring=np.zeros(len(rows) - 1, np.int32))


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import RangeImageBatch
    c = rr.case("constructed")
    rows, n = c["rows"], len(c["rows"])
    pc, ring = _t(rows), _t(c["ring"])
    who = "snowgpu_range_image_device"
    for kw, words in ((dict(num_features=2), "n_features must be 3, 4 or 5"), (dict(num_features=6), "n_features must be 3, 4 or 5"),
                      (dict(height=0), "height and width must be at least 1"), (dict(width=-1), "height and width must be at least 1"),
                      (dict(height=2 ** 16, width=2 ** 15), "n_frames * height * width exceeds 2^31 - 1"), (dict(height=2.5), "integer"),
                      (dict(fov_up=-25.0, fov_down=3.0), who + ": the field of view needs fov_down < fov_up"),
                      (dict(fov_up=3.0, fov_down=3.0), who + ": the field of view needs fov_down < fov_up"),
                      (dict(fov_up=91.0), who + ": fov_up and fov_down must lie within [-pi/2, pi/2]"),
                      (dict(fov_down=float("nan")), who + ": fov_up and fov_down must lie within [-pi/2, pi/2]"),
                      (dict(range_limits=(float("nan"), 5.0)), who + ": a range limit is NaN"),
                      (dict(range_limits=(-1.0, 5.0)), who + ": the range limits need 0 <= lo < hi"),
                      (dict(range_limits=(5.0, 5.0)), who + ": the range limits need 0 <= lo < hi"),
                      (dict(range_limits=(0.0, 1.0, 2.0)), "range_limits holds 2 numbers"),
                      (dict(ring=ring[:-1]), "ring must be a contiguous int32 tensor"), (dict(ring=ring.long()), "ring must be a contiguous int32 tensor"),
                      (dict(ring=c["ring"]), "ring must be a contiguous int32 tensor")):
        args = dict(height=64, width=96)
        args.update(kw)
        with pytest.raises(ValueError, match=re.escape(words)):
            _project(pc, **args)
    _project(pc, 64, 96, fov_up=90.0, fov_down=-90.0)                        # the inner side of the fov's domain
    _project(pc, 64, 96, ring=ring, fov_up=float("nan"))                     # not read by channel
    with pytest.raises(ValueError, match="torch CUDA tensors"):
        _project(rows, 64, 96)
    with pytest.raises(ValueError):
        _project(pc, 64, 96, keep=torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError, match="out must be a RangeImageBatch whose count"):
        _project(pc, 64, 96, out=RangeImageBatch.empty(1, 64, 96, n))
    with pytest.raises(ValueError, match="out must be a RangeImageBatch whose image"):
        _project(pc, 64, 96, out=RangeImageBatch.empty(1, 64, 96, n, 5, with_count=True))
    with pytest.raises(ValueError, match="out must be a RangeImageBatch whose pixel_of"):
        _project(pc, 64, 96, out=RangeImageBatch.empty(1, 64, 96, n + 1, with_count=True))
    # the C entry refuses on its own: the overlaps, a null output and a call without a mode; the nullable output may be null
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    off = _t(np.array([0, n], np.int64))
    out = RangeImageBatch.empty(1, 64, 96, n, with_count=True)
    keep = torch.ones(n + 4096, dtype=torch.uint8, device="cuda:0")
    fov = np.radians(np.array(rr.FOV))
    args = (1, n, n, off.data_ptr(), pc.data_ptr(), 0, 64, 96)
    tail = (None, 4)
    with pytest.raises(ValueError, match="d_out_pixel_of overlaps d_keep_in"):
        ctx.range_image_device(*args, fov, 0, *tail, keep.data_ptr(), out.image.data_ptr(), out.index.data_ptr(), keep.data_ptr() + 8, out.count.data_ptr())
    with pytest.raises(ValueError, match="d_out_image overlaps d_rows"):
        ctx.range_image_device(*args, fov, 0, *tail, 0, pc.data_ptr(), out.index.data_ptr(), out.pixel_of.data_ptr(), out.count.data_ptr())
    with pytest.raises(ValueError, match="d_out_index overlaps d_ring"):             # (a 1 x 1 image: the index is the ring's last element)
        ctx.range_image_device(*args[:6], 1, 1, None, ring.data_ptr(), *tail, 0, out.image.data_ptr(), ring.data_ptr() + 4 * (n - 1), out.pixel_of.data_ptr(),
                               out.count.data_ptr())
    with pytest.raises(ValueError, match="d_out_count overlaps d_out_index; every output needs memory of its own"):
        ctx.range_image_device(*args, fov, 0, *tail, 0, out.image.data_ptr(), out.index.data_ptr(), out.pixel_of.data_ptr(), out.index.data_ptr() + 4)
    with pytest.raises(ValueError, match="null pointer or bad dtype"):
        ctx.range_image_device(*args, fov, 0, *tail, 0, out.image.data_ptr(), 0, out.pixel_of.data_ptr(), out.count.data_ptr())
    with pytest.raises(ValueError, match="needs fov2 .image rows by elevation. or d_ring"):
        ctx.range_image_device(*args, None, 0, *tail, 0, out.image.data_ptr(), out.index.data_ptr(), out.pixel_of.data_ptr(), out.count.data_ptr())
    want = rr.project(rows, 64, 96)
    for f in FIELDS[:3]:
        getattr(out, f).view(torch.uint8).fill_(9)
    ctx.range_image_device(*args, fov, 0, *tail, 0, out.image.data_ptr(), out.index.data_ptr(), out.pixel_of.data_ptr(), 0)
    torch.cuda.synchronize()
    _same(out, want, "no count", FIELDS[:3])


# ---- every refusal of the Python boundary word for word, and which of two faults is reported -----------------------------------------------------
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _image_out(*args, **kw):
    from lidar_snow_sim_amd.tensors import RangeImageBatch
    return RangeImageBatch.empty(2, *args, **kw)


HOST_WORDS = "range_image: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.range_image.project)"
RING_WORDS = "range_image: ring must be a contiguous int32 tensor with one element per row of the batch, on the device of the rows"
KEEP_WORDS = "keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)"
OUT_WORDS = "range_image: out must be a RangeImageBatch whose %s tensor on the device of the rows"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)), HOST_WORDS),
    ("height 2.5", lambda: dict(height=2.5), "range_image: height must be an integer"),
    ("width True", lambda: dict(width=True), "range_image: width must be an integer"),
    ("num_features 4.5", lambda: dict(num_features=4.5), "range_image: num_features must be an integer"),
    ("three limits", lambda: dict(range_limits=(0.0, 1.0, 2.0)), "range_image: range_limits holds 2 numbers (lo, hi)"),
    ("a short ring", lambda: dict(ring=torch.zeros(127, dtype=torch.int32, device="cuda:0")), RING_WORDS),
    ("a ring of int64", lambda: dict(ring=torch.zeros(128, dtype=torch.int64, device="cuda:0")), RING_WORDS),
    ("num_features 6", lambda: dict(num_features=6), "range_image: n_features must be 3, 4 or 5: the columns of a row that a pixel stores"),
    ("height 0", lambda: dict(height=0), "range_image: height and width must be at least 1"),
    ("2^31 pixels", lambda: dict(height=2 ** 15, width=2 ** 15), "range_image: n_frames * height * width exceeds 2^31 - 1; split the batch"),
    ("out of another shape", lambda: dict(out=_image_out(5, 8, 128)), OUT_WORDS % "image is a contiguous (2, 5, 4, 8) torch.float32"),
    ("out of another kind", lambda: dict(out=object()), OUT_WORDS % "image is a contiguous (2, 5, 4, 8) torch.float32"),
    ("out for other rows", lambda: dict(out=_image_out(4, 8, 127)), OUT_WORDS % "pixel_of is a contiguous (128,) torch.int32"),
    ("out without count", lambda: dict(out=_image_out(4, 8, 128), return_count=True), OUT_WORDS % "count is a contiguous (2, 4, 8) torch.int32"),
    # two faults: the earlier step of the call reports
    ("host rows before a count", lambda: dict(frames=np.zeros((4, 5), np.float32), height=2.5), HOST_WORDS),
    ("a count before the limits", lambda: dict(height=2.5, range_limits=(0.0,)), "range_image: height must be an integer"),
    ("the limits before the device", lambda: dict(range_limits=(0.0,), device=1), "range_image: range_limits holds 2 numbers (lo, hi)"),
    ("the device before the ring", lambda: dict(device=1, ring=torch.zeros(127, dtype=torch.int32, device="cuda:0")), "the tensors live on cuda:0, device=1 was asked for"),
    ("keep before the ring", lambda: dict(keep=torch.ones(127, dtype=torch.bool, device="cuda:0"), ring=torch.zeros(127, dtype=torch.int32, device="cuda:0")), KEEP_WORDS),
    ("the ring before the domain", lambda: dict(ring=torch.zeros(127, dtype=torch.int32, device="cuda:0"), height=0), RING_WORDS),
    ("the domain before out", lambda: dict(height=0, out=object()), "range_image: height and width must be at least 1"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    from lidar_snow_sim_amd.tensors import range_image
    args = dict(frames=_pin_batch(), height=4, width=8)
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        range_image(**args)


@pytest.mark.parametrize("fov, limits, words", (((0.1,), (0.0, 1.0), "snowgpu_range_image_device: fov holds 2 numbers"),
                                                ((0.1, -0.4), (0.0, 1.0, 2.0), "snowgpu_range_image_device: range_limits holds 2 numbers")), ids=("fov", "limits"))
def test_the_wrapper_refuses_a_pair_of_another_length_word_for_word(fov, limits, words):
    from lidar_snow_sim_amd import engine
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        engine.get_engine(0).ctx.range_image_device(2, 128, 64, 0, 0, 0, 4, 8, fov, 0, limits, 4, 0, 0, 0, 0, 0)
