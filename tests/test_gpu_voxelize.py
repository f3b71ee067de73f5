"""-m gpu: point-to-voxel grouping on the device (tensors.voxelize, voxel.points_to_voxels, snowgpu_voxelize_device;
csrc/snowgpu_voxel.hip, csrc/sg_voxel.h) against the sequential NumPy restatement of its definition (tests/voxel_reference.py, whose
inputs tests/test_voxel_reference.py holds to the conditions that keep these comparisons from being vacuous).  The outputs are integers
and copied bits: every comparison is equality."""
import re

import numpy as np
import pytest
import torch

import voxel_reference as vr

pytestmark = pytest.mark.gpu

DTYPES = vr.DTYPES
FIELDS = ("voxels", "coords", "num_points", "voxel_offsets", "voxel_of")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared inputs are read-only)


def _frames(rows, offsets):
    from lidar_snow_sim_amd.tensors import DeviceBatch
    return DeviceBatch(_t(rows), offsets)


def _voxelize(*args, **kw):
    from lidar_snow_sim_amd.tensors import voxelize
    return voxelize(*args, **kw)


def _run_case(name, dtype, num_features=4, max_points=None, max_voxels=None, **kw):
    rows, offsets, keep, (rng, size, T, V) = vr.case(name, dtype)
    T, V = (T if max_points is None else max_points), (V if max_voxels is None else max_voxels)
    return _voxelize(_frames(rows, offsets), rng, size, T, V, keep=None if keep is None else _t(keep), num_features=num_features,
                     return_voxel_of=True, **kw)


def _same(got, want, what, fields=FIELDS):
    for name in fields:
        g = getattr(got, name).cpu().numpy()
        assert g.dtype == want[name].dtype and g.shape == want[name].shape, (what, name, g.dtype, g.shape)
        assert g.tobytes() == want[name].tobytes(), (what, name)      # (bytes: NaN columns and -0.0 are copied as they are)


# ---- 1. every shared input --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", vr.CASES)
def test_shared_inputs_equal_the_restatement(name, dtype):
    _same(_run_case(name, dtype), vr.expected(name, dtype), (name, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", (dict(num_features=3), dict(num_features=5), dict(max_points=1), dict(max_voxels=1)), ids=str)
def test_edges_of_the_domain(variant, dtype):
    for name in ("constructed", "batch", "straddle"):
        _same(_run_case(name, dtype, **variant), vr.expected(name, dtype, **variant), (name, dtype, variant))


# ---- 2. every element is written --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_element_is_written(dtype):
    from lidar_snow_sim_amd.tensors import VoxelBatch
    for name in ("batch", "faces", "own_voxel"):
        rows, offsets, _, (_, _, T, V) = vr.case(name, dtype)
        out = VoxelBatch.empty(len(offsets) - 1, T, V, 4, getattr(torch, dtype), n_rows=len(rows))
        for f in FIELDS:
            getattr(out, f).view(torch.uint8).fill_(0x7f)
        got = _run_case(name, dtype, out=out)
        assert got is out
        _same(out, vr.expected(name, dtype), (name, dtype))


# ---- 3. the input mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_keep_equals_the_compacted_frames(dtype):
    rows, offsets, keep, (rng, size, T, V) = vr.case("batch", dtype)
    masked = _run_case("batch", dtype)
    parts = [_t(rows[a:b][keep[a:b]]) for a, b in zip(offsets[:-1], offsets[1:])]
    compact = _voxelize(parts, rng, size, T, V, return_voxel_of=True)
    for f in FIELDS[:4]:
        assert torch.equal(getattr(masked, f), getattr(compact, f)), f
    vo = masked.voxel_of.cpu().numpy()
    assert np.array_equal(vo[keep], compact.voxel_of.cpu().numpy()) and (vo[~keep] == -1).all()
    assert int(masked.voxel_offsets[-1]) >= 300
    # the mask as uint8, as a list per frame, and on an F x N x 5 tensor whose padding is NaN
    m8 = _voxelize(_frames(rows, offsets), rng, size, T, V, keep=_t(keep.astype(np.uint8)), return_voxel_of=True)
    assert all(torch.equal(getattr(masked, f), getattr(m8, f)) for f in FIELDS)
    sizes = (1000, 1500, 37)
    batch = np.full((3, 1500, 5), np.nan, rows.dtype)
    for f, n in enumerate(sizes):
        batch[f, :n] = rows[f * 13:f * 13 + n]
    pad = np.arange(1500)[None, :] < np.array(sizes)[:, None]
    want = vr.voxelize(batch.reshape(-1, 5), rng, size, T, V, 4, pad.reshape(-1), np.arange(4) * 1500)
    _same(_voxelize(_t(batch), rng, size, T, V, keep=_t(pad), return_voxel_of=True), want, "padded")
    _same(_voxelize(_t(batch), rng, size, T, V, return_voxel_of=True), want, "padded, no mask")      # NaN rows are unusable anyway


# ---- 4. the chain -----------------------------------------------------------------------------------------------------------------------------
def test_chain_behind_the_aligned_snowfall(tables):
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import augment_batch
    tl = [tables["t"][i % 4] for i in range(64)]
    plane, bd = (np.array([0.0, 0.0, -1.0]), -1.7), float(np.degrees(3e-3))
    frames = [np.ascontiguousarray(synthetic_sweep(64, 128, seed=1600 + k, intensity="lambert")) for k in range(2)]
    orders = [list(np.random.default_rng(3 + k).permutation(64)) for k in range(2)]
    res = augment_batch([_t(f) for f in frames], "unused", bd, particles=tl, orders=orders, planes=[plane, plane], layout="aligned", sync=False)
    rng, size, T, V = vr.PILLARS[0], vr.PILLARS[1], 32, 4000
    got = _voxelize(res, rng, size, T, V, return_voxel_of=True)
    res.wait()
    rows, rk = res.rows.cpu().numpy(), res.keep.cpu().numpy()
    assert 500 < rk.sum() < len(rk) - 100 and int((rows[rk][:, 4] == 2).sum()) > 5      # rows were removed, and rows were scattered
    kept_off = np.concatenate(([0], np.cumsum([rk[a:b].sum() for a, b in zip(res.offsets[:-1], res.offsets[1:])])))
    want = vr.voxelize(rows[rk], rng, size, T, V, 4, None, kept_off)
    _same(got, want, "chain", FIELDS[:4])
    vo = got.voxel_of.cpu().numpy()
    assert np.array_equal(vo[rk], want["voxel_of"]) and (vo[~rk] == -1).all()
    assert want["voxel_offsets"][1] >= 500 and want["voxel_offsets"][2] - want["voxel_offsets"][1] >= 500
    per_frame = got.frames()
    assert len(per_frame) == 2 and [int(v.shape[0]) for v, _, _ in per_frame] == list(np.diff(want["voxel_offsets"]))
    assert all(int(c[:, 0].min()) == int(c[:, 0].max()) == f for f, (_, c, _) in enumerate(per_frame))


# ---- 5. run to run ----------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    for name in ("batch", "straddle"):
        a, b = _run_case(name, "float32"), _run_case(name, "float32")
        for f in FIELDS:
            assert getattr(a, f).data_ptr() != getattr(b, f).data_ptr() and torch.equal(getattr(a, f).view(torch.uint8), getattr(b, f).view(torch.uint8)), (name, f)


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture():
    """voxelize(..., out=batch) captured on one stream after a warm-up and replayed on other rows in the same tensor: the tables, the
    voxels and every tail are rewritten by the captured sequence itself."""
    from lidar_snow_sim_amd.tensors import VoxelBatch
    names = ("straddle", "straddle_firing")
    clouds = [vr.case(n)[0] for n in names]
    rng, size, T, V = vr.case(names[0])[3]
    want = [vr.expected(n) for n in names]
    assert clouds[0].shape == clouds[1].shape and not np.array_equal(want[0]["coords"], want[1]["coords"])
    s = torch.cuda.Stream()
    rows = _t(clouds[0])
    out = VoxelBatch.empty(1, T, V, 4, torch.float32, n_rows=len(rows))
    with torch.cuda.stream(s):
        _voxelize(rows, rng, size, T, V, out=out, return_voxel_of=True)      # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            got = _voxelize(rows, rng, size, T, V, out=out, return_voxel_of=True)
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
    from lidar_snow_sim_amd.voxel import points_to_voxels
    for dtype in DTYPES:
        rows, _, _, (rng, size, T, V) = vr.case("constructed", dtype)
        for cols, C in ((5, None), (4, None), (3, None), (5, 4)):
            want = vr.expected("constructed", dtype, num_features=C or cols)
            m = int(want["voxel_offsets"][1])
            voxels, coords, num = points_to_voxels(rows[:, :cols], rng, size, T, V, num_features=C)
            assert voxels.dtype == rows.dtype and coords.dtype == np.int32 and num.dtype == np.int32
            assert voxels.tobytes() == want["voxels"][:m].tobytes() and np.array_equal(coords, want["coords"][:m, 1:]) and np.array_equal(num, want["num_points"][:m])
    with pytest.raises(ValueError):
        points_to_voxels(rows[:, :2], rng, size, T, V)
    with pytest.raises(ValueError):
        points_to_voxels(rows[:, :3], rng, size, T, V, num_features=4)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from lidar_snow_sim_amd.tensors import VoxelBatch
    rows, _, _, (rng, size, T, V) = vr.case("faces")
    pc, n = _t(rows), len(rows)
    who = "snowgpu_voxelize_device"
    for kw, words in ((dict(num_features=2), "n_features must be 3, 4 or 5"), (dict(num_features=6), "n_features must be 3, 4 or 5"),
                      (dict(max_points=0), "at least 1"), (dict(max_voxels=0), "at least 1"), (dict(max_voxels=2 ** 31), "exceeds 2\\^31 - 1"),
                      (dict(voxel_size=(1.0, 0.0, 1.0)), who + ": every voxel size must be positive and finite"),
                      (dict(voxel_size=(1.0, float("nan"), 1.0)), who + ": every voxel size"),
                      (dict(point_cloud_range=(0, 0, 0, 0.25, 1, 1)), who + ": the range must be finite and hold at least one voxel"),
                      (dict(point_cloud_range=(0, 0, 0, float("inf"), 1, 1)), who + ": the range must be finite"),
                      (dict(point_cloud_range=(0, 0, 0, 2 ** 31 - 1, 1, 1)), who + ": the grid has more than 2\\^31 - 2 cells"),
                      (dict(point_cloud_range=(0, 0, 0, 1, 1)), "6 numbers"), (dict(max_points=2.5), "integer")):
        args = dict(point_cloud_range=rng, voxel_size=size, max_points=T, max_voxels=V)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            _voxelize(pc, **args)
    with pytest.raises(ValueError, match="torch CUDA tensors"):
        _voxelize(rows, rng, size, T, V)
    with pytest.raises(ValueError):
        _voxelize(pc, rng, size, T, V, keep=torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError):
        _voxelize(pc, rng, size, T, V, keep=np.ones(n, bool))
    with pytest.raises(ValueError, match="out must be a VoxelBatch whose voxel_of"):
        _voxelize(pc, rng, size, T, V, out=VoxelBatch.empty(1, T, V), return_voxel_of=True)
    with pytest.raises(ValueError, match="out must be a VoxelBatch whose voxels"):
        _voxelize(pc, rng, size, T, V, out=VoxelBatch.empty(1, T + 1, V))
    with pytest.raises(ValueError, match="out must be a VoxelBatch whose voxels"):
        _voxelize(pc, rng, size, T, V, out=VoxelBatch.empty(1, T, V, dtype=torch.float64))
    # the C entry refuses on its own: the overlap, and a null output
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    off = _t(np.array([0, n], np.int64))
    out = VoxelBatch.empty(1, T, V, n_rows=n)
    ptrs = (out.voxels.data_ptr(), out.coords.data_ptr(), out.num_points.data_ptr(), out.voxel_offsets.data_ptr())
    with pytest.raises(ValueError, match="d_out_voxel_of overlaps d_keep_in"):
        ctx.voxelize_device(1, n, n, off.data_ptr(), pc.data_ptr(), 0, rng, size, T, V, 4, out.voxel_of.data_ptr() + 8, *ptrs, out.voxel_of.data_ptr())
    with pytest.raises(ValueError, match="null pointer or bad dtype"):
        ctx.voxelize_device(1, n, n, off.data_ptr(), pc.data_ptr(), 0, rng, size, T, V, 4, 0, ptrs[0], 0, ptrs[2], ptrs[3])
    torch.cuda.synchronize()
    # an empty batch: offsets of zero, and the tails in every output
    out.voxel_offsets.fill_(9)
    ctx.voxelize_device(1, 0, 0, off.data_ptr(), 0, 0, rng, size, T, V, 4, 0, 0, 0, 0, out.voxel_offsets.data_ptr())
    assert out.voxel_offsets.tolist() == [0, 0]
    empty = _voxelize(pc[:0], rng, size, T, V, return_voxel_of=True)
    assert empty.voxel_offsets.tolist() == [0, 0] and not empty.voxels.any() and bool((empty.coords == -1).all()) and not empty.num_points.any()
    assert empty.voxel_of.shape == (0,) and [tuple(v.shape) for v in empty.frames()[0]] == [(0, T, 4), (0, 4), (0,)]


# ---- 9. every refusal of the Python boundary word for word, and which of two faults is reported --------------------------------------------------
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _short_keep():
    return torch.ones(127, dtype=torch.bool, device="cuda:0")


def _voxel_out(**kw):
    from lidar_snow_sim_amd.tensors import VoxelBatch
    return VoxelBatch.empty(2, **kw)


KEEP_WORDS = "keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)"
DEVICE_WORDS = "the tensors live on cuda:0, device=1 was asked for"
OUT_WORDS = "voxelize: out must be a VoxelBatch whose %s tensor on the device of the rows"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)),
     "voxelize: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.voxel.points_to_voxels)"),
    ("max_points 2.5", lambda: dict(max_points=2.5), "voxelize: max_points must be an integer"),
    ("max_voxels True", lambda: dict(max_voxels=True), "voxelize: max_voxels must be an integer"),
    ("num_features 4.5", lambda: dict(num_features=4.5), "voxelize: num_features must be an integer"),
    ("range of 5", lambda: dict(point_cloud_range=(0, 0, 0, 4, 4)), "voxelize: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1), voxel_size 3"),
    ("size of 2", lambda: dict(voxel_size=(1, 1)), "voxelize: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1), voxel_size 3"),
    ("num_features 6", lambda: dict(num_features=6), "voxelize: n_features must be 3, 4 or 5: the columns of a row that a voxel stores"),
    ("max_points 0", lambda: dict(max_points=0), "voxelize: max_points and max_voxels must be at least 1"),
    ("max_voxels 2^31", lambda: dict(max_voxels=2 ** 31), "voxelize: n_frames * max_voxels exceeds 2^31 - 1; split the batch"),
    ("out of another shape", lambda: dict(out=_voxel_out(max_points=5, max_voxels=8)), OUT_WORDS % "voxels is a contiguous (16, 4, 4) torch.float32"),
    ("out of another kind", lambda: dict(out=object()), OUT_WORDS % "voxels is a contiguous (16, 4, 4) torch.float32"),
    ("out without voxel_of", lambda: dict(out=_voxel_out(max_points=4, max_voxels=8), return_voxel_of=True), OUT_WORDS % "voxel_of is a contiguous (128,) torch.int32"),
    # two faults: the earlier step of the call reports
    ("host rows before a count", lambda: dict(frames=np.zeros((4, 5), np.float32), max_points=2.5),
     "voxelize: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.voxel.points_to_voxels)"),
    ("a count before out", lambda: dict(max_points=2.5, out=object()), "voxelize: max_points must be an integer"),
    ("the device before the domain", lambda: dict(device=1, max_points=0), DEVICE_WORDS),
    ("keep before the domain", lambda: dict(keep=_short_keep(), num_features=6), KEEP_WORDS),
    ("the domain before out", lambda: dict(max_points=0, out=object()), "voxelize: max_points and max_voxels must be at least 1"),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    args = dict(frames=_pin_batch(), point_cloud_range=(0, 0, 0, 4, 4, 4), voxel_size=(1, 1, 1), max_points=4, max_voxels=8)
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        _voxelize(**args)


def test_the_wrapper_refuses_a_short_range_word_for_word():
    from lidar_snow_sim_amd import engine
    with pytest.raises(ValueError, match="^" + re.escape("snowgpu_voxelize_device: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1), voxel_size 3") + "$"):
        engine.get_engine(0).ctx.voxelize_device(2, 128, 64, 0, 0, 0, (0, 0, 0, 4, 4), (1, 1, 1), 4, 8, 4, 0, 0, 0, 0, 0)
