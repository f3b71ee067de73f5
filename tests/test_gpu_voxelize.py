"""-m gpu: point-to-voxel grouping on the device (tensors.voxelize, voxel.points_to_voxels, snowgpu_voxelize_device;
csrc/snowgpu_voxel.hip, csrc/sg_voxel.h) against the sequential NumPy restatement of its definition (tests/voxel_reference.py, whose
inputs tests/test_voxel_reference.py holds to the conditions that keep these comparisons from being vacuous).  The outputs are integers
and copied bits: every comparison is equality."""
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
