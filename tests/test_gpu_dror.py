"""-m gpu: dynamic radius outlier removal on the device (tensors.dror_keep, dror.dynamic_radius_outlier_filter,
snowgpu_dror_mask_device; csrc/snowgpu_dror.hip, csrc/sg_dror.h) against the float64 NumPy restatement of its definition
(tests/dror_reference.py, held to SciPy's kd-tree by tests/test_dror_reference.py).  Masks and counts are integers: every comparison is
equality."""
import re

import numpy as np
import pytest
import torch

import dror_reference as dr

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float64")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # (a copy: the shared clouds are read-only)


def _keep(frames, *args, **kw):
    from lidar_snow_sim_amd.tensors import dror_keep
    return dror_keep(frames, *args, **kw)


def _same(got, want, what):
    keep, nb = got
    assert keep.dtype == torch.bool and nb.dtype == torch.int32
    assert np.array_equal(keep.cpu().numpy(), want[0]), what
    assert np.array_equal(nb.cpu().numpy(), want[1]), what


# ---- 1. clouds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("setting", dr.SETTINGS)
def test_clouds_equal_the_restatement(setting, dtype):
    alpha, beta, k_min, sr_min = setting
    for name in dr.cloud_names(setting):
        pc = dr.cloud(name, dtype)
        want = dr.expected(name, dtype, setting)
        _same(_keep(_t(pc), alpha, beta, k_min, sr_min, return_neighbours=True), want, (name, setting))
        # k_min = 1000: nothing saturates -- the full counts, and every row dropped; k_min = 0: every usable row kept
        keep, nb = _keep(_t(pc), alpha, beta, 1000, sr_min, return_neighbours=True)
        assert want[2].max() < 1000 and not bool(keep.any()) and np.array_equal(nb.cpu().numpy(), want[2]), name
        keep, nb = _keep(_t(pc), alpha, beta, 0, sr_min, return_neighbours=True)
        assert bool(keep.all()) and not bool(nb.any()), name


# ---- 2. the constructed frame -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_constructed_frame(dtype):
    pc, info = dr.constructed_frame(np.dtype(dtype).type)
    want = dr.dror(pc)
    xyz = np.asarray(pc[:, :3], np.float64)
    s2, _ = dr.search_radius2(xyz, 0.45, 3, 0.04)
    a, b = np.array([p[0] for p in info["pairs"]]), np.array([p[1] for p in info["pairs"]])
    d = xyz[b] - xyz[a]
    inside = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= s2[a]
    assert inside.sum() >= 100 and (~inside).sum() >= 100
    with np.errstate(invalid="ignore"):
        _same(_keep(_t(pc), return_neighbours=True), want, dtype)
        keep, nb = _keep(_t(pc), k_min=1000, return_neighbours=True)
    nb = nb.cpu().numpy()
    assert np.array_equal(nb, want[2])
    assert not keep[info["unusable"]].any().item() and not nb[info["unusable"]].any()
    assert np.all(nb[info["dups"]] == 4)                       # the five duplicates count each other, and none of the eight unusable rows beside them


# ---- 3. frames stay apart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_frames_stay_apart(dtype):
    """Frames of 0, 1, 2, 1 023, 1 024, 1 025 and 4 096 rows, all the first rows of ONE cloud: a neighbour that leaked over a frame's
    border would be counted.  Every frame equals its own call and the restatement."""
    pc = dr.cloud("sector2", dtype)
    sizes = (0, 1, 2, 1023, 1024, 1025, 4096)
    frames = [np.ascontiguousarray(pc[:n]) for n in sizes]
    offsets = np.concatenate(([0], np.cumsum(sizes)))
    want = dr.dror(np.concatenate(frames), offsets=offsets)
    keep, nb = _keep([_t(f) for f in frames], return_neighbours=True)
    _same((keep, nb), want, dtype)
    for f, (lo, hi) in zip(frames, zip(offsets[:-1], offsets[1:])):
        if len(f):
            k1, n1 = _keep(_t(f), return_neighbours=True)
            assert torch.equal(k1, keep[lo:hi]) and torch.equal(n1, nb[lo:hi]), len(f)
    assert 0 < int(keep[offsets[3]:offsets[4]].sum()) < int(keep[offsets[6]:].sum())
    full = _keep(_t(np.concatenate(frames)))                 # as ONE frame every row of the 1 023 has three copies beside it
    assert bool(full[offsets[3]:offsets[4]].all())


# ---- 4. the input mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_input_mask(dtype):
    pc = dr.cloud("sector5", dtype)
    m = np.random.default_rng(11).random(len(pc)) < 0.5
    want = dr.dror(pc[m])
    for mask in (_t(m), _t(m.astype(np.uint8)), [_t(m)]):
        keep, nb = _keep(_t(pc), keep=mask, return_neighbours=True)
        keep, nb = keep.cpu().numpy(), nb.cpu().numpy()
        assert np.array_equal(keep[m], want[0]) and np.array_equal(nb[m], want[1])
        assert not keep[~m].any() and not nb[~m].any()
    # an F x Nmax batch whose padding is NaN
    sizes = (1000, 4000, 37)
    batch = np.full((3, 4096, 5), np.nan, pc.dtype)
    for f, n in enumerate(sizes):
        batch[f, :n] = pc[f * 13:f * 13 + n]
    lengths = torch.tensor(sizes, device="cuda:0")
    pad = torch.arange(4096, device="cuda:0")[None, :] < lengths[:, None]
    keep, nb = _keep(_t(batch), keep=pad, return_neighbours=True)
    keep, nb = keep.cpu().numpy().reshape(3, 4096), nb.cpu().numpy().reshape(3, 4096)
    for f, n in enumerate(sizes):
        want = dr.dror(batch[f, :n])
        assert np.array_equal(keep[f, :n], want[0]) and np.array_equal(nb[f, :n], want[1]), f
        assert not keep[f, n:].any() and not nb[f, n:].any(), f
    nomask = _keep(_t(batch)).cpu().numpy().reshape(3, 4096)  # NaN rows are unusable with or without the mask
    assert np.array_equal(nomask, keep)


# ---- 5. the chain -----------------------------------------------------------------------------------------------------------------------------
def test_chain_with_the_aligned_snowfall(tables):
    """DROR in front: augment_batch(layout='aligned', keep=dror_keep(...)) is the aligned call on the frames the test compacted with that
    mask.  DROR behind: dror_keep(res.rows, keep=res.keep) is the restatement on res.rows[res.keep]."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import augment_batch
    tl = [tables["t"][i % 4] for i in range(64)]
    plane, bd = (np.array([0.0, 0.0, -1.0]), -1.7), float(np.degrees(3e-3))
    pc = np.ascontiguousarray(synthetic_sweep(64, 128, seed=1600, intensity="lambert"))
    order = [list(np.random.default_rng(3).permutation(64))]
    setting = (1.0, 3, 3, 0.04)
    mask = _keep(_t(pc), *setting)
    m = mask.cpu().numpy()
    assert np.array_equal(m, dr.dror(pc, *setting)[0]) and 500 < m.sum() < len(pc) - 500
    kw = dict(particles=tl, orders=order, planes=[plane], layout="aligned")
    (s1, rows, keep), = augment_batch(_t(pc), "unused", bd, keep=mask, **kw)
    (s0, r0, k0), = augment_batch(_t(pc[m]), "unused", bd, **kw)
    rows, keep = rows.cpu().numpy(), keep.cpu().numpy()
    assert tuple(int(v) for v in s1) == tuple(int(v) for v in s0)
    assert rows[m].tobytes() == r0.cpu().numpy().tobytes() and np.array_equal(keep[m], k0.cpu().numpy()) and not keep[~m].any()
    assert int((r0[:, 4] == 2).sum()) > 5
    # behind the weather: how much of the augmented sweep a de-noiser takes out again
    res = augment_batch(_t(pc), "unused", bd, sync=False, **kw)
    after = _keep(res.rows, *setting, keep=res.keep, return_neighbours=True)
    res.wait()
    rk = res.keep.cpu().numpy()
    want = dr.dror(res.rows.cpu().numpy()[rk], *setting)
    assert np.array_equal(after[0].cpu().numpy()[rk], want[0]) and np.array_equal(after[1].cpu().numpy()[rk], want[1])
    assert not after[0].cpu().numpy()[~rk].any() and 0 < want[0].sum() < rk.sum()


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture():
    """dror_keep(..., out=mask) captured after a warm-up and replayed on new rows in the same tensor: the cell counters are cleared by
    the captured sequence itself."""
    inputs = [dr.cloud("sector1"), dr.cloud("sector4"), dr.cloud("sector1")]
    want = [dr.expected(n, "float32", dr.SETTINGS[0]) for n in ("sector1", "sector4", "sector1")]
    assert not np.array_equal(want[0][0], want[1][0])
    s = torch.cuda.Stream()
    rows = _t(inputs[0])
    mask = torch.zeros(len(rows), dtype=torch.bool, device="cuda:0")
    with torch.cuda.stream(s):
        _keep(rows, out=mask)                                   # warm-up: the captured call allocates nothing
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = _keep(rows, out=mask)
        assert out is mask
        got = []
        for inp in (inputs[1], inputs[2], inputs[0]):
            rows.copy_(_t(inp))
            g.replay()
            got.append(mask.clone())
        s.synchronize()
    for k, w in zip(got, (want[1], want[2], want[0])):
        assert np.array_equal(k.cpu().numpy(), w[0])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    pc = _t(dr.cloud("sector0"))
    n = len(pc)
    for kw in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=5.0, beta=3), dict(alpha=float("nan")), dict(sr_min=-0.01), dict(sr_min=float("inf")),
               dict(sr_min=float("nan")), dict(k_min=-1), dict(k_min=65536), dict(k_min=2.5)):
        with pytest.raises(ValueError):
            _keep(pc, **kw)
    m = torch.ones(n, dtype=torch.bool, device="cuda:0")
    with pytest.raises(ValueError, match="overlap"):
        _keep(pc, keep=m, out=m)
    with pytest.raises(ValueError):
        _keep(pc, keep=m[:-1])
    with pytest.raises(ValueError):
        _keep(pc, out=torch.ones(n - 1, dtype=torch.bool, device="cuda:0"))
    with pytest.raises(ValueError):
        _keep(dr.cloud("sector0"))
    with pytest.raises(ValueError):
        _keep(pc, keep=np.ones(n, bool))
    # the C entry refuses the same on its own
    from lidar_snow_sim_amd import engine
    ctx = engine.get_engine(0).ctx
    off = _t(np.array([0, n], np.int64))
    out = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    for a, b, sr, k, ki, ko in ((5.0, 3.0, 0.04, 3, 0, out), (0.45, 3.0, -1.0, 3, 0, out), (0.45, 3.0, 0.04, 65536, 0, out), (0.45, 3.0, 0.04, 3, m, m),
                                (0.45, 3.0, 0.04, 3, m, m[1:])):
        with pytest.raises(ValueError):
            ctx.dror_mask_device(1, n, n, off.data_ptr(), pc.data_ptr(), 0, a, b, sr, k, 0 if isinstance(ki, int) else ki.data_ptr(), ko.data_ptr())
    torch.cuda.synchronize()
    ctx.dror_mask_device(1, 0, 0, off.data_ptr(), 0, 0, 0.45, 3.0, 0.04, 3, 0, 0)       # an empty batch: OK, nothing launched
    assert _keep(pc[:0]).shape == (0,)


# ---- 8. the NumPy entry -----------------------------------------------------------------------------------------------------------------------
def test_numpy_entry():
    from lidar_snow_sim_amd.dror import dynamic_radius_outlier_filter
    pc = dr.cloud("sector1")
    want = dr.expected("sector1", "float32", dr.SETTINGS[0])[0]
    for arr in (pc[:, :3], pc, pc.astype(np.float64)[:, :3]):
        got = dynamic_radius_outlier_filter(arr)
        assert got.dtype == np.bool_ and np.array_equal(got, want)
    got = dynamic_radius_outlier_filter(pc[:, :3], 0.16, 3, 3, 0.04)
    assert np.array_equal(got, dr.expected("sector1", "float32", dr.SETTINGS[1])[0])


# ---- every refusal of the Python boundary word for word, and which of two faults is reported -----------------------------------------------------
def _pin_batch():
    """Two float32 frames of 64 rows."""
    from lidar_snow_sim_amd.tensors import DeviceBatch
    rows = (torch.arange(640, dtype=torch.float32, device="cuda:0").reshape(128, 5) % 17) / 4
    return DeviceBatch(rows, np.array([0, 64, 128], np.int64))


def _mask(n=128, dtype=torch.bool):
    return torch.ones(n, dtype=dtype, device="cuda:0")


def _out_is_keep():
    m = _mask()
    return dict(keep=m, out=m)


HOST_WORDS = "dror_keep: torch CUDA tensors or an aligned result (host arrays: lidar_snow_sim_amd.dror.dynamic_radius_outlier_filter)"
OUT_WORDS = "dror_keep: out must be a contiguous torch.bool tensor with one element per row, on the device of the rows"
KEEP_WORDS = "keep must have one element per row of the batch (N_total, F x N, or a list of per-frame tensors)"
PINNED = (
    ("host rows", lambda: dict(frames=np.zeros((4, 5), np.float32)), HOST_WORDS),
    ("alpha 0", lambda: dict(alpha=0.0), "dror_keep: beta * radians(alpha) must lie in (0, 0.25]"),
    ("beta 40", lambda: dict(beta=40), "dror_keep: beta * radians(alpha) must lie in (0, 0.25]"),
    ("sr_min -1", lambda: dict(sr_min=-1.0), "dror_keep: sr_min must be finite and >= 0"),
    ("sr_min inf", lambda: dict(sr_min=float("inf")), "dror_keep: sr_min must be finite and >= 0"),
    ("k_min 2.5", lambda: dict(k_min=2.5), "dror_keep: k_min must be an integer in 0 .. 65535"),
    ("k_min 65536", lambda: dict(k_min=65536), "dror_keep: k_min must be an integer in 0 .. 65535"),
    ("a short out", lambda: dict(out=_mask(127)), OUT_WORDS),
    ("out of uint8", lambda: dict(out=_mask(dtype=torch.uint8)), OUT_WORDS),
    ("out is keep", _out_is_keep, "dror_keep: out must not be (or overlap) the keep tensor; the query of one row reads other rows' keep elements"),
    # two faults: the earlier step of the call reports
    ("host rows before alpha", lambda: dict(frames=np.zeros((4, 5), np.float32), alpha=0.0), HOST_WORDS),
    ("alpha before sr_min", lambda: dict(alpha=0.0, sr_min=-1.0), "dror_keep: beta * radians(alpha) must lie in (0, 0.25]"),
    ("sr_min before k_min", lambda: dict(sr_min=-1.0, k_min=2.5), "dror_keep: sr_min must be finite and >= 0"),
    ("k_min before the device", lambda: dict(k_min=2.5, device=1), "dror_keep: k_min must be an integer in 0 .. 65535"),
    ("the device before out", lambda: dict(device=1, out=_mask(127)), "the tensors live on cuda:0, device=1 was asked for"),
    ("keep before out", lambda: dict(keep=_mask(127), out=_mask(127)), KEEP_WORDS),
)


@pytest.mark.parametrize("overrides, words", [c[1:] for c in PINNED], ids=[c[0] for c in PINNED])
def test_every_refusal_word_for_word(overrides, words):
    from lidar_snow_sim_amd.tensors import dror_keep
    args = dict(frames=_pin_batch())
    args.update(overrides())
    with pytest.raises(ValueError, match="^" + re.escape(words) + "$"):
        dror_keep(**args)
