"""-m gpu: the INPUT keep mask of the aligned snowfall entry (augment_batch(..., layout='aligned', keep=mask),
snowgpu_augment_batch_device_aligned_masked; csrc/snowgpu_mask.hip: k_mask_count / k_mask_scan / k_mask_offsets, k_finish_aligned_masked,
k_fov_mask) and of the fused aligned chain.

The reference for byte equality is the unmasked aligned call of the same library on the frames the TEST compacted (f[m]), which
tests/test_gpu_aligned.py holds to the oracle: present rows, keep bytes, statistics, counts and the fitted polynomials are byte-equal,
absent rows come back with the input's bytes and keep 0.  Inputs and their claimed properties: tests/aligned_mask_inputs.py, checked
without a GPU by tests/test_aligned_mask_inputs.py."""
import numpy as np
import pytest
import torch

import aligned_mask_inputs as ami

pytestmark = pytest.mark.gpu

PLANE, BD = ami.PLANE, ami.BD


@pytest.fixture(scope="module")
def eng():
    from lidar_snow_sim_amd import engine
    return engine.get_engine(0)


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    snow_oracle.build()
    return snow_oracle


@pytest.fixture(scope="module")
def tl(tables):
    return [tables["t"][i % 4] for i in range(64)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats(st):
    return tuple(int(v) for v in st)


def _orders(nf, seed):
    return [list(np.random.default_rng(seed + f).permutation(64)) for f in range(nf)]


def _compacted_reference(frames, masks, tl, **kw):
    """The unmasked aligned call on the frames compacted by the test: per frame (stats, rows, keep) as NumPy."""
    from lidar_snow_sim_amd.tensors import augment_batch
    ref = augment_batch([_t(f[m]) for f, m in zip(frames, masks)], "unused", BD, particles=tl, layout="aligned", **kw)
    return [(_stats(s), r.cpu().numpy(), k.cpu().numpy()) for s, r, k in ref]


def _same_as_compacted(got, ref, frames, masks):
    """got: per frame (stats, rows, keep) of a masked call (tensors or NumPy).  Returns (scattered, removed) over the present rows."""
    assert len(got) == len(ref) == len(frames)
    scattered = removed = 0
    for f, ((s1, rows, keep), (s0, r0, k0)) in enumerate(zip(got, ref)):
        m = masks[f]
        r = rows.cpu().numpy() if torch.is_tensor(rows) else rows
        k = keep.cpu().numpy() if torch.is_tensor(keep) else keep
        assert r.dtype == frames[f].dtype and r.shape == frames[f].shape and k.dtype == np.bool_ and k.shape == m.shape, f
        assert _stats(s1) == s0, (f, s1, s0)
        assert r[m].tobytes() == r0.tobytes(), f
        assert np.array_equal(k[m], k0), f
        assert not k[~m].any(), f
        assert r[~m].tobytes() == frames[f][~m].tobytes(), f
        scattered += int((r0[k0, 4] == 2).sum())
        removed += int((~k0).sum())
    return scattered, removed


def _raw(eng, rows, offsets, tids, keep=None, plane=None, poly=None, out=None, out_keep=None, perm=None):
    """snowgpu_augment_batch_device_aligned_masked through the ctypes binding on the context's own stream (keep=None: the unmasked
    entry it forwards to): (out rows, out keep, counts, stats, out_thr_poly, status), waited for."""
    dev = rows.device
    nf, n = len(offsets) - 1, int(offsets[-1])
    d_off = torch.from_numpy(np.asarray(offsets, np.int64)).to(dev)
    out = torch.empty_like(rows) if out is None else out
    ok = torch.empty(n, dtype=torch.bool, device=dev) if out_keep is None else out_keep
    cnt, st = torch.zeros(nf, dtype=torch.int64, device=dev), torch.zeros(nf, 3, dtype=torch.int64, device=dev)
    thr, status = torch.zeros(nf, 3, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()   # noqa: E731
    torch.cuda.synchronize()
    eng.ctx.augment_batch_device_aligned_masked(nf, n, int(np.diff(offsets).max()), d_off.data_ptr(), rows.data_ptr(), 0 if rows.dtype == torch.float32 else 1,
                                                tids.data_ptr(), BD, ptr(poly), ptr(plane), 0.7, ptr(perm), ptr(keep), out.data_ptr(), ok.data_ptr(),
                                                cnt.data_ptr(), st.data_ptr(), thr.data_ptr(), status.data_ptr(), 0)
    torch.cuda.synchronize()
    return out, ok, cnt, st, thr, status


def _tids(eng, tl, orders):
    return torch.tensor([eng.table_ids_from_arrays(tl, list(o)) for o in orders], dtype=torch.int32, device="cuda:0")


def _offsets(frames):
    return np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)


# ---- 1. against the call on compacted frames ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_masked_call_against_the_call_on_compacted_frames(eng, tl, dtype):
    """Three ragged frames (the middle one in firing order) under a Bernoulli(0.7) mask, with the device prepass (planes=) and with caller
    polynomials (thr_polys=): present rows, keep bytes, statistics and counts byte-equal to the call on f[m]; absent rows as they came
    with keep 0; and -- through the C entry -- out_thr_poly, counts and statistics of the device prepass byte-equal too."""
    from lidar_snow_sim_amd.tensors import augment_batch
    frames, masks = ami.ragged_frames(dtype), ami.ragged_masks()
    orders = _orders(3, 5)
    t_frames, t_masks = [_t(f) for f in frames], [_t(m) for m in masks]
    for kw in (dict(planes=[PLANE] * 3), dict(thr_polys=[[1e-3, 0.05, 12.0]] * 3)):
        got = augment_batch(t_frames, "unused", BD, particles=tl, orders=orders, layout="aligned", keep=t_masks, **kw)
        ref = _compacted_reference(frames, masks, tl, orders=orders, **kw)
        scattered, removed = _same_as_compacted(got, ref, frames, masks)
        assert scattered > 20 and removed >= 1, (scattered, removed)
    # one N_total mask (torch.bool and uint8) is the list's concatenation
    flat = augment_batch(t_frames, "unused", BD, particles=tl, orders=orders, layout="aligned", keep=torch.cat(t_masks).to(torch.uint8), planes=[PLANE] * 3)
    _same_as_compacted(flat, _compacted_reference(frames, masks, tl, orders=orders, planes=[PLANE] * 3), frames, masks)
    # the C entry: out_thr_poly of the device prepass
    tids = _tids(eng, tl, orders)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * 3, dtype=torch.float64, device="cuda:0")
    rows, keep = _t(np.concatenate(frames)), _t(np.concatenate(masks))
    sub = [f[m] for f, m in zip(frames, masks)]
    o1, k1, c1, s1, thr1, st1 = _raw(eng, rows, _offsets(frames), tids, keep=keep, plane=plane)
    o0, k0, c0, s0, thr0, st0 = _raw(eng, _t(np.concatenate(sub)), _offsets(sub), tids, plane=plane)
    assert int(st1[0]) == 0 and int(st0[0]) == 0
    assert thr1.cpu().numpy().tobytes() == thr0.cpu().numpy().tobytes() and float(thr0.abs().sum()) > 0
    assert torch.equal(c1, c0) and torch.equal(s1, s0)
    assert o1[keep].cpu().numpy().tobytes() == o0.cpu().numpy().tobytes() and torch.equal(k1[keep], k0)


# ---- 2. against the oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_masked_call_against_the_oracle(so, tl, dtype):
    """oracle.snow_oracle.augment on f[m]: its kept set is nonzero(keep) mapped through the present rows, labels and intensities are
    exact, coordinates within the tolerances of tests/test_gpu_aligned.py (rtol 1e-6 float32, 1e-12 float64), statistics equal."""
    from lidar_snow_sim_amd.tensors import augment_batch
    frames, masks = ami.ragged_frames(dtype), ami.ragged_masks()
    orders = _orders(3, 5)
    res = augment_batch([_t(f) for f in frames], "unused", BD, planes=[PLANE] * 3, orders=orders, particles=tl, layout="aligned",
                        keep=[_t(m) for m in masks])
    for f in range(3):
        st, rows, keep = res[f]
        P = np.flatnonzero(masks[f])
        s0, a0, src0 = so.augment(frames[f][masks[f]], tl, BD, orders[f], plane=PLANE)
        got, flags = rows.cpu().numpy(), keep.cpu().numpy()
        assert _stats(st) == _stats(s0), f
        assert np.array_equal(np.flatnonzero(flags), P[np.sort(src0)]), f
        assert np.array_equal(got[P[src0]][:, 3:], a0[:, 3:]), f
        np.testing.assert_allclose(got[P[src0]][:, :3], a0[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
def test_tile_edges_lone_rows_and_empty_frames_in_one_batch(tl):
    """Exactly 1 023 / 1 024 / 1 025 present rows of a 5 000-row firing-order frame, a 1 025-row frame with only its last row, all
    present, all absent, empty, and the first and last lane of every wave -- one batch, caller polynomials (a one-row frame has no
    ground rows to fit any to), byte-equal to the call on compacted frames."""
    from lidar_snow_sim_amd.tensors import augment_batch
    frames, masks = ami.edge_batch()
    nf = len(frames)
    assert tuple(int(m.sum()) for m in masks) == ami.EDGE_PRESENT
    kw = dict(thr_polys=[[1e-3, 0.05, 12.0]] * nf, orders=[list(range(64))] * nf)
    got = augment_batch([_t(f) for f in frames], "unused", BD, particles=tl, layout="aligned", keep=[_t(m) for m in masks], **kw)
    scattered, removed = _same_as_compacted(got, _compacted_reference(frames, masks, tl, **kw), frames, masks)
    assert removed > 0
    for f in (5, 6):                                                      # all absent / empty: an empty frame's statistics
        assert _stats(got[f][0]) == (0, 0, 0) and int(got[f][2].sum()) == 0


# ---- 4. absent rows are never looked at ------------------------------------------------------------------------------------------------
def test_poisoned_absent_rows_change_nothing(tl):
    """The batch of test 1 with NaN coordinates, a range of 500 m and the channels 999 / -3 / 0.5 in its absent rows: status word 0,
    present rows, flags, counts and statistics byte-equal to the run with benign absent rows, the poisoned rows back bit for bit."""
    from lidar_snow_sim_amd.tensors import augment_batch
    frames, masks = ami.ragged_frames(), ami.ragged_masks()
    orders = _orders(3, 5)
    poisoned = [f.copy() for f in frames]
    for f, m in zip(poisoned, masks):
        a = np.flatnonzero(~m)
        f[a[0::4], 0:3] = np.nan
        f[a[1::4], 0] = 500.0
        f[a[2::4], 4] = np.resize(np.array([999.0, -3.0, 0.5], np.float32), len(a[2::4]))
        f[a[3::4], 0:5] = np.array([np.nan, 500.0, np.inf, -np.inf, 999.0], np.float32)
    kw = dict(planes=[PLANE] * 3, orders=orders, particles=tl, layout="aligned", sync=False)
    want = augment_batch([_t(f) for f in frames], "unused", BD, keep=[_t(m) for m in masks], **kw).wait()
    got = augment_batch([_t(f) for f in poisoned], "unused", BD, keep=[_t(m) for m in masks], **kw).wait()
    assert int(got.status[0]) == 0 and torch.equal(got.status, want.status)
    m = np.concatenate(masks)
    w, g = want.rows.cpu().numpy(), got.rows.cpu().numpy()
    assert g[m].tobytes() == w[m].tobytes() and torch.equal(got.keep, want.keep)
    assert torch.equal(got.counts, want.counts) and torch.equal(got.stats, want.stats)
    assert g[~m].tobytes() == np.concatenate(poisoned)[~m].tobytes() and np.isnan(g[~m]).any()


# ---- 5. in place and aliasing -----------------------------------------------------------------------------------------------------------
def test_in_place_and_keep_aliasing(eng, tl):
    """in_place=True on a DeviceBatch: present rows hold the out-of-place bytes, absent rows (poisoned with NaN) are untouched.
    d_out_keep == d_keep_in through the C entry gives the same bytes; a partially overlapping keep buffer and a mask together with a
    permutation answer SNOWGPU_E_INVALID."""
    from lidar_snow_sim_amd import _native
    from lidar_snow_sim_amd.tensors import AlignedResult, DeviceBatch, augment_batch
    fr, ms = ami.ragged_frames(), ami.ragged_masks()
    frames, masks = [fr[2][:8192].copy(), fr[1].copy()], [ms[2][:8192], ms[1]]
    for f, m in zip(frames, masks):
        f[~m, 0:3] = np.nan
    orders = _orders(2, 70)
    m = np.concatenate(masks)
    keep = _t(m)
    kw = dict(planes=[PLANE] * 2, orders=orders, particles=tl, layout="aligned", sync=False)
    inp = _t(np.concatenate(frames))
    before = inp.cpu().numpy().copy()
    want = augment_batch(DeviceBatch(inp.clone(), frame_rows=8192), "unused", BD, keep=keep, **kw).wait()
    got = augment_batch(DeviceBatch(inp, frame_rows=8192), "unused", BD, keep=keep, in_place=True, **kw).wait()
    assert isinstance(got, AlignedResult) and got.rows.data_ptr() == inp.data_ptr() and torch.equal(keep, _t(m))
    w, g = want.rows.cpu().numpy(), inp.cpu().numpy()
    assert g[m].tobytes() == w[m].tobytes() and g[~m].tobytes() == before[~m].tobytes() == w[~m].tobytes()
    assert torch.equal(got.keep, want.keep) and torch.equal(got.counts, want.counts) and torch.equal(got.stats, want.stats)
    assert int((want.rows[:, 4] == 2).sum()) > 0 and int((~want.keep[keep]).sum()) > 0
    # the C entry with d_out_keep == d_keep_in
    tids = _tids(eng, tl, orders)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * 2, dtype=torch.float64, device="cuda:0")
    rows, off = _t(before), np.array([0, 8192, 16384], np.int64)
    kbuf = _t(m)
    o, k, c, s, _, st = _raw(eng, rows, off, tids, keep=kbuf, plane=plane, out_keep=kbuf)
    assert k.data_ptr() == kbuf.data_ptr() and int(st[0]) == 0
    assert o.cpu().numpy().tobytes() == w.tobytes() and torch.equal(kbuf, want.keep) and torch.equal(c, want.counts) and torch.equal(s, want.stats)
    # refusals
    wide = torch.zeros(16385, dtype=torch.bool, device="cuda:0")
    with pytest.raises(_native.SnowGPUError, match="overlaps") as ei:
        _raw(eng, rows, off, tids, keep=wide[:16384], plane=plane, out_keep=wide[1:])
    assert ei.value.code == _native.E_INVALID
    perm = torch.arange(8192, dtype=torch.int32, device="cuda:0").repeat(2)
    with pytest.raises(_native.SnowGPUError, match="d_perm") as ei:
        _raw(eng, rows, off, tids, keep=_t(m), plane=plane, perm=perm)
    assert ei.value.code == _native.E_INVALID
    with pytest.raises(ValueError, match="aligned"):
        augment_batch([rows], "unused", BD, planes=[PLANE], particles=tl, keep=_t(m))
    # ... and the engine is as usable as before
    again = augment_batch(DeviceBatch(_t(before), frame_rows=8192), "unused", BD, keep=keep, **kw).wait()
    assert torch.equal(again.keep, want.keep) and again.rows.cpu().numpy().tobytes() == w.tobytes()


# ---- 6. a padded batch -------------------------------------------------------------------------------------------------------------------
def test_padded_batch_equals_the_ragged_list(tl):
    """An F x Nmax x 5 tensor (4 frames, Nmax 16 384, lengths 16 384 / 9 000 / 1 / 0, padding NaN) with keep = arange(Nmax) < lengths
    equals the ragged list of the unpadded frames, frame by frame; the padding comes back as it came, keep False."""
    from lidar_snow_sim_amd.tensors import augment_batch
    fr = ami.ragged_frames()
    lengths = [16384, 9000, 1, 0]
    ragged = [fr[0], ami.firing(fr[2])[:9000], fr[0][5000:5001], np.zeros((0, 5), np.float32)]
    padded = np.full((4, 16384, 5), np.nan, np.float32)
    for f, r in enumerate(ragged):
        padded[f, :len(r)] = r
    t_len = torch.tensor(lengths, device="cuda:0")
    keep = torch.arange(16384, device="cuda:0") < t_len[:, None]
    kw = dict(thr_polys=[[1e-3, 0.05, 12.0]] * 4, orders=_orders(4, 90), particles=tl, layout="aligned")
    got = augment_batch(_t(padded), "unused", BD, keep=keep, **kw)
    ref = augment_batch([_t(r) for r in ragged], "unused", BD, **kw)
    for f, n in enumerate(lengths):
        (s1, r1, k1), (s0, r0, k0) = got[f], ref[f]
        assert _stats(s1) == _stats(s0), f
        r1 = r1.cpu().numpy()
        assert r1[:n].tobytes() == r0.cpu().numpy().tobytes() and torch.equal(k1[:n], k0), f
        assert r1[n:].tobytes() == padded[f, n:].tobytes() and not bool(k1[n:].any()), f
    assert sum(int((~k).sum()) for _, _, k in ref) > 0


# ---- 7. size switches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["half", "dense"])
def test_both_sides_of_the_size_switches(tl, case):
    """20 quarter sweeps of 32 768 rows (655 360: above the 16-frame prepass switch and above 2^19 rows), device prepass, against the
    call on compacted frames.  `half`: Bernoulli(0.5) leaves the present total BELOW 2^19 while n_total is above it -- the masked call
    takes the large-batch side of every switch, its reference the small-batch side.  `dense`: Bernoulli(0.9), both above."""
    from lidar_snow_sim_amd.tensors import DeviceBatch, augment_batch
    frames, masks = ami.quarter_sweeps(), ami.switch_masks(case)
    present = sum(int(m.sum()) for m in masks)
    assert (present < (1 << 19)) == (case == "half") and sum(len(f) for f in frames) == 655360
    kw = dict(planes=[PLANE] * 20, orders=_orders(20, 60))
    batch = DeviceBatch(_t(np.concatenate(frames)), frame_rows=32768)
    res = augment_batch(batch, "unused", BD, particles=tl, layout="aligned", keep=_t(np.concatenate(masks)), **kw)
    scattered, removed = _same_as_compacted(res, _compacted_reference(frames, masks, tl, **kw), frames, masks)
    assert scattered > 0 and removed > 0


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------------------------
def test_masked_entry_and_a_consumer_in_one_hip_graph(eng, tl):
    """The masked entry AND a consumer of its result -- (rows[:, 3] * keep).sum() per frame -- captured into one graph and replayed three
    times on changed rows and a changed mask (the present counts change between replays) with no host read in between: every replay
    equals the eager call on that input."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    dev = torch.device("cuda:0")
    F, n = 2, 64 * 256
    a = np.concatenate([synthetic_sweep(64, 256, seed=1050 + f, intensity="lambert") for f in range(F)])
    b = np.concatenate([synthetic_sweep(64, 256, seed=1070 + f, intensity="lambert") for f in range(F)])
    inputs = [(_t(a), _t(ami.bernoulli(F * n, 0.7, 1))), (_t(b), _t(ami.bernoulli(F * n, 0.4, 2))), (_t(a), _t(ami.bernoulli(F * n, 0.9, 3)))]
    rows, mask = inputs[0][0].clone(), inputs[0][1].clone()
    off = torch.arange(F + 1, dtype=torch.int64, device=dev) * n
    tids = _tids(eng, tl, [list(range(64))] * F)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    out = torch.empty_like(rows)
    keep = torch.zeros(F * n, dtype=torch.bool, device=dev)
    cnt, st = torch.zeros(F, dtype=torch.int64, device=dev), torch.zeros(F, 3, dtype=torch.int64, device=dev)
    status = torch.zeros(8, dtype=torch.int32, device=dev)
    sums = torch.zeros(F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()

    def call():
        eng.ctx.augment_batch_device_aligned_masked(F, F * n, n, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), BD, 0, plane.data_ptr(), 0.7, 0,
                                                    mask.data_ptr(), out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0,
                                                    status.data_ptr(), s.cuda_stream)
        sums.copy_((out[:, 3].double() * keep).view(F, n).sum(1))         # the consumer: same stream, static shapes

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        want = []
        for r, m in inputs:                                               # eager calls (two each: the second allocates nothing)
            rows.copy_(r)
            mask.copy_(m)
            call()
            call()
            s.synchronize()
            assert int(status[0]) == 0
            want.append((sums.clone(), cnt.clone(), st.clone(), keep.clone()))
        assert not torch.equal(want[0][0], want[2][0]) and float(want[0][0].min()) > 0
        rows.copy_(inputs[0][0])
        mask.copy_(inputs[0][1])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        got = []
        for r, m in inputs:                                               # no host read between the replays
            rows.copy_(r)
            mask.copy_(m)
            g.replay()
            got.append((sums.clone(), cnt.clone(), st.clone(), keep.clone()))
        s.synchronize()
    assert int(status[0]) == 0
    for k in range(3):
        for x, y in zip(got[k], want[k]):
            assert torch.equal(x, y), k
        assert int(got[k][3][~inputs[k][1]].sum()) == 0


# ---- 9. pre-crop on tensors against the host entry -------------------------------------------------------------------------------------------
def test_pre_crop_on_tensors_against_the_host_entry(tl):
    """augment_batch(tensor, layout='aligned', calib=c, pre_crop=True) against augment_batch([numpy], calib=c, pre_crop=True,
    return_src=True) on one 64 x 512 sweep under the narrow camera: statistics equal, nonzero(keep) == sort(src), rows[src] its rows."""
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    pc, cal = ami.precrop_sweep(), ami.narrow_calib()
    kw = dict(particles=tl, orders=[list(range(64))], planes=[PLANE], calib=cal, pre_crop=True)
    (s0, aug, src), = augment_batch([pc], "unused", BD, return_src=True, **kw)
    (s1, rows, keep), = augment_batch([_t(pc)], "unused", BD, layout="aligned", **kw)
    assert _stats(s0) == _stats(s1) and 500 < len(src) < len(pc) // 4
    assert np.array_equal(np.flatnonzero(keep.cpu().numpy()), np.sort(src))
    assert rows.cpu().numpy()[src].tobytes() == np.ascontiguousarray(aug).tobytes()
    with pytest.raises(ValueError, match="pre_crop"):                     # the compact layout keeps raising
        augment_batch([_t(pc)], "unused", BD, **kw)


# ---- 10. fov_keep against NumPy ----------------------------------------------------------------------------------------------------------------
def test_fov_keep_against_numpy(tl):
    """tensors.fov_keep against calibration.get_fov_flag in float64 NumPy on every row whose pixel coordinates lie farther than 1e-6
    from an image edge and whose depth lies farther than 1e-9 from 0 (at most 8 rows are left out); with keep= it is the AND."""
    from lidar_snow_sim_amd.tensors import fov_keep
    pc, cal = ami.precrop_sweep(), ami.narrow_calib()
    flag, decided = ami.fov_reference(pc, cal)
    assert int((~decided).sum()) <= 8 and int(flag.sum()) >= 1000 and int((~flag).sum()) >= 1000
    for dt in (np.float32, np.float64):
        got = fov_keep([_t(pc.astype(dt))], cal)
        assert got.dtype == torch.bool and got.shape == (len(pc),)
        assert np.array_equal(got.cpu().numpy()[decided], flag[decided]), dt
    m = ami.bernoulli(len(pc), 0.5, 9)
    poisoned = pc.copy()
    poisoned[~m, 0:3] = np.nan
    both = fov_keep(_t(poisoned), cal, keep=_t(m)).cpu().numpy()
    assert np.array_equal(both[decided], (flag & m)[decided]) and not both[~m].any()


def test_fov_keep_refuses_host_rows_word_for_word():
    from lidar_snow_sim_amd.tensors import fov_keep
    with pytest.raises(ValueError, match=r"^fov_keep: torch CUDA tensors \(host arrays: lidar_snow_sim_amd\.calibration\.get_fov_flag\)$"):
        fov_keep(np.zeros((4, 5), np.float32), None)


# ---- 11. the fused chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_fused_chain_equals_the_two_masked_stages(tl, dtype):
    """augment_wet_batch_aligned(..., keep=mask) equals, byte for byte, the masked snowfall call followed by wet_ground_batch_aligned on
    its rows and keep mask, flags included: two frames with thousands of present ground rows, one below 1 000 (flag 1)."""
    from lidar_snow_sim_amd.tensors import DeviceBatch, augment_batch, augment_wet_batch_aligned, wet_ground_batch_aligned
    frames, masks = ami.fused_frames(dtype)
    t_frames, keep = [_t(f) for f in frames], _t(np.concatenate(masks))
    wet = dict(water_height=0.0008, pavement_depth=0.001, power_factor=15, flat_earth=False, delta=0.5, replace=True, noise_floor=0.7)
    kw = dict(planes=[PLANE] * 3, orders=[list(range(64))] * 3, particles=tl, sync=False)
    res = augment_wet_batch_aligned(t_frames, "unused", BD, wet=dict(wet, plane=PLANE), keep=keep, **kw).wait()
    snow = augment_batch(t_frames, "unused", BD, layout="aligned", keep=keep, **kw).wait()
    two = wet_ground_batch_aligned(DeviceBatch(snow.rows.clone(), snow.offsets), snow.keep.clone(), plane=PLANE, sync=False, **wet).wait()
    assert res.rows.dtype == t_frames[0].dtype
    assert res.rows.cpu().numpy().tobytes() == two.rows.cpu().numpy().tobytes()
    assert torch.equal(res.keep, two.keep) and torch.equal(res.flags, two.flags) and torch.equal(res.counts, two.counts)
    assert torch.equal(res.stats, snow.stats)
    assert res.flags.tolist() == [0, 0, 1]
    assert not bool(res.keep[~keep].any()) and int((snow.keep & ~res.keep).sum()) > 1000      # the wet stage dropped rows of its own
    m = np.concatenate(masks)
    assert res.rows.cpu().numpy()[~m].tobytes() == np.concatenate(frames)[~m].tobytes()
