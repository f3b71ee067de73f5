"""-m gpu: the ALIGNED wet-ground stage (csrc/snowgpu_wet.hip: k_pre_ground<T, true>, k_wet_apply_aligned, k_wet_count) through
wet_ground_batch_aligned (snowgpu_wet_ground_batch_device_aligned) and, fused behind the aligned snowfall finish, through
augment_wet_batch_aligned (snowgpu_augment_wet_batch_device_aligned).

The expectation for a frame `pc` with keep mask `m` is the oracle on the gathered rows:
    ref, src = so.ground_water_augmentation(pc[m], plane=..., return_src=True, **kw);  idx = np.flatnonzero(m)[src]
keep is true exactly at idx; rows[idx] against ref: coordinates and column 4 exact, zero intensities on the same rows, intensities at
rtol 1e-9 on float64 rows and, on float32 rows, against np.float32(ref) at rtol 1e-7 + 2^-23 (the project's float32 wet tolerance plus
one rounding to float32 on each side); rows with m == 0 equal the input byte for byte; counts == len(ref); flags equal.
tests/test_wet_aligned_reference.py shows on any machine that the masked frames are still settings (mask() is imported from there).

Observed on an MI355X (test_settings_under_a_mask prints its own with -s): largest relative intensity error 0 on float32 rows (against
np.float32(ref): the same float32 value everywhere) and 2.5e-16 .. 4.1e-14 on float64 rows; the fitted lines 7.1e-4 .. 1.9e-3 of their bound.
All 30 tests of this file passed there, 4.5 s together.  That the in-place test bites: its first run caught k_wet_apply_aligned storing the
(never loaded) intensity of a non-ground row as 0 when it patched the row's label in place under `replace`.
"""
import numpy as np
import pytest
import torch

import prepass_reference as pr
from test_wet_aligned_reference import mask

pytestmark = pytest.mark.gpu

TAGS = ("f32", "f64")
PLANE = (pr.PLANE_W, pr.PLANE_H)
SNOW_PLANE = (np.array([0.0, 0.0, -1.0]), -1.7)
BD = float(np.degrees(3e-3))
RTOL = {"f64": 1e-9, "f32": 1e-7 + 2.0 ** -23}


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


def _run(frames, masks, kw, **extra):
    """wet_ground_batch_aligned on host frames / masks (None: no keep tensor at all) -> per frame (rows, keep, flag) as NumPy, counts."""
    from lidar_snow_sim_amd.tensors import wet_ground_batch_aligned
    t_frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    keep = None if masks is None else torch.from_numpy(np.concatenate(masks)).cuda()
    res = wet_ground_batch_aligned(t_frames, keep, plane=PLANE, sync=False, **kw, **extra).wait()
    off = res.offsets
    rows, kp, flags, counts = res.rows.cpu().numpy(), res.keep.cpu().numpy(), res.flags.cpu().numpy(), res.counts.cpu().numpy()
    assert res.rows.dtype == t_frames[0].dtype and res.keep.dtype == torch.bool and res.stats is None
    return [(rows[off[f]:off[f + 1]], kp[off[f]:off[f + 1]], int(flags[f])) for f in range(len(frames))], counts


def _check(so, name, pc, m, kw, rows, keep, count, flag, tag, ref_flag=None):
    """One frame against the oracle on its gathered rows -> (failures, largest relative intensity error)."""
    fails = []
    sub = np.ascontiguousarray(pc[m])
    ref, src = so.ground_water_augmentation(sub, plane=PLANE, return_src=True, **kw)
    ref = np.asarray(ref, np.float64)
    if ref_flag is None:
        ref_flag = pr.wet_restated(sub, **kw).flag
    idx = np.flatnonzero(m)[src]
    if flag != ref_flag:
        fails.append(f"{name}: flag {flag}, reference {ref_flag}")
    if int(count) != len(ref):
        fails.append(f"{name}: count {int(count)}, reference {len(ref)}")
    if not np.array_equal(np.flatnonzero(keep), np.sort(idx)):
        return fails + [f"{name}: {int(keep.sum())} rows kept, reference {len(idx)}; the kept sets differ"], np.nan
    if rows[~m].tobytes() != pc[~m].tobytes():
        fails.append(f"{name}: rows that were not there changed")
    got = rows[idx]
    want = ref if tag == "f64" else ref.astype(np.float32)
    if not np.array_equal(got[:, [0, 1, 2, 4]], want[:, [0, 1, 2, 4]]):
        fails.append(f"{name}: coordinates or labels differ")
    a, b = got[:, 3].astype(np.float64), want[:, 3].astype(np.float64)
    if not np.array_equal(a == 0, b == 0):
        fails.append(f"{name}: {int(((a == 0) != (b == 0)).sum())} rows are zero on one side only")
    nz = (a != 0) & (b != 0)
    rel = float(np.max(np.abs(a[nz] - b[nz]) / np.abs(b[nz]))) if nz.any() else 0.0
    if rel > RTOL[tag]:
        fails.append(f"{name}: intensities off by a relative {rel:.3e} (rtol {RTOL[tag]:.3g})")
    return fails, rel


def _fit_fraction(fit, r, kw):
    ld = pr.estimate_ld(r.g, r.e64, kw["noise_floor"])
    want = (ld.p[0], ld.p[1], ld.pmin[0], ld.pmin[1])
    bound = (ld.b_p[0], ld.b_p[1], ld.b_pmin[0], ld.b_pmin[1])
    got = (fit[1], fit[2], fit[4], fit[5])
    assert fit[0] == 0 and fit[3] == 0
    return max(float(abs(pr.L(g) - w) / b) for g, w, b in zip(got, want, bound))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("i", range(len(pr.WET_PARAMS)))
def test_settings_under_a_mask(eng, so, i, tag):
    """One batch [wet (masked), empty, wet (all ones), g999, g1000] per parameter set.  The ground count of the masked frame's fit is the
    count of its PRESENT ground rows (a ground pass without the mask fails here on the count alone), its two lines lie inside the bounds
    of the long-double estimate on pc[m]."""
    kw = pr.WET_PARAMS[i]
    names = ("wet", "empty", "wet", "g999", "g1000")
    frames = [pr.frame(n, tag) for n in names]
    masks = [mask(frames[0], i)] + [np.ones(len(f), bool) for f in frames[1:]]
    out, counts = _run(frames, masks, kw)
    fits = eng.ctx.wet_last_fit(len(names))
    failures, worst, worst_fit = [], 0.0, 0.0
    for f, (name, pc, m) in enumerate(zip(names, frames, masks)):
        r = pr.wet_restated(np.ascontiguousarray(pc[m]), **kw)
        rows, keep, flag = out[f]
        fl, rel = _check(so, f"{name}[{f}]", pc, m, kw, rows, keep, counts[f], flag, tag, ref_flag=r.flag)
        failures += fl
        worst = max(worst, rel)
        if fits[f][6] != r.g.mask.sum():
            failures.append(f"{name}[{f}]: the fit saw {int(fits[f][6])} ground rows, {int(r.g.mask.sum())} are present")
        if r.flag == 0:
            frac = _fit_fraction(fits[f], r, kw)
            worst_fit = max(worst_fit, frac)
            if frac > 1:
                failures.append(f"{name}[{f}]: fitted lines {fits[f][[1, 2, 4, 5]].tolist()} are {frac:.3g} of their bound from the long-double ones")
    assert out[0][2] == 0 and out[1][2] == 1 and counts[1] == 0 and fits[0][6] < fits[2][6]
    print(f"\n[wet-aligned] parameters {i} {tag}: largest relative intensity error {worst:.2e}; fitted lines: largest error / bound {worst_fit:.2e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tag", TAGS)
def test_tiles_under_a_mask(so, tag):
    """wet_tiles (65 tiles + 1 row: the second trip of every per-frame wave) under the mask rule; with every row of tile 2 masked as
    well (a tile whose rows are all not there); with an all-zero mask (flag 1, count 0, nothing written)."""
    kw = pr.WET_PARAMS[0]
    pc = pr.frame("wet_tiles", tag)
    m0 = mask(pc, 0)
    m1 = m0.copy()
    m1[2 * pr.TILE:3 * pr.TILE] = False
    m2 = np.zeros(len(pc), bool)
    out, counts = _run([pc] * 3, [m0, m1, m2], kw)
    failures = []
    for f, m in enumerate((m0, m1)):
        rows, keep, flag = out[f]
        failures += _check(so, f"wet_tiles[{f}]", pc, m, kw, rows, keep, counts[f], flag, tag, ref_flag=0)[0]
    rows, keep, flag = out[2]
    assert flag == 1 and counts[2] == 0 and not keep.any() and rows.tobytes() == pc.tobytes()
    assert 0 < counts[1] < counts[0]
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tag", TAGS)
def test_the_1000_row_rule_counts_present_rows(so, tag):
    """g1000 whole is processed; g1000 with exactly ONE ground row masked and g999 come back untouched with flag 1."""
    kw = pr.WET_PARAMS[2] | dict(delta=0.5)
    a, b = pr.frame("g1000", tag), pr.frame("g999", tag)
    one = np.ones(len(a), bool)
    one[np.flatnonzero(pr.ground_rows(a).mask)[500]] = False
    masks = [np.ones(len(a), bool), one, np.ones(len(b), bool)]
    out, counts = _run([a, a, b], masks, kw)
    assert [o[2] for o in out] == [0, 1, 1]
    failures = []
    for f, (pc, m) in enumerate(zip((a, a, b), masks)):
        rows, keep, flag = out[f]
        failures += _check(so, f"frame {f}", pc, m, kw, rows, keep, counts[f], flag, tag)[0]
    assert out[1][0].tobytes() == a.tobytes() and np.array_equal(out[1][1], one) and counts[1] == len(a) - 1
    assert out[2][0].tobytes() == b.tobytes() and out[2][1].all() and counts[2] == len(b)
    assert counts[0] < len(a) and out[0][0].tobytes() != a.tobytes()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tag", TAGS)
def test_no_mask_against_the_compact_entry(eng, tag):
    """keep=None: the tiles are the compact entry's own, so rows[src] are Context.wet_ground_batch's rows byte for byte on float64 rows
    and those rows cast to float32 on float32 rows; keep is true exactly at src."""
    kw = pr.WET_PARAMS[0]
    names = ("wet", "empty", "m3", "m4", "wet_tiles")
    frames = [pr.frame(n, tag) for n in names]
    rows_h, off = pr.concat(frames)
    c_out, c_src, c_counts, c_flags = eng.ctx.wet_ground_batch(rows_h, off, [pr.PLANE4] * len(names), kw["water_height"], kw["pavement_depth"],
                                                              kw["noise_floor"], kw["power_factor"], kw["flat_earth"], kw["delta"], kw["replace"])
    out, counts = _run(frames, None, kw)
    assert c_flags.tolist() == [o[2] for o in out] and np.array_equal(c_counts, counts) and 0 in c_flags and 1 in c_flags
    for f in range(len(names)):
        a, n = int(off[f]), int(c_counts[f])
        rows, keep, _ = out[f]
        src = c_src[a:a + n]
        assert np.array_equal(np.flatnonzero(keep), np.sort(src)), names[f]
        assert rows[src].tobytes() == c_out[a:a + n].astype(rows.dtype).tobytes(), names[f]


@pytest.mark.parametrize("tag", TAGS)
def test_in_place_gives_the_out_of_place_bytes(eng, tag):
    """out_rows is rows and out_keep is keep_in: the two tensors hold afterwards what the out-of-place call returned (replace on and off:
    the rows an in-place call patches differ); an output one row into the input is E_INVALID."""
    from lidar_snow_sim_amd import _native
    from lidar_snow_sim_amd.tensors import AlignedWetResult, DeviceBatch, wet_ground_batch_aligned
    frames = [pr.frame(n, tag) for n in ("wet", "g999", "wet")]
    masks = [mask(frames[0], 1), mask(frames[1], 1), np.ones(len(frames[2]), bool)]
    rows_h, off = pr.concat(frames)
    for i in (0, 1):
        kw = pr.WET_PARAMS[i]
        inp, kin = torch.from_numpy(rows_h).cuda(), torch.from_numpy(np.concatenate(masks)).cuda()
        want = wet_ground_batch_aligned(DeviceBatch(inp.clone(), off), kin.clone(), plane=PLANE, sync=False, **kw).wait()
        got = wet_ground_batch_aligned(DeviceBatch(inp, off), kin, plane=PLANE, in_place=True, sync=False, **kw).wait()
        assert isinstance(got, AlignedWetResult) and got.rows.data_ptr() == inp.data_ptr() and got.keep.data_ptr() == kin.data_ptr()
        assert want.rows.data_ptr() != inp.data_ptr() and want.flags.tolist() == [0, 1, 0]
        assert torch.equal(inp, want.rows) and torch.equal(kin, want.keep)
        assert torch.equal(got.counts, want.counts) and torch.equal(got.flags, want.flags)
        assert int((~want.keep).sum()) > int((~torch.from_numpy(np.concatenate(masks))).sum())
    n = int(off[-1])
    dev = inp.device
    buf = torch.zeros(n + 1, 5, dtype=inp.dtype, device=dev)
    kbuf = torch.ones(n + 1, dtype=torch.bool, device=dev)
    d_off = torch.from_numpy(off).to(dev)
    plane = torch.tensor([pr.PLANE4] * 3, dtype=torch.float64, device=dev)
    cnt, flags, status = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    code = 0 if tag == "f32" else 1
    for o_rows, k_in, o_keep in ((buf[1:], kbuf, kbuf), (buf, kbuf, kbuf[1:])):
        with pytest.raises(_native.SnowGPUError, match="overlaps") as ei:
            eng.ctx.wet_ground_batch_device_aligned(3, n, int(np.diff(off).max()), d_off.data_ptr(), buf.data_ptr(), code, k_in.data_ptr(),
                                                    plane.data_ptr(), 0.0008, 0.001, 0.7, 15, False, 0.5, True, o_rows.data_ptr(),
                                                    o_keep.data_ptr(), cnt.data_ptr(), flags.data_ptr(), status.data_ptr(), 0)
        assert ei.value.code == _native.E_INVALID


def _firing(frame, channels=64):
    return np.ascontiguousarray(frame.reshape(channels, -1, 5).transpose(1, 0, 2).reshape(-1, 5))


@pytest.fixture(scope="module")
def fused_reference(so, tl):
    """Per dtype: the three frames of the fused test and the oracle's snowfall stage on each (computed once, shared, left unchanged)."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    base = [synthetic_sweep(64, 512, seed=1300, intensity="lambert"), _firing(synthetic_sweep(64, 256, seed=1301, intensity="lambert")),
            synthetic_sweep(64, 17, seed=1303, intensity="lambert")]
    assert np.any(np.diff(base[1][:, 4]) < 0) and not np.any(np.diff(base[0][:, 4]) < 0)
    ref = {}
    for tag in TAGS:
        frames = [f.astype(np.float32 if tag == "f32" else np.float64) for f in base]
        ref[tag] = (frames, [so.augment(f, tl, BD, list(range(64)), plane=SNOW_PLANE) for f in frames])
    return ref


@pytest.mark.parametrize("replace", [False, True], ids=["keep_labels", "replace"])
@pytest.mark.parametrize("tag", TAGS)
def test_fused_chain_against_the_oracle_chain(so, tl, fused_reference, tag, replace):
    """augment_wet_batch_aligned against so.augment -> so.ground_water_augmentation(return_src=True): a channel-sorted frame, one in
    firing order and one with 748 ground rows, which comes back as the snowfall result with flag 1.  keep is true exactly at
    src0[wsrc0], labels exact, statistics equal, coordinates and intensities at the fused compact test's rtol 1e-6; the rows the
    snowfall stage removed equal the rows of augment_batch(layout='aligned') byte for byte."""
    from lidar_snow_sim_amd.tensors import augment_batch, augment_wet_batch_aligned
    frames, snow = fused_reference[tag]
    wet = dict(water_height=0.0008, pavement_depth=0.001, power_factor=15, flat_earth=False, delta=0.5, replace=replace)
    t_frames = [torch.from_numpy(f).cuda() for f in frames]
    kw = dict(planes=[SNOW_PLANE] * 3, orders=[list(range(64))] * 3, particles=tl)
    res = augment_wet_batch_aligned(t_frames, "unused", BD, wet=dict(wet, noise_floor=0.7, plane=SNOW_PLANE), **kw)
    snow_only = augment_batch(t_frames, "unused", BD, layout="aligned", **kw)
    dropped = []
    for f in range(3):
        st, rows, keep, flag = res[f]
        s0, a0, src0 = snow[f]
        o0, wsrc0 = so.ground_water_augmentation(a0, noise_floor=0.7, plane=SNOW_PLANE, return_src=True, **wet)
        assert rows.dtype == t_frames[f].dtype and tuple(rows.shape) == frames[f].shape and keep.dtype == torch.bool
        assert tuple(int(v) for v in st) == tuple(int(v) for v in s0)
        assert flag == (1 if o0 is a0 else 0), f
        idx = src0[wsrc0]
        got, kp = rows.cpu().numpy(), keep.cpu().numpy()
        assert np.array_equal(np.flatnonzero(kp), np.sort(idx)), f
        assert np.array_equal(got[idx][:, 4], np.asarray(o0)[:, 4]), f
        np.testing.assert_allclose(got[idx][:, :4], np.asarray(o0)[:, :4], rtol=1e-6, atol=0)
        _, r1, k1 = snow_only[f]
        gone = ~k1.cpu().numpy()
        assert gone.sum() == len(frames[f]) - len(a0) and got[gone].tobytes() == r1.cpu().numpy()[gone].tobytes(), f
        dropped.append(len(a0) - len(o0))
    assert [r[3] for r in res] == [0, 0, 1] and dropped[0] > 5000 and dropped[1] > 1600 and dropped[2] == 0, dropped


@pytest.mark.parametrize("tag", TAGS)
def test_poly_under_a_mask_against_the_compact_entry(eng, tag):
    """estimation_method='poly' (same seed, frame 0 in both calls): the masked `wet` frame against the library's compact entry on pc[m]:
    the kept set is equal, the intensities agree at the tolerances of tests/test_gpu_poly.py::test_L9_poly_on_the_reference_clouds."""
    from lidar_snow_sim_amd.tensors import wet_ground_batch_aligned
    kw = pr.WET_PARAMS[1]
    pc = pr.frame("wet", tag)
    m = mask(pc, 1)
    sub = np.ascontiguousarray(pc[m])
    eng.ctx.set_wet_estimation("poly", 5)
    try:
        c_out, c_src, c_counts, c_flags = eng.ctx.wet_ground_batch(sub, [0, len(sub)], [pr.PLANE4], kw["water_height"], kw["pavement_depth"], kw["noise_floor"],
                                                                  kw["power_factor"], kw["flat_earth"], kw["delta"], kw["replace"])
        fit_c = eng.ctx.wet_last_fit(1)[0]
    finally:
        eng.ctx.set_wet_estimation("linear")
    (_, rows, keep, flag), = wet_ground_batch_aligned([torch.from_numpy(pc).cuda()], torch.from_numpy(m).cuda(), plane=PLANE, estimation_method="poly",
                                                      poly_seed=5, **kw)
    fit_a = eng.ctx.wet_last_fit(1)[0]
    n = int(c_counts[0])
    assert flag == 0 and c_flags[0] == 0 and fit_a[6] == fit_c[6] and fit_a[7] == fit_c[7] and fit_c[0] != 0.0
    idx = np.flatnonzero(m)[c_src[:n]]
    got, kp = rows.cpu().numpy(), keep.cpu().numpy()
    assert np.array_equal(np.flatnonzero(kp), np.sort(idx)) and 100 < n - (~pr.ground_rows(sub, delta=kw["delta"]).mask).sum() < len(idx)
    assert np.array_equal(got[idx][:, [0, 1, 2, 4]], c_out[:n][:, [0, 1, 2, 4]].astype(got.dtype))
    np.testing.assert_allclose(got[idx][:, 3], c_out[:n, 3], rtol=1e-9 if tag == "f64" else 1e-6, atol=1e-9)
    assert got[~m].tobytes() == pc[~m].tobytes()


def test_fused_entry_in_place_and_a_consumer_in_one_hip_graph(eng, tl):
    """snowgpu_augment_wet_batch_device_aligned IN PLACE and a consumer of rows and keep -- the kept intensity per frame -- captured into
    one graph and replayed three times on changing input with no host read in between: every replay equals the plain calls."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    dev = torch.device("cuda:0")
    F, n = 2, 64 * 256
    frames = [synthetic_sweep(64, 256, seed=1050 + f, intensity="lambert") for f in range(F)]
    other = [synthetic_sweep(64, 256, seed=1070 + f, intensity="lambert") for f in range(F)]
    rows = torch.from_numpy(np.concatenate(frames)).to(dev)
    off = torch.arange(F + 1, dtype=torch.int64, device=dev) * n
    tids = torch.tensor([eng.table_ids_from_arrays(tl, list(range(64))) for _ in range(F)], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    keep = torch.zeros(F * n, dtype=torch.bool, device=dev)
    cnt = torch.zeros(F, dtype=torch.int64, device=dev)
    st = torch.zeros(F, 3, dtype=torch.int64, device=dev)
    flags = torch.zeros(F, dtype=torch.int32, device=dev)
    status = torch.zeros(8, dtype=torch.int32, device=dev)
    sums = torch.zeros(F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()

    def call():
        eng.ctx.augment_wet_batch_device_aligned(F, F * n, n, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), BD, 0, plane.data_ptr(), 0.7, 0,
                                                 rows.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream,
                                                 plane.data_ptr(), 0.0008, 0.001, 0.7, 15, False, 0.5, False, flags.data_ptr())
        sums.copy_((rows[:, 3].double() * keep).view(F, n).sum(1))        # the consumer: same stream, static shapes

    inputs = [rows.clone(), torch.from_numpy(np.concatenate(other)).to(dev), rows.clone()]
    with torch.cuda.stream(s):
        want = []
        for inp in inputs:                                                # plain calls; a warm-up on a copy first: the second allocates nothing
            rows.copy_(inp)
            call()
            rows.copy_(inp)
            call()
            s.synchronize()
            assert int(status[0]) == 0 and flags.tolist() == [0, 0]
            want.append((sums.clone(), cnt.clone(), st.clone(), keep.clone(), rows.clone()))
        assert not torch.equal(want[0][0], want[1][0]) and float(want[0][0].min()) > 0
        assert int((want[0][4][:, 4] == 1).sum()) > 0 and int((~want[0][3]).sum()) > 0
        rows.copy_(inputs[0])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        got = []
        for inp in inputs:                                                # no host read between the replays
            rows.copy_(inp)
            g.replay()
            got.append((sums.clone(), cnt.clone(), st.clone(), keep.clone(), rows.clone()))
        s.synchronize()
    assert int(status[0]) == 0
    for k in range(3):
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k


def test_refusals_leave_the_engine_usable(eng):
    """A NULL plane under the plane method 'lsq', a context with the packed result transfer set, a null pointer: each is E_INVALID, and
    the next call on the engine gives the bytes of the call before them."""
    from lidar_snow_sim_amd import _native
    from lidar_snow_sim_amd.tensors import wet_ground_batch_aligned
    kw = pr.WET_PARAMS[0]
    pc = pr.frame("wet", "f32")
    t, k = torch.from_numpy(pc).cuda(), torch.from_numpy(mask(pc, 0)).cuda()
    first = wet_ground_batch_aligned([t], k, plane=PLANE, sync=False, **kw).wait()

    def again():
        r = wet_ground_batch_aligned([t], k, plane=PLANE, sync=False, **kw).wait()
        assert torch.equal(r.rows, first.rows) and torch.equal(r.keep, first.keep) and torch.equal(r.counts, first.counts) and int(r.flags[0]) == 0

    eng.ctx.set_plane_method("lsq")
    try:
        with pytest.raises(_native.SnowGPUError, match="plane") as ei:
            wet_ground_batch_aligned([t], k, **kw)
    finally:
        eng.ctx.set_plane_method("reference")
    assert ei.value.code == _native.E_INVALID
    again()
    flat = wet_ground_batch_aligned([t], k, sync=False, **kw).wait()      # a NULL plane under 'reference': the flat-earth plane, no row read
    assert int(flat.flags[0]) in (0, 1) and int(flat.status[0]) == 0
    eng.ctx.set_result_transfer("packed")
    try:
        with pytest.raises(_native.SnowGPUError, match="packed") as ei:
            wet_ground_batch_aligned([t], k, plane=PLANE, **kw)
    finally:
        eng.ctx.set_result_transfer("rows")
    assert ei.value.code == _native.E_INVALID
    again()
    dev = t.device
    d_off = torch.tensor([0, len(pc)], dtype=torch.int64, device=dev)
    plane = torch.tensor([pr.PLANE4], dtype=torch.float64, device=dev)
    o_rows, o_keep = torch.empty_like(t), torch.empty_like(k)
    flags, status = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(_native.SnowGPUError, match="null pointer") as ei:
        eng.ctx.wet_ground_batch_device_aligned(1, len(pc), len(pc), d_off.data_ptr(), t.data_ptr(), 0, k.data_ptr(), plane.data_ptr(), 0.0, 0.001, 0.7,
                                                15, False, 0.5, True, o_rows.data_ptr(), o_keep.data_ptr(), 0, flags.data_ptr(), status.data_ptr(), 0)
    assert ei.value.code == _native.E_INVALID
    again()
