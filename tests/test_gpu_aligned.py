"""-m gpu: the ALIGNED result layout of the device-resident boundary (augment_batch(..., layout='aligned'), snowgpu_augment_batch_device_aligned,
k_finish_aligned): every input row's output row at the input's own index plus one keep flag per row -- against the oracle, against the CPU
twin's aligned form byte for byte (removed rows included), against the compact call of the same library on the tile edges, on both sides of
every size switch and under every option, in place, and captured into a HIP graph TOGETHER with a consumer of the result."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PLANE = (np.array([0.0, 0.0, -1.0]), -1.7)
BD = float(np.degrees(3e-3))


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    snow_oracle.build()
    return snow_oracle


@pytest.fixture(scope="module")
def tl(tables):
    return [tables["t"][i % 4] for i in range(64)]


def _firing(frame, channels=64):
    """A channel-major frame (channels x azimuths) re-ordered azimuth-major: firing order, which the channel sort has to permute."""
    return np.ascontiguousarray(frame.reshape(channels, -1, 5).transpose(1, 0, 2).reshape(-1, 5))


def _ragged_frames(dtype=np.float32):
    """The three ragged frames of tests/test_gpu_tensors.py (16 384 / 8 192 / 16 384 rows), the middle one in firing order."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    full = [synthetic_sweep(64, 2048, seed=1200 + f, intensity="lambert").reshape(64, 2048, 5) for f in range(3)]
    fr = [np.ascontiguousarray(full[0][:, ::8, :].reshape(-1, 5)), _firing(np.ascontiguousarray(full[1][:, 1::16, :].reshape(-1, 5))),
          np.ascontiguousarray(full[2][:, 3::8, :].reshape(-1, 5))]
    assert np.any(np.diff(fr[1][:, 4]) < 0) and not np.any(np.diff(fr[0][:, 4]) < 0)
    return [f.astype(dtype) for f in fr]


def _stats(st):
    return tuple(int(v) for v in st)


def _same_as_compact(frames, tl, **kw):
    """The aligned call against the compact call of the same library with the same arguments: rows_f[src] equals the compact rows byte for
    byte, keep is true exactly at src, statistics are equal.  Returns (kept, removed) row counts."""
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    compact = augment_batch(frames, "unused", BD, particles=tl, return_src=True, **kw)
    aligned = augment_batch(frames, "unused", BD, particles=tl, layout="aligned", **kw)
    assert len(compact) == len(aligned)
    kept = removed = 0
    for f, ((s0, aug, src), (s1, rows, keep)) in enumerate(zip(compact, aligned)):
        assert rows.is_cuda and keep.dtype == torch.bool and rows.shape[1] == 5 and rows.dtype == aug.dtype and keep.shape[0] == rows.shape[0], f
        assert _stats(s0) == _stats(s1), (f, s0, s1)
        assert torch.equal(rows[src.long()], aug), f
        assert torch.equal(torch.nonzero(keep).flatten(), torch.sort(src.long()).values), f
        kept += int(keep.sum())
        removed += int((~keep).sum())
    return kept, removed


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_aligned_batch_matches_the_oracle_and_the_cpu_twin(so, tl, dtype):
    """Three ragged frames, one of them in firing order.  With the device's own prepass: rows_f[src0] are the oracle's rows (labels and
    intensities exact, coordinates to the tolerance of the compact layout's test), keep_f is true exactly at src0, statistics are equal.
    With the oracle's polynomials handed to both: every row and every flag equals the CPU twin's aligned form byte for byte, removed rows too."""
    from lidar_snow_sim_amd import _cpu_twin, build
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    build.build_cpu_twin(verbose=False)
    frames = _ragged_frames(dtype)
    orders = [list(np.random.default_rng(5 + f).permutation(64)) for f in range(3)]
    t_frames = [torch.from_numpy(f).cuda() for f in frames]
    res = augment_batch(t_frames, "unused", BD, planes=[PLANE] * 3, orders=orders, particles=tl, layout="aligned")
    polys, scattered, removed = [], 0, 0
    for f in range(3):
        st, rows, keep = res[f]
        assert rows.is_cuda and rows.dtype == t_frames[f].dtype and tuple(rows.shape) == frames[f].shape and keep.dtype == torch.bool
        s0, a0, src0, extra = so.augment(frames[f], tl, BD, orders[f], plane=PLANE, return_full=True)
        polys.append(np.asarray(extra["thr_poly"], np.float64))
        got, flags = rows.cpu().numpy(), keep.cpu().numpy()
        assert _stats(st) == _stats(s0)
        assert np.array_equal(np.flatnonzero(flags), np.sort(src0)) and np.array_equal(got[src0][:, 3:], a0[:, 3:])
        np.testing.assert_allclose(got[src0][:, :3], a0[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
        scattered += int((got[flags, 4] == 2).sum())
        removed += int((~flags).sum())
    assert scattered > 20 and removed >= 1, (scattered, removed)
    twin = _cpu_twin.augment_batch(frames, tl, orders, BD, polys, layout="aligned")
    res = augment_batch(t_frames, "unused", BD, thr_polys=polys, orders=orders, particles=tl, layout="aligned")
    for f in range(3):
        (st, rows, keep), (s1, r1, k1) = res[f], twin[f]
        assert _stats(st) == _stats(s1)
        assert rows.cpu().numpy().tobytes() == r1.tobytes() and np.array_equal(keep.cpu().numpy(), k1), f
    assert sum(int((~k).sum()) for _, _, k in twin) >= 1


def test_tile_edges_and_an_empty_frame(tl):
    """Frames of 1, 63, 1023, 1024, 1025 and 5000 rows and an empty one in ONE batch (a tile is 1024 rows; a block's four rounds are 256
    apart), channel-sorted, shuffled and in firing order, against the compact call.  (Caller polynomials: a one-row frame has no ground
    rows to fit any to.)"""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    full = synthetic_sweep(64, 2048, seed=1410, intensity="lambert").reshape(64, 2048, 5)
    rng = np.random.default_rng(3)
    sl = lambda k, n: np.ascontiguousarray(full[:, k::16].reshape(-1, 5)[:n])     # noqa: E731  (channel-sorted)
    frames = [sl(0, 8192)[4000:4001], sl(1, 63), rng.permutation(sl(2, 1023)), sl(3, 1024), sl(4, 1025),
              _firing(np.ascontiguousarray(full[:, 5::16].reshape(-1, 5)))[:5000], np.zeros((0, 5), np.float32)]
    assert [len(f) for f in frames] == [1, 63, 1023, 1024, 1025, 5000, 0]
    t_frames = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    kept, removed = _same_as_compact(t_frames, tl, thr_polys=[[1e-3, 0.05, 12.0]] * 7, orders=[list(range(64))] * 7)
    assert kept > 0 and removed > 0


@pytest.mark.parametrize("shape", ["five_sweeps", "twenty_quarter_sweeps"])
def test_both_sides_of_the_size_switches(tl, shape):
    """655 360 rows -- above the 2^19-row switch (the per-frame scan as a launch of its own instead of inside the finishing kernel; the
    tests above are below it) -- as five full 64 x 2048 sweeps and as 20 quarter sweeps (above the 16-frame switches of the prepass),
    device prepass and all, against the compact call."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    from lidar_snow_sim_amd.tensors import DeviceBatch
    full = [synthetic_sweep(64, 2048, seed=1420 + f, intensity="lambert") for f in range(5)]
    if shape == "five_sweeps":
        frames = full
    else:
        frames = [np.ascontiguousarray(s.reshape(64, 2048, 5)[:, q::4].reshape(-1, 5)) for s in full for q in range(4)]
    nf = len(frames)
    batch = DeviceBatch(torch.from_numpy(np.concatenate(frames)).cuda(), frame_rows=len(frames[0]))
    assert batch.rows.shape[0] == 655360 > (1 << 19) and len(batch) == nf
    orders = [list(np.random.default_rng(60 + f).permutation(64)) for f in range(nf)]
    kept, removed = _same_as_compact(batch, tl, planes=[PLANE] * nf, orders=orders)
    assert kept > 0 and removed > 0


def test_in_place_overwrites_the_input_with_the_out_of_place_bytes(tl):
    """in_place=True on a DeviceBatch of one channel-sorted and one firing-order frame: `rows` of the result IS the input tensor, which
    afterwards holds the bytes the out-of-place call returned; flags, counts and statistics are the same."""
    from lidar_snow_sim_amd.tensors import AlignedResult, DeviceBatch, augment_batch
    fr = _ragged_frames()
    frames = [fr[2][:8192], fr[1]]
    orders = [list(np.random.default_rng(70 + f).permutation(64)) for f in range(2)]
    kw = dict(planes=[PLANE] * 2, orders=orders, particles=tl, layout="aligned", sync=False)
    inp = torch.from_numpy(np.concatenate(frames)).cuda()
    want = augment_batch(DeviceBatch(inp.clone(), frame_rows=8192), "unused", BD, **kw).wait()
    assert want.rows.data_ptr() != inp.data_ptr()
    got = augment_batch(DeviceBatch(inp, frame_rows=8192), "unused", BD, in_place=True, **kw).wait()
    assert isinstance(got, AlignedResult) and got.rows.data_ptr() == inp.data_ptr()
    assert torch.equal(inp, want.rows) and torch.equal(got.keep, want.keep)
    assert torch.equal(got.counts, want.counts) and torch.equal(got.stats, want.stats)
    assert int((want.rows[:, 4] == 2).sum()) > 0 and int((~want.keep).sum()) > 0
    stack = torch.from_numpy(np.stack(frames)).cuda()                     # F x N x 5: read where it lies, too
    r3 = augment_batch(stack, "unused", BD, in_place=True, **kw).wait()
    assert r3.rows.data_ptr() == stack.data_ptr() and torch.equal(stack.reshape(-1, 5), want.rows)
    with pytest.raises(ValueError, match="concatenated"):
        augment_batch([stack[0], stack[1]], "unused", BD, in_place=True, **kw)
    with pytest.raises(ValueError, match="aligned"):
        augment_batch(stack, "unused", BD, in_place=True, **dict(kw, layout="compact"))


def test_options_against_the_compact_call(tl):
    """calib= (the flags follow the camera crop and num_removed counts it), thr_polys=, planes=None (calculate_plane on the device), rows
    of a channel without a laser (Q5: column 4 keeps the channel value), lane=0 -- each against the compact call -- and out= reuse with
    sync=False on a side stream."""
    from lidar_snow_sim_amd.calibration import Calibration
    from lidar_snow_sim_amd.tensors import AlignedResult, augment_batch
    cal = Calibration(P2=np.array([[700.0, 0, 960, 0], [0, 700.0, 512, 0], [0, 0, 1, 0]]), R0=np.eye(3),
                      V2C=np.array([[0, -1.0, 0, 0], [0, 0, -1.0, 0], [1.0, 0, 0, 0]]))
    frames = _ragged_frames()[:2]
    t_frames = [torch.from_numpy(f).cuda() for f in frames]
    orders = [list(np.random.default_rng(80 + f).permutation(64)) for f in range(2)]
    plain = _same_as_compact(t_frames, tl, planes=[PLANE] * 2, orders=orders)
    crop = _same_as_compact(t_frames, tl, planes=[PLANE] * 2, orders=orders, calib=cal)
    assert 0 < crop[0] < plain[0] and crop[0] + crop[1] == plain[0] + plain[1]      # the crop removed rows the noise filter kept
    _same_as_compact(t_frames, tl, thr_polys=[[0.0, 0.01, 2.0]] * 2, orders=orders)
    _same_as_compact(t_frames, tl, planes=None, orders=orders)
    _same_as_compact(t_frames, tl, planes=[PLANE] * 2, orders=orders, lane=0)
    q5 = [f.copy() for f in frames]
    q5[0][100:140, 4] = 70.0                                               # no such laser: copied through with its channel value
    q5[1][::97, 4] = 70.0
    t_q5 = [torch.from_numpy(f).cuda() for f in q5]
    _same_as_compact(t_q5, tl, planes=[PLANE] * 2, orders=orders)
    (_, rows, keep), _ = augment_batch(t_q5, "unused", BD, planes=[PLANE] * 2, orders=orders, particles=tl, layout="aligned")
    assert torch.all(rows[100:140, 4] == 70.0)
    # out= on a side stream: the second call writes the first one's tensors and sees the input changed on that stream
    s = torch.cuda.Stream()
    kw = dict(planes=[PLANE] * 2, orders=orders, particles=tl, layout="aligned")
    want = [augment_batch(t, "unused", BD, **kw) for t in (t_frames, t_frames[::-1])]
    with torch.cuda.stream(s):
        a, b = t_frames[0].clone(), t_frames[1].clone()
        r1 = augment_batch([a, b], "unused", BD, sync=False, **kw)
        assert isinstance(r1, AlignedResult) and r1.stream == s
        first = [(st, r.clone(), k.clone()) for st, r, k in r1.frames()]
        r2 = augment_batch([b, a], "unused", BD, sync=False, out=r1, **kw)
        assert r2.rows.data_ptr() == r1.rows.data_ptr() and r2.keep.data_ptr() == r1.keep.data_ptr()
        second = r2.frames()
    for got, ref in ((first, want[0]), (second, want[1])):
        for (s0, r0, k0), (s1, r1_, k1) in zip(got, ref):
            assert _stats(s0) == _stats(s1) and torch.equal(r0, r1_) and torch.equal(k0, k1)


def test_aligned_entry_and_a_consumer_in_one_hip_graph(tl):
    """snowgpu_augment_batch_device_aligned AND a consumer of its result -- the kept intensity per frame, (rows[:, 3] * keep).sum() --
    captured into one graph: replayed three times on changing input with no host read in between, every replay's sums equal those of
    plain calls.  (With the compact layout the consumer would need counts on the host to know its shapes.)"""
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    eng = engine.get_engine(0)
    dev = torch.device("cuda:0")
    F, n = 2, 64 * 256
    frames = [synthetic_sweep(64, 256, seed=1050 + f, intensity="lambert") for f in range(F)]
    other = [synthetic_sweep(64, 256, seed=1070 + f, intensity="lambert") for f in range(F)]
    rows = torch.from_numpy(np.concatenate(frames)).to(dev)
    off = torch.arange(F + 1, dtype=torch.int64, device=dev) * n
    tids = torch.tensor([eng.table_ids_from_arrays(tl, list(range(64))) for _ in range(F)], dtype=torch.int32, device=dev)
    plane = torch.tensor([[0.0, 0.0, -1.0, -1.7]] * F, dtype=torch.float64, device=dev)
    out = torch.empty_like(rows)
    keep = torch.zeros(F * n, dtype=torch.bool, device=dev)
    cnt = torch.zeros(F, dtype=torch.int64, device=dev)
    st = torch.zeros(F, 3, dtype=torch.int64, device=dev)
    status = torch.zeros(8, dtype=torch.int32, device=dev)
    sums = torch.zeros(F, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()

    def call():
        eng.ctx.augment_batch_device_aligned(F, F * n, n, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), BD, 0, plane.data_ptr(), 0.7, 0,
                                             out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)
        sums.copy_((out[:, 3].double() * keep).view(F, n).sum(1))         # the consumer: same stream, static shapes (integers: exact in float64)

    inputs = [rows.clone(), torch.from_numpy(np.concatenate(other)).to(dev), rows.clone()]
    with torch.cuda.stream(s):
        want = []
        for inp in inputs:                                                # plain calls (two each: the second allocates nothing)
            rows.copy_(inp)
            call()
            call()
            s.synchronize()
            assert int(status[0]) == 0
            want.append((sums.clone(), cnt.clone(), st.clone(), keep.clone()))
        assert not torch.equal(want[0][0], want[1][0]) and float(want[0][0].min()) > 0
        rows.copy_(inputs[0])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        got = []
        for inp in inputs:                                                # no host read between the replays
            rows.copy_(inp)
            g.replay()
            got.append((sums.clone(), cnt.clone(), st.clone(), keep.clone()))
        s.synchronize()
    assert int(status[0]) == 0
    for k in range(3):
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k


def test_errors(tl):
    """A point at >= 120 m sets the status words and raises the reference's IndexError through wait(); an output that overlaps the input
    without being it is rejected; wet= and NumPy input raise ValueError naming the reason."""
    from lidar_snow_sim_amd import _native, engine
    from lidar_snow_sim_amd.tensors import augment_batch as t_augment_batch
    from lidar_snow_sim_amd.tools.snowfall.simulation import augment_batch
    far = np.array([[125.0, 1.0, 0.0, 30.0, 3.0], [10.0, 1.0, -1.0, 30.0, 3.0]], np.float32)
    kw = dict(thr_polys=[[0.0, 0.0, 0.0]], shuffle=False, particles=tl, layout="aligned")
    r = t_augment_batch([torch.from_numpy(far).cuda()], "unused", float(np.degrees(3e-2)), sync=False, **kw)
    with pytest.raises(IndexError, match="range grid"):
        r.wait()
    assert int(r.status[0]) == _native.E_RANGE
    with pytest.raises(IndexError, match="range grid"):
        augment_batch([torch.from_numpy(far).cuda()], "unused", float(np.degrees(3e-2)), **kw)
    # partial aliasing: the output one row into the input
    eng = engine.get_engine(0)
    dev = torch.device("cuda:0")
    n = 1024
    buf = torch.zeros(n + 1, 5, dtype=torch.float32, device=dev)
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    tids = torch.tensor([eng.table_ids_from_arrays(tl, list(range(64)))], dtype=torch.int32, device=dev)
    poly = torch.zeros(1, 3, dtype=torch.float64, device=dev)
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    cnt, st, status = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, 3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
    with pytest.raises(_native.SnowGPUError, match="overlaps") as ei:
        eng.ctx.augment_batch_device_aligned(1, n, n, off.data_ptr(), buf.data_ptr(), 0, tids.data_ptr(), BD, poly.data_ptr(), 0, 0.7, 0,
                                             buf[1:].data_ptr(), keep.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), 0)
    assert ei.value.code == _native.E_INVALID
    pc = _ragged_frames()[1]
    with pytest.raises(ValueError, match="wet"):
        augment_batch([torch.from_numpy(pc).cuda()], "unused", BD, planes=[PLANE], particles=tl, layout="aligned", wet=dict(plane=PLANE))
    with pytest.raises(ValueError, match="aligned"):
        augment_batch([pc], "unused", BD, planes=[PLANE], particles=tl, layout="aligned")
    with pytest.raises(ValueError, match="layout"):
        augment_batch([torch.from_numpy(pc).cuda()], "unused", BD, planes=[PLANE], particles=tl, layout="sorted")


def test_compact_fused_entry_ignores_wet_lines_and_the_aligned_wet_entry_takes_them(tl):
    """Lines left by snowgpu_set_wet_lines: snowgpu_augment_wet_batch_device never looks at them -- rows, src, counts and flags of the compact
    fused call are the same bytes with and without -- and they stay set; the next wet_ground_batch_aligned(lines=None) on the context
    takes them (its result is that of lines=LINES, not that of the device's fit) and clears them.  Two float32 frames of 1 200 rows, all
    of them ground rows (prepass_reference.road, the generator of the wet aligned tests' frames), under tables thinned to 40 flakes a
    line: the snowfall stage removes the frames' dark rows (186 and 177) and scatters a dozen, so both keep more than 1 000 ground rows
    and the wet model runs (flag 0; with 1 150 ground rows of 1 200 it does not)."""
    import prepass_reference as pr
    from lidar_snow_sim_amd import engine
    from lidar_snow_sim_amd.tensors import augment_batch, wet_ground_batch_aligned
    eng = engine.get_engine(0)
    frames = [torch.from_numpy(pr.road(1200, 0, 430 + k, np.float32)).cuda() for k in (1, 2)]
    thin = [np.ascontiguousarray(t[:40]) for t in tl]
    lines = np.array([pr.LINES] * 2, np.float64)
    kw = dict(planes=[PLANE] * 2, orders=[list(range(64))] * 2, particles=thin, return_src=True, wet=dict(pr.LINES_PARAMS, plane=PLANE), sync=True)

    def fused():
        out = augment_batch(frames, "unused", BD, **kw)
        return [(tuple(int(v) for v in st), aug.cpu().numpy().tobytes(), src.cpu().numpy().tobytes(), int(aug.shape[0])) for st, aug, src in out]

    def wet_only(given):
        r = wet_ground_batch_aligned(frames, None, plane=PLANE, lines=given, sync=False, **pr.LINES_PARAMS).wait()
        assert r.flags.tolist() == [0, 0]
        return r
    try:
        flags = augment_batch(frames, "unused", BD, **dict(kw, sync=False)).wait().flags.tolist()
        assert flags == [0, 0], flags                      # the wet model did run behind the snowfall
        without = fused()
        eng.ctx.set_wet_lines(lines)
        with_lines = fused()
        assert with_lines == without and all(0 < f[3] < 1000 for f in without)       # (fewer than the snowfall stage left: the wet stage dropped rows)
        left = wet_only(None)                              # the lines are still there: this call consumes them
        plain = wet_only(None)
        given = wet_only(lines)
    finally:
        eng.ctx.set_wet_lines(None)
    assert torch.equal(left.rows, given.rows) and torch.equal(left.keep, given.keep) and torch.equal(left.counts, given.counts)
    assert not torch.equal(left.rows, plain.rows) and not torch.equal(given.counts, plain.counts)
