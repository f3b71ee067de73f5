"""-m gpu: the pass over all rows with the step-major range index (csrc/sg_range_index.h; sg_beam.h: sg_wave_scan) against the CPU twin,
which runs the same per-beam code with no index at all, on inputs that lean on the index (tests/range_index_inputs.py): waves that
straddle the 0 / 2 pi seam, ranges exactly on the index's steps, beyond its last step and NaN -- on small random tables, empty tables
and a table with nearly half its flakes in one bin.  tests/test_range_index.py holds the twin to the oracle on the same inputs."""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded: PyTorch bundles its own HIP runtime, and the process must end up with one

import range_index_inputs as rii

pytestmark = pytest.mark.gpu

ORDER = list(range(64))


@pytest.fixture(scope="module")
def twin():
    from lidar_snow_sim_amd import build, _cpu_twin
    build.build_cpu_twin(verbose=False)
    return _cpu_twin


@pytest.fixture(scope="module")
def sets():
    return rii.table_sets()


@pytest.fixture(scope="module")
def reference(twin, sets):
    """name, dtype -> the twin's [(stats, rows, src)] of the two frames, computed once"""
    cache = {}

    def get(name, dtype):
        key = (name, np.dtype(dtype).name)
        if key not in cache:
            frames = [rii.seam_frame(dtype), rii.edge_frame(dtype)]
            cache[key] = (frames, twin.augment_batch(frames, sets[name], [ORDER, ORDER], rii.BD, [rii.POLY, rii.POLY], threads=8))
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["small", "empty", "heavy"])
def test_seam_and_step_edge_frames_match_the_cpu_twin(reference, sets, name, dtype):
    from lidar_snow_sim_amd import engine
    frames, want = reference(name, dtype)
    n = frames[0].shape[0]
    eng = engine.Engine(0)
    try:
        tids = eng.table_ids_from_arrays(sets[name], ORDER)
        out, src, counts, stats, _ = eng.ctx.augment_batch(np.concatenate(frames), [0, n, 2 * n], [tids, tids], rii.BD, thr_poly=[rii.POLY, rii.POLY])
    finally:
        eng.ctx.close()
    for f, (st, aug, src0) in enumerate(want):
        m = int(counts[f])
        assert tuple(int(v) for v in stats[f]) == tuple(int(v) for v in st), (f, stats[f], st)
        assert m == aug.shape[0] and np.array_equal(src[f * n:f * n + m], src0), f
        got = out[f * n:f * n + m]
        assert np.array_equal(got[:, 3:], aug[:, 3:]), f
        np.testing.assert_allclose(got[:, :3], aug[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
    if name == "empty":
        assert all(not np.isin(aug[:, 4], (1, 2)).any() for _, aug, _ in want)        # no flake: nothing attenuated, nothing scattered
    else:
        assert sum(int((aug[:, 4] == 2).sum()) + int((aug[:, 4] == 1).sum()) for _, aug, _ in want) > 20


def test_the_indexed_scan_replays_from_a_hip_graph(reference, sets):
    """The device entry on the two frames, captured once and replayed: the rows of the plain call, which are the twin's."""
    from lidar_snow_sim_amd import engine
    frames, want = reference("small", np.float32)
    dev = torch.device("cuda:0")
    F, n = 2, frames[0].shape[0]
    eng = engine.Engine(0)
    try:
        rows = torch.from_numpy(np.concatenate(frames)).to(dev)
        off = torch.arange(F + 1, dtype=torch.int64, device=dev) * n
        tids = torch.tensor([eng.table_ids_from_arrays(sets["small"], ORDER)] * F, dtype=torch.int32, device=dev)
        thr = torch.tensor([rii.POLY] * F, dtype=torch.float64, device=dev)
        out = torch.empty_like(rows)
        src = torch.empty(F * n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(F, dtype=torch.int64, device=dev)
        st = torch.zeros(F, 3, dtype=torch.int64, device=dev)
        status = torch.zeros(8, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream()

        def call():
            eng.ctx.augment_batch_device(F, F * n, n, off.data_ptr(), rows.data_ptr(), 0, tids.data_ptr(), rii.BD, thr.data_ptr(), 0, 0.7, 0,
                                         out.data_ptr(), src.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0, status.data_ptr(), s.cuda_stream)

        with torch.cuda.stream(s):
            call()
            call()                                   # the second call allocates nothing
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                call()
            for _ in range(2):
                out.zero_(); src.zero_(); cnt.zero_(); st.zero_()
                g.replay()
                s.synchronize()
                assert int(status[0]) == 0
                for f, (st0, aug, src0) in enumerate(want):
                    m = int(cnt[f])
                    assert m == aug.shape[0] and tuple(int(v) for v in st[f]) == tuple(int(v) for v in st0), f
                    assert np.array_equal(src[f * n:f * n + m].cpu().numpy(), src0), f
                    got = out[f * n:f * n + m].cpu().numpy()
                    assert np.array_equal(got[:, 3:], aug[:, 3:]), f
                    np.testing.assert_allclose(got[:, :3], aug[:, :3], rtol=1e-6, atol=0)
    finally:
        eng.ctx.close()
