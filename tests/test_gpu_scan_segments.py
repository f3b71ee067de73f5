"""-m gpu: the segment order of the pass over all rows (csrc/snowgpu_kernels.hip: k_beams, SEG -- a block serves one (frame, channel)
segment and keeps its frame, channel, row base and table descriptor in scalar registers; sg_beam.h: sg_wave_scan_t, UTAB) against the CPU
twin, which runs the same per-beam code one beam at a time, on one batch of ragged segments (tests/scan_segment_inputs.py): segments
shorter than a wave, of two blocks, an empty channel between full ones, channels without a laser, a frame read in place beside one read
through its sorted copy, an empty frame, rows on the 0 / 2 pi seam and with NaN coordinates; every table set, and a wedge three bins wide.
tests/test_scan_segments.py holds the twin to the oracle on the same inputs."""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded: PyTorch bundles its own HIP runtime, and the process must end up with one

import scan_segment_inputs as ssi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin():
    from lidar_snow_sim_amd import build, _cpu_twin
    build.build_cpu_twin(verbose=False)
    return _cpu_twin


@pytest.fixture(scope="module")
def sets():
    return ssi.table_sets()


@pytest.fixture(scope="module")
def reference(twin, sets):
    """name, wide, dtype -> the frames and the twin's [(stats, rows, src)], computed once"""
    cache = {}

    def get(name, wide, dtype):
        key = (name, wide, np.dtype(dtype).name)
        if key not in cache:
            frames = ssi.frames(dtype)
            cache[key] = (frames, twin.augment_batch(frames, sets[name], ssi.orders(), ssi.BD * wide, [ssi.POLY] * len(frames), threads=8))
        return cache[key]
    return get


def _offsets(frames):
    return [0] + [int(v) for v in np.cumsum([f.shape[0] for f in frames])]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,wide", ssi.CASES)
def test_ragged_segments_match_the_cpu_twin(reference, sets, name, wide, dtype):
    from lidar_snow_sim_amd import engine
    frames, want = reference(name, wide, dtype)
    off = _offsets(frames)
    eng = engine.Engine(0)
    try:
        tids = [eng.table_ids_from_arrays(sets[name], o) for o in ssi.orders()]
        out, src, counts, stats, _ = eng.ctx.augment_batch(np.concatenate(frames), off, tids, ssi.BD * wide, thr_poly=[ssi.POLY] * len(frames))
    finally:
        eng.ctx.close()
    for f, (st, aug, src0) in enumerate(want):
        m, a = int(counts[f]), off[f]
        assert tuple(int(v) for v in stats[f]) == tuple(int(v) for v in st), (f, stats[f], st)
        assert m == aug.shape[0] and np.array_equal(src[a:a + m], src0), f
        got = out[a:a + m]
        assert np.array_equal(got[:, 3:], aug[:, 3:]), f
        np.testing.assert_allclose(got[:, :3], aug[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
    assert int(counts[2]) == 0                                                        # the empty frame
    hit = sum(int((aug[:, 4] == 2).sum()) + int((aug[:, 4] == 1).sum()) for _, aug, _ in want)
    assert hit == 0 if name == "empty" else hit > 20
    through = sum(int((aug[:, 4] >= ssi.N_LASERS).sum()) for _, aug, _ in want)
    assert through > 100                                                              # channels without a laser: copied through


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_unknown_table_id_of_one_segment_fails_the_call(sets, dtype):
    """One (frame, channel) of the batch names a table that was never uploaded: the block-uniform branch of the scan reports what the per-lane
    test reported -- SNOWGPU_E_INVALID and the message of status_to_error (snowgpu_batch.cpp)."""
    from lidar_snow_sim_amd import engine, _native
    frames = ssi.frames(dtype)
    off = _offsets(frames)
    eng = engine.Engine(0)
    try:
        tids = [list(eng.table_ids_from_arrays(sets["small"], o)) for o in ssi.orders()]
        tids[1][8] = 12345                                                            # frame 1 (sorted copy), channel 8: 300 rows, two blocks
        with pytest.raises(_native.SnowGPUError) as e:
            eng.ctx.augment_batch(np.concatenate(frames), off, tids, ssi.BD, thr_poly=[ssi.POLY] * len(frames))
        assert e.value.code == _native.E_INVALID
        assert "a table id in table_ids was never uploaded" in str(e.value)
        tids[1][8] = tids[1][9]                                                       # the engine is usable afterwards
        counts = eng.ctx.augment_batch(np.concatenate(frames), off, tids, ssi.BD, thr_poly=[ssi.POLY] * len(frames))[2]
        assert int(counts[0]) > 0 and int(counts[2]) == 0
    finally:
        eng.ctx.close()
