"""-m gpu: the pass over all rows on the step-major range index the library files, whose scan searches nothing and drops the candidates at or
beyond the target in its pair loop (csrc/sg_range_index.h; sg_beam.h: sg_wave_scan), against the CPU twin byte for byte.  The twin runs the
same per-beam code with no index at all, so it does not depend on the index or on the missing search.  Inputs: the seam and step-edge
frames and the table sets of tests/range_index_inputs.py -- `heavy` sends its seam beams to the global-list tier, the fallback of the list
tiers -- and, in the same call, the frame of tests/fine_index_inputs.py on its hand-made table: ranges on the 2 m edges and at records'
exact ranges.  tests/test_range_index.py and tests/test_fine_index.py hold the twin to the oracle on these inputs."""
import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded: PyTorch bundles its own HIP runtime, and the process must end up with one

import fine_index_inputs as fii
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
def fine_reference(twin):
    """dtype -> (frame, the twin's (stats, rows, src) of the fine frame on its table), computed once"""
    cache = {}

    def get(dtype):
        key = np.dtype(dtype).name
        if key not in cache:
            pc = fii.fine_frame(dtype)
            cache[key] = (pc, twin.augment_batch([pc], fii.tables(), [ORDER], rii.BD, [rii.POLY], threads=8)[0])
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["small", "empty", "heavy"])
def test_three_frames_equal_the_cpu_twin_byte_for_byte(twin, sets, fine_reference, name, dtype):
    from lidar_snow_sim_amd import engine
    two = [rii.seam_frame(dtype), rii.edge_frame(dtype)]
    fine, want_fine = fine_reference(dtype)
    want = list(twin.augment_batch(two, sets[name], [ORDER, ORDER], rii.BD, [rii.POLY, rii.POLY], threads=8)) + [want_fine]
    frames = two + [fine]
    n = frames[0].shape[0]
    eng = engine.Engine(0)
    try:
        tids = eng.table_ids_from_arrays(sets[name], ORDER)
        tids_fine = eng.table_ids_from_arrays(fii.tables(), ORDER)
        out, src, counts, stats, _ = eng.ctx.augment_batch(np.concatenate(frames), [0, n, 2 * n, 3 * n], [tids, tids, tids_fine], rii.BD,
                                                           thr_poly=[rii.POLY] * 3)
    finally:
        eng.ctx.close()
    for f, (st, aug, src0) in enumerate(want):
        m = int(counts[f])
        assert tuple(int(v) for v in stats[f]) == tuple(int(v) for v in st), (f, stats[f], st)
        assert m == aug.shape[0] and np.array_equal(src[f * n:f * n + m], src0), f
        got = np.ascontiguousarray(out[f * n:f * n + m])
        assert got.dtype == aug.dtype and got.tobytes() == np.ascontiguousarray(aug).tobytes(), f
    assert int(np.isin(want_fine[1][:, 4], (1, 2)).sum()) > 20
