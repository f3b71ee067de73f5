"""-m gpu: the dict queue of the pass over all rows as words (csrc/sg_queue.h: range, azimuth, one word per listed flake; the readers resolve
the words against the table's records) through every kernel that writes or reads it, against the oracle -- occlusion dicts, output rows and
status words, the way tests/test_gpu_row_tiers.py checks (its references and checks are used as they are).

Writers: k_beams in the segment order, in linear chunks (a caller's permutation) and in the exact-math form.  Readers: k_power_few (the plain
call) and k_power<4> (the occlusion tap switches k_power_few off, so the one- and two-flake slots go through k_power's loader); the loaders of
the capacities 8 and 16 (SNOWGPU_FIRST_TIER), the latter in k_power's three-column form, which fetches the ranges a second time.  Frames:
main, plain and wide of tests/row_tier_inputs.py, and `crowd` (tests/queue_words_inputs.py): one region with a front run that crosses a group
of 64 slots, back-filled slots behind it and items that do not fill their wave -- tests/test_queue_words.py shows that on the CPU."""
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded: PyTorch bundles its own HIP runtime, and the process must end up with one

import queue_words_inputs as qwi
import row_tier_inputs as rti
import test_gpu_row_tiers as trt

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@lru_cache(maxsize=None)
def _crowd_reference(dtype_name):
    """the oracle on the crowd frame, computed once (the shape of test_gpu_row_tiers._reference)"""
    from oracle import snow_oracle as so
    fr = qwi.crowd(np.dtype(dtype_name).type)
    rows, tl, bd, las = fr["rows"], fr["tables"], fr["bd"], so.load_lasers()
    dicts = [None] * rows.shape[0]
    for ch in np.unique(rows[:, 4]).astype(int):
        idx = np.flatnonzero(rows[:, 4] == ch)
        _, _, (cnt, _, rj, ratio) = so.process_single_channel(rows[idx], tl[ch], bd, las, ch, dump=True)
        start = np.concatenate(([0], np.cumsum(cnt)))
        for k, i in enumerate(idx):
            dicts[i] = (rj[start[k]:start[k + 1]].copy(), ratio[start[k]:start[k + 1]].copy())
    return dict(fr, dicts=dicts, aug=so.augment(rows, tl, bd, trt.ORDER, thr_poly=np.array(rti.POLY)))


def _reference(dtype, frame):
    if frame == "crowd":
        return _crowd_reference(np.dtype(dtype).name), qwi.EXPECTED
    return trt.reference(dtype, frame), rti.EXPECTED[frame]


def _run(monkeypatch, dtype, frame, first=4, exact=False, perm=False):
    """the occlusion tap and the plain call on one frame: dicts, rows, status words"""
    from lidar_snow_sim_amd import engine
    if first != 4:
        monkeypatch.setenv("SNOWGPU_FIRST_TIER", str(first))
    ref, expected = _reference(dtype, frame)
    rows, bd, n = ref["rows"], ref["bd"], ref["rows"].shape[0]
    e = engine.Engine(0)
    try:
        if exact:
            e.ctx.set_exact_math(True)
        tids = e.table_ids_from_arrays(ref["tables"], trt.ORDER)
        occ = e.ctx.debug_occlusions(rows, tids, bd, cap=80)
        st_occ = e.ctx.last_status().copy()
        # the rows are channel-major: the identity is their channel sort, and with it the pass over all rows walks linear chunks
        got = e.ctx.augment_batch(rows, [0, n], [tids], bd, thr_poly=[rti.POLY], perm=np.arange(n, dtype=np.int32) if perm else None)
        st = e.ctx.last_status().copy()
    finally:
        e.ctx.close()
    what = (frame, np.dtype(dtype).name, first, exact, perm)
    trt._check_dicts(ref, occ, what)
    trt._check_rows(ref, got, what)
    pop, redo = expected[first]
    for s in (st_occ, st):
        assert s[0] == 0 and s[2:6].tolist() == pop and s[6] == redo, (what, s)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", ["main", "plain", "wide", "crowd"])
def test_both_readers_on_every_frame(monkeypatch, frame, dtype):
    _run(monkeypatch, dtype, frame)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", ["main", "crowd"])
def test_linear_chunks_of_a_callers_permutation(monkeypatch, frame, dtype):
    _run(monkeypatch, dtype, frame, perm=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frame", ["main", "crowd"])
def test_exact_math_form(monkeypatch, frame, dtype):
    _run(monkeypatch, dtype, frame, exact=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("first", [8, 16])
@pytest.mark.parametrize("frame", ["main", "crowd"])
def test_longer_first_lists(monkeypatch, frame, first, dtype):
    _run(monkeypatch, dtype, frame, first=first)
