"""-m gpu: per-frame weather in one aligned call -- snowgpu_augment_weather_batch_device_aligned (gates and wet settings per frame, in
device memory) and snowgpu_draw_weather_device (csrc/snowgpu_weather.hip: k_draw_weather) -- through the ctypes bindings and through
augment_wet_batch_aligned(weather=, table_ids=), weather_records and WeatherPlan.

The yardstick for frame f is an EXISTING entry called on the same batch (same keep-in, tables, planes, camera crop) with frame f's
values as its scalars, sliced to frame f, byte for byte:
    snow wet   entry                                                    flag
     1    1    snowgpu_augment_wet_batch_device_aligned_masked          its flag
     1    0    snowgpu_augment_batch_device_aligned_masked              2
     0    1    snowgpu_wet_ground_batch_device_aligned on the input     its flag   (statistics / polynomial row of an empty frame)
     0    0    the input itself, keep = keep-in                         2
tests/test_gpu_aligned_mask.py and tests/test_gpu_wet_aligned.py hold those entries to the oracle; two frames go there directly here.
Inputs and their claimed properties: tests/weather_reference.py, checked without a GPU by tests/test_weather_reference.py."""
import numpy as np
import pytest
import torch

import aligned_mask_inputs as ami
import weather_reference as wr

pytestmark = pytest.mark.gpu

BD = ami.BD
PLANE = ami.PLANE
DEV = "cuda:0"


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
def sets(tables):
    return wr.table_sets(tables["t"])


@pytest.fixture(scope="module")
def set_ids(eng, sets):
    return np.asarray([eng.table_ids_from_arrays(s, list(range(64))) for s in sets], np.int32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class Batch:
    """Device arrays of one batch: rows, offsets, table ids, planes, keep-in (or None), optional caller polynomials."""

    def __init__(self, frames, tids, masks=None, poly=None):
        self.frames, self.masks = frames, masks
        self.off = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
        self.nf, self.n, self.max = len(frames), int(self.off[-1]), int(np.diff(self.off).max())
        self.rows, self.d_off, self.tids = _t(np.concatenate(frames)), _t(self.off), _t(np.asarray(tids, np.int32))
        self.keep = None if masks is None else _t(np.concatenate(masks))
        self.plane = torch.tensor([wr.PLANE4] * self.nf, dtype=torch.float64, device=DEV)
        self.poly = None if poly is None else torch.tensor([poly] * self.nf, dtype=torch.float64, device=DEV)
        self.code = 0 if frames[0].dtype == np.float32 else 1

    def outputs(self, in_place=False):
        o = dict(rows=self.rows.clone() if in_place else torch.empty_like(self.rows),
                 keep=(self.keep.clone() if in_place and self.keep is not None else torch.empty(self.n, dtype=torch.bool, device=DEV)),
                 cnt=torch.zeros(self.nf, dtype=torch.int64, device=DEV), st=torch.full((self.nf, 3), -1, dtype=torch.int64, device=DEV),
                 thr=torch.zeros(self.nf, 3, dtype=torch.float64, device=DEV), status=torch.zeros(8, dtype=torch.int32, device=DEV),
                 flags=torch.full((self.nf,), -1, dtype=torch.int32, device=DEV))
        # in place: the input IS the output (rows, and the keep bytes when a mask came in)
        o["in_rows"] = o["rows"] if in_place else self.rows
        o["in_keep"] = o["keep"] if in_place and self.keep is not None else self.keep
        return o

    def head(self, o):
        return (self.nf, self.n, self.max, self.d_off.data_ptr(), o["in_rows"].data_ptr(), self.code, self.tids.data_ptr(), BD, _ptr(self.poly),
                0 if self.poly is not None else self.plane.data_ptr(), 0.7, 0)


def _host(o):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items() if k not in ("in_rows", "in_keep")}


def run_weather(eng, b, rec, in_place=False, flat_earth=False, replace=False, stream=0):
    o = b.outputs(in_place)
    w = _t(rec)
    torch.cuda.synchronize()
    eng.ctx.augment_weather_batch_device_aligned(*b.head(o), _ptr(o["in_keep"]), o["rows"].data_ptr(), o["keep"].data_ptr(), o["cnt"].data_ptr(),
                                                 o["st"].data_ptr(), o["thr"].data_ptr(), o["status"].data_ptr(), stream, b.plane.data_ptr(),
                                                 w.data_ptr(), flat_earth, replace, o["flags"].data_ptr())
    return _host(o)


def run_snow_masked(eng, b, keep):
    o = b.outputs()
    torch.cuda.synchronize()
    eng.ctx.augment_batch_device_aligned_masked(*b.head(o), _ptr(keep), o["rows"].data_ptr(), o["keep"].data_ptr(), o["cnt"].data_ptr(),
                                                o["st"].data_ptr(), o["thr"].data_ptr(), o["status"].data_ptr(), 0)
    return _host(o)


def run_wet_masked(eng, b, setting, flat_earth=False, replace=False):
    o = b.outputs()
    wh, pd, nf_, pf, delta = setting
    torch.cuda.synchronize()
    eng.ctx.augment_wet_batch_device_aligned_masked(*b.head(o), _ptr(b.keep), o["rows"].data_ptr(), o["keep"].data_ptr(), o["cnt"].data_ptr(),
                                                    o["st"].data_ptr(), o["thr"].data_ptr(), o["status"].data_ptr(), 0, b.plane.data_ptr(), wh, pd,
                                                    nf_, pf, flat_earth, delta, replace, o["flags"].data_ptr())
    return _host(o)


def run_wet_only(eng, b, setting, flat_earth=False, replace=False):
    o = b.outputs()
    wh, pd, nf_, pf, delta = setting
    torch.cuda.synchronize()
    eng.ctx.wet_ground_batch_device_aligned(b.nf, b.n, b.max, b.d_off.data_ptr(), b.rows.data_ptr(), b.code, _ptr(b.keep), b.plane.data_ptr(), wh, pd,
                                            nf_, pf, flat_earth, delta, replace, o["rows"].data_ptr(), o["keep"].data_ptr(), o["cnt"].data_ptr(),
                                            o["flags"].data_ptr(), o["status"].data_ptr(), 0)
    return _host(o)


def yardsticks(eng, b, rec, **kw):
    """Per frame the expected (rows, keep, count, stats, thr row, flag) from the existing entries, and those entries' own results."""
    rec = np.asarray(rec)
    settings = {f: tuple(rec[f, 2:7]) for f in range(b.nf)}
    snow_y = run_snow_masked(eng, b, b.keep)
    # a frame the snowfall stage leaves out: statistics and polynomial row of the masked entry for a frame with no present row
    gate = np.concatenate([np.full(len(fr), bool(rec[f, 0])) for f, fr in enumerate(b.frames)])
    if b.masks is not None:
        gate &= np.concatenate(b.masks)
    empty_y = run_snow_masked(eng, b, _t(gate))
    wet_y, only_y = {}, {}
    keep_in = np.concatenate(b.masks) if b.masks is not None else np.ones(b.n, bool)
    inp = np.concatenate(b.frames)
    want = []
    for f in range(b.nf):
        a, e = int(b.off[f]), int(b.off[f + 1])
        snow, wet = bool(rec[f, 0]), bool(rec[f, 1])
        if snow and wet:
            if settings[f] not in wet_y:
                wet_y[settings[f]] = run_wet_masked(eng, b, settings[f], **kw)
            y = wet_y[settings[f]]
            want.append((y["rows"][a:e], y["keep"][a:e], y["cnt"][f], y["st"][f], y["thr"][f], int(y["flags"][f])))
        elif snow:
            y = snow_y
            want.append((y["rows"][a:e], y["keep"][a:e], int(y["keep"][a:e].sum()), y["st"][f], y["thr"][f], 2))
        elif wet:
            if settings[f] not in only_y:
                only_y[settings[f]] = run_wet_only(eng, b, settings[f], **kw)
            y = only_y[settings[f]]
            want.append((y["rows"][a:e], y["keep"][a:e], y["cnt"][f], np.zeros(3, np.int64), empty_y["thr"][f], int(y["flags"][f])))
        else:
            want.append((inp[a:e], keep_in[a:e], int(keep_in[a:e].sum()), np.zeros(3, np.int64), empty_y["thr"][f], 2))
        if not snow:
            assert tuple(empty_y["st"][f]) == (0, 0, 0)
    return want, dict(snow=snow_y, wet=wet_y, only=only_y)


def same(got, want, b):
    for f, (rows, keep, cnt, st, thr, flag) in enumerate(want):
        a, e = int(b.off[f]), int(b.off[f + 1])
        assert got["rows"][a:e].tobytes() == np.ascontiguousarray(rows).tobytes(), f"rows of frame {f}"
        assert np.array_equal(got["keep"][a:e], keep), f"keep bytes of frame {f}"
        assert int(got["cnt"][f]) == int(cnt), f"count of frame {f}: {int(got['cnt'][f])}, expected {int(cnt)}"
        assert tuple(got["st"][f]) == tuple(st), f"statistics of frame {f}"
        assert got["thr"][f].tobytes() == np.ascontiguousarray(thr).tobytes(), f"polynomial row of frame {f}"
        assert int(got["flags"][f]) == flag, f"flag of frame {f}: {int(got['flags'][f])}, expected {flag}"


@pytest.fixture(scope="module")
def main_tids(set_ids):
    return wr.draw(wr.MAIN_SEED, wr.MAIN_STEP, 8, set_ids, wr.DEFAULT_PLAN)[0]


_MAIN = {}


def main_batch(eng, main_tids, dtype, masked):
    """The main batch and its yardsticks, computed once per (dtype, mask) and left unchanged."""
    key = (np.dtype(dtype).name, masked)
    if key not in _MAIN:
        frames = wr.main_frames(dtype)
        b = Batch(frames, main_tids, wr.main_masks(frames) if masked else None)
        _MAIN[key] = (b,) + yardsticks(eng, b, wr.main_records())
    return _MAIN[key]


# ---- 1. the main batch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_main_batch_equals_the_existing_entries_frame_by_frame(eng, main_tids, dtype, in_place, masked):
    """8 frames, two of each gate pair, three wet settings, five table sets in drawn per-frame orders: every frame byte for byte the
    existing entry's; on the yardsticks themselves: every snow frame scatters and removes, every processed wet frame drops ground rows,
    the small wet = 1 frame gives flag 1 beside wet = 0 frames giving flag 2."""
    b, want, y = main_batch(eng, main_tids, dtype, masked)
    got = run_weather(eng, b, wr.main_records(), in_place=in_place)
    assert int(got["status"][0]) == 0
    same(got, want, b)
    present = np.concatenate(b.masks) if masked else np.ones(b.n, bool)
    for f, (snow, wet, _) in enumerate(wr.MAIN_FRAMES):
        a, e = int(b.off[f]), int(b.off[f + 1])
        rows, keep, cnt, st, thr, flag = want[f]
        if snow:
            sy = y["snow"]
            assert int((sy["rows"][a:e][sy["keep"][a:e], 4] == 2).sum()) >= 1 and int((present[a:e] & ~sy["keep"][a:e]).sum()) >= 1, f
            assert np.abs(thr).sum() > 0, f
        if wet and flag == 0:
            before = y["snow"]["keep"][a:e] if snow else present[a:e]
            assert int((before & ~keep).sum()) >= 1, f
    flags = [w[5] for w in want]
    assert flags[wr.MAIN_SMALL] == 1 and flags[1] == flags[2] == flags[6] == flags[7] == 2 and flags[0] == flags[3] == flags[4] == 0


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_a_snow_only_and_a_wet_only_frame_against_the_oracle(eng, so, sets, set_ids, main_tids, dtype):
    """Frame 2 (snow only) against oracle.snow_oracle.augment on f[m] with the comparisons of tests/test_gpu_aligned_mask.py (labels and
    intensities exact, coordinates rtol 1e-6 float32 / 1e-12 float64, statistics equal); frame 3 (wet only) against
    ground_water_augmentation on f[m] through the check of tests/test_gpu_wet_aligned.py (its tolerances)."""
    import test_gpu_wet_aligned as twa
    b, want, _ = main_batch(eng, main_tids, dtype, True)
    got = run_weather(eng, b, wr.main_records())
    _, _, s, _, _, order = wr.draw_frame(wr.MAIN_SEED, wr.MAIN_STEP, 2, 64, wr.MAIN_SETS, wr.DEFAULT_PLAN)
    assert np.array_equal(main_tids[2], set_ids[s][order])
    a, e = int(b.off[2]), int(b.off[3])
    pc, m = b.frames[2], b.masks[2]
    P = np.flatnonzero(m)
    s0, a0, src0 = so.augment(pc[m], sets[s], BD, order, plane=PLANE)
    rows, flags = got["rows"][a:e], got["keep"][a:e]
    assert tuple(int(v) for v in got["st"][2]) == tuple(int(v) for v in s0)
    assert np.array_equal(np.flatnonzero(flags), P[np.sort(src0)])
    assert np.array_equal(rows[P[src0]][:, 3:], a0[:, 3:])
    np.testing.assert_allclose(rows[P[src0]][:, :3], a0[:, :3], rtol=1e-6 if dtype == np.float32 else 1e-12, atol=0)
    a, e = int(b.off[3]), int(b.off[4])
    wh, pd, nf_, pf, delta = wr.SETTINGS[wr.MAIN_FRAMES[3][2]]
    kw = dict(water_height=wh, pavement_depth=pd, noise_floor=nf_, power_factor=pf, delta=delta, flat_earth=False, replace=False)
    assert twa.PLANE[1] == wr.PLANE4[3] and list(twa.PLANE[0]) == wr.PLANE4[:3]
    fails, _ = twa._check(so, "frame 3", b.frames[3], b.masks[3], kw, got["rows"][a:e], got["keep"][a:e], got["cnt"][3], int(got["flags"][3]),
                          "f32" if dtype == np.float32 else "f64")
    assert not fails, "\n".join(fails)


# ---- 3. a frame with both gates off is never looked at -----------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
def test_poisoned_gated_frames_change_nothing(eng, main_tids, masked):
    """NaN, a 500 m range and channel 999 in every row of the (0, 0) frames: status word 0, those rows back bit for bit, every other
    frame's bytes as in the benign run."""
    b, want, _ = main_batch(eng, main_tids, np.float32, masked)
    off = [f for f, g in enumerate(wr.MAIN_FRAMES) if g[:2] == (0, 0)]
    bad = wr.poison(b.frames, off)
    pb = Batch(bad, main_tids, b.masks)
    benign = run_weather(eng, b, wr.main_records())
    for in_place in (False, True):
        got = run_weather(eng, pb, wr.main_records(), in_place=in_place)
        assert int(got["status"][0]) == 0 and np.array_equal(got["status"], benign["status"])
        poisoned = list(want)
        for f in off:
            poisoned[f] = (bad[f],) + want[f][1:]
            assert np.isnan(got["rows"][int(b.off[f]):int(b.off[f + 1])]).any()
        same(got, poisoned, pb)


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------------
def test_all_gates_off_and_all_gates_on(eng, main_tids):
    """All off: the input back bit for bit, keep = keep-in, flags 2, status 0.  All on without a mask: the bytes of
    snowgpu_augment_wet_batch_device_aligned."""
    b, _, _ = main_batch(eng, main_tids, np.float32, True)
    rec = wr.main_records()
    rec[:, :2] = 0.0
    got = run_weather(eng, b, rec)
    assert got["rows"].tobytes() == np.concatenate(b.frames).tobytes() and np.array_equal(got["keep"], np.concatenate(b.masks))
    assert got["flags"].tolist() == [2] * 8 and not got["st"].any() and int(got["status"][0]) == 0
    assert got["cnt"].tolist() == [int(m.sum()) for m in b.masks]
    b, _, _ = main_batch(eng, main_tids, np.float32, False)
    setting = wr.SETTINGS[0]
    rec = np.zeros((8, 8))
    rec[:, :7] = (1.0, 1.0) + setting
    got = run_weather(eng, b, rec)
    o = b.outputs()
    wh, pd, nf_, pf, delta = setting
    torch.cuda.synchronize()
    eng.ctx.augment_wet_batch_device_aligned(*b.head(o), o["rows"].data_ptr(), o["keep"].data_ptr(), o["cnt"].data_ptr(), o["st"].data_ptr(),
                                             o["thr"].data_ptr(), o["status"].data_ptr(), 0, b.plane.data_ptr(), wh, pd, nf_, pf, False, delta, False,
                                             o["flags"].data_ptr())
    ref = _host(o)
    for k in ("rows", "keep", "cnt", "st", "thr", "flags", "status"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert 0 in ref["flags"] and 1 in ref["flags"]


def test_only_the_last_frame_snows(eng, main_tids):
    frames = wr.main_frames()[5:8]
    b = Batch(frames, main_tids[5:8], wr.main_masks(wr.main_frames())[5:8])
    rec = wr.main_records(((0, 0, 0), (0, 1, 0), (1, 1, 2)))
    want, _ = yardsticks(eng, b, rec)
    got = run_weather(eng, b, rec)
    assert int(got["status"][0]) == 0 and int((got["rows"][int(b.off[2]):, 4] == 2).sum()) > 0
    same(got, want, b)


def test_snow_only_frames_of_1023_1024_1025_present_rows(eng, main_tids):
    """The tile edges of the masked front end under a gate: the first three frames of the edge batch of tests/aligned_mask_inputs.py
    (1 023 / 1 024 / 1 025 present rows of a 5 000-row frame in firing order) as (1, 0) frames, caller polynomials, with a (0, 0) frame
    between them."""
    frames, masks = ami.edge_batch()
    frames, masks = [frames[0], frames[4], frames[1], frames[2]], [masks[0], masks[4], masks[1], masks[2]]
    assert [int(m.sum()) for m in masks] == [1023, 2000, 1024, 1025]
    b = Batch(frames, main_tids[:4], masks, poly=[1e-3, 0.05, 12.0])
    rec = wr.main_records(((1, 0, 0), (0, 0, 0), (1, 0, 1), (1, 0, 2)))
    want, _ = yardsticks(eng, b, rec)
    for in_place in (False, True):
        got = run_weather(eng, b, rec, in_place=in_place)
        assert int(got["status"][0]) == 0
        same(got, want, b)
    assert got["cnt"].tolist()[1] == 2000 and got["flags"].tolist() == [2, 2, 2, 2]


def test_seventeen_frames(eng, set_ids):
    """17 frames (above the 16-frame switches of the prepass and the finish) of 64 x 64 sweeps, the gate pairs in turn, device prepass."""
    from lidar_snow_sim_amd.synthetic import synthetic_sweep
    frames = [synthetic_sweep(64, 64, seed=1400 + f, intensity="lambert").astype(np.float32) for f in range(17)]
    masks = [ami.bernoulli(len(f), 0.9, 5200 + i) for i, f in enumerate(frames)]
    tids = wr.draw(7, 0, 17, set_ids, wr.DEFAULT_PLAN)[0]
    b = Batch(frames, tids, masks)
    pairs = ((1, 1), (0, 0), (1, 0), (0, 1))
    rec = wr.main_records(tuple(pairs[f % 4] + (f % 3,) for f in range(17)))
    want, _ = yardsticks(eng, b, rec)
    got = run_weather(eng, b, rec)
    assert int(got["status"][0]) == 0
    same(got, want, b)
    assert {w[5] for w in want} >= {0, 2}


# ---- 5. the draw on the device -------------------------------------------------------------------------------------------------------------
def test_device_draw_equals_the_restated_specification(eng):
    from lidar_snow_sim_amd import _native
    for nf, nl, ns, step, sh in wr.draw_cases():
        ids = wr.abstract_set_ids(ns, nl)
        plan = dict(wr.DEFAULT_PLAN, shuffle=bool(sh))
        st = _native.weather_plan_struct(plan["p_snow"], plan["p_wet"], plan["water_heights"], plan["pavement_depths"], plan["noise_floor"],
                                         plan["power_factor"], plan["delta"], sh)
        d_ids, d_step = _t(ids), torch.tensor([step], dtype=torch.int64, device=DEV)
        tids = torch.full((nf, nl), -1, dtype=torch.int32, device=DEV)
        rec = torch.full((nf, 8), -1.0, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        eng.ctx.draw_weather_device(nf, nl, ns, d_ids.data_ptr(), st, wr.DRAW_SEED, d_step.data_ptr(), tids.data_ptr(), rec.data_ptr(), 0)
        torch.cuda.synchronize()
        want_t, want_r, _ = wr.draw(wr.DRAW_SEED, step, nf, ids, plan)
        assert np.array_equal(tids.cpu().numpy(), want_t), (nf, nl, ns, step, sh)
        assert rec.cpu().numpy().tobytes() == want_r.tobytes(), (nf, nl, ns, step, sh)


# ---- 6. draw, augment and step += 1 in one HIP graph ---------------------------------------------------------------------------------------
def test_draw_augment_and_step_in_one_hip_graph(eng, set_ids):
    """snowgpu_draw_weather_device, snowgpu_augment_weather_batch_device_aligned and step += 1 captured once on one stream and replayed
    three times: after each replay rows, keep, counts, statistics and flags equal the plain call given the restated draw of that step."""
    from lidar_snow_sim_amd import _native
    frames = wr.main_frames()[:4]
    plan = dict(wr.DEFAULT_PLAN, water_heights=(0.0008, 0.002), pavement_depths=(0.001,))
    st = _native.weather_plan_struct(plan["p_snow"], plan["p_wet"], plan["water_heights"], plan["pavement_depths"], plan["noise_floor"],
                                     plan["power_factor"], plan["delta"], True)
    seed, F = 11, 4
    draws = [wr.draw(seed, k, F, set_ids, plan) for k in range(4)]
    assert not np.array_equal(draws[0][1][:, :2], draws[1][1][:, :2]) and not np.array_equal(draws[0][0], draws[1][0])
    want = []
    for k in range(1, 4):                                                 # (the warm-up below runs step 0)
        want.append(run_weather(eng, Batch(frames, draws[k][0]), draws[k][1]))
        assert int(want[-1]["status"][0]) == 0
    b = Batch(frames, draws[0][0])
    b.tids = torch.zeros(F, 64, dtype=torch.int32, device=DEV)
    o = b.outputs()
    d_ids, step, rec = _t(set_ids), torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(F, 8, dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()

    def call():
        eng.ctx.draw_weather_device(F, 64, len(set_ids), d_ids.data_ptr(), st, seed, step.data_ptr(), b.tids.data_ptr(), rec.data_ptr(), s.cuda_stream)
        eng.ctx.augment_weather_batch_device_aligned(*b.head(o), 0, o["rows"].data_ptr(), o["keep"].data_ptr(), o["cnt"].data_ptr(), o["st"].data_ptr(),
                                                     o["thr"].data_ptr(), o["status"].data_ptr(), s.cuda_stream, b.plane.data_ptr(), rec.data_ptr(),
                                                     False, False, o["flags"].data_ptr())
        step.add_(1)

    with torch.cuda.stream(s):
        call()                                                            # warm-up: the captured call allocates nothing
        s.synchronize()
        assert int(step[0]) == 1 and np.array_equal(rec.cpu().numpy(), draws[0][1]) and np.array_equal(b.tids.cpu().numpy(), draws[0][0])
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        got = []
        for k in range(3):                                                # no host read between the replays
            g.replay()
            got.append({n: o[n].clone() for n in ("rows", "keep", "cnt", "st", "flags", "status")} | dict(rec=rec.clone(), tids=b.tids.clone()))
        s.synchronize()
    assert int(step[0]) == 4
    for k in range(3):
        assert np.array_equal(got[k]["rec"].cpu().numpy(), draws[k + 1][1]) and np.array_equal(got[k]["tids"].cpu().numpy(), draws[k + 1][0]), k
        for n in ("rows", "keep", "cnt", "st", "flags", "status"):
            assert got[k][n].cpu().numpy().tobytes() == want[k][n].tobytes(), (k, n)


# ---- 7. refusals and the Python layer --------------------------------------------------------------------------------------------------------
def test_refusals(eng, set_ids, main_tids):
    from lidar_snow_sim_amd import _native
    b, _, _ = main_batch(eng, main_tids, np.float32, False)
    o = b.outputs()
    with pytest.raises(_native.SnowGPUError, match="d_weather") as ei:
        eng.ctx.augment_weather_batch_device_aligned(*b.head(o), 0, o["rows"].data_ptr(), o["keep"].data_ptr(), o["cnt"].data_ptr(), o["st"].data_ptr(),
                                                     o["thr"].data_ptr(), o["status"].data_ptr(), 0, b.plane.data_ptr(), 0, False, False, o["flags"].data_ptr())
    assert ei.value.code == _native.E_INVALID
    d_ids, step = _t(np.zeros((65, 129), np.int32)), torch.zeros(1, dtype=torch.int64, device=DEV)
    tids, rec = torch.full((4, 129), -1, dtype=torch.int32, device=DEV), torch.full((4, 8), -1.0, dtype=torch.float64, device=DEV)
    ok = dict(p_snow=0.5, p_wet=0.5, water_heights=(0.001,), pavement_depths=(0.001,), noise_floor=0.7, power_factor=15, delta=0.5, shuffle=True)
    cases = [(dict(ok, water_heights=[0.001] * 17), 4, 64, 5), (dict(ok, pavement_depths=[0.001] * 17), 4, 64, 5), (dict(ok, water_heights=()), 4, 64, 5),
             (ok, 4, 129, 5), (ok, 4, 64, 65), (ok, (1 << 22) + 1, 64, 5), (dict(ok, p_snow=1.5), 4, 64, 5)]
    for plan, nf, nl, ns in cases:
        with pytest.raises(_native.SnowGPUError) as ei:
            eng.ctx.draw_weather_device(nf, nl, ns, d_ids.data_ptr(), _native.weather_plan_struct(**plan), 0, step.data_ptr(), tids.data_ptr(), rec.data_ptr(), 0)
        assert ei.value.code == _native.E_INVALID
    torch.cuda.synchronize()
    assert int((tids != -1).sum()) == 0 and float((rec != -1).sum()) == 0          # refused before any launch


def test_python_layer(eng, sets, set_ids, main_tids):
    """augment_wet_batch_aligned(weather=, table_ids=) returns the entry's bytes; weather_records builds the records; WeatherPlan draws what
    the restatement draws and advances with its device step; the ValueErrors."""
    from lidar_snow_sim_amd.tensors import WeatherPlan, augment_wet_batch_aligned, weather_records
    b, want, _ = main_batch(eng, main_tids, np.float32, True)
    spec = wr.MAIN_FRAMES
    cols = list(zip(*[wr.SETTINGS[k] for _, _, k in spec]))
    w = weather_records(8, snow=[g[0] for g in spec], wet=torch.tensor([g[1] for g in spec]), water_height=cols[0], pavement_depth=cols[1],
                        noise_floor=cols[2], power_factor=torch.tensor(cols[3]), delta=np.asarray(cols[4]), device=0)
    assert w.dtype == torch.float64 and w.is_cuda and np.array_equal(w.cpu().numpy(), wr.main_records())
    assert np.array_equal(weather_records(3, device=0).cpu().numpy(), np.array([[1, 1, 0.001, 0.0012, 0.7, 15, 0.5, 0]] * 3))
    t_frames, t_masks = [_t(f) for f in b.frames], [_t(m) for m in b.masks]
    kw = dict(planes=[PLANE] * 8, wet=dict(plane=PLANE, replace=False), keep=t_masks)
    res = augment_wet_batch_aligned(t_frames, None, BD, weather=w, table_ids=b.tids, sync=False, **kw).wait()
    assert res.rows.cpu().numpy().tobytes() == np.concatenate([x[0] for x in want]).tobytes()
    assert np.array_equal(res.keep.cpu().numpy(), np.concatenate([x[1] for x in want]))
    assert res.flags.tolist() == [x[5] for x in want] and res.counts.tolist() == [int(x[2]) for x in want]
    assert np.array_equal(res.stats.cpu().numpy(), np.stack([x[3] for x in want]))
    with pytest.raises(ValueError, match="weather records"):
        augment_wet_batch_aligned(t_frames, None, BD, weather=w, table_ids=b.tids, planes=[PLANE] * 8, wet=dict(water_height=0.001))
    with pytest.raises(ValueError, match="table_ids"):
        augment_wet_batch_aligned(t_frames, None, BD, weather=w, table_ids=b.tids, orders=[list(range(64))] * 8, **kw)
    with pytest.raises(ValueError, match="table_ids"):
        augment_wet_batch_aligned(t_frames, None, BD, weather=w, table_ids=b.tids, particles=sets[0], **kw)
    with pytest.raises(ValueError, match="weather must be"):
        augment_wet_batch_aligned(t_frames, None, BD, weather=w[:7], table_ids=b.tids, **kw)
    with pytest.raises(ValueError, match="one prefix per frame"):
        augment_wet_batch_aligned(t_frames, ["gunn_0.5_1"] * 7, BD, weather=w, particles="device", **kw)
    with pytest.raises(ValueError, match="one value per frame"):
        weather_records(8, snow=[1, 0], device=0)
    plan = WeatherPlan(["a", "b", "c", "d", "e"], particles=sets, seed=wr.MAIN_SEED, device=0, **wr.DEFAULT_PLAN)
    assert np.array_equal(plan.set_ids.cpu().numpy(), set_ids) and plan.step.dtype == torch.int64 and plan.step.is_cuda
    tids, rec = plan.draw(8)
    torch.cuda.synchronize()
    want_t, want_r, _ = wr.draw(wr.MAIN_SEED, 0, 8, set_ids, wr.DEFAULT_PLAN)
    assert np.array_equal(tids.cpu().numpy(), want_t) and np.array_equal(rec.cpu().numpy(), want_r)
    assert np.array_equal(want_t, main_tids)
    plan.step += 1
    out = plan.draw(8, out=(tids, rec))
    torch.cuda.synchronize()
    want_t, want_r, _ = wr.draw(wr.MAIN_SEED, 1, 8, set_ids, wr.DEFAULT_PLAN)
    assert out[0] is tids and np.array_equal(tids.cpu().numpy(), want_t) and np.array_equal(rec.cpu().numpy(), want_r)
