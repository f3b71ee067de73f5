"""CPU: the settings of tests/test_gpu_wet_aligned.py (the aligned wet-ground stage: k_pre_ground<T, true>, k_wet_apply_aligned,
k_wet_count) on any machine, in the manner of tests/test_prepass_reference.py.

The mask rule of the settings, for frame `pc` and parameter set i (mask() below; the GPU file imports it from here):
    m  = np.random.default_rng(900 + i).random(len(pc)) >= 1/3
    m &= ~np.isin(pc[:, 4], (5, 40))
A masked frame's expectation is the oracle on the gathered rows pc[m]; so what has to hold on the CPU is that pc[m] is still a
setting: at least 1000 ground rows stay present, more than 100 ground rows are kept and more than 100 dropped, keep agrees between the
float64 and the long-double chain, every keep / drop decision is clear by a relative 1e-7, and the restatement on pc[m] equals the
oracle bit for bit -- for every WET_PARAMS[i] and both dtypes on `wet`, and for i = 0 on `wet_tiles`.  (m3 and m4 fall below 1000
ground rows under this rule and are not used.)

The device-free entry test: the NumPy-input ValueError of augment_wet_batch_aligned and wet_ground_batch_aligned comes before anything
touches the device (no engine is asked for), the two C entries are exported, bound and refuse a null context, and on a machine without
a HIP device asking for the engine they would run on raises what every entry raises there, E_NO_DEVICE.
"""
import numpy as np
import pytest

import prepass_reference as pr

TAGS = ("f32", "f64")


def mask(pc, i):
    """The mask rule of the aligned wet settings: about a third of the rows and two whole channels are not there."""
    m = np.random.default_rng(900 + i).random(len(pc)) >= 1 / 3
    m &= ~np.isin(pc[:, 4], (5, 40))
    return m


@pytest.fixture(scope="module")
def so():
    from oracle import snow_oracle
    return snow_oracle


def _masked_setting(so, name, i, tag):
    kw = pr.WET_PARAMS[i]
    pc = pr.frame(name, tag)
    m = mask(pc, i)
    assert 0.5 * len(pc) < m.sum() < 0.75 * len(pc) and not np.isin(pc[m, 4], (5, 40)).any()
    sub = np.ascontiguousarray(pc[m])
    r = pr.wet_restated(sub, **kw)
    assert r.flag == 0 and r.g.mask.sum() >= 1000
    ref, src = so.ground_water_augmentation(sub, plane=(pr.PLANE_W, pr.PLANE_H), return_src=True, **kw)
    assert np.array_equal(ref, r.out) and np.array_equal(src, r.src)
    ch, ld = r.chain, r.chain_ld
    kept, dropped = int(ch.keep.sum()), int((~ch.keep).sum())
    assert kept > 100 and dropped > 100
    assert np.array_equal(ch.keep, ld.keep)
    margin = float((np.abs(ld.new_i - ld.lim) / np.abs(ld.lim)).min())
    assert margin > 1e-7
    print(f"\n[wet-aligned-reference] {name} {i} {tag}: {int(r.g.mask.sum())} present ground rows, kept {kept}, dropped {dropped}, "
          f"smallest keep / drop margin {margin:.1e}")
    return r, m


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("i", range(len(pr.WET_PARAMS)))
def test_masked_wet_settings_stay_settings(so, i, tag):
    _masked_setting(so, "wet", i, tag)


@pytest.mark.parametrize("tag", TAGS)
def test_masked_wet_tiles_stays_a_setting(so, tag):
    """65 tiles + 1 row under the mask; and with every row of tile 2 masked as well (a tile without a present row)."""
    r, m = _masked_setting(so, "wet_tiles", 0, tag)
    pc = pr.frame("wet_tiles", tag)
    assert len(pc) == 65 * pr.TILE + 1 and m[-1:].size == 1
    m2 = m.copy()
    m2[2 * pr.TILE:3 * pr.TILE] = False
    r2 = pr.wet_restated(np.ascontiguousarray(pc[m2]), **pr.WET_PARAMS[0])
    assert r2.flag == 0 and 1000 <= r2.g.mask.sum() < r.g.mask.sum()
    assert np.array_equal(r2.chain.keep, r2.chain_ld.keep)
    assert float((np.abs(r2.chain_ld.new_i - r2.chain_ld.lim) / np.abs(r2.chain_ld.lim)).min()) > 1e-7


@pytest.mark.parametrize("tag", TAGS)
def test_the_1000_row_rule_under_a_mask(tag):
    """g1000 with exactly one ground row masked has 999 present ground rows: the rule decides on the PRESENT rows."""
    pc = pr.frame("g1000", tag)
    g = pr.ground_rows(pc)
    m = np.ones(len(pc), bool)
    m[np.flatnonzero(g.mask)[500]] = False
    kw = pr.WET_PARAMS[2] | dict(delta=0.5)
    assert pr.wet_restated(pc, **kw).flag == 0 and pr.wet_restated(np.ascontiguousarray(pc[m]), **kw).flag == 1


def test_the_entries_exist_and_refuse_numpy_before_they_touch_a_device(monkeypatch):
    from lidar_snow_sim_amd import _native, engine, tensors
    from lidar_snow_sim_amd.tools.snowfall import simulation

    def no_engine(*a, **k):
        raise AssertionError("the engine was asked for before the input was refused")
    monkeypatch.setattr(engine, "get_engine", no_engine)
    pc = pr.frame("g999", "f32")
    with pytest.raises(ValueError, match="aligned"):
        tensors.wet_ground_batch_aligned([pc])
    with pytest.raises(ValueError, match="aligned"):
        tensors.wet_ground_batch_aligned([pc], np.ones(len(pc), bool), in_place=True)
    for fn in (tensors.augment_wet_batch_aligned, simulation.augment_wet_batch_aligned):
        with pytest.raises(ValueError, match="aligned"):
            fn([pc], "gunn_5.0_0.0", 0.17, wet=dict(plane=(pr.PLANE_W, pr.PLANE_H)))
    monkeypatch.undo()
    lib = _native.lib()
    for name in ("snowgpu_wet_ground_batch_device_aligned", "snowgpu_augment_wet_batch_device_aligned"):
        assert name in _native.EXPORTS and hasattr(lib, name)
    assert callable(_native.Context.wet_ground_batch_device_aligned) and callable(_native.Context.augment_wet_batch_device_aligned)
    assert lib.snowgpu_wet_ground_batch_device_aligned(None, 1, 0, 0, None, None, 0, None, None, 0.0, 1.0, 0.7, 15.0, 0, 0.5, 1, None, None,
                                                       None, None, None, None) == _native.E_INVALID
    assert lib.snowgpu_augment_wet_batch_device_aligned(None, 1, 0, 0, None, None, 0, None, 0.17, None, None, 0.7, None, None, None, None, None,
                                                        None, None, None, None, 0.0, 1.0, 0.7, 15.0, 0, 0.5, 1, None) == _native.E_INVALID
    import torch
    if not torch.cuda.is_available():                                   # no device: the engine the entries run on raises what every entry raises
        with pytest.raises(_native.SnowGPUError) as e:
            engine.get_engine(0)
        assert e.value.code == _native.E_NO_DEVICE
