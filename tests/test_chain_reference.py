"""No GPU: the inputs of tests/test_gpu_chain.py held to the conditions that keep its comparisons against tests/chain_reference.py from being
vacuous -- on the UN-augmented batches, which is what can be run here; the GPU test asserts the same conditions on the augmented rows.
These are conditions on inputs, not measurements of the library."""
import numpy as np
import pytest

import chain_reference as cr
import weather_reference as wr


@pytest.mark.parametrize("name", ["ragged", "weather"])
def test_every_full_size_frame_exercises_every_stage(name):
    """The first filter keeps 25 .. 90 % of the rows, at least 1000 of them inside the range; a voxel at max_points and one below; balls
    below and above their sample count; the image's and the keypoints' verdicts each clear rows and leave rows; every box but the
    padding holds a row and one holds five; the second filter differs from the first; and a row that the verdicts cleared is kept by
    the second filter because it lies in a box."""
    b = cr.batch(name)
    e = cr.expected_of(name)
    full = cr.FULL if name == "ragged" else range(len(b["frames"]))
    cond = cr.conditions(e, b["offsets"], b["boxes"], full)
    print(name, cond)
    cr.check(cond)
    for f in full:
        a, z = int(b["offsets"][f]), int(b["offsets"][f + 1])
        va, vz = int(e["vox.voxel_offsets"][f]), int(e["vox.voxel_offsets"][f + 1])
        assert vz - va < cr.VOXEL[3]                                    # (no cell is dropped: voxel_of names every usable row's voxel)
        assert cr.VOXEL[2] < np.bincount(e["vox.voxel_of"][a:z][e["vox.voxel_of"][a:z] >= 0] - va).max() <= cr.CLUSTER      # the cap cuts rows off
        assert not e["K1"][a:z][~b["keep0"][a:z]].any() and (e["back.rows_in"][a:z] <= e["K1"][a:z]).all()


def test_the_ragged_batch_is_what_the_gpu_tests_take_it_for():
    for dtype in cr.DTYPES:
        fr, masks = cr.frames("ragged", dtype)
        assert tuple(len(p) for p in fr) == cr.RAGGED_SIZES == (8192, 6144, 1025, 1, 0, 1023) and all(p.dtype == np.dtype(dtype) for p in fr)
        assert [len(m) for m in masks] == [len(p) for p in fr]
        assert np.any(np.diff(fr[1][:, 4]) < 0) and not np.any(np.diff(fr[0][:, 4]) < 0)              # firing order / channel-major
        assert not masks[5].any() and all(m.all() for m in masks[2:4]) and all(0.9 < m.mean() < 1.0 for m in masks[:2])
        rev, rev_masks = cr.frames("ragged_reversed", dtype)
        assert all(np.array_equal(p, q) for p, q in zip(rev, fr[::-1])) and all(np.array_equal(p, q) for p, q in zip(rev_masks, masks[::-1]))
    assert sum(cr.RAGGED_SIZES) <= 25000 and [len(p) for p in cr.frames("small")[0]] == [1023]
    b, r = cr.batch("ragged"), cr.batch("ragged_reversed")
    assert np.array_equal(b["boxes"][::-1], r["boxes"]) and b["boxes"].shape == (6, cr.B, 8) and not b["boxes"][:, cr.PADDING].any()
    assert b["channel"].dtype == np.int32 and 0 <= b["channel"].min() and b["channel"].max() == 63
    assert np.array_equal(np.unique(b["boxes"][:3, :, 7]), [0, 1, 2, 3])


def test_the_weather_batch_has_ground_for_the_wet_stage():
    fr, masks = cr.frames("weather")
    ground = [wr.ground_rows(p, m, 0.5) for p, m in zip(fr, masks)]
    print("ground rows", ground)
    assert len(fr) == 3 and all(len(p) == 8192 for p in fr) and min(ground) >= 1000
    # the filter's setting: 5493 and 5509 of the 8192 rows of the sweeps of seeds 1600 and 1601 (the default setting keeps none of them)
    b = cr.batch("weather")
    K1 = cr.expected_of("weather")["K1"]
    assert [int(K1[a:z].sum()) for a, z in zip(b["offsets"][:2], b["offsets"][1:3])] == [5493, 5509]
    assert [int(cr.fps.usable_rows(p, cr.PCR).sum()) for p in fr[:2]] == [3852, 3865]                     # rows inside the range


def test_the_twins_are_neighbours_of_each_other():
    """Read as ONE frame, the two sweeps change each other's neighbour counts: the reason dror_keep(res.rows, keep=res.keep) is not the
    filter of a batch of several frames."""
    b = cr.batch("twins")
    per_frame = cr.first_filter(b["rows"], b["keep0"], b["offsets"])
    as_one = cr.first_filter(b["rows"], b["keep0"], np.array([0, len(b["rows"])], np.int64))
    assert int((per_frame != as_one).sum()) > 100 and (per_frame <= as_one).all()


@pytest.mark.parametrize("dtype", cr.DTYPES)
def test_frames_without_a_usable_row_get_the_fills(dtype):
    """The one-row frame (no neighbour: the filter drops it), the empty frame and the all-absent frame: every stage's expected output is
    the fill its docstring names -- -1 for indices, 0 for counts, points and weights, +inf for distances, False for masks."""
    b = cr.batch("ragged", dtype)
    e = cr.expected_of("ragged", dtype)
    off = b["offsets"]
    for f in cr.TRIVIAL:
        a, z = int(off[f]), int(off[f + 1])
        assert not e["K1"][a:z].any() and not e["K2"][a:z].any()
        assert e["vox.voxel_offsets"][f] == e["vox.voxel_offsets"][f + 1] and (e["vox.voxel_of"][a:z] == -1).all()
        assert (e["kp.index"][f] == -1).all() and not e["kp.points"][f].any() and e["kp.usable"][f] == 0
        assert (e["nb.index"][f] == -1).all() and not e["nb.count"][f].any() and not e["nb.points"][f].any()
        assert (e["nn.index"][a:z] == -1).all() and np.isposinf(e["nn.dist2"][a:z]).all() and not e["nn.weight"][a:z].any()
        assert (e["img.image"][f] == -1).all() and (e["img.index"][f] == -1).all() and (e["img.pixel_of"][a:z] == -1).all()
        assert (e["lab.box_of"][a:z] == -1).all() and not e["lab.count"][f].any() and not e["lab.local"][a:z].any()
        assert not e["back.to_rows"][a:z].any() and not e["back.nearest"][a:z].any() and not e["back.interpolate"][a:z].any()
        assert not e["back.labels"][a:z].any() and not e["back.keep_boxes"][f].any() and not e["back.rows_in"][a:z].any()
        assert (e["back.kp_labels"][f] == -1).all()
    last = int(e["vox.voxel_offsets"][-1])
    assert not e["vox.voxels"][last:].any() and (e["vox.coords"][last:] == -1).all() and not e["vox.num_points"][last:].any() and last < len(e["vox.num_points"])
    assert e["kp.index"].dtype == e["back.kp_labels"].dtype == np.int32 and e["back.labels"].dtype == np.int64 and e["back.interpolate"].dtype == np.dtype(dtype)


def test_compose_is_cached_by_its_inputs_and_read_only():
    b = cr.batch("small")
    one = cr.expected(b["rows"], b["keep0"], b["offsets"], b["channel"], b["boxes"], b["pose"])
    assert cr.expected(b["rows"].copy(), b["keep0"], b["offsets"], b["channel"], b["boxes"], b["pose"]) is one
    other = cr.expected(b["rows"], ~b["keep0"], b["offsets"], b["channel"], b["boxes"], b["pose"])
    assert other is not one and not other["K1"].any() and one["K1"].any()
    with pytest.raises(ValueError):
        one["K1"][0] = True
