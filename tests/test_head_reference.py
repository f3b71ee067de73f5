"""No GPU: the inputs of tests/test_gpu_head_chain.py held to the conditions that keep its comparisons against tests/head_reference.py from
being vacuous, on the restatement alone and under NumPy's poses (the GPU test asserts them again on what the device gave), and the
properties of the composition that the GPU tests lean on: which fields follow their frame when the frames change places, and what a move
of `step` reaches.  These are conditions on inputs, not measurements of the library.

Seen here, float32 and float64 alike (-s prints all of it).  ragged: NMS keeps 48, 29, 33, 0, 7, 31 of the 96 proposals of the six frames;
sample_rois takes the branches a, a, a, d, b, c from (fg, hard, easy) = (3, 2, 43), (3, 4, 22), (4, 3, 26), (0, 0, 0), (7, 0, 0), (0, 0, 31)
candidates; 42 sampled rois are regression targets, 118 are not; 75 sampled rois hold no row, 72 fewer than 32 and 13 more; 94 sub-voxels are at
max_points or beyond; sectors of (528, 1184, 1027, 1032) and (854, 1156, 882, 0) usable rows in the two full frames -- the 96-step frame has
no row in its last quadrant --, 3771 of 7954 and 2892 of 5942 present rows within reach of a roi; keep_boxes(5) keeps 5 and drops 2 of the 7
present gts of either full frame; 5, 5 and 1 positives; 3 ignored anchors."""
import numpy as np
import pytest

import chain_reference as cr
import head_reference as hr
import targets_reference as tr

BATCHES = ("ragged", "ragged_reversed", "small", "scenes0", "scenes1", "scenes2")


@pytest.mark.parametrize("dtype", hr.DTYPES)
@pytest.mark.parametrize("name", BATCHES)
def test_every_batch_exercises_every_stage(name, dtype):
    """check(conditions(...)) on the composition: for the ragged batch, in either order of its frames, every condition of the chain -- a
    frame with post_max kept boxes, one with 4 < count < post_max, one with every score below the threshold; the branches a, b and c of
    the sampler, a frame with fewer rois than slots, a frame without a gt, regression targets set and clear; sampled rois without a row,
    below and above n_samples; a sub-voxel at max_points, an empty and a non-empty roi; a share for every sector that holds a row, rows
    beyond every roi's reach, no keypoint in the one-row, empty and all-absent frames; a ball over its sample count and an empty one;
    gts kept and dropped by keep_boxes(5) and positives in each full frame, all three kinds of label.  For the other batches: that no
    stage sees padding only."""
    b = hr.batch(name, dtype)
    c = hr.conditions(hr.expected(name, dtype), b)
    print(name, dtype, c)
    hr.check(c)
    assert b["rows"].dtype == np.dtype(dtype) and b["proposals"].dtype == np.dtype(dtype) and b["gt_boxes"].dtype == np.dtype(dtype)


def test_the_batches_are_what_the_gpu_tests_take_them_for():
    for dtype in hr.DTYPES:
        b, r, s = hr.batch("ragged", dtype), hr.batch("ragged_reversed", dtype), hr.batch("small", dtype)
        ref = cr.batch("ragged", dtype)
        assert b["rows"].tobytes() == ref["rows"].tobytes() and np.array_equal(b["keep"], ref["keep0"]) and b["sizes"] == cr.RAGGED_SIZES
        assert b["proposals"].shape == (6, 96, 8) and b["gt_boxes"].shape == (6, 12, 8) and b["point_features"].shape == (len(b["rows"]), 3)
        assert b["point_features"].dtype == np.float32
        zero_rows = (~b["gt_boxes"].any(axis=2)).sum(axis=1)
        assert zero_rows.tolist() == [5, 5, 5, 5, 5, 12]
        A = b["anchors"].shape[0]
        assert 1600 <= A <= 3300 and A % 256 and s["anchors"].shape[0] < A
        assert r["sizes"] == b["sizes"][::-1] and r["proposals"].tobytes() == b["proposals"][::-1].tobytes() and r["gt_boxes"].tobytes() == b["gt_boxes"][::-1].tobytes()
        assert s["sizes"] == (300, 40) and s["proposals"].shape == (2, 16, 8) and s["gt_boxes"].shape == (2, 3, 8)
        scenes = [hr.batch(f"scenes{v}", dtype) for v in range(hr.SCENES)]
        for x in scenes[1:]:
            for name in ("rows", "keep", "proposals", "scores", "gt_boxes"):
                assert x[name].shape == scenes[0][name].shape and x[name].dtype == scenes[0][name].dtype and x[name].tobytes() != scenes[0][name].tobytes(), name
            assert np.array_equal(x["offsets"], scenes[0]["offsets"]) and x["anchors"].tobytes() == scenes[0]["anchors"].tobytes()
            assert x["point_features"].tobytes() == scenes[0]["point_features"].tobytes()          # (a replay rewrites the five inputs above, nothing else)
        with pytest.raises(ValueError):
            b["rows"][0, 0] = 0
    assert hr.batch("ragged") is hr.batch("ragged") and hr.expected("ragged") is hr.expected("ragged")


def test_small_is_smaller_in_everything_that_sizes_scratch():
    """Every quantity by which a stage of the chain sizes the context's grow-only scratch is strictly smaller in `small` than in `ragged`: a
    run of small behind ragged writes the front of buffers that still hold ragged's records, run tables and offsets."""
    big, small = hr.scratch_sizes(hr.batch("ragged")), hr.scratch_sizes(hr.batch("small"))
    print(big, small)
    assert set(big) == set(small) and len(big) == 8
    for name in big:
        assert 0 < small[name] < big[name], name
    assert hr.NS == 32 and hr.shape_of("small")["K"] < hr.shape_of("ragged")["K"]


def _per_frame(e, b, name):
    """A field of a composition as a list per frame, indices into the batch made frame-local."""
    v, off = e[name], b["offsets"]
    F = len(off) - 1
    if v.shape[:1] == (len(b["rows"]),) and name.startswith("lab."):
        return [v[off[f]:off[f + 1]] for f in range(F)]
    assert v.shape[0] == F, name
    if name in ("kp.index", "groups.index", "rp.index", "rv.index", "rv.argmax"):
        return [np.where(v[f] >= 0, v[f] - off[f], -1) for f in range(F)]
    return [v[f] for f in range(F)]


@pytest.mark.parametrize("dtype", hr.DTYPES)
def test_reversed_frames_permute_what_is_defined_per_frame(dtype):
    """compose() of the reversed batch is compose() of the ragged batch with the frames in reverse, for every field up to the sampler and
    for the box labels and the anchor targets (indices into the batch taken frame-local).  The sampler's picks are NOT: the draw of frame f
    is keyed by (seed, step, f), and a frame's number changes when the frames change places -- so rt.index differs, and with it the two
    poolings.  Given the forward numbers as `frames=`, the restatement's picks follow their frame too."""
    b, r = hr.batch("ragged", dtype), hr.batch("ragged_reversed", dtype)
    e, x = hr.expected("ragged", dtype), hr.expected("ragged_reversed", dtype)
    assert set(e) == set(x)
    followed = [name for name in e if name.split(".")[0] in hr.BEFORE_SAMPLING or name in ("_branch", "rt.segments", "rt.class_count", "back.keep_boxes", "back.live")
                or name.startswith("back.at_")]
    assert len(followed) >= 30
    for name in followed:
        fwd, rev = _per_frame(e, b, name), _per_frame(x, r, name)
        for f in range(6):
            assert fwd[f].tobytes() == rev[5 - f].tobytes(), (name, f)
    assert not np.array_equal(e["rt.index"][::-1], x["rt.index"])
    for f in range(6):                                                       # every frame that has a candidate and a choice draws differently
        drew = (e["rt.class_count"][f] > 1).any()
        assert np.array_equal(e["rt.index"][f], x["rt.index"][5 - f]) != drew, f
    keyed = tr.sample_rois(x["nb.boxes"], r["gt_boxes"], x["io.best_iou"], x["io.best"],
                           np.where((x["nb.index"] >= 0)[..., None], np.take_along_axis(r["pose_proposals"], np.maximum(x["nb.index"], 0).astype(np.int64)[..., None], axis=1), 0.0),
                           tr.settings(roi_per_image=b["shape"]["S"]), hr.SEED, 0, frames=[5, 4, 3, 2, 1, 0])
    for name in tr.FIELDS:
        assert keyed[name][::-1].tobytes() == e["rt." + name].tobytes(), name


def test_step_moves_the_picks_and_nothing_in_front_of_them():
    e0, e1 = hr.expected("ragged", "float32", 0), hr.expected("ragged", "float32", 1)
    assert e0 is not e1 and not np.array_equal(e0["rt.index"], e1["rt.index"])
    for name in e0:
        if name.split(".")[0] in hr.BEFORE_SAMPLING or name in ("back.keep_boxes", "back.live", "rt.segments", "rt.class_count", "back.rt_valid") or name.startswith("back.at_"):
            assert e0[name].tobytes() == e1[name].tobytes(), name
    moved = [name for name in e0 if e0[name].tobytes() != e1[name].tobytes()]
    print("moved by step:", moved)
    assert {"rt.rois", "rp.index", "rv.count", "back.rt_scores", "back.rp_labels"} <= set(moved)
    s0, s1 = hr.expected("scenes0", "float32", 1), hr.expected("scenes0", "float32", 4)           # the graph test's first and last replay
    assert not np.array_equal(s0["rt.index"], s1["rt.index"]) and s0["at.label"].tobytes() == s1["at.label"].tobytes()


@pytest.mark.parametrize("dtype", hr.DTYPES)
def test_frames_behind_an_empty_keep_list_see_only_padding(dtype):
    """The frame whose scores all lie below the threshold: no kept box, zero rows as rois, and the fills every class documents in every
    stage behind -- -1 for indices and the classification label, 0 for counts, rows, poses and weights."""
    b, e = hr.batch("ragged", dtype), hr.expected("ragged", dtype)
    f = b["kinds"].index("below")
    assert e["nb.count"][f] == 0 and (e["nb.index"][f] == -1).all() and not e["nb.boxes"][f].any() and not e["nb.scores"][f].any()
    assert (e["kp.index"][f] == -1).all() and not e["kp.points"][f].any() and not e["kp.sector_count"][f].any()
    assert (e["groups.index"][f] == -1).all() and not e["groups.count"][f].any()
    assert (e["io.best"][f] == -1).all() and not e["io.best_iou"][f].any()
    assert (e["rt.index"][f] == -1).all() and not e["rt.rois"][f].any() and (e["rt.cls_label"][f] == -1).all() and not e["rt.pose"][f].any() and e["_branch"][f] == "d"
    assert (e["rp.index"][f] == -1).all() and not e["rp.count"][f].any() and e["back.rp_empty"][f].all() and (e["back.rp_labels"][f] == -1).all()
    assert not e["rv.roi_count"][f].any() and (e["rv.index"][f] == -1).all() and (e["rv.argmax"][f] == -1).all() and not e["rv.pose"][f].any()
    assert not e["back.rt_valid"][f].any() and not e["back.rt_scores"][f].any() and not e["back.rv_max_grid"][f].any()
    g = b["kinds"].index("no_gt")
    assert not e["back.live"][g].any() and (e["at.label"][g] <= 0).all() and (e["at.gt_index"][g] == -1).all() and not e["back.at_matched"][g].any()
    assert e["back.at_reg_weights"].dtype == np.float32 and e["back.at_matched"].dtype == np.dtype(dtype) and e["back.rv_max_grid"].shape[2:5] == (4, 4, 4)
