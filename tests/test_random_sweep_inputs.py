"""CPU: the configurations of tests/test_gpu_random_sweep.py (tests/random_sweep_inputs.py) on any machine -- the conditions without which
a random sweep would be a weaker copy of the hand-built cases: per stage and dtype, every border size, keep kind and form occurs, frames
start off the 64-row and 1024-row grids, a frame without a usable row lies between frames that have some; the edges at which the kernels
decide by rule are REACHED, counted from the restatements' own outputs; and every drawn dimension changes the expected bytes of some
config.  These are requirements on the generator: if one fails, the draws change, not the condition.  Nothing here needs a GPU or the
package's native code."""
import numpy as np
import pytest

import box_reference as br
import random_sweep_inputs as rs

CASES = [(stage, dtype) for stage in rs.STAGES for dtype in rs.DTYPES]


def _frames(c):
    return list(zip(c["offsets"][:-1].tolist(), c["offsets"][1:].tolist()))


def _arrays(v):
    """Every array of a config, by path."""
    if isinstance(v, np.ndarray):
        yield "", v
    elif isinstance(v, dict):
        for k, x in v.items():
            for path, a in _arrays(x):
                yield f"{k}.{path}", a


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage, dtype", CASES)
def test_configs_are_deterministic_and_read_only(stage, dtype):
    first, again = rs.configs(stage, dtype), rs.configs.__wrapped__(stage, dtype)
    assert len(first) == len(again) == rs.N_CONFIGS
    for a, b in zip(first, again):
        assert a is not b and a["sizes"] == b["sizes"] and a["form"] == b["form"] and a["flags"] == b["flags"]
        pa, pb = dict(_arrays(a)), dict(_arrays(b))
        assert pa.keys() == pb.keys() and "rows." in pa and "offsets." in pa
        for path in pa:
            assert pa[path].dtype == pb[path].dtype and pa[path].tobytes() == pb[path].tobytes(), path
            assert not pa[path].flags.writeable, path
        assert a["rows"].dtype == np.dtype(dtype) and a["rows"].shape == (int(a["offsets"][-1]), 5) and 0 < len(a["rows"]) <= rs.MAX_ROWS
        assert a["keep"] is None or (a["keep"].dtype == np.bool_ and a["keep"].shape == (len(a["rows"]),))
        assert 1 <= len(a["sizes"]) <= 7 and all(s <= n for s, n in zip(a["sizes"], np.diff(a["offsets"])))
    for a in rs.expected(stage, first[0]).values():
        assert not a.flags.writeable
    assert rs.expected(stage, first[0]) is rs.expected(stage, first[0])


@pytest.mark.parametrize("stage, dtype", CASES)
def test_coverage_of_the_shared_draws(stage, dtype):
    cs = rs.configs(stage, dtype)
    unpadded = [c for c in cs if c["form"] != "padded"]
    lengths = {int(n) for c in unpadded for n in np.diff(c["offsets"])}
    assert set(rs.BORDERS) <= lengths, sorted(set(rs.BORDERS) - lengths)
    assert any(n not in rs.BORDERS for n in lengths) and max(lengths) == 2049
    assert {c["keep_kind"] for c in cs} == set(rs.KEEP_KINDS) and {c["form"] for c in cs} == set(rs.FORMS)
    assert {c["keep_form"] for c in cs if c["keep"] is not None} == set(rs.KEEP_FORMS) and {c["out"] for c in cs} == {False, True}
    assert {(c["form"], c["out"]) for c in cs} == {(f, o) for f in rs.FORMS for o in (False, True)}
    assert {c["step"] for c in cs} == set(rs.STEPS) and {len(c["sizes"]) for c in cs} >= {1, 2, 3, 4}
    for name in cs[0]["flags"]:
        assert {c["flags"][name] for c in cs} == {False, True}, name
    # frames that start off the wave and inside a tile; the empty frames
    starts = [a for c in cs for a, b in _frames(c) if b > a]
    assert any(a % 64 for a in starts) and any(a % 1024 for a in starts)
    sizes = [list(np.diff(c["offsets"])) for c in unpadded]
    assert any(s[0] == 0 and len(s) > 1 for s in sizes) and any(s[-1] == 0 and len(s) > 1 for s in sizes)
    assert any(s[f] == 0 and s[f + 1] == 0 and f > 0 and f + 2 < len(s) for s in sizes for f in range(len(s) - 1))
    # ... and the issue's own example: a frame without a usable row between frames that have some
    between = 0
    for c in cs:
        ok = br.usable_rows(c["rows"], c["keep"])
        has = [bool(ok[a:b].any()) for a, b in _frames(c)]
        between += sum(1 for f in range(1, len(has) - 1) if not has[f] and has[f - 1] and has[f + 1])
    assert between >= 2
    # coincident rows, unusable rows of every kind, rows the mask takes
    rows = np.concatenate([c["rows"][:, :3].astype(np.float64) for c in cs])
    assert np.isnan(rows).any() and (rows == np.inf).any() and (rows == -np.inf).any() and (np.abs(rows[np.isfinite(rows)]) > 1e6).any()
    assert any(len(np.unique(c["rows"][a:b, :3], axis=0)) < b - a for c in cs for a, b in _frames(c) if b - a > 100)
    assert any(c["keep"] is not None and c["keep"].any() and not c["keep"].all() for c in cs)


# ---- the edges, counted from the restatements' own outputs -----------------------------------------------------------------------------------
def _edges_dror(c, e):
    k = c["args"]["k_min"]
    ok = br.usable_rows(c["rows"], c["keep"])
    return dict(below_k_min=k > 0 and bool((e["full_counts"][ok] < k).any()), at_or_above_k_min=k > 0 and bool((e["full_counts"][ok] >= k).any()),
                saturated=k > 0 and bool((e["full_counts"] > k).any()), keeps_and_drops=bool(e["keep"].any() and not e["keep"][ok].all()))


def _edges_voxelize(c, e):
    a = c["args"]
    T, V = a["max_points"], a["max_voxels"]
    per = np.diff(e["voxel_offsets"])
    dropped = [bool((e["usable"][x:y] & (e["voxel_of"][x:y] < 0)).any()) for x, y in _frames(c)]
    lo, hi = np.array(a["range"][:3]), np.array(a["range"][3:])
    p = c["rows"][:, :3].astype(np.float64)
    return dict(voxel_at_max_points=bool((e["rows_per_voxel"] > T).any()), voxel_below_max_points=bool(((e["rows_per_voxel"] < T) & (e["rows_per_voxel"] > 0)).any()),
                frame_at_max_voxels_with_rows_dropped=any(n == V and d for n, d in zip(per, dropped)), frame_below_max_voxels=bool(((per < V) & (per > 0)).any()),
                row_on_the_low_face=bool((e["usable"] & (p == lo).any(axis=1)).any()), row_on_the_high_face=bool(((p == hi).any(axis=1) & ~np.isnan(p).any(axis=1)).any()))


def _edges_fps(c, e):
    K = c["args"]["n_samples"]
    return dict(round_decided_by_the_tie_rule=bool((e["ties"] >= 2).any()), more_samples_than_usable_rows=bool(((e["usable"] > 0) & (e["usable"] < K)).any()),
                fewer_samples_than_usable_rows=bool((e["usable"] > K).any()), frame_without_a_usable_row=bool((e["usable"] == 0).any()))


def _edges_sectors(c, e):
    K = c["args"]["n_samples"]
    return dict(more_samples_than_usable_rows=bool(((e["usable"] > 0) & (e["usable"] < K)).any()), fewer_samples_than_usable_rows=bool((e["usable"] > K).any()),
                empty_sector_beside_a_full_one=bool(((e["sector_count"] == 0).any(axis=1) & (e["usable"] > 0)).any()), with_rois=c["args"]["rois"] is not None,
                without_rois=c["args"]["rois"] is None, rois_take_rows=c["args"]["rois"] is not None and bool((e["usable"] > 0).any()) and
                int(e["usable"].sum()) < int(rs.fr.usable_rows(c["rows"], c["args"]["range"], c["keep"]).sum()))


def _edges_ball(c, e):
    samples = np.asarray(c["args"]["samples"])
    usable = rs.qr.centre_usable(c["args"]["centres"])
    return dict(more_rows_than_n_neighbours=bool((e["count"] > samples).any()), fewer_rows_than_n_neighbours=bool(((e["count"] < samples) & (e["count"] > 0)).any()),
                empty_ball_of_a_usable_centre=bool(((e["count"] == 0) & usable[..., None]).any()), unusable_centre=bool((~usable).any()))


def _edges_nearest(c, e):
    k = c["args"]["k"]
    d, i = e["dist2"], e["index"]
    tie = k > 1 and bool(((d[:, 0] == d[:, 1]) & np.isfinite(d[:, 1]) & (i[:, 0] != i[:, 1])).any())
    return dict(equal_distances_to_two_centres=tie, row_on_a_centre=bool((d[:, 0] == 0).any()), fewer_centres_than_k=bool(((i[:, 0] >= 0) & (i[:, -1] < 0)).any()))


def _edges_range(c, e):
    return dict(contested_pixel=bool((e["count"] > 1).any()), empty_pixel=bool((e["count"] == 0).any()), by_ring=c["args"]["ring"] is not None,
                by_elevation=c["args"]["ring"] is None, no_usable_row=not (e["pixel_of"] >= 0).any())


def _edges_boxes(c, e):
    inside = e["box_of"] >= 0
    frame = np.searchsorted(c["offsets"], np.arange(len(c["rows"])), side="right") - 1
    half = c["args"]["boxes"][frame[inside], e["box_of"][inside], 5].astype(np.float64) * 0.5
    return dict(row_in_two_boxes=int(e["count"].sum()) > int(inside.sum()), row_on_a_face=bool((np.abs(e["local"][inside, 2].astype(np.float64)) == half).any()),
                row_in_no_box=bool((~inside & br.usable_rows(c["rows"], c["keep"])).any()), absent_box=bool((e["pose"] == 0).all(axis=-1).any()))


def _edges_roipool(c, e):
    S = c["args"]["n_samples"]
    return dict(pool_below_n_samples=bool(((e["count"] > 0) & (e["count"] < S)).any()), pool_above_n_samples=bool((e["count"] > S).any()),
                empty_roi=bool(((e["count"] == 0) & (e["pose"] != 0).any(axis=-1)).any()), absent_roi=bool((e["pose"] == 0).all(axis=-1).any()),
                rois_that_overlap=int(e["count"].sum()) > len(np.unique(e["index"][e["index"] >= 0])) and S >= int(e["count"].max()))


def _edges_roiaware(c, e):
    a = c["args"]
    return dict(members_above_the_capacity=bool((e["roi_count"] > a["roi_capacity"]).any()), members_below_the_capacity=bool(((e["roi_count"] > 0) & (e["roi_count"] < a["roi_capacity"])).any()),
                voxel_above_max_points=bool((e["count"] > a["max_points"]).any()), with_features=a["features"] is not None, without_features=a["features"] is None)


EDGES = dict(zip(rs.STAGES, (_edges_dror, _edges_voxelize, _edges_fps, _edges_sectors, _edges_ball, _edges_nearest, _edges_range, _edges_boxes, _edges_roipool,
                             _edges_roiaware)))


@pytest.mark.parametrize("stage, dtype", CASES)
def test_edges_are_reached(stage, dtype):
    reached = {}
    for c in rs.configs(stage, dtype):
        for name, hit in EDGES[stage](c, rs.expected(stage, c)).items():
            reached[name] = reached.get(name, 0) + bool(hit)
    print(f"\n[random-sweep] {stage} {dtype}: configs that reach " + ", ".join(f"{k} {v}" for k, v in reached.items()))
    assert all(reached.values()), [k for k, v in reached.items() if not v]


# ---- every drawn dimension decides something ---------------------------------------------------------------------------------------------------
def _differs(stage, c, **replaced):
    want, other = rs.expected(stage, c), rs.restate(stage, c, **replaced)
    return any(other[f].shape != want[f].shape or other[f].tobytes() != want[f].tobytes() for f in rs.fields(stage, dict(c, flags={k: True for k in c["flags"]})))


@pytest.mark.parametrize("stage, dtype", CASES)
def test_every_drawn_dimension_decides_something(stage, dtype):
    cs = rs.configs(stage, dtype)
    assert any(_differs(stage, c, keep=None) for c in cs if c["keep"] is not None)
    assert any(_differs(stage, c, offsets="one frame") for c in cs if len(c["sizes"]) > 1)
    if stage in rs.FEATURE_STAGES:
        assert {c["args"]["num_features"] for c in cs} == {3, 4, 5}
        assert any(_differs(stage, c, num_features=4) for c in cs if c["args"]["num_features"] != 4)
    if stage == "range_image":
        assert any(_differs(stage, c, range=rs.INF_RANGE) for c in cs if c["args"]["limits"] != rs.rr.NO_LIMITS)
    elif stage in rs.RANGE_STAGES:
        assert any(_differs(stage, c, range=rs.INF_RANGE) for c in cs if c["args"]["range"] is not None)
        if stage != "voxelize":
            assert any(c["args"]["range"] is None for c in cs)
