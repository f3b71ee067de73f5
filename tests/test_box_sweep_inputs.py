"""CPU: the configurations of tests/test_gpu_box_sweep.py (tests/box_sweep_inputs.py) on any machine -- the conditions without which a
random sweep of the box stages would be a weaker copy of their hand-built cases: per stage and dtype every positional draw occurs (the
size borders, the all-absent frames, one frame alone, the box widths, the pose sources, out= on every second config); the edges at which
the kernels decide by rule are REACHED, counted from the restatements' own outputs; and every drawn dimension changes the expected bytes
of some config.  These are requirements on the generator: if one fails, the draws change, not the condition.  Nothing here needs a GPU or
the package's native code."""
import math

import numpy as np
import pytest

import anchors_reference as ar
import box_reference as br
import box_sweep_inputs as bs
import iou_reference as ir
import paste_reference as pr
import random_sweep_inputs as rs
import scene_reference as sr
import targets_reference as tr

CASES = [(stage, dtype) for stage in bs.STAGES for dtype in bs.DTYPES]
ROW_STAGES = ("paste_objects", "transform_scene")


def _arrays(v):
    """Every array of a config, by path."""
    if isinstance(v, np.ndarray):
        yield "", v
    elif isinstance(v, dict):
        for k, x in v.items():
            for path, a in _arrays(x):
                yield f"{k}.{path}", a


def _main(stage, c):
    """(the stage's main box set (F, B, C), its pose): the one whose frames `gone` empties."""
    a = c["args"]
    name = dict(boxes_iou="b", nms="boxes", sample_rois="rois")[stage] if stage in ("boxes_iou", "nms", "sample_rois") else "gt_boxes"
    return a[name], br.numpy_pose(a[name])


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage, dtype", CASES)
def test_configs_are_deterministic_and_read_only(stage, dtype):
    first, again = bs.configs(stage, dtype), bs.configs.__wrapped__(stage, dtype)
    assert len(first) == len(again) == bs.N_CONFIGS
    for a, b in zip(first, again):
        assert a is not b and a["flags"] == b["flags"] and a["out"] == b["out"] and a["pose_source"] == b["pose_source"] and a["gone"] == b["gone"]
        pa, pb = dict(_arrays(a)), dict(_arrays(b))
        assert pa.keys() == pb.keys() and len(pa) >= 3
        for path in pa:
            assert pa[path].dtype == pb[path].dtype and pa[path].tobytes() == pb[path].tobytes(), path
            assert not pa[path].flags.writeable, path
        boxes, _ = _main(stage, a)
        assert boxes.dtype == np.dtype(dtype) and boxes.shape[0] == a["frames"] and 1 <= a["frames"] <= bs.F_TOP
        if stage in ROW_STAGES:
            assert a["rows"].dtype == np.dtype(dtype) and a["rows"].shape == (int(a["offsets"][-1]), 5) and len(a["offsets"]) == a["frames"] + 1
            assert a["keep"] is None or (a["keep"].dtype == np.bool_ and a["keep"].shape == (len(a["rows"]),))
    for a in bs.expected(stage, first[0]).values():
        assert not a.flags.writeable
    assert bs.expected(stage, first[0]) is bs.expected(stage, first[0])


def _sizes(stage, c):
    a = c["args"]
    return dict(boxes_iou=lambda: (a["a"].shape[1], a["b"].shape[1]), nms=lambda: (a["boxes"].shape[1],), sample_rois=lambda: (a["rois"].shape[1],),
                assign_anchors=lambda: (a["anchors"].shape[0],), paste_objects=lambda: (sum(a["groups"]),), transform_scene=lambda: (a["gt_boxes"].shape[1],))[stage]()


def _widths(stage, c):
    a = c["args"]
    return dict(boxes_iou=lambda: (a["a"].shape[2], a["b"].shape[2]), nms=lambda: (a["boxes"].shape[2],), sample_rois=lambda: (a["rois"].shape[2], a["gt_boxes"].shape[2]),
                assign_anchors=lambda: (a["anchors"].shape[1], a["gt_boxes"].shape[2]), paste_objects=lambda: (a["gt_boxes"].shape[2],),
                transform_scene=lambda: (a["gt_boxes"].shape[2],))[stage]()


LEGAL_WIDTHS = dict(boxes_iou=((7, 8, 9, 10),) * 2, nms=((7, 8, 9, 10),), sample_rois=((7, 8, 9, 10),) * 2, assign_anchors=((7, 8, 9, 10), (8, 9, 10)),
                    paste_objects=((8, 9, 10),), transform_scene=((7, 8, 9, 10),))


@pytest.mark.parametrize("stage, dtype", CASES)
def test_coverage_of_the_positional_draws(stage, dtype):
    cs = bs.configs(stage, dtype)
    # the size borders in turn, and sizes off them where the stage draws some
    sizes = [_sizes(stage, c) for c in cs]
    for k in range(len(sizes[0])):
        seen = {s[k] for s in sizes}
        assert set(bs.SIZES[stage]) <= seen, (k, sorted(set(bs.SIZES[stage]) - seen))
        if stage in ("boxes_iou", "assign_anchors"):
            assert any(3 <= v <= 700 and v not in bs.SIZES[stage] for v in seen)
    # the frames without a present box: first, last, two in a row, one between two full frames; one frame alone
    empties = []
    for c in cs:
        boxes, pose = _main(stage, c)
        has = br.present(boxes, pose).any(axis=1)
        assert [f for f in range(c["frames"]) if not has[f]] == sorted(c["gone"]), c["i"]
        assert not has[list(c["gone"])].any()
        empties.append(has.tolist())
    assert any(len(h) > 1 and not h[0] and h[1] for h in empties) and any(len(h) > 1 and not h[-1] and h[-2] for h in empties)
    assert any(not h[f] and not h[f + 1] and h[f - 1] and h[f + 2] for h in empties for f in range(1, len(h) - 2))
    assert any(not h[f] and h[f - 1] and h[f + 1] for h in empties for f in range(1, len(h) - 1))
    assert cs[5]["frames"] == 1 and {c["frames"] for c in cs} >= {1, 2, 3, 4}
    # the widths walk 7 .. 10 (where the stage takes them), two box sets independently
    widths = [_widths(stage, c) for c in cs]
    for k, legal in enumerate(LEGAL_WIDTHS[stage]):
        assert {w[k] for w in widths} == set(legal), (k, widths)
    if len(LEGAL_WIDTHS[stage]) == 2:
        assert len(set(widths)) == len(LEGAL_WIDTHS[stage][0]) * len(LEGAL_WIDTHS[stage][1])
        assert (10, 7) in widths or (7, 10) in widths
    # the pose source in turn, out= on every second config, every optional output on and off, every lattice step
    assert [c["pose_source"] for c in cs] == [None if stage == "assign_anchors" else bs.POSE_SOURCES[i % 3] for i in range(len(cs))]
    assert [c["out"] for c in cs] == [bool(i % 2) for i in range(len(cs))]
    for name in cs[0]["flags"]:
        assert {c["flags"][name] for c in cs} == {False, True}, name
        assert {(c["out"], c["flags"][name]) for c in cs} == {(o, v) for o in (False, True) for v in (False, True)}, name
    assert {c["step"] for c in cs} == set(bs.STEPS)
    assert {(c["pose_source"], c["out"]) for c in cs} == {(None if stage == "assign_anchors" else p, o) for p in bs.POSE_SOURCES for o in (False, True)}
    # headings from the three sources: exact right angles, neighbours 1 ulp apart, and others
    h = np.concatenate([_main(stage, c)[0][..., 6].reshape(-1) for c in cs])
    h = h[np.isfinite(h) & (h != 0)]
    right = np.isin(h, (np.arange(-2, 3) * (np.pi / 2)).astype(h.dtype))
    s = np.unique(h)
    assert right.any() and (np.nextafter(s[:-1], s.dtype.type(10)) == s[1:]).any() and (~right).sum() > 10
    STAGE_COVERAGE[stage](cs)


def _cover_boxes_iou(cs):
    assert {c["args"]["mode"] for c in cs} == set(ir.MODES)
    assert {(c["flags"]["iou"], c["flags"]["best"]) for c in cs} == {(True, False), (False, True), (True, True)}
    assert {(c["args"]["mode"], c["flags"]["iou"], c["flags"]["best"]) for c in cs} == {(m, a, b) for m in ir.MODES for a, b in ((True, False), (False, True), (True, True))}


def _cover_nms(cs):
    assert {c["post_kind"] for c in cs} == set(bs.POST_MAX_KINDS) and {c["score_kind"] for c in cs} == set(bs.SCORE_KINDS)
    assert {c["thresh_kind"] for c in cs} == {"lattice", "equal"} and {c["args"]["mode"] for c in cs} == set(ir.MODES)
    assert {(c["thresh_kind"], c["args"]["mode"]) for c in cs} == {(k, m) for k in ("lattice", "equal") for m in ir.MODES}
    assert {tuple(c["flags"].values()) for c in cs} == {(a, b, k) for a in (False, True) for b in (False, True) for k in (False, True)}
    for c in cs:
        a, B = c["args"], c["args"]["boxes"].shape[1]
        want = dict(zip(bs.POST_MAX_KINDS, (1, c["natural"] - 1, c["natural"], c["natural"] + 1, B + 7)))[c["post_kind"]]
        assert a["post_max"] == min(max(want, 1), B)
        s = a["scores"][~np.isnan(a["scores"])]
        assert {"-inf": a["score_thresh"] == -math.inf, "occurs": a["score_thresh"] in s, "above": (s < a["score_thresh"]).all()}[c["score_kind"]]
    assert all((c["natural"] > 0) == ("count" in c["post_kind"]) or c["score_kind"] == "above" or c["gone"] for c in cs)
    assert any(c["post_kind"] == "count" and 1 < c["natural"] < c["args"]["boxes"].shape[1] for c in cs)
    assert any(np.isnan(c["args"]["scores"]).any() for c in cs) and max(c["args"]["boxes"].shape[1] * c["frames"] for c in cs) >= 2049
    assert any(c["args"]["boxes"].shape[1] in (255, 256, 257, 1023, 1024, 1025) and c["post_kind"] in ("count-1", "count", "count+1") for c in cs)   # B on a border, post_max on the count


def _cover_sample_rois(cs):
    assert {c["args"]["cfg"]["roi_per_image"] for c in cs} == set(bs.ROI_PER_IMAGE) and {c["args"]["cfg"]["fg_ratio"] for c in cs} == set(bs.FG_RATIOS)
    assert {c["dyadic"] for c in cs} == {False, True} and {c["args"]["cfg"]["cls_score_type"] for c in cs} == {"roi_iou", "cls"}
    assert {c["rois_form"] for c in cs} == {"tensor", "nms_batch"} and {c["overlaps_form"] for c in cs} == {"pair", "iou_batch"}
    assert {(c["args"]["seed"] >= bs.BIG, c["args"]["step"] >= bs.BIG) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
    assert cs[0]["gone"] == (0,) and cs[0]["args"]["seed"] >= bs.BIG and cs[0]["args"]["step"] >= bs.BIG          # past 2^32 in a batch whose first frame is empty
    assert {k for c in cs for k in c["kinds"]} == set(tr.BRANCH_FRAMES)
    assert all(1 <= c["args"]["gt_boxes"].shape[1] <= 64 for c in cs)
    for c in cs:
        t = c["args"]["cfg"]
        assert all(t[k] == (tr.DYADIC if c["dyadic"] else tr.DEFAULTS)[k] for k in tr.DYADIC)
        ov = c["args"]["overlap"].astype(np.float64)
        assert (ov[~np.isnan(ov)] * 8 % 1 == 0).all()


def _cover_assign_anchors(cs):
    assert {len(c["args"]["matched"]) for c in cs} == {1, 2, 3, 4} and {c["defaults"] for c in cs} == {False, True}
    assert all(1 <= c["args"]["gt_boxes"].shape[1] <= 65 for c in cs)
    used = {(m, u) for c in cs if not c["defaults"] for m, u in zip(c["args"]["matched"], c["args"]["unmatched"])}
    assert used <= set(ar.THRESHOLD_SETTINGS) and len(used) >= 10
    for c in cs:
        a, NC = c["args"], len(c["args"]["matched"])
        assert ((a["anchor_class"] < 1) | (a["anchor_class"] > NC)).any() or len(a["anchor_class"]) < 3
    cls = np.concatenate([c["args"]["gt_boxes"][..., 7].reshape(-1) for c in cs])
    assert (cls % 1 != 0).any() and (cls == 0).any()
    assert any((c["args"]["anchors"][:, 3:6] == 0).any() for c in cs) and any((c["args"]["gt_boxes"][..., 3:6] == 0).any(axis=-1).sum() > 0 for c in cs)


def _cover_rows(cs):
    unpadded = [c for c in cs if c["form"] != "padded"]
    lengths = {int(n) for c in unpadded for n in np.diff(c["offsets"])}
    assert set(rs.BORDERS) <= lengths, sorted(set(rs.BORDERS) - lengths)
    assert {c["keep_kind"] for c in cs} == set(rs.KEEP_KINDS) and {c["form"] for c in cs} == set(rs.FORMS)
    assert {c["keep_form"] for c in cs if c["keep"] is not None} == set(rs.KEEP_FORMS) and any(c["keep"] is None for c in cs)
    assert {(c["form"], c["out"]) for c in cs} == {(f, o) for f in rs.FORMS for o in (False, True)}
    assert {(c["args"]["seed"] >= bs.BIG, c["args"]["step"] >= bs.BIG) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
    assert cs[0]["gone"] == (0,) and cs[0]["args"]["seed"] >= bs.BIG and cs[0]["args"]["step"] >= bs.BIG


def _cover_paste_objects(cs):
    _cover_rows(cs)
    total = [c["args"]["gt_boxes"].shape[1] + sum(c["args"]["groups"]) for c in cs]
    assert max(total) == 256 and total.count(256) == 1
    for c in cs:
        bank, groups = c["args"]["bank"], c["args"]["groups"]
        O, per = len(bank["boxes"]), np.diff(bank["class_offsets"])[1:1 + len(groups)]
        assert 1 <= O <= 40 and 0 <= np.diff(bank["offsets"]).min() and np.diff(bank["offsets"]).max() <= 600
        assert (per == 0).any(), "a class without a bank object"
    assert {len(c["args"]["bank"]["boxes"]) for c in cs} & {1, 2, 3, 4, 5} and max(len(c["args"]["bank"]["boxes"]) for c in cs) >= 30
    assert max(int(np.diff(c["args"]["bank"]["offsets"]).max()) for c in cs) > 400 and any((np.diff(c["args"]["bank"]["offsets"]) == 0).any() for c in cs)
    assert any(not any(c["args"]["ew"]) for c in cs) and any(any(c["args"]["ew"]) for c in cs)
    assert any(g > 0 and n == 0 for c in cs for g, n in zip(c["args"]["groups"], np.diff(c["args"]["bank"]["class_offsets"])[1:]))


def _cover_transform_scene(cs):
    _cover_rows(cs)
    assert {c["tries"] for c in cs} == set(bs.TRIES) and {c["args"]["cfg"]["flip"] for c in cs} == set(bs.FLIPS)
    assert {c["world_kinds"] for c in cs} == {(a, b) for a in bs.RANGE_KINDS for b in bs.RANGE_KINDS}
    for part in ("rotation", "scaling"):
        kinds = set()
        for c in cs:
            loc = c["args"]["cfg"]["local"]
            if loc:
                kinds.add("off" if loc[part] is None else ("degenerate" if loc[part][0] == loc[part][1] else "wide"))
        assert kinds == set(bs.RANGE_KINDS), part
    assert {c["args"]["cfg"]["local"]["translation"] is None for c in cs if c["tries"]} == {False, True}
    assert {c["args"]["box_of_given"] for c in cs if c["tries"]} == {False, True} and {c["args"]["in_place"] for c in cs} == {False, True}
    assert {(c["args"]["in_place"], c["out"]) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c["args"]["gt_boxes"].shape[1], c["tries"]) for c in cs} >= {(256, 16), (256, 0), (1, 0), (65, 8)}


STAGE_COVERAGE = dict(zip(bs.STAGES, (_cover_boxes_iou, _cover_nms, lambda cs: _cover_sample_rois(cs), _cover_assign_anchors, _cover_paste_objects, _cover_transform_scene)))


# ---- the edges, counted from the restatements' own outputs -----------------------------------------------------------------------------------
def _edges_boxes_iou(c, e):
    a, b = c["args"]["a"][..., :7].astype(np.float64), c["args"]["b"][..., :7].astype(np.float64)
    v = e["iou64"]
    ok = br.present(c["args"]["a"], c["args"]["pose_a"])[:, :, None] & br.present(c["args"]["b"], c["args"]["pose_b"])[:, None, :]
    flat = (a[:, :, None, 6] == 0) & (b[:, None, :, 6] == 0)
    touch = (np.abs(a[:, :, None, 0] - b[:, None, :, 0]) == (a[:, :, None, 3] + b[:, None, :, 3]) * 0.5) & \
            (np.abs(a[:, :, None, 1] - b[:, None, :, 1]) < (a[:, :, None, 4] + b[:, None, :, 4]) * 0.5)
    assert not (v[ok & flat & touch] != 0).any()                            # (on the lattice a shared face IS area 0)
    top = v.max(axis=2)
    return dict(exactly_0_between_touching_boxes=bool((ok & flat & touch).any()), exactly_1=bool((v == 1.0).any()),
                best_tie_resolved_by_index=bool((((v == top[..., None]).sum(axis=2) >= 2) & (top > 0)).any()),
                best_tie_across_b_tiles=bool(any(np.ptp(np.flatnonzero(v[f, m] == top[f, m]) // 64) > 0 for f, m in zip(*np.nonzero(top > 0)))),
                row_whose_best_is_absent=bool((e["best"] == -1).any()), present_row_whose_best_is_absent=bool(((e["best"] == -1) & ok.any(axis=2)).any()))


def _edges_nms(c, e):
    a = c["args"]
    B, P = a["boxes"].shape[1], a["post_max"]
    b64 = a["boxes"][..., :7].astype(np.float64)
    out = dict(frame_cut_by_post_max=False, frame_with_nothing_kept=bool((e["count"] == 0).any()), kept_pair_at_iou_thresh=False, suppression_beside_it=False,
               equal_scores_in_different_tiles=False, equal_scores_in_different_groups=False, nan_score=bool(np.isnan(a["scores"]).any()))
    for f in range(c["frames"]):
        order = ir.ranking(a["boxes"][f], a["scores"][f], a["pose"][f], a["score_thresh"])
        n = int(e["count"][f])
        k = e["index"][f, :n].astype(np.int64)
        out["frame_cut_by_post_max"] |= n == P and len(order) > n and len(ir.nms_frame(a["boxes"][f], a["scores"][f], a["pose"][f], a["iou_thresh"], B, a["score_thresh"], a["mode"])) > n
        s = a["scores"][f][order].astype(np.float64)
        same = np.flatnonzero(s[1:] == s[:-1])
        out["equal_scores_in_different_tiles"] |= bool((order[same] // 1024 != order[same + 1] // 1024).any())
        out["equal_scores_in_different_groups"] |= bool((order[same] // 256 != order[same + 1] // 256).any())
        if 2 <= n <= 400:
            jj, ii = np.triu_indices(n, 1)
            ones = np.ones(len(ii), bool)
            v = ir.pair_iou(b64[f][k[ii]], a["pose"][f][k[ii]], ones, b64[f][k[jj]], a["pose"][f][k[jj]], ones, a["mode"])      # (candidate, earlier kept box)
            at = bool((v == a["iou_thresh"]).any())
            out["kept_pair_at_iou_thresh"] |= at
            out["suppression_beside_it"] |= at and len(order) > n and n < P
    return out


def _edges_sample_rois(c, e):
    cfg = c["args"]["cfg"]
    per = tr.fg_per_image(cfg)
    out = {k: False for k in tr.BRANCH_FRAMES}
    for (n_fg, n_hard, n_easy) in e["class_count"].tolist():
        bg = n_hard + n_easy
        kind = ("many_fg" if n_fg > per else "few_fg") if n_fg and bg else ("fg_only" if n_fg else ("hard_only" if n_hard and not n_easy else ("easy_only" if n_easy and not n_hard else
                                                                                                                                                   ("nothing" if not bg else None))))
        if kind:
            out[kind] = True
    picked = e["roi_iou"][e["index"] >= 0].astype(np.float64)
    for name in tr.DYADIC:
        out["picked_overlap_on_" + name] = c["dyadic"] and bool((picked == tr.DYADIC[name]).any())
    out["slots_filled_by_repetition"] = any(len(set(r[r >= 0].tolist())) < (r >= 0).sum() for r in e["index"])
    out["hard_and_easy_in_one_frame"] = bool(((e["segments"][:, 1] > 0) & (e["segments"][:, 2] > 0)).any())
    return out


def _edges_assign_anchors(c, e):
    a = c["args"]
    NC = len(a["matched"])
    m_of = np.array(a["matched"])[np.clip(a["anchor_class"], 1, NC) - 1][None, :]
    pos = e["label"] > 0
    tie = False
    for f in range(c["frames"]):
        g_cls = ar.gt_class(a["gt_boxes"][f], NC)
        for k in range(1, NC + 1):
            ai, gi = np.flatnonzero(e["anchor_ok"] & (a["anchor_class"] == k)), np.flatnonzero(g_cls == k)
            if len(ai) and len(gi) > 1:
                m = ar.overlaps(a["anchors"][ai], a["gt_boxes"][f, gi])
                tie |= bool((((m == m.max(axis=1)[:, None]).sum(axis=1) >= 2) & (m.max(axis=1) > 0)).any())
    return dict(positive_by_threshold=bool((pos & ~e["forced"]).any()), positive_forced_below_matched=bool((pos & e["forced"] & (e["best"] < m_of)).any()),
                tie_between_two_gts=tie, frame_with_count_0=bool((e["count"][:, 0] == 0).any()), background=bool((e["label"] == 0).any()),
                ignored=bool(((e["label"] < 0) & e["anchor_ok"][None]).any()), best_on_matched=bool((e["best"] == m_of).any()),
                best_on_unmatched=bool((e["best"] == np.array(a["unmatched"])[np.clip(a["anchor_class"], 1, NC) - 1][None, :]).any()))


def _edges_paste_objects(c, e):
    B = c["args"]["gt_boxes"].shape[1]
    out = {f"state_{s}": bool((e["state"] == s).any()) for s in range(6)}
    straddle = False
    for f in range(c["frames"]):
        a, b = int(c["offsets"][f]), int(c["offsets"][f + 1])
        src = e["source"][a:b]
        for q in np.flatnonzero(e["state"][f] == pr.PASTED):
            at = np.flatnonzero(src == B + q)
            straddle |= len(at) > 0 and at[0] // pr.RUN != at[-1] // pr.RUN
    out.update(paste_that_straddles_a_run=bool(straddle), scene_rows_removed=bool((e["count"][:, 2] > 0).any()), frame_without_a_free_slot=bool((e["count"][:, 3] == 0).any()))
    return out


def _edges_transform_scene(c, e):
    T = c["tries"]
    return dict(still=bool((e["state"] == sr.STILL).any()), moved=bool((e["state"] == sr.MOVED).any()), blocked=bool((e["state"] == sr.BLOCKED).any()),
                blocked_on_every_try=T >= 2 and bool(((e["state"] == sr.BLOCKED) & (e["tries"][..., 7] == 1).all(axis=-1)).any()),
                tried_at_T_minus_1=T >= 2 and bool((e["tried"] == T - 1).any()), first_try_taken=T >= 2 and bool((e["tried"] == 0).any()),
                flipped_about_both=bool((e["world"][:, :2] == 1).all(axis=1).any()), rows_moved_with_their_box=T > 0 and bool((e["state"] == sr.MOVED).any()))


EDGES = dict(zip(bs.STAGES, (_edges_boxes_iou, _edges_nms, _edges_sample_rois, _edges_assign_anchors, _edges_paste_objects, _edges_transform_scene)))


@pytest.mark.parametrize("stage, dtype", CASES)
def test_edges_are_reached(stage, dtype):
    reached = {}
    for c in bs.configs(stage, dtype):
        for name, hit in EDGES[stage](c, bs.expected(stage, c)).items():
            reached[name] = reached.get(name, 0) + bool(hit)
    print(f"\n[box-sweep] {stage} {dtype}: configs that reach " + ", ".join(f"{k} {v}" for k, v in reached.items()))
    assert all(reached.values()), [k for k, v in reached.items() if not v]


# ---- every drawn dimension decides something ---------------------------------------------------------------------------------------------------
def _differs(stage, c, **replaced):
    want, other = bs.expected(stage, c), bs.restate(stage, c, **replaced)
    return any(other[f].shape != want[f].shape or other[f].tobytes() != want[f].tobytes() for f in bs.fields(stage, dict(c, flags={k: True for k in c["flags"]})))


def _cfg(c, **changed):
    return dict(cfg={**c["args"]["cfg"], **changed})


def _dimensions(stage):
    """{name: (which configs, the replacement)}: each drawn dimension of the stage, replaced alone."""
    other_mode = lambda c: dict(mode=ir.MODES[1 - ir.MODES.index(c["args"]["mode"])])      # noqa: E731
    every = lambda c: True                                                                # noqa: E731
    counter = dict(step=(every, lambda c: dict(step=c["args"]["step"] + 1)), seed=(every, lambda c: dict(seed=c["args"]["seed"] + 1)),
                   step_high_word=(every, lambda c: dict(step=c["args"]["step"] ^ bs.BIG)), seed_high_word=(every, lambda c: dict(seed=c["args"]["seed"] ^ bs.BIG)))
    rows = dict(keep=(lambda c: c["keep"] is not None and c["form"] != "padded", lambda c: dict(keep=None)),
                frames=(lambda c: c["frames"] > 1 and c["form"] != "padded", lambda c: dict(offsets=np.array([0, len(c["rows"])], np.int64), gt_boxes=c["args"]["gt_boxes"][:1],
                                                                                           pose=c["args"]["pose"][:1])))
    if stage == "boxes_iou":
        return dict(mode=(every, other_mode), heading=(every, lambda c: dict(pose_b=np.where(c["args"]["pose_b"] == c["args"]["pose_b"], (1.0, 0.0), 0.0))))
    if stage == "nms":
        return dict(mode=(every, other_mode), iou_thresh_at_equality=(lambda c: c["thresh_kind"] == "equal", lambda c: dict(iou_thresh=float(np.nextafter(c["args"]["iou_thresh"], -1.0)))),
                    iou_thresh=(lambda c: c["thresh_kind"] == "lattice", lambda c: dict(iou_thresh=0.9375)),
                    post_max=(every, lambda c: dict(post_max=c["args"]["boxes"].shape[1])), score_thresh=(lambda c: c["score_kind"] != "-inf", lambda c: dict(score_thresh=-math.inf)),
                    score_ties=(every, lambda c: dict(scores=(c["args"]["scores"] + (np.arange(c["args"]["boxes"].shape[1]) % 7) / 1024).astype(c["args"]["scores"].dtype))))
    if stage == "sample_rois":
        return dict(counter, roi_per_image=(every, lambda c: _cfg(c, roi_per_image=3)), fg_ratio=(every, lambda c: _cfg(c, fg_ratio=0.25)),
                    cls_score_type=(every, lambda c: _cfg(c, cls_score_type="cls" if c["args"]["cfg"]["cls_score_type"] == "roi_iou" else "roi_iou")),
                    thresholds=(every, lambda c: _cfg(c, **(tr.DYADIC if not c["dyadic"] else {k: tr.DEFAULTS[k] for k in tr.DYADIC}))),
                    hard_bg_ratio=(every, lambda c: _cfg(c, hard_bg_ratio=0.5)), assignment=(every, lambda c: dict(assignment=np.zeros_like(c["args"]["assignment"]))))
    if stage == "assign_anchors":
        return dict(thresholds=(lambda c: not c["defaults"], lambda c: dict(matched=(0.6,) * len(c["args"]["matched"]), unmatched=(0.45,) * len(c["args"]["matched"]))),
                    n_classes=(lambda c: len(c["args"]["matched"]) > 1, lambda c: dict(matched=c["args"]["matched"][:-1], unmatched=c["args"]["unmatched"][:-1])),
                    anchor_class=(every, lambda c: dict(anchor_class=np.ones_like(c["args"]["anchor_class"]))))
    if stage == "paste_objects":
        return dict(counter, **rows, extra_width=(every, lambda c: dict(ew=(0.0, 0.0, 0.0) if any(c["args"]["ew"]) else (0.5, 0.5, 0.5))),
                    groups=(lambda c: sum(c["args"]["groups"]) > 1, lambda c: dict(groups=c["args"]["groups"][::-1])))
    sc = lambda c, **kw: dict(cfg={**c["args"]["cfg"], **kw})                             # noqa: E731
    loc = lambda c, **kw: dict(cfg={**c["args"]["cfg"], "local": {**c["args"]["cfg"]["local"], **kw}})      # noqa: E731
    has = lambda part: (lambda c: c["tries"] > 0 and c["args"]["cfg"]["local"][part] is not None)           # noqa: E731
    return dict(counter, **rows, flip=(lambda c: c["args"]["cfg"]["flip"] != (), lambda c: sc(c, flip=())), rotation=(lambda c: c["world_kinds"][0] != "off", lambda c: sc(c, rotation=None)),
                scaling=(lambda c: c["world_kinds"][1] != "off", lambda c: sc(c, scaling=None)), local=(lambda c: c["tries"] > 0, lambda c: sc(c, local=None)),
                tries=(lambda c: c["tries"] > 1, lambda c: loc(c, tries=1)), local_translation=(has("translation"), lambda c: loc(c, translation=None)),
                local_rotation=(has("rotation"), lambda c: loc(c, rotation=None)), local_scaling=(has("scaling"), lambda c: loc(c, scaling=None)))


@pytest.mark.parametrize("stage, dtype", CASES)
def test_every_drawn_dimension_decides_something(stage, dtype):
    cs = bs.configs(stage, dtype)
    for name, (applies, replacement) in _dimensions(stage).items():
        some = [c for c in cs if applies(c)]
        assert some, name
        assert any(_differs(stage, c, **replacement(c)) for c in some), name
