"""Seeded random configurations of the six stages that work on box sets -- boxes_iou, nms, sample_rois, assign_anchors, paste_objects,
transform_scene -- and their expected outputs: the CROSS PRODUCT that the hand-built cases of the stages' own test files never run --
box counts on the kernels' borders, two box widths, frames without a present box, the pose source, out=, the optional outputs and the
stage arguments at their thresholds, all drawn together.  Pure NumPy; the expected outputs come from the stages' restatements
(tests/*_reference.py), which are exact.  Box centres, sizes, scores and overlaps lie on a lattice that is exact in float32 (a step of
random_sweep_inputs.STEPS; sizes are multiples of 0.5, which every step divides), so touching faces, equal IoUs and equal scores are
frequent; headings come from three sources: multiples of pi / 2, values 0 .. 2 ulps of the dtype apart, and a continuous range.  Nothing
here imports the package's native code.

configs(stage, dtype) is a tuple of 24 read-only dicts, config i seeded by [2027, crc32(stage), dtype == "float64", i]:

  args        the stage's arguments as its restatement takes them, arrays among them; every pose in it is NumPy's
  flags       the optional outputs by field name, on or off
  out         whether the call gets out= with exactly the requested fields, pre-filled with 0x7f bytes (every second config)
  pose_source "given" (args' pose is handed over), "device" (pose=None) or "fed_back" (the device's own pose, read back and handed over
              as test_gpu_iou._device_pose does); None for assign_anchors, which takes no pose
  frames, gone  the frames of the call and those in which every box of the stage's main box set is absent
  rows, offsets, keep, sizes, form, keep_kind, keep_form   paste_objects and transform_scene: the batch, as random_sweep_inputs draws it

Drawn by position, so that tests/test_box_sweep_inputs.py finds them whatever the stream gives: the size borders in turn (SIZES), an
all-absent first frame (i = 0), an all-absent last frame (i = 2), two all-absent frames in a row (i = 3), one all-absent frame between
two full ones (i = 7), F = 1 (i = 5), the box widths 7 .. 10 walking independently, the pose source in turn, out= on every second
config.  Everything else comes from the stream.

COST.  The restatements of nms, paste_objects and transform_scene walk pairs in Python, so what the issue leaves free is capped: F <= 4,
the uniform box counts end at 300, frames of the two row stages at 600 rows (the borders up to 2049 stay), a B > 1000 nms call has
one frame, a paste with 63 or 64 slots few present gts, and a scene call keeps present^2 x tries below 60 000 by making more
boxes absent.  No border is dropped.  nms's post_max of B + 7 is clipped to B, the largest value the entry takes."""
import functools
import math
import zlib

import numpy as np

import anchors_reference as ar
import box_reference as br
import iou_reference as ir
import paste_reference as pr
import random_sweep_inputs as rs
import scene_reference as sr
import targets_reference as tr

DTYPES = br.DTYPES
STAGES = ("boxes_iou", "nms", "sample_rois", "assign_anchors", "paste_objects", "transform_scene")
N_CONFIGS = 24
STEPS = rs.STEPS
POSE_SOURCES = ("given", "device", "fed_back")
WIDTHS = (7, 8, 9, 10)
SIZES = dict(boxes_iou=(1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257),              # the 64-wide b tiles and SG_IOU_BLOCK
             nms=(1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049),            # SG_NMS_TILE, SG_NMS_BLOCK and the groups of k_nms_rank
             sample_rois=(1, 2, 63, 64, 65, 129, 511, 512, 513),                       # SG_TGT_BLOCK
             assign_anchors=(1, 2, 255, 256, 257, 511, 512, 513, 2049),                # SG_ANCHORS_GROUP
             paste_objects=(1, 64, 2, 63),                                             # Q
             transform_scene=(1, 3, 64, 65, 256))                                      # B
TRIES = (0, 1, 2, 8, 16)
ROI_PER_IMAGE = (1, 2, 64, 128, 1024)
FG_RATIOS = (0.0, 0.5, 1.0)
POST_MAX_KINDS = ("one", "count-1", "count", "count+1", "B+7")
SCORE_KINDS = ("-inf", "occurs", "above")
RANGE_KINDS = ("off", "degenerate", "wide")
FLIPS = ((), ("x",), ("y",), ("x", "y"))
BIG = 1 << 32
REACH = 12.0
UNIFORM_TOP, ROWS_TOP, F_TOP = 300, 600, 4


# ---- the shared draws ---------------------------------------------------------------------------------------------------------------------
_pick, _on = rs._pick, rs._on


def _plan(rng, i, at_least=1, at_most=F_TOP):
    """(F, gone): the frames of config i and those without a present box."""
    F = 1 if i == 5 else int(rng.integers(1, at_most + 1))
    gone = ()
    if i in (0, 2):
        F = max(F, 2)
        gone = (0,) if i == 0 else (F - 1,)
    if i == 3:
        F, gone = 4, (1, 2)
    if i == 7:
        F, gone = max(F, 3), (1,)
    if i != 5:
        F = max(F, at_least)
    return F, gone


def _headings(rng, shape, dtype):
    """Multiples of pi / 2 (0 among them: cos and sin exact), values 0 .. 2 ulps of the dtype above one base value, and U(-7, 7)."""
    n = int(np.prod(shape))
    src = rng.integers(0, 3, n)
    right = rng.integers(-2, 3, n) * (np.pi / 2)
    base = np.full(n, rng.uniform(-3, 3)).astype(dtype)
    near = ir._ulps(base, np.full(n, 10.0), rng.integers(0, 3, n)).astype(np.float64)
    return np.where(src == 0, right, np.where(src == 1, near, rng.uniform(-7, 7, n))).reshape(shape)


def _boxes(rng, F, B, C, dtype, step, reach=REACH, absent=0.15, classes=3, flat=0.3):
    """(F, B, C) boxes on the lattice: centres multiples of `step` within +-reach, sizes multiples of 0.5 in 1 .. 4 x 1 .. 2 x 1 .. 2, a
    share `flat` with heading exactly 0, class 1 .. classes in column 7; `absent` of them a zero row, a zero size or a NaN."""
    k = int(round(reach / step))
    b = np.zeros((F, B, 10))
    b[..., :2] = rng.integers(-k, k + 1, (F, B, 2)) * step
    b[..., 2] = rng.integers(-2, 3, (F, B)) * 0.5
    b[..., 3], b[..., 4], b[..., 5] = rng.integers(2, 9, (F, B)) * 0.5, rng.integers(2, 5, (F, B)) * 0.5, rng.integers(2, 5, (F, B)) * 0.5
    b[..., 6] = np.where(rng.random((F, B)) < flat, 0.0, _headings(rng, (F, B), dtype))
    b[..., 7] = rng.integers(1, classes + 1, (F, B))
    b[..., 8:] = rng.uniform(-3, 3, (F, B, 2))
    for f, m in zip(*np.nonzero(rng.random((F, B)) < absent)):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            b[f, m] = 0.0
        elif kind == 1:
            b[f, m, 3 + int(rng.integers(0, 3))] = 0.0
        else:
            b[f, m, int(rng.integers(0, 7))] = np.nan
    return np.ascontiguousarray(b[..., :C].astype(dtype))


def _empty(boxes, gone):
    """Every box of the frames `gone` a zero row; every other frame holds a present box (box 0 is made one where the draw left none)."""
    boxes[list(gone)] = 0.0
    for f in np.flatnonzero(~br.present(boxes, br.numpy_pose(boxes)).any(axis=1)):
        if f not in gone:
            boxes[f, 0, :7] = (0.0, 0.0, 0.0, 2.0, 1.0, 1.0, 0.0)
    return boxes


def _size(rng, i, borders, shift=0):
    """Border i - shift where there is one, else uniform in 3 .. UNIFORM_TOP."""
    j = i - shift
    return int(borders[j]) if 0 <= j < len(borders) else int(rng.integers(3, UNIFORM_TOP + 1))


def _counter(i):
    """(seed, step): each small or past 2^32; config 0, whose first frame is empty, has both past it."""
    return (7 + i + (BIG * 3 if (i // 2) % 2 == 0 else 0), i % 5 + (BIG + (1 << 40) if i % 2 == 0 else 0))


def _common(i, F, gone, step, pose=True):
    return dict(out=bool(i % 2), pose_source=POSE_SOURCES[i % 3] if pose else None, frames=F, gone=tuple(gone), step=step)


# ---- the stages' own draws ------------------------------------------------------------------------------------------------------------------
def _boxes_iou(rng, i, dtype):
    n = len(SIZES["boxes_iou"])
    M = _size(rng, i, SIZES["boxes_iou"]) if i < 2 * n else int(SIZES["boxes_iou"][(3 * i) % n])
    B = _size(rng, i, SIZES["boxes_iou"], n) if i < 2 * n else int(SIZES["boxes_iou"][(5 * i) % n])
    F, gone = _plan(rng, i)
    step = _pick(rng, STEPS)
    a, b = _boxes(rng, F, M, WIDTHS[i % 4], dtype, step), _boxes(rng, F, B, WIDTHS[(i // 4) % 4], dtype, step)
    a, b = np.array(a), np.array(b)
    for f in range(F):
        twin = np.flatnonzero(rng.random(M) < 0.3)                      # a boxes that ARE b boxes: exact ones, and ties for best where b repeats
        a[f, twin, :7] = b[f, rng.integers(0, B, len(twin)), :7]
        if B >= 3 and M >= 2:
            one = (1.0, -2.0, 0.5, 3.0, 1.5, 1.0, 0.0)
            a[f, 0, :7], b[f, 0, :7] = one, one
            b[f, 0, 0] += 3.0                                           # b 0 touches a 0 along a face: area exactly 0
            a[f, 1, :7] = b[f, 1, :7] = b[f, 2, :7] = (-3.0, 4.0, 0.0, 2.0, 1.0, 1.5, 0.0)
            if B > 65:
                b[f, B - 1, :7] = b[f, 1, :7]                           # ... and once more in the last tile of b: the tie spans tiles
    _empty(b, gone)
    c = _common(i, F, gone, step)
    c["args"] = dict(a=a, b=b, pose_a=br.numpy_pose(a), pose_b=br.numpy_pose(b), mode=ir.MODES[(i // 2) % 2])
    c["flags"] = dict(zip(("iou", "best"), ((True, False), (False, True), (True, True))[(i // 4) % 3]))
    return c


def _nms(rng, i, dtype):
    B = int(SIZES["nms"][i % len(SIZES["nms"])])
    F, gone = _plan(rng, i, at_most=1 if B > 1000 else F_TOP)
    step = _pick(rng, STEPS)
    boxes = np.array(_boxes(rng, F, B, WIDTHS[i % 4], dtype, step))
    scores = rng.integers(0, 17, (F, B)) / 16.0                          # ties in every tile
    scores[rng.random((F, B)) < 0.03] = np.nan
    mode = ir.MODES[(i // 3) % 2]
    equal = (i // 2) % 2 == 1 and B >= 4
    if B >= 4:                                                           # a pair apart from the rest, the two best scores: IoU 3 / 5 in either mode
        boxes[:, B - 1, :7], boxes[:, B - 2, :7] = (100.0, 0.0, 0.0, 4.0, 2.0, 1.0, 0.0), (101.0, 0.0, 0.0, 4.0, 2.0, 1.0, 0.0)
        scores[:, B - 1], scores[:, B - 2] = 2.0, 1.5
    boxes, scores = _empty(boxes, gone).astype(dtype), scores.astype(dtype)
    pose = br.numpy_pose(boxes)
    if equal:
        p = boxes[0, [B - 2, B - 1], :7].astype(np.float64)
        q = np.array([[1.0, 0.0]])
        iou_thresh = float(ir.pair_iou(p[:1], q, np.ones(1, bool), p[1:], q, np.ones(1, bool), mode)[0])
    else:
        iou_thresh = _pick(rng, (0.125, 0.25, 0.5, 0.75))
    kind = "above" if i % 12 == 7 else SCORE_KINDS[(i // 3) % 2]
    seen = np.sort(scores[~np.isnan(scores)].astype(np.float64))
    score_thresh = -math.inf if kind == "-inf" or not len(seen) else (float(seen[len(seen) // 2]) if kind == "occurs" else 3.0)
    post_kind = POST_MAX_KINDS[i % 5]
    count = int(ir.nms(boxes, scores, pose, iou_thresh, B, score_thresh, mode)["count"].max()) if "count" in post_kind else 0      # (the largest of the frames)
    post_max = dict(zip(POST_MAX_KINDS, (1, count - 1, count, count + 1, B + 7)))[post_kind]
    c = _common(i, F, gone, step)
    c.update(post_kind=post_kind, score_kind=kind, thresh_kind="equal" if equal else "lattice", natural=count)
    c["args"] = dict(boxes=boxes, scores=scores, pose=pose, iou_thresh=iou_thresh, post_max=int(min(max(post_max, 1), B)), score_thresh=score_thresh, mode=mode)
    k = (i // 2 + i) % 8                                                   # every combination, each with and without out=
    c["flags"] = dict(boxes=bool(k & 1), scores=bool(k & 2), kept=bool(k & 4))
    return c


BRANCH_KINDS = tuple(sorted(tr.BRANCH_FRAMES, key=tr.BRANCH_FRAMES.get))


def _overlaps(rng, kind, M, cfg):
    """M overlaps in eighths of one frame of this branch kind (targets_reference.BRANCH_FRAMES) under cfg's thresholds."""
    fg_lo = int(math.ceil(min(cfg["reg_fg_thresh"], cfg["cls_fg_thresh"]) * 8))
    hard = (1, max(1, int(math.ceil(cfg["reg_fg_thresh"] * 8)) - 1))
    if kind == "many_fg":
        k = rng.integers(0, 9, M)
    elif kind == "few_fg":
        k = np.where(rng.random(M) < 0.1, rng.integers(fg_lo, 9, M), np.where(rng.random(M) < 0.05, rng.integers(hard[0], hard[1] + 1, M), 0))
        k[0] = 8
    elif kind == "fg_only":
        k = rng.integers(fg_lo, 9, M)
    elif kind == "hard_only":
        k = rng.integers(hard[0], hard[1] + 1, M)
    else:
        k = np.zeros(M, np.int64)
    ov = k / 8.0
    if kind == "nothing":
        ov[::2] = np.nan
    elif M > 8:
        ov[rng.random(M) < 0.03] = np.nan
    return ov


def _sample_rois(rng, i, dtype):
    M = int(SIZES["sample_rois"][i % len(SIZES["sample_rois"])])
    B = int(rng.integers(1, 65))
    F, gone = _plan(rng, i)
    step = _pick(rng, STEPS)
    dyadic = (i // 2) % 2 == 0
    cfg = tr.settings(roi_per_image=ROI_PER_IMAGE[i % 5], fg_ratio=FG_RATIOS[(i // 3) % 3], hard_bg_ratio=_pick(rng, (0.8, 0.4, 0.0, 1.0)),
                      cls_score_type=("roi_iou", "cls")[(i // 4) % 2], **(tr.DYADIC if dyadic else {}))
    rois, gt = np.array(_boxes(rng, F, M, WIDTHS[i % 4], dtype, step)), _boxes(rng, F, B, WIDTHS[(i // 4) % 4], dtype, step)
    kinds = ["nothing" if f in gone else BRANCH_KINDS[(i + f) % 6] for f in range(F)]
    ov = np.stack([_overlaps(rng, k, M, cfg) for k in kinds])
    for f, k in enumerate(kinds):
        if k == "nothing":
            rois[f, 1::2] = 0.0
    _empty(rois, gone)
    seed, stp = _counter(i)
    c = _common(i, F, gone, step)
    c.update(kinds=tuple(kinds), dyadic=dyadic, rois_form=("tensor", "nms_batch")[(i // 3) % 2], overlaps_form=("pair", "iou_batch")[(i // 2) % 2])
    c["args"] = dict(rois=rois, gt_boxes=gt, overlap=np.ascontiguousarray(ov.astype(dtype)), assignment=rng.integers(-1, B + 1, (F, M)).astype(np.int32),
                     pose=br.numpy_pose(rois), cfg=cfg, seed=seed, step=stp)
    c["flags"] = dict(gt_local=_on(rng), pose=_on(rng))
    return c


def _assign_anchors(rng, i, dtype):
    n = len(SIZES["assign_anchors"])
    A = int(SIZES["assign_anchors"][i % n]) if i < 2 * n else int(rng.integers(3, 701))
    B = int(rng.integers(1, 66))
    F, gone = _plan(rng, i)
    step = _pick(rng, STEPS)
    NC = 1 + i % 4
    anchors = np.array(_boxes(rng, 1, A, WIDTHS[(i // 4) % 4], dtype, step, absent=0.08, flat=0.6)[0])
    gt = np.array(_boxes(rng, F, B, 8 + i % 3, dtype, step, classes=NC, flat=0.6))
    cls = rng.integers(0, NC + 2, A).astype(np.int32)                    # 0 and NC + 1: absent anchors
    for f in range(F):                                                   # gts ON anchors, equal or half as long: exact 1, 1 / 2, and bit-equal twins
        on = np.flatnonzero(rng.random(B) < 0.5)
        at = rng.integers(0, A, len(on))
        gt[f, on, :7] = anchors[at, :7]
        gt[f, on, 7] = np.where(rng.random(len(on)) < 0.8, cls[at], rng.integers(0, NC + 2, len(on)))
        half = on[rng.random(len(on)) < 0.5]
        gt[f, half, 3] *= 0.5
    gt[..., 7] = np.where(rng.random((F, B)) < 0.05, 1.5, gt[..., 7])    # a class that is no whole number: absent
    gt[..., 7] = np.where(gt[..., 7] == 0, 1.0, gt[..., 7]) if B < 3 else gt[..., 7]
    _empty(gt, gone)
    if (i // 2) % 2:
        pairs = [_pick(rng, ar.THRESHOLD_SETTINGS) for _ in range(NC)]
        matched, unmatched = tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)
    else:
        matched, unmatched = (ar.MATCHED + (0.5,))[:NC], (ar.UNMATCHED + (0.35,))[:NC]
    c = _common(i, F, gone, step, pose=False)
    c.update(defaults=(i // 2) % 2 == 0)
    c["args"] = dict(anchors=anchors, anchor_class=cls, gt_boxes=np.ascontiguousarray(gt.astype(dtype)), matched=matched, unmatched=unmatched)
    c["flags"] = dict(iou=_on(rng))
    return c


def _rows(rng, i, dtype, F, step):
    """The batch of the two row stages as random_sweep_inputs._batch makes it, with F given: border j in one frame of the j-th unpadded
    config, the other frames uniform in 3 .. ROWS_TOP rows; its KEEP_KINDS, FORMS and KEEP_FORMS in turn."""
    form, keep_kind = rs.FORMS[i % 3], rs.KEEP_KINDS[i % 7]
    sizes = [int(rng.integers(3, ROWS_TOP + 1)) for _ in range(F)]
    if form != "padded":
        j = (i - (i + 1) // 3) % len(rs.BORDERS)
        free = [f for f in range(F) if not (keep_kind == "frame_false" and f < 3)] or [F - 1]
        sizes[free[int(rng.integers(0, len(free)))]] = int(rs.BORDERS[j])
    if not sum(sizes):
        sizes[0] = 5
    frames = [rs._frame(rng, n, rs._cluster(rng, rs._grown(rs.CENTRED), step) if rng.random() < 0.4 else rs._grown(rs.CENTRED), step, dtype) for n in sizes]
    keep = rs._keep(rng, keep_kind, sizes)
    if form == "padded":
        N = max(sizes)
        rows, mask = np.full((F, N, 5), np.nan, dtype), np.zeros((F, N), bool)
        for f, p in enumerate(frames):
            rows[f, :len(p)] = p
            mask[f, :len(p)] = True if keep is None else keep[f]
        rows, offsets, keep = rows.reshape(-1, 5), np.arange(F + 1, dtype=np.int64) * N, mask.reshape(-1)      # (the padding is absent: a mask always)
    else:
        rows = np.ascontiguousarray(np.concatenate(frames))
        offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        keep = None if keep is None else np.concatenate(keep)
    return dict(rows=np.ascontiguousarray(rows), offsets=offsets, keep=keep, sizes=tuple(sizes), form=form, keep_kind=keep_kind, keep_form=rs.KEEP_FORMS[(i // 3 + i) % 3])


def _paste_objects(rng, i, dtype):
    Q = int(SIZES["paste_objects"][i % 4])
    full = i == 5                                                         # B + Q = 256, once
    B = 256 - Q if full else int(rng.integers(1, 7 if Q > 2 else 41))
    F, gone = _plan(rng, i, at_least=3 if i % 7 == 4 else 1, at_most=3)
    step = _pick(rng, STEPS)
    NC = int(rng.integers(2, 6))
    void = int(rng.integers(1, NC + 1))                                   # the class without a bank object
    groups = np.bincount(rng.integers(0, NC, Q), minlength=NC)
    if Q > 1 and not groups[void - 1]:
        groups[void - 1], groups[int(np.argmax(groups))] = 1, groups.max() - 1
    O = int(rng.integers(1, 41))
    bank_boxes = np.array(_boxes(rng, 1, O, 8, dtype, step, reach=20.0, absent=0.1)[0])
    bank_boxes[:, 7] = np.sort(rng.choice([k for k in range(1, NC + 1) if k != void], O))
    counts = np.where(rng.random(O) < 0.15, 0, rng.integers(0, 601 if O < 12 else 121, O))
    bank = _bank(rng, bank_boxes, counts, dtype)
    gt = np.array(_boxes(rng, F, B, 8 + i % 3, dtype, step, reach=20.0, absent=0.85 if full else 0.2, classes=NC))
    _empty(gt, gone)
    seed, stp = _counter(i)
    c = _common(i, F, gone, step)
    c.update(_rows(rng, i, dtype, F, step))
    c["args"] = dict(gt_boxes=gt, pose=br.numpy_pose(gt), bank=bank, groups=tuple(int(v) for v in groups), seed=seed, step=stp,
                     ew=_pick(rng, ((0.0, 0.0, 0.0), (0.25, 0.25, 0.125), (0.5, 0.0, 0.0))))
    c["flags"] = dict(source=_on(rng), pose=_on(rng))
    return c


def _bank(rng, boxes, counts, dtype):
    """paste_reference._bank_of for boxes some of which are absent: an absent box (a zero size, a NaN) gets its points about the origin."""
    shape = np.nan_to_num(np.asarray(boxes, np.float64))
    shape[:, 3:6] = np.where(shape[:, 3:6] > 0, shape[:, 3:6], 1.0)
    pts = [pr._points_in(rng, s, int(n), dtype) for s, n in zip(shape, counts)]
    return pr.make_bank(np.concatenate(pts) if pts else np.zeros((0, 5), dtype), np.concatenate(([0], np.cumsum(counts))), np.asarray(boxes, np.float64).astype(dtype))


def _range(rng, kind, wide, at):
    return None if kind == "off" else ((at, at) if kind == "degenerate" else wide)


def _transform_scene(rng, i, dtype):
    B = int(SIZES["transform_scene"][i % 5])
    T = TRIES[(i + i // 5) % 5]
    F, gone = _plan(rng, i, at_least=3 if i % 7 == 4 else 1, at_most=3)
    step = _pick(rng, STEPS)
    target = math.sqrt(60000.0 / max(T, 1) / F)
    gt = np.array(_boxes(rng, F, B, WIDTHS[i % 4], dtype, step, reach=10.0 if B < 64 else 30.0, absent=max(0.15, 1.0 - target / B)))
    if B >= 3:                                                            # box 0 inside box 1, 12 m wide: every try of either collides
        gt[:, 0, :7], gt[:, 1, :7] = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.5), (0.0, 0.0, 0.0, 12.0, 12.0, 1.0, 0.0)
    _empty(gt, gone)
    local = None
    if T:
        local = dict(translation=_pick(rng, (None, (2.0, 2.0, 0.25), (0.5, 0.0, 0.0))), rotation=_range(rng, _pick(rng, RANGE_KINDS), (-sr.PI / 20, sr.PI / 20), 0.125),
                     scaling=_range(rng, _pick(rng, RANGE_KINDS), (0.95, 1.05), 1.25), tries=T)
    kinds = (RANGE_KINDS[i % 3], RANGE_KINDS[(i // 3) % 3])
    cfg = sr.config(FLIPS[i % 4], _range(rng, kinds[0], (-sr.PI / 4, sr.PI / 4), 0.3), _range(rng, kinds[1], (0.95, 1.05), 1.25), local)
    seed, stp = _counter(i)
    c = _common(i, F, gone, step)
    c.update(_rows(rng, i, dtype, F, step))
    c.update(world_kinds=kinds, tries=T)
    for f in range(F):                                                    # rows inside the frame's boxes, so that the local part moves some
        n, a = c["sizes"][f], int(c["offsets"][f])
        ok = np.flatnonzero(br.present(gt[f], br.numpy_pose(gt[f])))
        for r in (rng.integers(0, n, min(n, 40)) if n and len(ok) else ()):
            box = gt[f, int(_pick(rng, ok))].astype(np.float64)
            c["rows"][a + r, :3] = br.world(box, rng.uniform(-0.45, 0.45, 3) * box[3:6])[0].astype(dtype)
    c["args"] = dict(gt_boxes=gt, pose=br.numpy_pose(gt), cfg=cfg, seed=seed, step=stp, box_of_given=bool(T) and _on(rng), in_place=c["form"] == "batch" and _on(rng))
    c["flags"] = dict(pose=_on(rng), tries=bool(T) and _on(rng))
    return c


DRAW = dict(zip(STAGES, (_boxes_iou, _nms, _sample_rois, _assign_anchors, _paste_objects, _transform_scene)))


def _freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, dict):
        for x in v.values():
            _freeze(x)
    return v


@functools.lru_cache(maxsize=None)
def configs(stage, dtype, n=N_CONFIGS):
    out = []
    for i in range(n):
        rng = np.random.default_rng([2027, zlib.crc32(stage.encode()), dtype == "float64", i])
        c = DRAW[stage](rng, i, dtype)
        c.update(stage=stage, dtype=dtype, i=i)
        out.append(_freeze(c))
    return tuple(out)


# ---- the expected outputs -------------------------------------------------------------------------------------------------------------------
def restate(stage, c, **changed):
    """The restatement's outputs for config c as a dict of NumPy arrays, named as the fields of the stage's batch object, with some
    arguments replaced: the poses the device computed (pose, pose_a, pose_b, bank_pose), the cos / sin a transform_scene call returned
    (world_cs, tries_cs), or -- for tests/test_box_sweep_inputs.py -- any drawn dimension."""
    a = {**c["args"], **changed}
    if stage == "boxes_iou":
        return ir.boxes_iou(a["a"], a["b"], a["pose_a"], a["pose_b"], a["mode"])
    if stage == "nms":
        return ir.nms(a["boxes"], a["scores"], a["pose"], a["iou_thresh"], a["post_max"], a["score_thresh"], a["mode"])
    if stage == "sample_rois":
        e = tr.sample_rois(a["rois"], a["gt_boxes"], a["overlap"], a["assignment"], a["pose"], a["cfg"], a["seed"], a["step"])
        e["branch"] = np.array([ord(b) for b in e["branch"]], np.uint8)
        return e
    if stage == "assign_anchors":
        return ar.assign(a["anchors"], a["anchor_class"], a["gt_boxes"], a["matched"], a["unmatched"])
    rows, offsets, keep = a.get("rows", c["rows"]), a.get("offsets", c["offsets"]), a.get("keep", c["keep"])
    if stage == "paste_objects":
        bank = a["bank"] if a.get("bank_pose") is None else dict(a["bank"], pose=a["bank_pose"])
        return pr.paste_objects(rows, offsets, keep, a["gt_boxes"], a["pose"], bank, a["groups"], a["seed"], a["step"], a["ew"])
    if stage == "transform_scene":
        return sr.transform_scene(rows, offsets, keep, a["gt_boxes"], a["pose"], a["cfg"], a["seed"], a["step"], a.get("world_cs"), a.get("tries_cs"), a.get("box_of"))
    raise KeyError(stage)


@functools.lru_cache(maxsize=None)
def _expected(stage, dtype, i):
    return _freeze(restate(stage, configs(stage, dtype)[i]))


def expected(stage, cfg, **fed_back):
    """The restatement of config cfg -- computed once per (stage, dtype, i) and read-only when nothing is fed back; with what the device
    returned (restate's keywords) in the place of NumPy's cos / sin otherwise."""
    return restate(stage, cfg, **fed_back) if fed_back else _expected(stage, cfg["dtype"], cfg["i"])


ALWAYS = dict(boxes_iou=(), nms=("index", "count"), sample_rois=tr.FIELDS[:9], assign_anchors=ar.FIELDS[:4],
              paste_objects=("rows", "keep", "gt_boxes", "object", "state", "count"), transform_scene=sr.FIELDS[:7])


def fields(stage, cfg):
    """The fields the call of cfg produces: the stage's fixed ones and the optional ones that were drawn on."""
    more = tuple(name for name, on in cfg["flags"].items() if on)
    if stage == "boxes_iou" and cfg["flags"]["best"]:
        more += ("best_iou",)
    return ALWAYS[stage] + more
