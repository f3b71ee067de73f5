"""Ground-truth object paste (snowgpu_paste_objects_device) restated from its definition in include/snowgpu.h, one frame and one slot
after the other: NumPy for presence (box_reference), the overlap (iou_reference.clip_area) and membership in the enlarged boxes
(roipool_reference.enlarged, box_reference.frame_matrices), Python integers for the Philox words (seeded_reference.philox4x32_10), the
draw and the sweep.  The pose is an INPUT, for the gts and for the bank.  Nothing here touches a GPU, and this module is no conftest: the
tests import it by name.  The named cases the GPU tests run live here too, so that tests/test_paste_reference.py can check on any machine
that each of them decides something."""
from functools import lru_cache

import numpy as np

import box_reference as br
import iou_reference as ir
import roipool_reference as rp
from seeded_reference import philox4x32_10

DTYPES = br.DTYPES
TAG = 0x50415354                    # "PAST"
RUN = rp.RUN
FIELDS = ("rows", "keep", "gt_boxes", "object", "state", "source", "count", "pose")
INACTIVE, PASTED, HIT_GT, HIT_PASTED, NO_ROOM, ABSENT = range(6)
CLASSES_MAX = 16


def words(seed, step, frame, n):
    """r_0 .. r_(n-1) of frame `frame`."""
    out = []
    for b in range((n + 3) // 4):
        out.extend(philox4x32_10(seed, step, frame, TAG + b))
    return out[:n]


def class_offsets(classes):
    """The 18 int32 of a bank whose objects have these (ascending) classes."""
    return np.searchsorted(np.asarray(classes, np.int64), np.arange(18), side="left").astype(np.int32)


def make_bank(points, offsets, boxes, pose=None):
    """A bank as the restatement takes it: dict(points (P, 5), offsets (O + 1) int64, boxes (O, 8), pose (O, 2) float64 -- NumPy's unless
    given --, class_offsets (18) int32), read-only."""
    boxes = np.ascontiguousarray(boxes)
    cls = boxes[:, 7].astype(np.float64)
    assert (cls == np.floor(cls)).all() and (cls >= 1).all() and (cls <= CLASSES_MAX).all() and (np.diff(cls) >= 0).all()
    bank = dict(points=np.ascontiguousarray(points).reshape(-1, 5), offsets=np.asarray(offsets, np.int64), boxes=boxes,
                pose=np.ascontiguousarray(br.numpy_pose(boxes) if pose is None else pose), class_offsets=class_offsets(cls.astype(np.int64)))
    assert bank["offsets"][0] == 0 and bank["offsets"][-1] == len(bank["points"]) and (np.diff(bank["offsets"]) >= 0).all()
    for a in bank.values():
        a.setflags(write=False)
    return bank


def slots(groups):
    """[(class, j)] of every slot q, in slot order."""
    return [(c + 1, j) for c, n in enumerate(groups) for j in range(n)]


def class_counts(gt, pose):
    """cnt_c for c = 1 .. 16 of one frame (index c - 1): the present gts whose column 7 is integral and equals c."""
    ok = br.present(gt, pose)
    with np.errstate(invalid="ignore"):
        cls = gt[:, 7].astype(np.float64)
        return [int((ok & (cls == float(c))).sum()) for c in range(1, CLASSES_MAX + 1)]


def draws(groups, cnt, bank, seed, step, frame):
    """The object of every slot, -1 for an inactive one."""
    co, r, out = bank["class_offsets"], words(seed, step, frame, sum(groups)), []
    for q, (c, j) in enumerate(slots(groups)):
        L = int(co[c + 1]) - int(co[c])
        active = j < max(groups[c - 1] - cnt[c - 1], 0) and L > 0
        out.append(int(co[c]) + ((r[q] * L) >> 32) if active else -1)
    return out


def _area(a, pa, b, pb):
    """AREA(a, b) of one pair of present boxes."""
    return float(ir.clip_area(a[None, :7].astype(np.float64), pa[None], b[None, :7].astype(np.float64), pb[None])[0])


def sweep_frame(obj, bank, gt, pose, free_total, trace=None):
    """(state, base) of every slot of one frame; trace, a dict, receives the areas that were zero against a present gt, per slot."""
    Q = len(obj)
    gt_ok = br.present(gt, pose)
    cand_ok = [o >= 0 and bool(br.present(bank["boxes"][o], bank["pose"][o])) for o in obj]
    points = [int(bank["offsets"][o + 1] - bank["offsets"][o]) if o >= 0 else 0 for o in obj]
    state, base, pasted, free_left = [INACTIVE] * Q, [0] * Q, [], free_total
    for q, o in enumerate(obj):
        if o < 0:
            continue
        hit_gt = hit_pasted = False
        if cand_ok[q]:
            a, pa = bank["boxes"][o], bank["pose"][o]
            areas = [_area(a, pa, gt[b], pose[b]) for b in np.flatnonzero(gt_ok)]
            hit_gt = any(v > 0.0 for v in areas)
            if trace is not None:
                trace[q] = areas
            hit_pasted = any(_area(a, pa, bank["boxes"][obj[p]], bank["pose"][obj[p]]) > 0.0 for p in pasted)
        if hit_gt:
            state[q] = HIT_GT
        elif hit_pasted:
            state[q] = HIT_PASTED
        elif points[q] > free_left:
            state[q] = NO_ROOM
        elif not cand_ok[q]:
            state[q] = ABSENT
        else:
            state[q], base[q] = PASTED, free_total - free_left
            free_left -= points[q]
            pasted.append(q)
    return state, base


def paste_objects(rows, offsets, keep, gt_boxes, pose, bank, groups, seed, step, ew=(0.0, 0.0, 0.0), frames=None):
    """Every output of the stage as a dict of NumPy arrays.  pose: (F, B, 2) float64, used as it is.  keep: (N) bool or None.  frames: the
    frame numbers that key the draws, 0 .. F - 1 unless given."""
    rows, gt_boxes, offsets = np.asarray(rows), np.asarray(gt_boxes), np.asarray(offsets, np.int64)
    F, B, Cb = gt_boxes.shape
    Q, N, dt = sum(groups), len(rows), rows.dtype
    assert gt_boxes.dtype == dt and bank["points"].dtype == dt and bank["boxes"].dtype == dt and pose.shape == (F, B, 2) and F == len(offsets) - 1
    present = np.ones(N, bool) if keep is None else np.asarray(keep).astype(bool)
    usable = br.usable_rows(rows, present)
    e = dict(rows=rows.copy(), keep=present.copy(), gt_boxes=np.zeros((F, B + Q, Cb), dt), object=np.full((F, Q), -1, np.int32), state=np.zeros((F, Q), np.int32),
             source=np.full(N, -1, np.int32), count=np.zeros((F, 4), np.int32), pose=np.zeros((F, B + Q, 2), np.float64))
    e["gt_boxes"][:, :B] = gt_boxes
    e["pose"][:, :B] = br.used_pose(gt_boxes, pose)
    for f in range(F):
        a, b = int(offsets[f]), int(offsets[f + 1])
        free = a + np.flatnonzero(~present[a:b])
        obj = draws(groups, class_counts(gt_boxes[f], pose[f]), bank, seed, step, f if frames is None else frames[f])
        state, base = sweep_frame(obj, bank, gt_boxes[f], pose[f], len(free))
        e["object"][f], e["state"][f] = obj, state
        pasted = [q for q in range(Q) if state[q] == PASTED]
        n_rows = 0
        for q in pasted:
            o = obj[q]
            lo, hi = int(bank["offsets"][o]), int(bank["offsets"][o + 1])
            at = free[base[q]:base[q] + hi - lo]
            e["rows"][at], e["keep"][at], e["source"][at] = bank["points"][lo:hi], True, B + q
            e["gt_boxes"][f, B + q, :8], e["pose"][f, B + q] = bank["boxes"][o], bank["pose"][o]
            n_rows += hi - lo
        removed = 0
        u = a + np.flatnonzero(usable[a:b])
        if pasted and len(u):
            picked = [obj[q] for q in pasted]
            big = rp.enlarged(bank["boxes"][picked], ew)
            inside = br.frame_matrices(rows[u, :3].astype(np.float64), big, bank["pose"][picked])[3].any(axis=1)
            e["keep"][u[inside]] = False
            removed = int(inside.sum())
        e["count"][f] = (len(pasted), n_rows, removed, len(free))
    return e


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
def _box(x, y, z, dx, dy, dz, h, cls):
    return [x, y, z, dx, dy, dz, h, cls]


def _points_in(rng, box, n, dtype):
    """n rows strictly inside `box` (well within its faces), in `dtype`, channel and intensity seeded."""
    local = rng.uniform(-0.45, 0.45, (n, 3)) * np.asarray(box[3:6], np.float64)
    xyz = br.world(np.asarray(box, np.float64), local) if n else np.zeros((0, 3))
    return np.column_stack((xyz, rng.integers(1, 255, n), rng.integers(0, 64, n))).astype(dtype)


def _bank_of(rng, boxes, counts, dtype):
    """A bank of these boxes (sorted by class already) with counts[o] points inside each (a box that is not present gets points about its centre)."""
    boxes = np.asarray(boxes, np.float64)
    pts = []
    for box, n in zip(boxes, counts):
        shape = box.copy()
        shape[3:6] = np.where(shape[3:6] > 0, shape[3:6], 1.0)
        pts.append(_points_in(rng, shape, n, dtype))
    return make_bank(np.concatenate(pts) if pts else np.zeros((0, 5), dtype), np.concatenate(([0], np.cumsum(counts))), boxes.astype(dtype))


def _scene(rng, n, dtype, absent=0.3, nan=0.2):
    """(rows, keep): n rows within +-55 m, a share absent, a share of those NaN / inf padding."""
    xyz = np.column_stack((rng.uniform(-55, 55, (n, 2)), rng.uniform(-2, 1, n)))
    rows = np.column_stack((xyz, rng.integers(1, 255, n), rng.integers(0, 64, n))).astype(dtype)
    keep = rng.uniform(size=n) >= absent
    bad = ~keep & (rng.uniform(size=n) < nan)
    rows[bad] = np.where(rng.uniform(size=(int(bad.sum()), 5)) < 0.5, np.nan, np.inf).astype(dtype)
    return rows, keep


def _finish(frames, keeps, gt, bank, groups, seed, step, ew=(0.0, 0.0, 0.0), **special):
    rows = np.ascontiguousarray(np.concatenate(frames))
    offsets = np.concatenate(([0], np.cumsum([len(p) for p in frames]))).astype(np.int64)
    gt = np.ascontiguousarray(gt)
    c = dict(rows=rows, offsets=offsets, keep=np.ascontiguousarray(np.concatenate(keeps)), gt_boxes=gt, pose=np.ascontiguousarray(br.numpy_pose(gt)), bank=bank,
             groups=tuple(int(v) for v in groups), seed=seed, step=step, ew=tuple(float(v) for v in ew), **special)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


STATE_GROUPS = (3, 2, 1, 1, 1, 1, 1, 1)          # classes 1 .. 8; see _states
STATE_SLOT = dict(first=0, twin=1, twin2=2, full=3, full2=4, on_gt=5, touching=6, no_bank=7, absent=8, exact=9, one_more=10)
STATE_POINTS = dict(A=20, D=6, C=9, E=7, Z=3, Y=1)
GT0 = _box(10.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0, 2.0)


def _states(dtype):
    """Two frames; every class of the bank but class 2 has ONE object, so the draw of its slots does not depend on the words.
    Frame 0: class 1 (n = 3) draws A = roipool_reference.FACE_ROI three times: 1, 3, 3; class 2 (n = 2) finds two gts of its class: 0, 0;
    C lies on gt 0: 2; E touches gt 0 along the edge x = 12, area exactly 0: 1; class 5 has no object: 0; Z has dx = 0: 5; X needs exactly
    the free slots that are left: 1; Y needs one more: 4.  The scene rows hold the face rows of A for no extra width and for
    roipool_reference.EW, rows that only the extra width takes, and fill; absent rows, some NaN, are strewn between them.
    Frame 1: no gt is present, 25 free slots: class 2 draws among its two objects, most candidates find no room."""
    rng = np.random.default_rng(7100)
    P = STATE_POINTS
    A = list(rp.FACE_ROI) + [1.0]
    boxes = [A, _box(40.0, 40.0, 0.0, 4.0, 2.0, 1.5, 0.3, 2.0), _box(-40.0, 30.0, 0.0, 4.0, 2.0, 1.5, -1.0, 2.0), _box(10.5, 0.3, 0.0, 4.0, 2.0, 1.5, 0.4, 3.0),
             _box(14.0, 0.0, 0.0, 4.0, 2.0, 1.5, 0.0, 4.0), _box(-30.0, 0.0, 0.0, 0.0, 2.0, 1.5, 0.0, 6.0), _box(0.0, 30.0, 0.0, 5.0, 2.0, 2.0, 2.0, 7.0),
             _box(-20.0, -20.0, 0.0, 4.0, 2.0, 1.5, 0.7, 8.0)]
    # frame 0: the scene rows
    names, pts = [], []
    for tag, e in (("", (0.0, 0.0, 0.0)), ("ew:", rp.EW)):
        for name, p in rp.face_rows(dtype, e).items():
            names.append(tag + name)
            pts.append(p)
    only = [(2.2, 0.0, 0.0), (-2.125, 0.5, 0.25), (0.0, 1.0625, 0.0), (0.5, 0.25, 1.0), (15.0, 0.5, -1.125)]       # inside A or E only by the extra width
    fill = np.column_stack((rng.uniform(-6, 18, (120, 2)), rng.uniform(-1, 1, 120))).tolist() + [(1e7, 0.0, 0.0), (0.5, 0.5, 0.0)]
    t = np.dtype(dtype).type
    xyz = np.array([[t(v) for v in p] for p in pts] + only + fill, dtype)
    scene = np.column_stack((xyz, rng.integers(1, 255, len(xyz)).astype(dtype), rng.integers(0, 64, len(xyz)).astype(dtype)))
    n_free = 70
    n_x = n_free - P["A"] - P["E"]
    n = len(scene) + n_free
    free_at = np.sort(rng.choice(n, n_free, replace=False))
    keep0 = np.ones(n, bool)
    keep0[free_at] = False
    frame0 = np.zeros((n, 5), dtype)
    frame0[keep0] = scene
    frame0[free_at[::3]] = np.nan
    frame0[free_at[1::3]] = rng.uniform(-3, 3, (len(free_at[1::3]), 5)).astype(dtype)           # absent rows inside A: never tested
    special = {nm: int(np.flatnonzero(keep0)[i]) for i, nm in enumerate(names)}
    special["only_ew"] = tuple(int(np.flatnonzero(keep0)[len(pts) + i]) for i in range(len(only)))
    special["unusable"] = int(np.flatnonzero(keep0)[len(pts) + len(only) + 120])
    bank = _bank_of(rng, boxes, [P["A"], P["D"], P["D"] + 1, P["C"], P["E"], P["Z"], n_x, P["Y"]], dtype)
    gt = np.zeros((2, 4, 8), dtype)
    gt[0, 0], gt[0, 1], gt[0, 3] = GT0, _box(-40.0, -40.0, 0.0, 4.0, 2.0, 1.5, 1.0, 2.0), _box(30.0, -30.0, 0.0, 4.0, 2.0, 1.5, 0.0, 2.5)
    gt[1, 1, 3] = np.nan                                                  # frame 1: zero rows and a NaN row, no gt present
    frame1, keep1 = _scene(rng, 300, dtype, 0.0)
    keep1[rng.choice(300, 25, replace=False)] = False
    return _finish([frame0, frame1], [keep0, keep1], gt, bank, STATE_GROUPS, 41, 3, rp.EW, special=special)


def _random_bank(rng, O, n_classes, dtype, max_points=700, spread=50.0):
    cls = np.sort(rng.integers(1, n_classes + 1, O))
    boxes = np.column_stack((rng.uniform(-spread, spread, (O, 2)), rng.uniform(-1.5, 0.0, O), rng.uniform(3.0, 5.0, O), rng.uniform(1.4, 2.2, O), rng.uniform(1.3, 2.0, O),
                             rng.uniform(-np.pi, np.pi, O), cls))
    counts = rng.integers(0, max_points + 1, O)
    return boxes, counts


def _random_gt(rng, F, B, Cb, n_classes, dtype, absent=0.3):
    gt = np.zeros((F, B, Cb))
    gt[..., 0:2] = rng.uniform(-50, 50, (F, B, 2))
    gt[..., 2] = rng.uniform(-1.5, 0.0, (F, B))
    gt[..., 3:6] = rng.uniform((3.0, 1.4, 1.3), (5.0, 2.2, 2.0), (F, B, 3))
    gt[..., 6] = rng.uniform(-7, 7, (F, B))
    gt[..., 7:] = rng.integers(1, n_classes + 1, (F, B, Cb - 7))
    gt[rng.uniform(size=(F, B)) < absent] = 0
    return gt.astype(dtype)


def _random(dtype, seed, sizes, B, Cb, groups, O=40, max_points=120, absent=0.5, gt_absent=0.3, ew=(0.2, 0.2, 0.1), spread=50.0):
    rng = np.random.default_rng(seed)
    boxes, counts = _random_bank(rng, O, len(groups), dtype, max_points, spread)
    bank = _bank_of(rng, boxes, counts, dtype)
    frames, keeps = zip(*(_scene(rng, n, dtype, absent) for n in sizes))
    return _finish(list(frames), list(keeps), _random_gt(rng, len(sizes), B, Cb, len(groups), dtype, gt_absent), bank, groups, seed, seed % 7, ew)


LENGTHS = (0, 1, 511, 512, 513, 1537)
STRADDLE_FREE = (tuple(range(58, 68)), tuple(range(505, 521)), tuple(range(1525, 1537)))
STRADDLE_POINTS = (8, 20, 10)
BIG_POINTS = (0, 64, 600)


def _straddle(dtype):
    """Frame 0 of 1537 rows has 38 absent rows in three stretches, three classes of one object each with 8, 20 and 10 points: object 0 takes
    rows 58 .. 65 (over the 64-lane border), object 1 rows 66, 67, 505 .. 520 and 1525, 1526 (over the 512-row border), object 2 rows
    1527 .. 1536 (through the frame's last row).  Frame 1 follows with absent rows of its own at its start."""
    rng = np.random.default_rng(7300)
    boxes = [_box(-30.0, 5.0, -0.5, 4.0, 2.0, 1.5, 0.2, 1.0), _box(0.0, 25.0, -0.5, 4.5, 1.8, 1.6, 1.1, 2.0), _box(30.0, -12.0, -0.5, 3.8, 1.7, 1.4, -2.0, 3.0)]
    bank = _bank_of(rng, boxes, STRADDLE_POINTS, dtype)
    f0, k0 = _scene(rng, 1537, dtype, 0.0)
    for stretch in STRADDLE_FREE:
        k0[list(stretch)] = False
    f0[[58, 510, 1536]] = np.nan
    f1, k1 = _scene(rng, 700, dtype, 0.0)
    k1[:40] = False
    gt = np.zeros((2, 3, 8), dtype)
    gt[0, 1] = _box(40.0, 40.0, 0.0, 4.0, 2.0, 1.5, 0.0, 9.0)
    return _finish([f0, f1], [k0, k1], gt, bank, (1, 1, 1), 43, 0)


def _big(dtype):
    """Three classes of one object each with 0, exactly 64 and 600 points.  Frame 0 has room for all, frame 1 no free slot at all (only the
    object of 0 points is pasted), frame 2 room for the first two only."""
    rng = np.random.default_rng(7400)
    boxes = [_box(-30.0, 5.0, -0.5, 4.0, 2.0, 1.5, 0.2, 1.0), _box(0.0, 25.0, -0.5, 4.5, 1.8, 1.6, 1.1, 2.0), _box(30.0, -12.0, -0.5, 3.8, 1.7, 1.4, -2.0, 3.0)]
    bank = _bank_of(rng, boxes, BIG_POINTS, dtype)
    f0, k0 = _scene(rng, 1500, dtype, 0.5)
    f1, k1 = _scene(rng, 600, dtype, 0.0)
    f2, k2 = _scene(rng, 900, dtype, 0.0)
    k2[100:300] = False
    return _finish([f0, f1, f2], [k0, k1, k2], np.zeros((3, 1, 8), dtype), bank, (1, 1, 1), 44, 5, (0.5, 0.5, 0.5))


CASE_NAMES = ("states", "q1", "q63", "q64", "lengths", "straddle", "big")


@lru_cache(maxsize=None)
def case(name, dtype):
    """dict(rows, offsets, keep, gt_boxes, pose, bank, groups, seed, step, ew[, special]) of a named case, read-only; the poses are NumPy's."""
    if name == "states":
        return _states(dtype)
    if name == "q1":
        return _random(dtype, 7201, (400, 300), 1, 8, (0, 1), O=6, absent=0.6, gt_absent=0.5)
    if name == "q63":
        return _random(dtype, 7202, (1500, 900), 65, 9, (20, 13, 30), O=40, gt_absent=0.6, spread=80.0)
    if name == "q64":
        return _random(dtype, 7203, (1600, 1200), 192, 10, (16, 0, 24, 24), O=40, gt_absent=0.85, spread=90.0)
    if name == "lengths":
        return _random(dtype, 7204, LENGTHS, 5, 8, (4, 4, 4), O=30, max_points=60)
    if name == "straddle":
        return _straddle(dtype)
    if name == "big":
        return _big(dtype)
    raise KeyError(name)


def expected_of(c, **changed):
    """The restatement on a case, with some of its entries replaced."""
    c = {**c, **changed}
    return paste_objects(c["rows"], c["offsets"], c["keep"], c["gt_boxes"], c["pose"], c["bank"], c["groups"], c["seed"], c["step"], c["ew"], c.get("frames"))


@lru_cache(maxsize=None)
def expected(name, dtype):
    e = expected_of(case(name, dtype))
    for a in e.values():
        a.setflags(write=False)
    return e
