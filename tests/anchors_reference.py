"""Anchor target assignment (snowgpu_assign_anchors_device) restated from its definition in include/snowgpu.h as brute-force NumPy: per
frame and class an anchors x gts float64 overlap matrix, every operation one NumPy call and so rounded on its own, two maxima and the
label rule.  Nothing here touches a GPU, and this module is no conftest: the tests import it by name.  The named cases the GPU tests run
live here too, so that tests/test_anchors_reference.py can check on any machine that each of them decides something."""
from functools import lru_cache

import numpy as np

DTYPES = ("float32", "float64")
FIELDS = ("label", "gt_index", "count", "gt_count", "iou")
PI, QUARTER_PI = np.pi, np.pi / 4
BOUND, EPS = 1e6, 1e-6
MATCHED, UNMATCHED = (0.6, 0.5, 0.5), (0.45, 0.35, 0.35)


def present(boxes):
    """Which boxes are present: the presence rule of points_in_boxes on the seven columns, no pose involved."""
    b = np.asarray(boxes)[..., :7].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.abs(b[..., 0:3]) <= BOUND).all(-1) & ((b[..., 3:6] > 0) & (b[..., 3:6] <= BOUND)).all(-1) & (np.abs(b[..., 6]) <= BOUND)


def gt_class(gt, n_classes):
    """The class number of every gt, 0 for an absent one."""
    with np.errstate(invalid="ignore"):
        c = np.asarray(gt)[..., 7].astype(np.float64)
        ok = present(gt) & (c >= 1.0) & (c <= float(n_classes)) & (np.floor(c) == c)
    return np.where(ok, np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0), 0.0).astype(np.int32)


def bev(boxes):
    """(x0, x1, y0, y1, area) of the nearest axis-aligned BEV boxes of present boxes (n, >= 7), float64."""
    b = np.asarray(boxes)[..., :7].astype(np.float64)
    cx, cy, dx, dy, h = b[..., 0], b[..., 1], b[..., 3], b[..., 4], b[..., 6]
    k = np.floor(np.add(np.divide(h, PI), 0.5))
    turn = np.abs(np.subtract(h, np.multiply(k, PI)))
    keep = turn < QUARTER_PI
    ex, ey = np.where(keep, dx, dy), np.where(keep, dy, dx)
    hx, hy = np.divide(ex, 2.0), np.divide(ey, 2.0)
    x0, x1, y0, y1 = np.subtract(cx, hx), np.add(cx, hx), np.subtract(cy, hy), np.add(cy, hy)
    return x0, x1, y0, y1, np.multiply(np.subtract(x1, x0), np.subtract(y1, y0))


def overlaps(anchors, gts):
    """The (n_a, n_g) float64 overlap matrix of present anchors and present gts."""
    ax0, ax1, ay0, ay1, aa = (v[:, None] for v in bev(anchors))
    gx0, gx1, gy0, gy1, ga = (v[None, :] for v in bev(gts))
    ix = np.maximum(np.subtract(np.minimum(ax1, gx1), np.maximum(ax0, gx0)), 0.0)
    iy = np.maximum(np.subtract(np.minimum(ay1, gy1), np.maximum(ay0, gy0)), 0.0)
    inter = np.multiply(ix, iy)
    return np.divide(inter, np.maximum(np.subtract(np.add(aa, ga), inter), EPS))


def assign(anchors, anchor_class, gt_boxes, matched=MATCHED, unmatched=UNMATCHED):
    """The outputs of the entry as a dict of arrays (FIELDS), and beside them `best` (F, A float64), `forced` (F, A bool: the anchor is some
    gt's best) and `top` (F, B float64)."""
    anchors, gt_boxes, anchor_class = np.asarray(anchors), np.asarray(gt_boxes), np.asarray(anchor_class)
    NC = len(matched)
    assert len(unmatched) == NC and all(0 < u <= m <= 1 for m, u in zip(matched, unmatched))
    F, B = gt_boxes.shape[:2]
    A = anchors.shape[0]
    a_ok = present(anchors) & (anchor_class >= 1) & (anchor_class <= NC)
    label, gt_index = np.full((F, A), -1, np.int32), np.full((F, A), -1, np.int32)
    best, forced, top = np.zeros((F, A)), np.zeros((F, A), bool), np.zeros((F, B))
    count, gt_count = np.zeros((F, 3), np.int32), np.zeros((F, B), np.int32)
    for f in range(F):
        g_cls = gt_class(gt_boxes[f], NC)
        for c in range(1, NC + 1):
            ai, gi = np.flatnonzero(a_ok & (anchor_class == c)), np.flatnonzero(g_cls == c)
            if not len(ai):
                continue
            b, arg, frc = np.zeros(len(ai)), np.full(len(ai), -1), np.zeros(len(ai), bool)
            if len(gi):
                m = overlaps(anchors[ai], gt_boxes[f, gi])
                b = m.max(axis=1)
                arg = np.where(b > 0, gi[m.argmax(axis=1)], -1)                # (NumPy's argmax: the first of equal maxima)
                t = m.max(axis=0)
                top[f, gi] = t
                frc = ((m == t[None, :]) & (t[None, :] > 0)).any(axis=1)
            pos = frc | (b >= matched[c - 1])
            neg = ~pos & (b < unmatched[c - 1])
            label[f, ai] = np.where(pos, c, np.where(neg, 0, -1))
            gt_index[f, ai] = np.where(pos, arg, -1)
            best[f, ai], forced[f, ai] = b, frc
        count[f] = ((label[f] > 0).sum(), (a_ok & (label[f] == 0)).sum(), (a_ok & (label[f] < 0)).sum())
        gt_count[f] = np.bincount(gt_index[f][gt_index[f] >= 0], minlength=B)
    return dict(label=label, gt_index=gt_index, count=count, gt_count=gt_count, iou=best.astype(anchors.dtype), best=best, forced=forced, top=top,
                anchor_ok=a_ok)


# ---- the shared cases ---------------------------------------------------------------------------------------------------------------------------
def box(cx, cy, dx, dy, h=0.0, cls=None, cz=0.0, dz=1.5):
    return [cx, cy, cz, dx, dy, dz, h] + ([] if cls is None else [cls])


def _case(dtype, anchors, anchor_class, gt, matched=MATCHED, unmatched=UNMATCHED):
    out = dict(anchors=np.array(anchors, np.float64).astype(dtype), anchor_class=np.array(anchor_class, np.int32), gt_boxes=np.array(gt, np.float64).astype(dtype),
               matched=tuple(float(v) for v in matched), unmatched=tuple(float(v) for v in unmatched))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _by_hand(dtype):
    """Six anchors, three gts, worked out in tests/test_anchors_reference.py."""
    anchors = [box(0, 0, 4, 2), box(1, 0, 4, 2), box(1.5, 0, 4, 2), box(20, 0, 4, 2), box(0, 5, 1, 1), box(3, 5, 1, 1)]
    gt = [[box(0, 0, 4, 2, 0, 1), box(22, 0, 4, 2, 0, 1), box(0.25, 5, 1, 1, 0, 2)]]
    return _case(dtype, anchors, [1, 1, 1, 1, 2, 2], gt, (0.6, 0.5), (0.45, 0.35))


def _after(v):
    return float(np.nextafter(v, 2.0))


def _before(v):
    return float(np.nextafter(v, 0.0))


THRESHOLD_SETTINGS = tuple([(m, u) for m in (_before(0.5), 0.5, _after(0.5)) for u in (_before(0.25), 0.25, _after(0.25))] +
                           [(_after(0.5), 0.5), (_after(0.5), _after(0.5)), (0.5, 0.5), (0.5, _before(0.5)), (0.25, 0.25), (_after(0.25), _after(0.25)),
                            (_before(0.25), _before(0.25)), (0.25, _before(0.25)), (_after(0.25), 0.25)])
P_HALF, Q_HALF, P_QUARTER, Q_QUARTER = 0, 1, 2, 3          # the anchors of `thresholds`


def _thresholds(dtype, which):
    """Anchor 4 x 2 and gt 2 x 2 on one centre: 4 / 8 = 0.5 exactly; a 1 x 2 gt: 2 / 8 = 0.25.  Beside each a second anchor that fits its gt,
    so that the first is not the gt's best and is judged by the thresholds alone."""
    anchors = [box(0, 0, 4, 2), box(0, 0, 2, 2), box(100, 0, 4, 2), box(100, 0, 1, 2)]
    gt = [[box(0, 0, 2, 2, 0, 1), box(100, 0, 1, 2, 0, 1)]]
    m, u = THRESHOLD_SETTINGS[which]
    return _case(dtype, anchors, [1, 1, 1, 1], gt, (m,), (u,))


def heading_values():
    """float64 headings: the double and the float nearest +-pi / 4, 3 pi / 4 and 5 pi / 4 with one step of their own format on either side,
    then 0, +-pi / 2, pi, 1e5 and -0.0."""
    out = []
    for base in (np.pi / 4, -np.pi / 4, 3 * np.pi / 4, 5 * np.pi / 4):
        d, s = np.float64(base), np.float32(base)
        out += [d, np.nextafter(d, np.inf), np.nextafter(d, -np.inf), np.float64(s), np.float64(np.nextafter(s, np.float32(np.inf))),
                np.float64(np.nextafter(s, np.float32(-np.inf)))]
    return [float(v) for v in out] + [0.0, np.pi / 2, -np.pi / 2, np.pi, 1e5, -0.0]


def _headings(dtype):
    """Site i, 20 m apart: in the row y = 0 the gt turns (4 x 2 under heading h_i), in the row y = 50 the anchor does.  A box that keeps its
    sides meets its 4 x 2 partner at 1, a box that swaps them at 4 / 12.  A second anchor (3.5 x 2) beside each: where the sides are
    swapped it is the better partner, so the first anchor is background there."""
    anchors, cls, gt = [], [], []
    for i, h in enumerate(heading_values()):
        x = 20.0 * i
        anchors += [box(x, 0, 4, 2), box(x, 0, 3.5, 2), box(x, 50, 4, 2, h), box(x, 50, 3.5, 2, h)]
        gt += [box(x, 0, 4, 2, h, 1), box(x, 50, 4, 2, 0, 1)]
        cls += [1, 1, 1, 1]
    return _case(dtype, anchors, cls, [gt], (0.6,), (0.45,))


FORCED = dict(low=0, tie_a=1, tie_b=2, quirk=3, quirk_rival=4, twin=5, far_a=10, far_b=70, far_c=1500, n=1600)
FORCED_GT = dict(low=0, tie=1, nothing=2, quirk_forcing=3, quirk_own=4, twin_a=5, twin_b=6, far=7, other_class=8)


def _forced(dtype):
    n = FORCED["n"]
    anchors = [box(-1000.0 - 10 * i, -1000, 4, 2) for i in range(n)]                 # filler: present, meeting nothing
    cls = [1] * n
    anchors[FORCED["low"]] = box(0, 0, 4, 2)                # meets gt `low` at 2 / 14: below unmatched, its best anchor
    anchors[FORCED["tie_a"]] = box(100, 0, 4, 2)            # gt `tie` lies between these two: 5 / 11 each
    anchors[FORCED["tie_b"]] = box(103, 0, 4, 2)
    anchors[FORCED["quirk"]] = box(200, 0, 4, 2)            # forced by gt `quirk_forcing` (2 / 14), its own arg is `quirk_own` (5 / 11)
    anchors[FORCED["quirk_rival"]] = box(201.5, 0, 4, 2)    # fits `quirk_own`: the quirk anchor is not that gt's best
    anchors[FORCED["twin"]] = box(300, 0, 4, 2)             # two bit-equal gts on it
    anchors[FORCED["far_a"]] = box(398.5, 0, 4, 2)          # three anchors tied at 5 / 11 on gt `far`: two waves of one workgroup, and
    anchors[FORCED["far_b"]] = box(398.5, 0, 4, 2)          # another workgroup
    anchors[FORCED["far_c"]] = box(401.5, 0, 4, 2)
    gt = [None] * 9
    gt[FORCED_GT["low"]] = box(3, 0, 4, 2, 0, 1)
    gt[FORCED_GT["tie"]] = box(101.5, 0, 4, 2, 0, 1)
    gt[FORCED_GT["nothing"]] = box(500, 500, 4, 2, 0, 1)
    gt[FORCED_GT["quirk_forcing"]] = box(197, 0, 4, 2, 0, 1)
    gt[FORCED_GT["quirk_own"]] = box(201.5, 0, 4, 2, 0, 1)
    gt[FORCED_GT["twin_a"]] = box(300.5, 0, 4, 2, 0, 1)
    gt[FORCED_GT["twin_b"]] = box(300.5, 0, 4, 2, 0, 1)
    gt[FORCED_GT["far"]] = box(400, 0, 4, 2, 0, 1)
    gt[FORCED_GT["other_class"]] = box(0, 0, 4, 2, 0, 2)    # on anchor `low`, of another class: it takes no part
    return _case(dtype, anchors, cls, [gt], (0.6, 0.5), (0.45, 0.35))


ABSENT_ANCHORS = dict(zero_size=3, class_0=4, class_4=5)


def _absent(dtype):
    """Three frames, three classes: frame 0 holds every kind of absent gt, each lying exactly on an anchor it would win, and gts of classes 1
    and 2 only; frame 1 holds no gt at all; frame 2 is ordinary."""
    anchors = [box(10.0 * i, 0, 4, 2) for i in range(12)] + [box(10.0 * i, 30, 1, 1) for i in range(4)] + [box(10.0 * i, 60, 2, 1) for i in range(4)]
    cls = [1] * 12 + [2] * 4 + [3] * 4
    anchors[ABSENT_ANCHORS["zero_size"]] = box(30, 0, 4, 0)
    cls[ABSENT_ANCHORS["class_0"]] = 0
    cls[ABSENT_ANCHORS["class_4"]] = 4
    nan = float("nan")
    f0 = [[0.0] * 8, box(nan, 0, 4, 2, 0, 1), box(10, 0, 4, 2, 0, 0), box(20, 0, 4, 2, 0, 4), box(60, 0, 4, 2, 0, 1.5), box(2e6, 0, 4, 2, 0, 1),
          box(70, 0, 4, 2, nan, 1), box(80, 0, 4, 2, 0, nan), box(80, 0, 4, -2, 0, 1),
          box(30, 0, 4, 2, 0, 1), box(40, 0, 4, 2, 0, 1), box(50, 0, 4, 2, 0, 1),     # on the three absent anchors
          box(90.5, 0, 4, 2, 0, 1), box(0.2, 30, 1, 1, 0, 2)]
    f1 = [[0.0] * 8 for _ in f0]
    f2 = [box(1, 0, 4, 2, 0, 1), box(10.4, 30, 1, 1, 0, 2), box(20.5, 60, 2, 1, 0, 3)] + [[0.0] * 8 for _ in f0[3:]]
    return _case(dtype, anchors, cls, [f0, f1, f2])


GRID_RANGE, GRID_N = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0), (22, 25)
GRID_SIZES, GRID_ROTATIONS, GRID_BOTTOMS = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73)), (0.0, np.pi / 2), (-1.78, -0.6, -0.6)
# one seed per frame; those of B = 1 were picked so that the single gt leaves all three labels behind (tests/test_anchors_reference.py checks it)
GRID_SEEDS = {1: (1005, 1016, 1027), 64: (64000, 64001, 64002), 65: (65000, 65001, 65002), 256: (256000, 256001, 256002)}


def grid_anchors(align_center=False):
    """(anchors (A, 7) float64, anchor_class (A) int32) of the grid: a = ((y nx + x) NC + c) R + r."""
    (nx, ny), lo, hi = GRID_N, GRID_RANGE[:3], GRID_RANGE[3:]

    def centres(a, b, n):
        i = np.arange(n, dtype=np.float64)
        return a + (i + 0.5) * ((b - a) / n) if align_center else a + i * ((b - a) / (n - 1))
    xs, ys = centres(lo[0], hi[0], nx), centres(lo[1], hi[1], ny)
    anchors, cls = [], []
    for y in range(ny):
        for x in range(nx):
            for c, (size, low) in enumerate(zip(GRID_SIZES, GRID_BOTTOMS)):
                for r in GRID_ROTATIONS:
                    anchors.append([xs[x], ys[y], low + size[2] / 2, *size, r])
                    cls.append(c + 1)
    return np.array(anchors, np.float64), np.array(cls, np.int32)


def grid_gts(seed, B, xs, ys):
    """B gts of one frame around grid positions: a random class, its size within 15 %, off the position by up to 0.35 of the size, any heading."""
    rng = np.random.default_rng(seed)
    out = np.zeros((B, 8))
    c = rng.integers(0, 3, B)
    size = np.array(GRID_SIZES)[c] * rng.uniform(0.85, 1.15, (B, 3))
    out[:, 0] = xs[rng.integers(0, len(xs), B)] + rng.uniform(-0.35, 0.35, B) * size[:, 0]
    out[:, 1] = ys[rng.integers(0, len(ys), B)] + rng.uniform(-0.35, 0.35, B) * size[:, 1]
    out[:, 2] = np.array(GRID_BOTTOMS)[c] + size[:, 2] / 2
    out[:, 3:6] = size
    out[:, 6] = rng.uniform(-np.pi, np.pi, B)
    out[:, 7] = c + 1
    return out


def _grid(dtype, B):
    anchors, cls = grid_anchors()
    xs, ys = np.unique(anchors[:, 0]), np.unique(anchors[:, 1])
    gt = np.stack([grid_gts(seed, B, xs, ys) for seed in GRID_SEEDS[B]])
    return _case(dtype, anchors, cls, gt)


GRID_NAMES = tuple(f"grid_b{B}" for B in GRID_SEEDS)
THRESHOLD_NAMES = tuple(f"thresholds_{i}" for i in range(len(THRESHOLD_SETTINGS)))
CASE_NAMES = ("by_hand",) + THRESHOLD_NAMES + ("headings", "forced", "absent") + GRID_NAMES


@lru_cache(maxsize=None)
def case(name, dtype):
    """The inputs of a named case: anchors, anchor_class, gt_boxes (read-only arrays), matched, unmatched."""
    if name.startswith("thresholds_"):
        return _thresholds(dtype, int(name.split("_")[1]))
    if name.startswith("grid_b"):
        return _grid(dtype, int(name[6:]))
    return {"by_hand": _by_hand, "headings": _headings, "forced": _forced, "absent": _absent}[name](dtype)


def expected_of(c, **changed):
    c = {**c, **changed}
    return assign(c["anchors"], c["anchor_class"], c["gt_boxes"], c["matched"], c["unmatched"])


@lru_cache(maxsize=None)
def expected(name, dtype):
    return expected_of(case(name, dtype))
